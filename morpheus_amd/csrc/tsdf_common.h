// What the dense TSDF store (tsdf.hip) and the pooled block-sparse one (tsdf_sparse.hip) share: the frame and box arguments,
// the usable-depth rule, the back-projection, the touch pass's block range and the update of one voxel.  Every fp32 expression
// is the text of include/morpheus_hip.h (TSDF fusion); both files are built without FP contraction, so the two stores give the
// same bits for the same voxel.
#pragma once
#include "common.h"

#define TSDF_BLOCK 8
#define TSDF_THREADS 256
#define TSDF_MAX_SIDE 16384

struct TsdfFrame {
    int32_t H, W;
    float fx, fy, cx, cy;
    float m[12];                // touch / bounds: camera-to-world; integrate: world-to-camera.  Row-major [3][4]
    float depth_scale, depth_trunc;
};

struct TsdfBox {
    float ox, oy, oz, voxel_length, sdf_trunc;
    int32_t nbx, nby, nbz;      // blocks per side
};

// d = depth / depth_scale when the pixel is usable, else a negative number
__device__ __forceinline__ float tsdf_depth(const float *__restrict__ depth, const uint8_t *__restrict__ mask, const TsdfFrame &f,
                                            int i, int j) {
    const int64_t q = (int64_t)j * f.W + i;
    if (mask && !mask[q]) return -1.f;
    const float d = depth[q] / f.depth_scale;
    if (!(d > 0.f && d <= f.depth_trunc)) return -1.f;        // NaN fails both; +inf fails the second
    return d;
}

// world-space point of pixel (i, j) at depth d: pc = (((i + 0.5) - cx) / fx * d, ((j + 0.5) - cy) / fy * d, d), P = R pc + t
__device__ __forceinline__ void tsdf_back_project(const TsdfFrame &f, int i, int j, float d, float P[3]) {
    const float xc = ((((float)i + 0.5f) - f.cx) / f.fx) * d;
    const float yc = ((((float)j + 0.5f) - f.cy) / f.fy) * d;
#pragma unroll
    for (int r = 0; r < 3; r++) P[r] = ((f.m[4 * r] * xc + f.m[4 * r + 1] * yc) + f.m[4 * r + 2] * d) + f.m[4 * r + 3];
}

// block range [lo, hi] along one axis of the interval [p - trunc, p + trunc]; false when it misses the box (or p is NaN)
__device__ __forceinline__ bool tsdf_block_range(float p, float trunc, float origin, float block_len, int32_t nb, int &lo, int &hi) {
    const float a = floorf(((p - trunc) - origin) / block_len), b = floorf(((p + trunc) - origin) / block_len);
    if (!(b >= 0.f && a <= (float)(nb - 1))) return false;
    lo = (int)fmaxf(a, 0.f);
    hi = (int)fminf(b, (float)(nb - 1));
    return true;
}

// the clipped block range of sampled pixel s of the touch pass; false when the pixel is not usable or misses the box
__device__ __forceinline__ bool tsdf_touch_range(const float *__restrict__ depth, const uint8_t *__restrict__ mask, const TsdfFrame &f,
                                                 const TsdfBox &b, int32_t stride, int32_t ns_w, int64_t s, int lo[3], int hi[3]) {
    const int j = (int)(s / ns_w) * stride, i = (int)(s % ns_w) * stride;
    const float d = tsdf_depth(depth, mask, f, i, j);
    if (!(d > 0.f)) return false;
    float P[3];
    tsdf_back_project(f, i, j, d, P);
    const float bl = 8.0f * b.voxel_length;
    return tsdf_block_range(P[0], b.sdf_trunc, b.ox, bl, b.nbx, lo[0], hi[0]) &&
           tsdf_block_range(P[1], b.sdf_trunc, b.oy, bl, b.nby, lo[1], hi[1]) &&
           tsdf_block_range(P[2], b.sdf_trunc, b.oz, bl, b.nbz, lo[2], hi[2]);
}

// one frame into the voxel at (px, py, pz): tsdf, weight and the three colours are the voxel's own five words
__device__ __forceinline__ void tsdf_update_voxel(const float *__restrict__ depth, const uint8_t *__restrict__ rgb,
                                                  const uint8_t *__restrict__ mask, const TsdfFrame &f, float sdf_trunc, float px,
                                                  float py, float pz, float *__restrict__ tsdf, float *__restrict__ weight,
                                                  float *__restrict__ c0, float *__restrict__ c1, float *__restrict__ c2) {
    float pc[3];
#pragma unroll
    for (int q = 0; q < 3; q++) pc[q] = ((f.m[4 * q] * px + f.m[4 * q + 1] * py) + f.m[4 * q + 2] * pz) + f.m[4 * q + 3];
    if (!(pc[2] > 0.f)) return;
    const float u = floorf((f.fx * pc[0]) / pc[2] + f.cx), v = floorf((f.fy * pc[1]) / pc[2] + f.cy);
    if (!(u >= 0.f && u < (float)f.W && v >= 0.f && v < (float)f.H)) return;
    const int pi = (int)u, pj = (int)v;
    const float d = tsdf_depth(depth, mask, f, pi, pj);
    if (!(d > 0.f)) return;
    const float a = (((float)pi + 0.5f) - f.cx) / f.fx, c = (((float)pj + 0.5f) - f.cy) / f.fy;
    const float m = sqrtf((1.0f + a * a) + c * c);
    const float sdf = (d - pc[2]) * m;
    if (!(sdf > -sdf_trunc)) return;
    const float q = sdf / sdf_trunc;
    const float t = q < 1.0f ? q : 1.0f;
    const float w = *weight, w1 = w + 1.0f;
    *tsdf = (*tsdf * w + t) / w1;
    const uint8_t *px8 = rgb + 3 * ((int64_t)pj * f.W + pi);
    *c0 = (*c0 * w + (float)px8[0]) / w1;
    *c1 = (*c1 * w + (float)px8[1]) / w1;
    *c2 = (*c2 * w + (float)px8[2]) / w1;
    *weight = w1;
}

static inline bool tsdf_frame(TsdfFrame *f, const float *depth, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                              const float *m_host, float depth_scale, float depth_trunc) {
    if (!depth || !m_host || H < 1 || W < 1 || H > TSDF_MAX_SIDE || W > TSDF_MAX_SIDE) return false;
    if (!(fx != 0.f) || !(fy != 0.f) || !(depth_scale > 0.f) || !(depth_trunc > 0.f)) return false;
    f->H = H, f->W = W, f->fx = fx, f->fy = fy, f->cx = cx, f->cy = cy;
    for (int q = 0; q < 12; q++) f->m[q] = m_host[q];
    f->depth_scale = depth_scale, f->depth_trunc = depth_trunc;
    return true;
}

// the dense store's box: fewer than 2^31 voxels
static inline bool tsdf_box(TsdfBox *b, float ox, float oy, float oz, float voxel_length, float sdf_trunc, int32_t nbx, int32_t nby,
                            int32_t nbz) {
    if (!(voxel_length > 0.f) || !(sdf_trunc > 0.f) || nbx < 1 || nby < 1 || nbz < 1) return false;
    if ((int64_t)nbx * nby * nbz * 512 >= ((int64_t)1 << 31)) return false;
    b->ox = ox, b->oy = oy, b->oz = oz, b->voxel_length = voxel_length, b->sdf_trunc = sdf_trunc;
    b->nbx = nbx, b->nby = nby, b->nbz = nbz;
    return true;
}

// the sparse store's logical box: at most TSDF_SPARSE_MAX_SIDE blocks a side and fewer than 2^31 blocks
#define TSDF_SPARSE_MAX_SIDE 4096
static inline bool tsdf_sparse_grid(int32_t nbx, int32_t nby, int32_t nbz) {
    if (nbx < 1 || nby < 1 || nbz < 1 || nbx > TSDF_SPARSE_MAX_SIDE || nby > TSDF_SPARSE_MAX_SIDE || nbz > TSDF_SPARSE_MAX_SIDE)
        return false;
    return (int64_t)nbx * nby * nbz < ((int64_t)1 << 31);
}
static inline bool tsdf_sparse_box(TsdfBox *b, float ox, float oy, float oz, float voxel_length, float sdf_trunc, int32_t nbx,
                                   int32_t nby, int32_t nbz) {
    if (!(voxel_length > 0.f) || !(sdf_trunc > 0.f) || !tsdf_sparse_grid(nbx, nby, nbz)) return false;
    b->ox = ox, b->oy = oy, b->oz = oz, b->voxel_length = voxel_length, b->sdf_trunc = sdf_trunc;
    b->nbx = nbx, b->nby = nby, b->nbz = nbz;
    return true;
}
