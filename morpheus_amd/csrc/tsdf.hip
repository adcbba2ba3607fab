// TSDF fusion of RGB-D frames into a dense box of voxels (run_tsdf_fusion / back_proj_frame, tools/vis.py:251-361: Open3D's
// ScalableTSDFVolume on the host there).  Conventions, limits and every fp32 expression are in include/morpheus_hip.h (TSDF
// fusion); this file is built without FP contraction and tests/tsdf_oracle.py restates it operator by operator.
//
//   tsdf_bounds_kernel     a lane per sampled pixel: back-projected point -> min / max per axis (wave butterfly, then integer
//                          atomics on ordered bit patterns: order-free)
//   tsdf_touch_kernel      a lane per sampled pixel: marks the 8^3 blocks that meet the cube of half side sdf_trunc around its
//                          back-projected point (plain byte stores of 1)
//   tsdf_integrate_kernel  a workgroup per TSDF_GROUP blocks that follow each other along z: 8 (y) x 32 (z) lanes walk the 8 x
//                          planes, so that every 32-lane row reads and writes one 128-byte line of each of the five per-voxel
//                          arrays; a group without an active block returns after its activity bytes
//   tsdf_vertex_colors_kernel  a lane per marching-cubes vertex
// Every loop is bounded by the box or the image; every index is formed from clamped integers.
#include "common.h"

#define TSDF_BLOCK 8
#define TSDF_GROUP 4                                    // blocks per workgroup along z: 32 voxels = one 128-byte line
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

// fp32 bits -> int32 that orders like the value (-0 below +0)
__device__ __forceinline__ int32_t tsdf_ordered(float v) {
    const int32_t b = __float_as_int(v);
    return b >= 0 ? b : b ^ 0x7fffffff;
}

__global__ __launch_bounds__(TSDF_THREADS) void tsdf_bounds_kernel(const float *__restrict__ depth, const uint8_t *__restrict__ mask,
                                                                   TsdfFrame f, int32_t stride, int32_t ns_w, int64_t n_samples,
                                                                   int32_t *__restrict__ bounds) {
    const int64_t s = (int64_t)blockIdx.x * TSDF_THREADS + threadIdx.x;
    int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    if (s < n_samples) {
        const int j = (int)(s / ns_w) * stride, i = (int)(s % ns_w) * stride;
        const float d = tsdf_depth(depth, mask, f, i, j);
        if (d > 0.f) {
            float P[3];
            tsdf_back_project(f, i, j, d, P);
            if (fabsf(P[0]) < INFINITY && fabsf(P[1]) < INFINITY && fabsf(P[2]) < INFINITY) {
#pragma unroll
                for (int a = 0; a < 3; a++) lo[a] = hi[a] = tsdf_ordered(P[a]);
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo[a] = min(lo[a], __shfl_xor(lo[a], o));
            hi[a] = max(hi[a], __shfl_xor(hi[a], o));
        }
    }
    if (mh_lane() == 0 && lo[0] != INT32_MAX) {                // a wave with a usable pixel has all six
#pragma unroll
        for (int a = 0; a < 3; a++) {
            atomicMin(bounds + a, lo[a]);
            atomicMax(bounds + 3 + a, hi[a]);
        }
    }
}

// block range [lo, hi] along one axis of the interval [p - trunc, p + trunc]; false when it misses the box (or p is NaN)
__device__ __forceinline__ bool tsdf_block_range(float p, float trunc, float origin, float block_len, int32_t nb, int &lo, int &hi) {
    const float a = floorf(((p - trunc) - origin) / block_len), b = floorf(((p + trunc) - origin) / block_len);
    if (!(b >= 0.f && a <= (float)(nb - 1))) return false;
    lo = (int)fmaxf(a, 0.f);
    hi = (int)fminf(b, (float)(nb - 1));
    return true;
}

__global__ __launch_bounds__(TSDF_THREADS) void tsdf_touch_kernel(const float *__restrict__ depth, const uint8_t *__restrict__ mask,
                                                                  TsdfFrame f, TsdfBox b, int32_t stride, int32_t ns_w,
                                                                  int64_t n_samples, uint8_t *__restrict__ active) {
    const int64_t s = (int64_t)blockIdx.x * TSDF_THREADS + threadIdx.x;
    if (s >= n_samples) return;
    const int j = (int)(s / ns_w) * stride, i = (int)(s % ns_w) * stride;
    const float d = tsdf_depth(depth, mask, f, i, j);
    if (!(d > 0.f)) return;
    float P[3];
    tsdf_back_project(f, i, j, d, P);
    const float bl = 8.0f * b.voxel_length;
    int x0, x1, y0, y1, z0, z1;
    if (!tsdf_block_range(P[0], b.sdf_trunc, b.ox, bl, b.nbx, x0, x1) || !tsdf_block_range(P[1], b.sdf_trunc, b.oy, bl, b.nby, y0, y1) ||
        !tsdf_block_range(P[2], b.sdf_trunc, b.oz, bl, b.nbz, z0, z1))
        return;
    for (int x = x0; x <= x1; x++)
        for (int y = y0; y <= y1; y++)
            for (int z = z0; z <= z1; z++) active[((int64_t)x * b.nby + y) * b.nbz + z] = 1;
}

__global__ __launch_bounds__(TSDF_THREADS) void tsdf_integrate_kernel(const float *__restrict__ depth, const uint8_t *__restrict__ rgb,
                                                                      const uint8_t *__restrict__ mask, TsdfFrame f, TsdfBox b,
                                                                      int32_t groups_z, const uint8_t *__restrict__ active,
                                                                      float *__restrict__ tsdf, float *__restrict__ weight,
                                                                      float *__restrict__ color) {
    const uint32_t g = blockIdx.x;
    const int gz = (int)(g % (uint32_t)groups_z);
    const uint32_t r = g / (uint32_t)groups_z;
    const int by = (int)(r % (uint32_t)b.nby), bx = (int)(r / (uint32_t)b.nby);
    const int bz0 = gz * TSDF_GROUP;
    const uint8_t *act = active + ((int64_t)bx * b.nby + by) * b.nbz + bz0;
    const int nb = min(TSDF_GROUP, b.nbz - bz0);
    uint32_t any = 0;
    for (int q = 0; q < nb; q++) any |= act[q];
    if (!any) return;                                          // uniform over the workgroup
    const int zz = threadIdx.x & 31, mine = zz >> 3;
    if (mine >= nb || !act[mine]) return;
    const int ny = b.nby * TSDF_BLOCK, nz = b.nbz * TSDF_BLOCK;
    const int j = by * TSDF_BLOCK + (threadIdx.x >> 5), k = bz0 * TSDF_BLOCK + zz;
    const int64_t plane = (int64_t)b.nbx * TSDF_BLOCK * ny * nz;
    const float py = b.oy + ((float)j + 0.5f) * b.voxel_length, pz = b.oz + ((float)k + 0.5f) * b.voxel_length;
#pragma unroll 4
    for (int xi = 0; xi < TSDF_BLOCK; xi++) {
        const int i = bx * TSDF_BLOCK + xi;
        const float px = b.ox + ((float)i + 0.5f) * b.voxel_length;
        float pc[3];
#pragma unroll
        for (int q = 0; q < 3; q++) pc[q] = ((f.m[4 * q] * px + f.m[4 * q + 1] * py) + f.m[4 * q + 2] * pz) + f.m[4 * q + 3];
        if (!(pc[2] > 0.f)) continue;
        const float u = floorf((f.fx * pc[0]) / pc[2] + f.cx), v = floorf((f.fy * pc[1]) / pc[2] + f.cy);
        if (!(u >= 0.f && u < (float)f.W && v >= 0.f && v < (float)f.H)) continue;
        const int pi = (int)u, pj = (int)v;
        const float d = tsdf_depth(depth, mask, f, pi, pj);
        if (!(d > 0.f)) continue;
        const float a = (((float)pi + 0.5f) - f.cx) / f.fx, c = (((float)pj + 0.5f) - f.cy) / f.fy;
        const float m = sqrtf((1.0f + a * a) + c * c);
        const float sdf = (d - pc[2]) * m;
        if (!(sdf > -b.sdf_trunc)) continue;
        const float q = sdf / b.sdf_trunc;
        const float t = q < 1.0f ? q : 1.0f;
        const int64_t p = ((int64_t)i * ny + j) * nz + k;
        const float w = weight[p], w1 = w + 1.0f;
        tsdf[p] = (tsdf[p] * w + t) / w1;
        const uint8_t *px8 = rgb + 3 * ((int64_t)pj * f.W + pi);
#pragma unroll
        for (int ch = 0; ch < 3; ch++) color[ch * plane + p] = (color[ch * plane + p] * w + (float)px8[ch]) / w1;
        weight[p] = w1;
    }
}

__global__ __launch_bounds__(TSDF_THREADS) void tsdf_vertex_colors_kernel(const float *__restrict__ vertices, int64_t V,
                                                                          const float *__restrict__ color, int32_t nx, int32_t ny,
                                                                          int32_t nz, float *__restrict__ out) {
    const int64_t v = (int64_t)blockIdx.x * TSDF_THREADS + threadIdx.x;
    if (v >= V) return;
    const int n[3] = {nx, ny, nz};
    const int64_t st[3] = {(int64_t)ny * nz, nz, 1};
    int64_t p0 = 0, step = 0;
    float t = 0.f;
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float x = vertices[3 * v + a], fl = floorf(x);
        if (!(fl >= 0.f && fl <= (float)(n[a] - 1))) {
            ok = false;
            continue;
        }
        const int q = (int)fl;
        const float fr = x - fl;
        p0 += q * st[a];
        if (fr > 0.f && step == 0 && q + 1 < n[a]) {           // the edge's axis: the one coordinate off the grid
            t = fr;
            step = st[a];
        }
    }
    const int64_t plane = (int64_t)nx * ny * nz;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        float c = 0.f;
        if (ok) {
            const float c0 = color[ch * plane + p0], c1 = color[ch * plane + p0 + step];
            c = ((1.0f - t) * c0 + t * c1) / 255.0f;
        }
        out[3 * v + ch] = c;
    }
}

static bool tsdf_frame(TsdfFrame *f, const float *depth, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                       const float *m_host, float depth_scale, float depth_trunc) {
    if (!depth || !m_host || H < 1 || W < 1 || H > TSDF_MAX_SIDE || W > TSDF_MAX_SIDE) return false;
    if (!(fx != 0.f) || !(fy != 0.f) || !(depth_scale > 0.f) || !(depth_trunc > 0.f)) return false;
    f->H = H, f->W = W, f->fx = fx, f->fy = fy, f->cx = cx, f->cy = cy;
    for (int q = 0; q < 12; q++) f->m[q] = m_host[q];
    f->depth_scale = depth_scale, f->depth_trunc = depth_trunc;
    return true;
}

static bool tsdf_box(TsdfBox *b, float ox, float oy, float oz, float voxel_length, float sdf_trunc, int32_t nbx, int32_t nby,
                     int32_t nbz) {
    if (!(voxel_length > 0.f) || !(sdf_trunc > 0.f) || nbx < 1 || nby < 1 || nbz < 1) return false;
    if ((int64_t)nbx * nby * nbz * 512 >= ((int64_t)1 << 31)) return false;
    b->ox = ox, b->oy = oy, b->oz = oz, b->voxel_length = voxel_length, b->sdf_trunc = sdf_trunc;
    b->nbx = nbx, b->nby = nby, b->nbz = nbz;
    return true;
}

extern "C" int32_t mh_tsdf_group_blocks(void) { return TSDF_GROUP; }

extern "C" int mh_tsdf_bounds(const float *depth, const uint8_t *mask, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                              const float *c2w_host, float depth_scale, float depth_trunc, int32_t stride, int32_t *bounds,
                              void *stream) {
    TsdfFrame f;
    if (!tsdf_frame(&f, depth, H, W, fx, fy, cx, cy, c2w_host, depth_scale, depth_trunc) || stride < 1 || !bounds) return MH_ERR_ARG;
    const int32_t ns_w = (W + stride - 1) / stride, ns_h = (H + stride - 1) / stride;
    const int64_t n = (int64_t)ns_w * ns_h;
    hipLaunchKernelGGL(tsdf_bounds_kernel, dim3((unsigned)((n + TSDF_THREADS - 1) / TSDF_THREADS)), dim3(TSDF_THREADS), 0,
                       mh_stream(stream), depth, mask, f, stride, ns_w, n, bounds);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_tsdf_touch(const float *depth, const uint8_t *mask, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                             const float *c2w_host, float depth_scale, float depth_trunc, int32_t stride, float ox, float oy,
                             float oz, float voxel_length, float sdf_trunc, int32_t nbx, int32_t nby, int32_t nbz, uint8_t *active,
                             void *stream) {
    TsdfFrame f;
    TsdfBox b;
    if (!tsdf_frame(&f, depth, H, W, fx, fy, cx, cy, c2w_host, depth_scale, depth_trunc) || stride < 1 || !active ||
        !tsdf_box(&b, ox, oy, oz, voxel_length, sdf_trunc, nbx, nby, nbz))
        return MH_ERR_ARG;
    const int32_t ns_w = (W + stride - 1) / stride, ns_h = (H + stride - 1) / stride;
    const int64_t n = (int64_t)ns_w * ns_h;
    hipLaunchKernelGGL(tsdf_touch_kernel, dim3((unsigned)((n + TSDF_THREADS - 1) / TSDF_THREADS)), dim3(TSDF_THREADS), 0,
                       mh_stream(stream), depth, mask, f, b, stride, ns_w, n, active);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_tsdf_integrate(const float *depth, const uint8_t *rgb, const uint8_t *mask, int32_t H, int32_t W, float fx,
                                 float fy, float cx, float cy, const float *w2c_host, float depth_scale, float depth_trunc, float ox,
                                 float oy, float oz, float voxel_length, float sdf_trunc, int32_t nbx, int32_t nby, int32_t nbz,
                                 const uint8_t *active, float *tsdf, float *weight, float *color, void *stream) {
    TsdfFrame f;
    TsdfBox b;
    if (!tsdf_frame(&f, depth, H, W, fx, fy, cx, cy, w2c_host, depth_scale, depth_trunc) || !rgb || !active || !tsdf || !weight ||
        !color || !tsdf_box(&b, ox, oy, oz, voxel_length, sdf_trunc, nbx, nby, nbz))
        return MH_ERR_ARG;
    const int32_t groups_z = (nbz + TSDF_GROUP - 1) / TSDF_GROUP;
    const int64_t groups = (int64_t)nbx * nby * groups_z;       // < 2^22 by tsdf_box
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)groups), dim3(TSDF_THREADS), 0, mh_stream(stream), depth, rgb, mask, f,
                       b, groups_z, active, tsdf, weight, color);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_tsdf_vertex_colors(const float *vertices, int64_t V, const float *color, int32_t nx, int32_t ny, int32_t nz,
                                     float *out, void *stream) {
    if (V < 0 || V >= ((int64_t)1 << 31) || nx < 1 || ny < 1 || nz < 1 || (int64_t)nx * ny * nz >= ((int64_t)1 << 31)) return MH_ERR_ARG;
    if (V == 0) return MH_OK;
    if (!vertices || !color || !out) return MH_ERR_ARG;
    hipLaunchKernelGGL(tsdf_vertex_colors_kernel, dim3((unsigned)((V + TSDF_THREADS - 1) / TSDF_THREADS)), dim3(TSDF_THREADS), 0,
                       mh_stream(stream), vertices, V, color, nx, ny, nz, out);
    MH_CHECK_LAUNCH();
    return MH_OK;
}
