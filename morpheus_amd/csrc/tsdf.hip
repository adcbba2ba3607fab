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
#include "tsdf_common.h"
#include "wave.h"

#define TSDF_GROUP 4                                    // blocks per workgroup along z: 32 voxels = one 128-byte line

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
        lo[a] = wave_min(lo[a]);
        hi[a] = wave_max(hi[a]);
    }
    if (mh_lane() == 0 && lo[0] != INT32_MAX) {                // a wave with a usable pixel has all six
#pragma unroll
        for (int a = 0; a < 3; a++) {
            atomicMin(bounds + a, lo[a]);
            atomicMax(bounds + 3 + a, hi[a]);
        }
    }
}

__global__ __launch_bounds__(TSDF_THREADS) void tsdf_touch_kernel(const float *__restrict__ depth, const uint8_t *__restrict__ mask,
                                                                  TsdfFrame f, TsdfBox b, int32_t stride, int32_t ns_w,
                                                                  int64_t n_samples, uint8_t *__restrict__ active) {
    const int64_t s = (int64_t)blockIdx.x * TSDF_THREADS + threadIdx.x;
    if (s >= n_samples) return;
    int lo[3], hi[3];
    if (!tsdf_touch_range(depth, mask, f, b, stride, ns_w, s, lo, hi)) return;
    for (int x = lo[0]; x <= hi[0]; x++)
        for (int y = lo[1]; y <= hi[1]; y++)
            for (int z = lo[2]; z <= hi[2]; z++) active[((int64_t)x * b.nby + y) * b.nbz + z] = 1;
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
        const int64_t p = ((int64_t)i * ny + j) * nz + k;
        tsdf_update_voxel(depth, rgb, mask, f, b.sdf_trunc, px, py, pz, tsdf + p, weight + p, color + p, color + plane + p,
                          color + 2 * plane + p);
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

// the touch pass over the sparse store's logical box (more voxels than mh_tsdf_touch takes): the same kernel, one byte per block
extern "C" int mh_tsdf_sparse_mark(const float *depth, const uint8_t *mask, int32_t H, int32_t W, float fx, float fy, float cx,
                                   float cy, const float *c2w_host, float depth_scale, float depth_trunc, int32_t stride, float ox,
                                   float oy, float oz, float voxel_length, float sdf_trunc, int32_t nbx, int32_t nby, int32_t nbz,
                                   uint8_t *active, void *stream) {
    TsdfFrame f;
    TsdfBox b;
    if (!tsdf_frame(&f, depth, H, W, fx, fy, cx, cy, c2w_host, depth_scale, depth_trunc) || stride < 1 || !active ||
        !tsdf_sparse_box(&b, ox, oy, oz, voxel_length, sdf_trunc, nbx, nby, nbz))
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
