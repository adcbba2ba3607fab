// Mesh evaluation: the device side of tools/culling.py of the reference (cull_from_one_pose, trimesh's sample_surface, the
// nearest-neighbour queries of accuracy / completion and of the ICP alignment).  Conventions, operator order and limits are in
// include/morpheus_hip.h (mh_nn_*, mh_cull_*, mh_mesh_area_weights, mh_sample_surface, mh_icp_*); tests/mesheval_oracle.py
// restates them in numpy.
//
// mh_nn_search, the hot path: exact brute force.
//   nn_init_kernel    keys = empty
//   nn_search_kernel  grid (query blocks, segments).  A lane owns one query; the workgroup streams its segment of the reference
//                     set through LDS in tiles of NN_TILE points (x, y, z planes, read back four points at a time as
//                     broadcasts), NaN-padded so the inner loop has no bounds test.  Each lane keeps its segment's best
//                     (d2, index) with a strict <, so the lowest index wins inside a segment; the segments meet in one 64-bit
//                     atomicMin per query on (bits(d2) << 32 | index), the depth-test idiom of raster.hip: d2 >= 0, so the key
//                     orders like (d2, index) and the result does not depend on the order of the segments.
//   nn_unpack_kernel  keys -> idx, d2
// Every loop is bounded by Nr, Nq, T or count.  No float atomics anywhere in this file.
#include "common.h"
#include "wave.h"

#pragma clang fp contract(off)

#define ME_THREADS 256
#define NN_TILE 1024                              // reference points per LDS tile: 3 planes x 4 KiB
#define NN_EMPTY 0x7f800000ffffffffull            // (bits(+inf) << 32) | 0xffffffff: unpacks to idx -1, d2 +inf
#define NN_MAX_SEGMENTS 4096
#define ICP_BLOCKS 512
#define ICP_SUMS 17

static inline bool me_count_valid(int64_t n) { return n >= 0 && n < ((int64_t)1 << 31); }

static inline unsigned me_blocks(int64_t n) { return (unsigned)((n + ME_THREADS - 1) / ME_THREADS); }

// ---- nearest neighbour ---------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(ME_THREADS) void nn_init_kernel(unsigned long long *__restrict__ keys, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = NN_EMPTY;
}

__global__ __launch_bounds__(ME_THREADS) void nn_search_kernel(const float *__restrict__ query, int64_t Nq,
                                                               const float *__restrict__ ref, int64_t Nr, int64_t seg_len,
                                                               float max_d2, unsigned long long *__restrict__ keys) {
    __shared__ __attribute__((aligned(16))) float tile[3][NN_TILE];
    const int64_t q = (int64_t)blockIdx.x * ME_THREADS + threadIdx.x;
    const bool live = q < Nq;
    float qx = NAN, qy = NAN, qz = NAN;            // a lane without a query computes NaN distances, which never win
    if (live) qx = query[3 * q], qy = query[3 * q + 1], qz = query[3 * q + 2];
    const int64_t seg0 = (int64_t)blockIdx.y * seg_len;
    const int64_t seg1 = seg0 + seg_len < Nr ? seg0 + seg_len : Nr;
    float best = INFINITY;
    int32_t bi = -1;
    for (int64_t base = seg0; base < seg1; base += NN_TILE) {
        const int32_t n = (int32_t)(seg1 - base < NN_TILE ? seg1 - base : NN_TILE);
        __syncthreads();                           // the previous tile has been read by every lane
        for (int32_t k = threadIdx.x; k < 3 * NN_TILE; k += ME_THREADS) {
            const int32_t p = k / 3, a = k - 3 * p;
            tile[a][p] = p < n ? ref[3 * base + k] : NAN;      // k < 3 n: inside ref's rows [base, seg1)
        }
        __syncthreads();
        const int32_t n4 = (n + 3) & ~3;           // <= NN_TILE; the padding is NaN
        const int32_t b32 = (int32_t)base;         // Nr < 2^31
        for (int32_t j = 0; j < n4; j += 4) {
            const f32x4 X = *reinterpret_cast<const f32x4 *>(&tile[0][j]);
            const f32x4 Y = *reinterpret_cast<const f32x4 *>(&tile[1][j]);
            const f32x4 Z = *reinterpret_cast<const f32x4 *>(&tile[2][j]);
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const float dx = qx - X[u], dy = qy - Y[u], dz = qz - Z[u];
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < best) {                   // strict: ties stay with the lower index; NaN and +inf never enter
                    best = d2;
                    bi = b32 + j + u;
                }
            }
        }
    }
    if (live && bi >= 0 && best <= max_d2) {
        const unsigned long long key = ((unsigned long long)__float_as_uint(best) << 32) | (unsigned long long)(uint32_t)bi;
        atomicMin(keys + q, key);
    }
}

__global__ __launch_bounds__(ME_THREADS) void nn_unpack_kernel(const unsigned long long *__restrict__ keys, int64_t n,
                                                               int32_t *__restrict__ idx, float *__restrict__ d2) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = keys[i];
    idx[i] = (int32_t)(uint32_t)(key & 0xffffffffull);
    d2[i] = __uint_as_float((uint32_t)(key >> 32));
}

extern "C" int64_t mh_nn_workspace_bytes(int64_t Nq) { return me_count_valid(Nq) ? Nq * 8 : -1; }

extern "C" int32_t mh_nn_tile_points(void) { return NN_TILE; }

static inline int64_t nn_default_segments(int64_t Nq, int64_t Nr) {
    // enough workgroups for ~8 per CU, never a segment shorter than one tile
    const int64_t qblocks = (Nq + ME_THREADS - 1) / ME_THREADS;
    const int64_t want = (8 * (int64_t)mh_cu_count() + qblocks - 1) / qblocks;
    const int64_t tiles = (Nr + NN_TILE - 1) / NN_TILE;
    return want < tiles ? want : tiles;
}

extern "C" int mh_nn_search(const float *query, int64_t Nq, const float *ref, int64_t Nr, float max_d2, int32_t segments,
                            void *workspace, int32_t *idx, float *d2, void *stream) {
    if (!me_count_valid(Nq) || !me_count_valid(Nr) || !(max_d2 >= 0.0f) || segments > NN_MAX_SEGMENTS) return MH_ERR_ARG;
    if (Nq == 0) return MH_OK;
    if (!query || !workspace || !idx || !d2 || (Nr > 0 && !ref)) return MH_ERR_ARG;
    hipStream_t s = mh_stream(stream);
    unsigned long long *keys = static_cast<unsigned long long *>(workspace);
    hipLaunchKernelGGL(nn_init_kernel, dim3(me_blocks(Nq)), dim3(ME_THREADS), 0, s, keys, Nq);
    MH_CHECK_LAUNCH();
    if (Nr > 0) {
        int64_t nseg = segments > 0 ? segments : nn_default_segments(Nq, Nr);
        if (nseg > NN_MAX_SEGMENTS) nseg = NN_MAX_SEGMENTS;
        if (nseg > Nr) nseg = Nr;
        if (nseg < 1) nseg = 1;
        const int64_t seg_len = (Nr + nseg - 1) / nseg;
        nseg = (Nr + seg_len - 1) / seg_len;       // no empty segment
        hipLaunchKernelGGL(nn_search_kernel, dim3(me_blocks(Nq), (unsigned)nseg), dim3(ME_THREADS), 0, s, query, Nq, ref, Nr,
                           seg_len, max_d2, keys);
        MH_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(nn_unpack_kernel, dim3(me_blocks(Nq)), dim3(ME_THREADS), 0, s, keys, Nq, idx, d2);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

// ---- culling -------------------------------------------------------------------------------------------------------------

struct CullCam {
    double w[12];                                  // world -> OpenCV camera, row-major [3][4]
    double K[9];
    int32_t H, W;
    float eps;
};

__global__ __launch_bounds__(ME_THREADS) void cull_vertex_kernel(CullCam cam, const float *__restrict__ vertices, int64_t V,
                                                                 const float *__restrict__ rendered_depth,
                                                                 const float *__restrict__ depth_gt,
                                                                 uint8_t *__restrict__ frustum, uint8_t *__restrict__ observed,
                                                                 uint8_t *__restrict__ invalid) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    const double x = vertices[3 * i], y = vertices[3 * i + 1], z = vertices[3 * i + 2];
    double c[3], uvz[3];
#pragma unroll
    for (int r = 0; r < 3; r++) c[r] = ((cam.w[4 * r] * x + cam.w[4 * r + 1] * y) + cam.w[4 * r + 2] * z) + cam.w[4 * r + 3];
#pragma unroll
    for (int r = 0; r < 3; r++) uvz[r] = (cam.K[3 * r] * c[0] + cam.K[3 * r + 1] * c[1]) + cam.K[3 * r + 2] * c[2];
    const double pz = uvz[2] + 1e-8;
    const double px = uvz[0] / pz, py = uvz[1] / pz;
    // every comparison is false for a NaN: such a vertex is outside the frustum and indexes nothing
    const bool in = 0.0 <= px && px <= (double)(cam.W - 1) && 0.0 <= py && py <= (double)(cam.H - 1) && pz > 0.0;
    bool obs = false, inv = false;
    if (in) {
        const int64_t pix = (int64_t)(int32_t)py * cam.W + (int32_t)px;       // truncation; 0 <= . <= H-1, W-1
        obs = pz < (double)(rendered_depth[pix] + cam.eps);                   // the sum in fp32, the comparison in fp64
        inv = depth_gt != nullptr && depth_gt[pix] <= 0.0f;
    }
    frustum[i] = in, observed[i] = obs, invalid[i] = inv;
}

__global__ __launch_bounds__(ME_THREADS) void cull_triangle_kernel(const int32_t *__restrict__ triangles, int64_t T, int64_t V,
                                                                   const uint8_t *__restrict__ observed,
                                                                   const uint8_t *__restrict__ invalid,
                                                                   uint8_t *__restrict__ keep) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    bool any_obs = false, all_inv = true, ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int32_t v = triangles[3 * t + k];
        if (v < 0 || v >= V) {
            ok = false;
        } else {
            any_obs = any_obs || observed[v];
            all_inv = all_inv && invalid[v];
        }
    }
    keep[t] = ok && any_obs && !all_inv;
}

extern "C" int mh_cull_vertices(const float *vertices, int64_t V, const double *w2c_host, const double *K_host, int32_t H,
                                int32_t W, const float *rendered_depth, const float *depth_gt, float eps, uint8_t *frustum,
                                uint8_t *observed, uint8_t *invalid, void *stream) {
    if (!me_count_valid(V) || H < 1 || W < 1 || H > 16384 || W > 16384 || !w2c_host || !K_host || !(eps == eps)) return MH_ERR_ARG;
    if (V == 0) return MH_OK;
    if (!vertices || !rendered_depth || !frustum || !observed || !invalid) return MH_ERR_ARG;
    CullCam cam;
    for (int k = 0; k < 12; k++) cam.w[k] = w2c_host[k];
    for (int k = 0; k < 9; k++) cam.K[k] = K_host[k];
    cam.H = H, cam.W = W, cam.eps = eps;
    hipLaunchKernelGGL(cull_vertex_kernel, dim3(me_blocks(V)), dim3(ME_THREADS), 0, mh_stream(stream), cam, vertices, V,
                       rendered_depth, depth_gt, frustum, observed, invalid);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_cull_triangles(const int32_t *triangles, int64_t T, int64_t V, const uint8_t *observed,
                                 const uint8_t *invalid, uint8_t *keep, void *stream) {
    if (!me_count_valid(T) || !me_count_valid(V)) return MH_ERR_ARG;
    if (T == 0) return MH_OK;
    if (!triangles || !keep || (V > 0 && (!observed || !invalid))) return MH_ERR_ARG;
    hipLaunchKernelGGL(cull_triangle_kernel, dim3(me_blocks(T)), dim3(ME_THREADS), 0, mh_stream(stream), triangles, T, V,
                       observed, invalid, keep);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

// ---- surface sampling ----------------------------------------------------------------------------------------------------

// |(b-a) x (c-a)| / 2 in fp32; 0 for an index outside [0, V) or an area that is not finite
__device__ __forceinline__ float ss_area(const float *__restrict__ vertices, int64_t V, const int32_t *__restrict__ triangles,
                                         int64_t t) {
    int32_t idx[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        idx[k] = triangles[3 * t + k];
        if (idx[k] < 0 || idx[k] >= V) return 0.0f;
    }
    const float *a = vertices + 3 * (int64_t)idx[0], *b = vertices + 3 * (int64_t)idx[1], *c = vertices + 3 * (int64_t)idx[2];
    const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const float e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const float nx = e1[1] * e2[2] - e1[2] * e2[1];
    const float ny = e1[2] * e2[0] - e1[0] * e2[2];
    const float nz = e1[0] * e2[1] - e1[1] * e2[0];
    const float area = sqrtf((nx * nx + ny * ny) + nz * nz) * 0.5f;
    return area < INFINITY ? area : 0.0f;          // NaN and +inf -> 0
}

__global__ __launch_bounds__(ME_THREADS) void ss_area_kernel(const float *__restrict__ vertices, int64_t V,
                                                             const int32_t *__restrict__ triangles, int64_t T,
                                                             float *__restrict__ areas, uint32_t *__restrict__ gmax_bits) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float a = 0.0f;
    if (t < T) {
        a = ss_area(vertices, V, triangles, t);
        areas[t] = a;
    }
    uint32_t m = __float_as_uint(a);               // bits of a float >= 0 order like it
    m = wave_max(m);
    if (mh_lane() == 0 && m) atomicMax(gmax_bits, m);
}

__global__ __launch_bounds__(ME_THREADS) void ss_quantise_kernel(const float *__restrict__ areas, int64_t T,
                                                                 const uint32_t *__restrict__ gmax_bits,
                                                                 int64_t *__restrict__ qarea) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const int E = (int)(*gmax_bits >> 23);         // biased exponent of the maximum: G = 2^(E - 126)
    qarea[t] = (int64_t)llrint((double)areas[t] * ldexp(1.0, 166 - E));       // <= 2^40
}

__global__ __launch_bounds__(ME_THREADS) void ss_sample_kernel(const float *__restrict__ vertices, int64_t V,
                                                               const int32_t *__restrict__ triangles, int64_t T,
                                                               const int64_t *__restrict__ cum,
                                                               const float *__restrict__ uniforms, int64_t count,
                                                               float *__restrict__ points, int32_t *__restrict__ face) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const int64_t total = cum[T - 1];
    const float u0 = uniforms[3 * k];
    int64_t target = 0;
    if (u0 >= 1.0f) target = total - 1;
    else if (u0 >= 0.0f) target = (int64_t)((double)u0 * (double)total);
    if (target > total - 1) target = total - 1;
    int64_t lo = 0, hi = T - 1;                    // the first face whose cumulative value exceeds target; <= 32 rounds
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (cum[mid] > target) hi = mid;
        else lo = mid + 1;
    }
    face[k] = (int32_t)lo;
    float p[3] = {NAN, NAN, NAN};
    int32_t idx[3];
    bool ok = total > 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        idx[a] = triangles[3 * lo + a];
        ok = ok && idx[a] >= 0 && idx[a] < V;
    }
    if (ok) {
        float r1 = uniforms[3 * k + 1], r2 = uniforms[3 * k + 2];
        if (r1 + r2 > 1.0f) r1 = 1.0f - r1, r2 = 1.0f - r2;
        const float *v0 = vertices + 3 * (int64_t)idx[0], *v1 = vertices + 3 * (int64_t)idx[1], *v2 = vertices + 3 * (int64_t)idx[2];
#pragma unroll
        for (int a = 0; a < 3; a++) p[a] = (v0[a] + r1 * (v1[a] - v0[a])) + r2 * (v2[a] - v0[a]);
    }
    points[3 * k] = p[0], points[3 * k + 1] = p[1], points[3 * k + 2] = p[2];
}

extern "C" int mh_mesh_area_weights(const float *vertices, int64_t V, const int32_t *triangles, int64_t T, float *areas,
                                    int64_t *qarea, void *stream) {
    if (!me_count_valid(V) || !me_count_valid(T)) return MH_ERR_ARG;
    if (T == 0) return MH_OK;
    if (!qarea || !triangles || !areas || (V > 0 && !vertices)) return MH_ERR_ARG;
    hipStream_t s = mh_stream(stream);
    if (!mh_zero_async(qarea + T, 8, s)) return MH_ERR_LAUNCH;
    uint32_t *gmax = reinterpret_cast<uint32_t *>(qarea + T);
    hipLaunchKernelGGL(ss_area_kernel, dim3(me_blocks(T)), dim3(ME_THREADS), 0, s, vertices, V, triangles, T, areas, gmax);
    MH_CHECK_LAUNCH();
    hipLaunchKernelGGL(ss_quantise_kernel, dim3(me_blocks(T)), dim3(ME_THREADS), 0, s, areas, T, gmax, qarea);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_sample_surface(const float *vertices, int64_t V, const int32_t *triangles, int64_t T, const int64_t *cum,
                                 const float *uniforms, int64_t count, float *points, int32_t *face, void *stream) {
    if (!me_count_valid(V) || !me_count_valid(T) || !me_count_valid(count)) return MH_ERR_ARG;
    if (count == 0) return MH_OK;
    if (T == 0 || V == 0 || !vertices || !triangles || !cum || !uniforms || !points || !face) return MH_ERR_ARG;
    hipLaunchKernelGGL(ss_sample_kernel, dim3(me_blocks(count)), dim3(ME_THREADS), 0, mh_stream(stream), vertices, V, triangles,
                       T, cum, uniforms, count, points, face);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

// ---- rigid alignment -----------------------------------------------------------------------------------------------------

struct IcpPose {
    double m[12];                                  // row-major [3][4]
};

__global__ __launch_bounds__(ME_THREADS) void icp_transform_kernel(IcpPose T, const float *__restrict__ src, int64_t N,
                                                                   float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
#pragma unroll
    for (int r = 0; r < 3; r++)
        out[3 * i + r] = (float)(((T.m[4 * r] * x + T.m[4 * r + 1] * y) + T.m[4 * r + 2] * z) + T.m[4 * r + 3]);
}

// partials [gridDim.x][17]: n, sum d2, sum p (3), sum q (3), sum p q^T (9, row-major: p_a q_b at 3a + b).  A lane adds its
// points i = first, first + stride, ... in that order; lanes meet in the butterfly, the four waves in wave order.
__global__ __launch_bounds__(ME_THREADS) void icp_partial_kernel(const float *__restrict__ p, int64_t N,
                                                                 const float *__restrict__ target, int64_t Nt,
                                                                 const int32_t *__restrict__ idx, const float *__restrict__ d2,
                                                                 double *__restrict__ partials) {
    __shared__ double wave_sums[ME_THREADS / MH_WAVE][ICP_SUMS];
    double s[ICP_SUMS];
#pragma unroll
    for (int k = 0; k < ICP_SUMS; k++) s[k] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * ME_THREADS + threadIdx.x; i < N; i += (int64_t)gridDim.x * ME_THREADS) {
        const int32_t j = idx[i];
        if (j < 0 || j >= Nt) continue;
        const double pv[3] = {p[3 * i], p[3 * i + 1], p[3 * i + 2]};
        const double qv[3] = {target[3 * (int64_t)j], target[3 * (int64_t)j + 1], target[3 * (int64_t)j + 2]};
        s[0] += 1.0;
        s[1] += (double)d2[i];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            s[2 + a] += pv[a];
            s[5 + a] += qv[a];
#pragma unroll
            for (int b = 0; b < 3; b++) s[8 + 3 * a + b] += pv[a] * qv[b];
        }
    }
#pragma unroll
    for (int k = 0; k < ICP_SUMS; k++) {
        const double w = wave_sum(s[k]);
        if (mh_lane() == 0) wave_sums[threadIdx.x >> 6][k] = w;
    }
    __syncthreads();
    if (threadIdx.x < ICP_SUMS) {
        double v = wave_sums[0][threadIdx.x];
        for (int w = 1; w < ME_THREADS / MH_WAVE; w++) v += wave_sums[w][threadIdx.x];
        partials[(int64_t)blockIdx.x * ICP_SUMS + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(MH_WAVE) void icp_final_kernel(const double *__restrict__ partials, int32_t blocks,
                                                            double *__restrict__ sums) {
    if (threadIdx.x >= ICP_SUMS) return;
    double v = 0.0;
    for (int32_t b = 0; b < blocks; b++) v += partials[(int64_t)b * ICP_SUMS + threadIdx.x];      // index order
    sums[threadIdx.x] = v;
}

extern "C" int64_t mh_icp_workspace_bytes(void) { return (int64_t)ICP_BLOCKS * ICP_SUMS * 8; }

extern "C" int mh_icp_transform(const float *src, int64_t N, const double *T_host, float *out, void *stream) {
    if (!me_count_valid(N) || !T_host) return MH_ERR_ARG;
    if (N == 0) return MH_OK;
    if (!src || !out) return MH_ERR_ARG;
    IcpPose T;
    for (int k = 0; k < 12; k++) T.m[k] = T_host[k];
    hipLaunchKernelGGL(icp_transform_kernel, dim3(me_blocks(N)), dim3(ME_THREADS), 0, mh_stream(stream), T, src, N, out);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_icp_sums(const float *p, int64_t N, const float *target, int64_t Nt, const int32_t *idx, const float *d2,
                           void *workspace, double *sums, void *stream) {
    if (!me_count_valid(N) || !me_count_valid(Nt)) return MH_ERR_ARG;
    if (N == 0) return MH_OK;
    if (!sums || !p || !idx || !d2 || !workspace || (Nt > 0 && !target)) return MH_ERR_ARG;
    hipStream_t s = mh_stream(stream);
    const int32_t blocks = (int32_t)(me_blocks(N) < ICP_BLOCKS ? me_blocks(N) : ICP_BLOCKS);
    hipLaunchKernelGGL(icp_partial_kernel, dim3((unsigned)blocks), dim3(ME_THREADS), 0, s, p, N, target, Nt, idx, d2,
                       static_cast<double *>(workspace));
    MH_CHECK_LAUNCH();
    hipLaunchKernelGGL(icp_final_kernel, dim3(1), dim3(MH_WAVE), 0, s, static_cast<const double *>(workspace), blocks, sums);
    MH_CHECK_LAUNCH();
    return MH_OK;
}
