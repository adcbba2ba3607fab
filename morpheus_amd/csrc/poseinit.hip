// Pose initialisation: the device side of preprocess/pose_init/registrate.py of the reference (mask2camera, and the robust
// rigid registration it hands to an external program).  Conventions, operator order and limits are in include/morpheus_hip.h
// (mh_depth_points_*, mh_knn_*, mh_icp_wsums); tests/poseinit_oracle.py restates them in numpy.
//
//   mh_depth_points_count / _emit   count -> the caller's integer prefix sum -> emit, one workgroup per tile of DP_TILE pixels
//                                   in row-major order: a wavefront's ballot gives a kept pixel its rank, the four wavefronts
//                                   meet in LDS in wave order, so the points come out in pixel order.
//   mh_knn_d2                       exact brute force like mh_nn_search: a lane owns one point, the workgroup streams all points
//                                   through LDS in NaN-padded tiles, the lane keeps its 8 smallest d2 sorted in registers
//                                   (one comparison per candidate once the list is warm) and writes the first k.
//   mh_icp_wsums                    mh_icp_sums' reduction, term for term and in its order, with a Welsch weight per term.
// Every loop is bounded by H * W, N or the block count.  No float atomics anywhere in this file.
#include "common.h"
#include "wave.h"

#pragma clang fp contract(off)

#define PI_THREADS 256
#define DP_TILE PI_THREADS                        // pixels per workgroup of the back-projection: one per lane
#define KNN_TILE 1024                             // points per LDS tile: 3 planes x 4 KiB
#define KNN_MAX 8
#define WS_BLOCKS 512                             // mh_icp_sums' ICP_BLOCKS: the same partition of the points
#define WS_SUMS 19

static inline bool pi_count_valid(int64_t n) { return n >= 0 && n < ((int64_t)1 << 31); }

static inline unsigned pi_blocks(int64_t n) { return (unsigned)((n + PI_THREADS - 1) / PI_THREADS); }

// ---- masked back-projection ----------------------------------------------------------------------------------------------

__device__ __forceinline__ bool dp_kept(const float *__restrict__ depth, const uint8_t *__restrict__ mask, int32_t i, int32_t n) {
    return i < n && mask[i] != 0 && depth[i] > 0.0f;               // a NaN depth fails the comparison
}

__global__ __launch_bounds__(PI_THREADS) void dp_count_kernel(const float *__restrict__ depth, const uint8_t *__restrict__ mask,
                                                              int32_t n_pix, int64_t *__restrict__ counts) {
    __shared__ int32_t wave_count[PI_THREADS / MH_WAVE];
    const int32_t i = (int32_t)blockIdx.x * DP_TILE + (int32_t)threadIdx.x;       // n_pix <= 2^28
    const unsigned long long kept = __ballot(dp_kept(depth, mask, i, n_pix));
    if (mh_lane() == 0) wave_count[threadIdx.x >> 6] = __popcll(kept);
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t c = 0;
        for (int w = 0; w < PI_THREADS / MH_WAVE; w++) c += wave_count[w];
        counts[blockIdx.x] = c;
    }
}

struct DpCam {
    double fx, fy, cx, cy;
};

__global__ __launch_bounds__(PI_THREADS) void dp_emit_kernel(DpCam cam, const float *__restrict__ depth,
                                                             const uint8_t *__restrict__ mask, int32_t n_pix, int32_t W,
                                                             const int64_t *__restrict__ tile_start, int64_t n,
                                                             float *__restrict__ points, int32_t *__restrict__ pixel) {
    __shared__ int32_t wave_count[PI_THREADS / MH_WAVE];
    const int32_t i = (int32_t)blockIdx.x * DP_TILE + (int32_t)threadIdx.x;
    const bool keep = dp_kept(depth, mask, i, n_pix);
    const unsigned long long kept = __ballot(keep);
    const int wave = threadIdx.x >> 6;
    if (mh_lane() == 0) wave_count[wave] = __popcll(kept);
    __syncthreads();
    if (!keep) return;
    int64_t at = tile_start[blockIdx.x];
    for (int w = 0; w < wave; w++) at += wave_count[w];
    at += wave_rank(kept, mh_lane());                              // the kept lanes below this one
    if (at < 0 || at >= n) return;                                 // starts that are not this image's prefix sum write nothing outside
    const int32_t v = i / W, u = i - v * W;
    const float d = depth[i];
    points[3 * at] = (float)(((double)d * ((double)u - cam.cx)) / cam.fx);
    points[3 * at + 1] = (float)(((double)d * ((double)v - cam.cy)) / cam.fy);
    points[3 * at + 2] = d;
    if (pixel) pixel[at] = i;
}

static inline bool dp_image_valid(int32_t H, int32_t W) { return H >= 0 && W >= 0 && H <= 16384 && W <= 16384; }

extern "C" int32_t mh_depth_points_tile(void) { return DP_TILE; }

extern "C" int mh_depth_points_count(const float *depth, const uint8_t *mask, int32_t H, int32_t W, int64_t *counts, void *stream) {
    if (!dp_image_valid(H, W)) return MH_ERR_ARG;
    if (H == 0 || W == 0) return MH_OK;
    if (!depth || !mask || !counts) return MH_ERR_ARG;
    const int32_t n_pix = H * W;
    hipLaunchKernelGGL(dp_count_kernel, dim3(pi_blocks(n_pix)), dim3(PI_THREADS), 0, mh_stream(stream), depth, mask, n_pix, counts);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_depth_points_emit(const float *depth, const uint8_t *mask, int32_t H, int32_t W, double fx, double fy, double cx,
                                    double cy, const int64_t *tile_start, int64_t n, float *points, int32_t *pixel, void *stream) {
    if (!dp_image_valid(H, W) || !pi_count_valid(n) || n > (int64_t)H * W) return MH_ERR_ARG;
    if (!(fx != 0.0) || !(fy != 0.0) || fx != fx || fy != fy || cx != cx || cy != cy) return MH_ERR_ARG;
    if (H == 0 || W == 0 || n == 0) return MH_OK;
    if (!depth || !mask || !tile_start || !points) return MH_ERR_ARG;
    const int32_t n_pix = H * W;
    DpCam cam = {fx, fy, cx, cy};
    hipLaunchKernelGGL(dp_emit_kernel, dim3(pi_blocks(n_pix)), dim3(PI_THREADS), 0, mh_stream(stream), cam, depth, mask, n_pix, W,
                       tile_start, n, points, pixel);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

// ---- k nearest distances -------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(PI_THREADS) void knn_d2_kernel(const float *__restrict__ points, int64_t N, int32_t k,
                                                            float *__restrict__ out_d2) {
    __shared__ __attribute__((aligned(16))) float tile[3][KNN_TILE];
    const int64_t q = (int64_t)blockIdx.x * PI_THREADS + threadIdx.x;
    const bool live = q < N;
    float qx = NAN, qy = NAN, qz = NAN;            // a lane without a point computes NaN distances, which never enter
    if (live) qx = points[3 * q], qy = points[3 * q + 1], qz = points[3 * q + 2];
    const int32_t self = live ? (int32_t)q : -1;   // N < 2^31
    float best[KNN_MAX];                           // ascending
#pragma unroll
    for (int t = 0; t < KNN_MAX; t++) best[t] = INFINITY;
    for (int64_t base = 0; base < N; base += KNN_TILE) {
        const int32_t n = (int32_t)(N - base < KNN_TILE ? N - base : KNN_TILE);
        __syncthreads();                           // the previous tile has been read by every lane
        for (int32_t e = threadIdx.x; e < 3 * KNN_TILE; e += PI_THREADS) {
            const int32_t p = e / 3, a = e - 3 * p;
            tile[a][p] = p < n ? points[3 * base + e] : NAN;       // e < 3 n: inside the rows [base, N)
        }
        __syncthreads();
        const int32_t n4 = (n + 3) & ~3;           // <= KNN_TILE; the padding is NaN
        const int32_t b32 = (int32_t)base;
        for (int32_t j = 0; j < n4; j += 4) {
            const f32x4 X = *reinterpret_cast<const f32x4 *>(&tile[0][j]);
            const f32x4 Y = *reinterpret_cast<const f32x4 *>(&tile[1][j]);
            const f32x4 Z = *reinterpret_cast<const f32x4 *>(&tile[2][j]);
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const float dx = qx - X[u], dy = qy - Y[u], dz = qz - Z[u];
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < best[KNN_MAX - 1] && b32 + j + u != self) {       // NaN and +inf never enter; the point itself by index
                    best[KNN_MAX - 1] = d2;
#pragma unroll
                    for (int t = KNN_MAX - 1; t > 0; t--) {
                        const float lo = fminf(best[t - 1], best[t]), hi = fmaxf(best[t - 1], best[t]);   // neither is a NaN
                        best[t - 1] = lo, best[t] = hi;
                    }
                }
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int t = 0; t < KNN_MAX; t++)
        if (t < k) out_d2[q * k + t] = best[t];
}

extern "C" int32_t mh_knn_tile_points(void) { return KNN_TILE; }

extern "C" int mh_knn_d2(const float *points, int64_t N, int32_t k, float *out_d2, void *stream) {
    if (!pi_count_valid(N) || k < 1 || k > KNN_MAX) return MH_ERR_ARG;
    if (N == 0) return MH_OK;
    if (!points || !out_d2) return MH_ERR_ARG;
    hipLaunchKernelGGL(knn_d2_kernel, dim3(pi_blocks(N)), dim3(PI_THREADS), 0, mh_stream(stream), points, N, k, out_d2);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

// ---- Welsch-weighted sums ------------------------------------------------------------------------------------------------

// partials [gridDim.x][19].  The partition of the points over workgroups and lanes, the order of a lane's additions and the
// meeting of lanes, wavefronts and workgroups are mh_icp_sums' (csrc/mesheval.hip): with w = 1 the first 17 are its bytes.
__global__ __launch_bounds__(PI_THREADS) void ws_partial_kernel(const float *__restrict__ p, int64_t N,
                                                                const float *__restrict__ target, int64_t Nt,
                                                                const int32_t *__restrict__ idx, const float *__restrict__ d2,
                                                                double inv_2nu2, double *__restrict__ partials) {
    __shared__ double wave_sums[PI_THREADS / MH_WAVE][WS_SUMS];
    double s[WS_SUMS];
#pragma unroll
    for (int k = 0; k < WS_SUMS; k++) s[k] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * PI_THREADS + threadIdx.x; i < N; i += (int64_t)gridDim.x * PI_THREADS) {
        const int32_t j = idx[i];
        if (j < 0 || j >= Nt) continue;
        const double pv[3] = {p[3 * i], p[3 * i + 1], p[3 * i + 2]};
        const double qv[3] = {target[3 * (int64_t)j], target[3 * (int64_t)j + 1], target[3 * (int64_t)j + 2]};
        const double dd = (double)d2[i];
        const double w = exp(-dd * inv_2nu2);
        s[0] += w;
        s[1] += w * dd;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double wp = w * pv[a];
            s[2 + a] += wp;
            s[5 + a] += w * qv[a];
#pragma unroll
            for (int b = 0; b < 3; b++) s[8 + 3 * a + b] += wp * qv[b];
        }
        s[17] += 1.0 - w;
        s[18] += 1.0;
    }
#pragma unroll
    for (int k = 0; k < WS_SUMS; k++) {
        const double w = wave_sum(s[k]);
        if (mh_lane() == 0) wave_sums[threadIdx.x >> 6][k] = w;
    }
    __syncthreads();
    if (threadIdx.x < WS_SUMS) {
        double v = wave_sums[0][threadIdx.x];
        for (int w = 1; w < PI_THREADS / MH_WAVE; w++) v += wave_sums[w][threadIdx.x];
        partials[(int64_t)blockIdx.x * WS_SUMS + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(MH_WAVE) void ws_final_kernel(const double *__restrict__ partials, int32_t blocks,
                                                           double *__restrict__ sums) {
    if (threadIdx.x >= WS_SUMS) return;
    double v = 0.0;
    for (int32_t b = 0; b < blocks; b++) v += partials[(int64_t)b * WS_SUMS + threadIdx.x];       // index order
    sums[threadIdx.x] = v;
}

extern "C" int64_t mh_icp_wsums_workspace_bytes(void) { return (int64_t)WS_BLOCKS * WS_SUMS * 8; }

extern "C" int mh_icp_wsums(const float *p, int64_t N, const float *target, int64_t Nt, const int32_t *idx, const float *d2,
                            double inv_2nu2, void *workspace, double *sums, void *stream) {
    if (!pi_count_valid(N) || !pi_count_valid(Nt) || !(inv_2nu2 >= 0.0) || inv_2nu2 == (double)INFINITY) return MH_ERR_ARG;
    if (N == 0) return MH_OK;
    if (!sums || !p || !idx || !d2 || !workspace || (Nt > 0 && !target)) return MH_ERR_ARG;
    hipStream_t s = mh_stream(stream);
    const int32_t blocks = (int32_t)(pi_blocks(N) < WS_BLOCKS ? pi_blocks(N) : WS_BLOCKS);
    hipLaunchKernelGGL(ws_partial_kernel, dim3((unsigned)blocks), dim3(PI_THREADS), 0, s, p, N, target, Nt, idx, d2, inv_2nu2,
                       static_cast<double *>(workspace));
    MH_CHECK_LAUNCH();
    hipLaunchKernelGGL(ws_final_kernel, dim3(1), dim3(MH_WAVE), 0, s, static_cast<const double *>(workspace), blocks, sums);
    MH_CHECK_LAUNCH();
    return MH_OK;
}
