// Importance resampling: inverse-CDF draws from per-interval weights.
//
//   mh_sample_pdf       the reference's utils.sample_pdf (utils.py:10-44) in its dense layout: bins [B,T], weights [B,T-1], u [B,n]
//   mh_resample_packed  the same draw on packed ragged samples, the coarse intervals cut at the drawn points (c + n intervals)
//   mh_resample_ranges  the new (ray_start, ray_cnt) and their total, on the device
//
// One wavefront per ray (wave_ray()).  The definition, statement by statement (utils.py:17-42), each statement one rounded fp32
// operation unless said otherwise:
//   w'_i  = w_i + eps                                      (eps = 1e-5 in the reference)
//   pdf_i = w'_i / sum(w')                                 the sum is taken in float64 and rounded to fp32 once
//   cdf_0 = 0, cdf_{i+1} = pdf_0 + ... + pdf_i             summed in float64, rounded to fp32 once, then a running maximum
//   inds  = #{ j : cdf_j <= u }                            searchsorted(right=True)
//   below = max(inds - 1, 0), above = min(inds, T - 1)
//   denom = cdf_above - cdf_below, 1 where it is < 1e-5;   t = (u - cdf_below) / denom
//   s     = b_below + t * (b_above - b_below),             then held inside [b_below, b_above]
// The hold is the one statement the reference does not have: its s can leave its own bin by an ulp of rounding (t = 1 and a
// rounded b_above - b_below); a sample inside its bin is what the packed form needs for its order, and both forms share the
// function.
//
// How the searched CDF is non-decreasing.  A Hillis-Steele scan with a carry across 64-wide chunks gives lane i and lane i + 1
// sums of different association, and in fp32 the later one can come out an ulp below the earlier.  Here the sums are float64
// (terms are fp32 values in [0, 1], at most a few thousand of them: every partial sum is exact to 2^-53 relative, far below
// the fp32 rounding that follows, so the stored value is the correctly rounded prefix sum in all but freak cases), and what
// GUARANTEES the order is the running maximum behind it (wave_incl_max and the chunk's carry): max is exact, so
// cdf_{i+1} >= cdf_i whatever the terms were, NaN terms included (fmaxf drops them).
//
// Draw order (packed form).  u_k = ((float)k + j_k) / (float)n with j_k in [0,1): k + j_k < k + 1 <= k' + j_k' for k < k', and
// rounding, the division by n > 0, the search in a non-decreasing CDF, t and s are all monotone in u, so draws inside one
// interval are non-decreasing in k; the hold to [ts_i, te_i] and te_i <= ts_{i+1} carry that across intervals.  The cut is
// therefore a merge by rank: draw k in interval i ends output interval i + k and starts output interval i + k + 1; coarse
// interval i starts output interval i + lo_i and ends i + lo_i + m_i, lo_i the number of draws in intervals before i and m_i
// in i (an LDS histogram and its scan).  A cut point is ONE value stored twice, so shared edges agree bit for bit, and every
// coarse ts / te is copied unchanged.  u at or above the last CDF value has below = T - 1 = above: it takes the last edge.
//
// Staging.  The CDF (c + 1 floats) and the histogram (c ints) of a ray live in LDS when c <= RS_STAGE = 384 intervals:
// mh_march_cap(0.01, 1.0) = 350 and mh_march_cap(0.01, 1.01) = 353 are the longest rays the shipped step and boxes march, so
// every ray of a default render is staged in LDS (4 waves x 3 076 B = 12.3 KB a block).  A longer ray uses the caller's
// global scratch at the ray's own packed offset (cdf: ray_start[r] + r, histogram: ray_start[r]) -- same code, other pointer.
#include "common.h"

// No FMA contraction: the statements above are separate IEEE round-to-nearest operations (tests/resample_oracle.py).
#pragma clang fp contract(off)

#include "wave.h"

#define RS_STAGE 384
constexpr float RS_DENOM_MIN = 1e-5f;

// what lane A stored to the staging is read by lane B of the same wavefront: a workgroup fence for LDS, a device fence for the
// global scratch of a long ray
template <bool GLOBAL>
__device__ __forceinline__ void stage_fence() {
    if (GLOBAL)
        __threadfence();
    else
        __threadfence_block();
}

// cdf[0 .. c] of the c weights w[0 .. c) (the header's statements); reached by all 64 lanes
__device__ __forceinline__ void build_cdf(const float *__restrict__ w, int c, float eps, float *cdf, int lane) {
    double part = 0.0;
    for (int i = lane; i < c; i += 64) part += (double)(w[i] + eps);
    const float total = (float)wave_sum(part);
    if (lane == 0) cdf[0] = 0.f;
    double carry = 0.0;
    float top = 0.f;
    for (int i0 = 0; i0 < c; i0 += 64) {
        const int i = i0 + lane;
        const float pdf = i < c ? (w[i] + eps) / total : 0.f;
        const double incl = carry + wave_incl_scan((double)pdf, lane);
        const float v = fmaxf(wave_incl_max((float)incl, lane), top);
        if (i < c) cdf[i + 1] = v;
        carry = __shfl(incl, 63);
        top = __shfl(v, 63);
    }
}

// The inverse-CDF step, once, for both entry points.  cdf[0 .. T), T >= 2; `edges` names the two ends of the bin:
// lo(below), hi(below, above).  -> the sample; *below_out = below.  Never reads outside cdf[0 .. T) or the edges' own arrays,
// whatever u is (a NaN u compares false everywhere: inds = 0).
template <class Edges>
__device__ __forceinline__ float inverse_cdf(const float *cdf, int T, float u, const Edges &edges, int *below_out) {
    int lo = 0, hi = T;                      // inds = #{ j : cdf[j] <= u } lies in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] <= u)
            lo = mid + 1;
        else
            hi = mid;
    }
    const int below = max(lo - 1, 0), above = min(lo, T - 1);
    const float cb = cdf[below];
    float denom = cdf[above] - cb;
    if (denom < RS_DENOM_MIN) denom = 1.0f;
    const float t = (u - cb) / denom;
    const float b0 = edges.lo(below), b1 = edges.hi(below, above);
    const float s = b0 + t * (b1 - b0);
    *below_out = below;
    return fminf(fmaxf(s, fminf(b0, b1)), fmaxf(b0, b1));
}

// dense layout: T bin edges
struct DenseEdges {
    const float *bins;
    __device__ __forceinline__ float lo(int below) const { return bins[below]; }
    __device__ __forceinline__ float hi(int, int above) const { return bins[above]; }
};
// packed layout: c intervals [ts_i, te_i]; edge i < c is ts_i seen from below and te_{i-1} seen from above (they differ across a
// gap, which so carries no probability), edge c is te_{c-1}.  On a contiguous ray these are DenseEdges' values.
struct PackedEdges {
    const float *ts, *te;
    int c;
    __device__ __forceinline__ float lo(int below) const { return below < c ? ts[below] : te[c - 1]; }
    __device__ __forceinline__ float hi(int below, int above) const { return above == below ? lo(below) : te[below]; }
};

template <bool GLOBAL>
__device__ __forceinline__ void sample_pdf_row(float *cdf, const float *__restrict__ bins, const float *__restrict__ w,
                                               const float *__restrict__ u, int T, int n, float *__restrict__ out, int lane) {
    build_cdf(w, T - 1, 1e-5f, cdf, lane);
    stage_fence<GLOBAL>();
    const DenseEdges e{bins};
    for (int k = lane; k < n; k += 64) {
        int below;
        out[k] = inverse_cdf(cdf, T, u[k], e, &below);
    }
}

__global__ __launch_bounds__(256) void sample_pdf_kernel(const float *__restrict__ bins, const float *__restrict__ weights,
                                                         const float *__restrict__ u, int B, int T, int n,
                                                         float *__restrict__ scratch, float *__restrict__ samples) {
    __shared__ float s_cdf[4][RS_STAGE + 1];
    const int lane = threadIdx.x & 63;
    const int b = wave_ray();
    if (b >= B) return;
    const float *row_b = bins + (int64_t)b * T, *row_w = weights + (int64_t)b * (T - 1), *row_u = u + (int64_t)b * n;
    float *row_s = samples + (int64_t)b * n;
    if (T - 1 <= RS_STAGE)
        sample_pdf_row<false>(s_cdf[threadIdx.x >> 6], row_b, row_w, row_u, T, n, row_s, lane);
    else
        sample_pdf_row<true>(scratch + (int64_t)b * T, row_b, row_w, row_u, T, n, row_s, lane);
}

// One ray of the packed form: c >= 1 coarse intervals at w / ts / te, n draws, c + n output intervals from position `ob` of the
// output arrays [M_out] (writes past M_out are suppressed).
template <bool GLOBAL>
__device__ __forceinline__ void resample_ray(float *cdf, int *cnt, const float *__restrict__ w, const float *__restrict__ ts,
                                             const float *__restrict__ te, int c, int n, const float *__restrict__ jit, float eps,
                                             int r, int64_t ob, int64_t M_out, int32_t *__restrict__ out_ri,
                                             float *__restrict__ out_ts, float *__restrict__ out_te, int lane) {
    build_cdf(w, c, eps, cdf, lane);
    for (int i = lane; i < c; i += 64) cnt[i] = 0;
    stage_fence<GLOBAL>();
    const PackedEdges e{ts, te, c};
    for (int k = lane; k < n; k += 64) {
        const float j = jit ? jit[k] : 0.5f;
        const float u = ((float)k + j) / (float)n;
        int below;
        const float s = inverse_cdf(cdf, c + 1, u, e, &below);      // inside [ts_i, te_i] by the function's hold
        const int i = min(below, c - 1);                             // u at or above the top: the last interval's end
        atomicAdd(&cnt[i], 1);
        const int64_t p = ob + i + k;
        if (p < M_out) out_te[p] = s;
        if (p + 1 < M_out) out_ts[p + 1] = s;
    }
    stage_fence<GLOBAL>();
    int carry = 0;
    for (int i0 = 0; i0 < c; i0 += 64) {
        const int i = i0 + lane;
        const int m = i < c ? cnt[i] : 0;
        const int incl = wave_incl_scan(m, lane);
        if (i < c) {
            const int64_t p = ob + i + (carry + incl - m);
            if (p < M_out) out_ts[p] = ts[i];
            if (p + m < M_out) out_te[p + m] = te[i];
        }
        carry += __shfl(incl, 63);
    }
    for (int p = lane; p < c + n; p += 64)
        if (ob + p < M_out) out_ri[ob + p] = r;
}

__global__ __launch_bounds__(256) void resample_packed_kernel(const float *__restrict__ weights, const float *__restrict__ t_starts,
                                                              const float *__restrict__ t_ends, const int32_t *__restrict__ ray_start,
                                                              const int32_t *__restrict__ ray_cnt, const int32_t *__restrict__ new_start,
                                                              int N, int64_t M, int n, const float *__restrict__ jitter, float eps,
                                                              float *__restrict__ scratch_cdf, int32_t *__restrict__ scratch_cnt,
                                                              int64_t M_out, int32_t *__restrict__ out_ri, float *__restrict__ out_ts,
                                                              float *__restrict__ out_te) {
    __shared__ float s_cdf[4][RS_STAGE + 1];
    __shared__ int s_cnt[4][RS_STAGE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r = wave_ray();
    if (r >= N) return;
    int64_t base;
    const int c = ray_range_clamped(ray_start, ray_cnt, r, M, &base);
    if (c <= 0) return;
    int64_t ob = new_start[r];
    if (ob < 0) ob = M_out;                   // never true for mh_resample_ranges' starts; nothing is written then
    const float *jit = jitter ? jitter + (int64_t)r * n : nullptr;
    if (c <= RS_STAGE)
        resample_ray<false>(s_cdf[wv], s_cnt[wv], weights + base, t_starts + base, t_ends + base, c, n, jit, eps, r, ob, M_out,
                            out_ri, out_ts, out_te, lane);
    else if (scratch_cdf && scratch_cnt)      // the host refuses M > RS_STAGE without scratch
        resample_ray<true>(scratch_cdf + base + r, scratch_cnt + base, weights + base, t_starts + base, t_ends + base, c, n, jit,
                           eps, r, ob, M_out, out_ri, out_ts, out_te, lane);
}

// new_cnt[r] = c_r + n for a ray with c_r >= 1 samples (its range clamped to [0, M) as the main kernel clamps it), else 0;
// new_start = the exclusive scan; *total = the sum.  Everything is held to `limit`, the output arrays' length, as
// ops.capped_ranges holds the marcher's: start <= limit, start + cnt <= limit.  One block.
__global__ __launch_bounds__(256) void resample_ranges_kernel(const int32_t *__restrict__ ray_start, const int32_t *__restrict__ ray_cnt,
                                                              int N, int64_t M, int n, int64_t limit, int32_t *__restrict__ new_start,
                                                              int32_t *__restrict__ new_cnt, int32_t *__restrict__ total) {
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int64_t carry = 0;
    for (int r0 = 0; r0 < N; r0 += 256) {
        const int r = r0 + (int)threadIdx.x;
        int m = 0;
        if (r < N) {
            int64_t s;
            const int c = ray_range_clamped(ray_start, ray_cnt, r, M, &s);
            m = c > 0 ? c + n : 0;
        }
        const int incl = wave_incl_scan(m, lane);
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        int64_t before = 0, all = 0;
        for (int w = 0; w < 4; w++) {
            if (w < wv) before += wsum[w];
            all += wsum[w];
        }
        if (r < N) {
            int64_t s = carry + before + (incl - m);
            if (s > limit) s = limit;
            new_start[r] = (int32_t)s;
            new_cnt[r] = (int32_t)(s + m > limit ? limit - s : m);
        }
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = (int32_t)(carry > limit ? limit : carry);
}

// midpoints' positions, the samplers' arithmetic: tm = (ts + te) / 2, x = o + d * tm
__global__ __launch_bounds__(256) void resample_xyz_kernel(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                           const int32_t *__restrict__ ri, const float *__restrict__ ts,
                                                           const float *__restrict__ te, int N, int64_t M_out,
                                                           float *__restrict__ xyz) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= M_out) return;
    const int r = min(max(ri[p], 0), N - 1);
    const float tm = (ts[p] + te[p]) / 2.0f;
#pragma unroll
    for (int a = 0; a < 3; a++) xyz[p * 3 + a] = rays_o[r * 3 + a] + rays_d[r * 3 + a] * tm;
}

extern "C" int32_t mh_resample_stage(void) { return RS_STAGE; }

extern "C" int mh_sample_pdf(const float *bins, const float *weights, const float *u, int32_t B, int32_t T, int32_t n,
                             float *scratch, float *samples, void *stream) {
    if (B == 0) return MH_OK;
    if (!bins || !weights || !u || !samples || B < 0 || T < 2 || n < 1) return MH_ERR_ARG;
    if (T - 1 > RS_STAGE && !scratch) return MH_ERR_ARG;
    hipLaunchKernelGGL(sample_pdf_kernel, dim3((B + 3) / 4), dim3(256), 0, mh_stream(stream), bins, weights, u, (int)B, (int)T,
                       (int)n, scratch, samples);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_resample_ranges(const int32_t *ray_start, const int32_t *ray_cnt, int32_t N, int64_t M, int32_t n, int64_t limit,
                                  int32_t *new_start, int32_t *new_cnt, int32_t *total, void *stream) {
    if (!total || N < 0 || M < 0 || n < 0 || limit < 0 || limit > 0x7fffffffLL) return MH_ERR_ARG;
    if (N > 0 && (!ray_start || !ray_cnt || !new_start || !new_cnt)) return MH_ERR_ARG;
    hipLaunchKernelGGL(resample_ranges_kernel, dim3(1), dim3(256), 0, mh_stream(stream), ray_start, ray_cnt, (int)N, M, (int)n,
                       limit, new_start, new_cnt, total);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_resample_packed(const float *weights, const float *t_starts, const float *t_ends, const int32_t *ray_start,
                                  const int32_t *ray_cnt, const int32_t *new_start, int32_t N, int64_t M, int32_t n,
                                  const float *jitter, float eps, float *scratch_cdf, int32_t *scratch_cnt, int64_t M_out,
                                  const float *rays_o, const float *rays_d, int32_t *out_ray_idx, float *out_t_starts,
                                  float *out_t_ends, float *xyz, void *stream) {
    if (N == 0 || M == 0 || M_out == 0) return MH_OK;
    if (!weights || !t_starts || !t_ends || !ray_start || !ray_cnt || !new_start || !out_ray_idx || !out_t_starts || !out_t_ends ||
        N < 0 || M < 0 || n < 1 || M_out < 0 || M_out > 0x7fffffffLL)
        return MH_ERR_ARG;
    if (M > RS_STAGE && (!scratch_cdf || !scratch_cnt)) return MH_ERR_ARG;
    if (xyz && (!rays_o || !rays_d)) return MH_ERR_ARG;
    hipLaunchKernelGGL(resample_packed_kernel, dim3((N + 3) / 4), dim3(256), 0, mh_stream(stream), weights, t_starts, t_ends,
                       ray_start, ray_cnt, new_start, (int)N, M, (int)n, jitter, eps, scratch_cdf, scratch_cnt, M_out, out_ray_idx,
                       out_t_starts, out_t_ends);
    MH_CHECK_LAUNCH();
    if (xyz) {
        hipLaunchKernelGGL(resample_xyz_kernel, dim3((unsigned)((M_out + 255) / 256)), dim3(256), 0, mh_stream(stream), rays_o,
                           rays_d, out_ray_idx, out_t_starts, out_t_ends, (int)N, M_out, xyz);
        MH_CHECK_LAUNCH();
    }
    return MH_OK;
}
