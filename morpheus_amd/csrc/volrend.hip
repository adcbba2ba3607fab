// nerfacc's volume-rendering functions as single launches: pack_info, transmittance / alpha / weights from densities or from
// alphas (forward + backward), accumulate_along_rays for any channel count (forward + backward).  morpheus_amd/volrend.py is the
// Python face; include/morpheus_hip.h states the definitions.
//
// The scans follow composite.hip: one wavefront per ray, four rays per 256-thread block, the ray's packed samples walked in chunks
// of 64, a 6-step wave scan plus a scalar carry -- no running value ever crosses a ray boundary, no atomics, so a ray's result does
// not depend on which rays lie beside it.  The scans are wave.h's, the density form's exclusive sum is the compositor's rule
// (wave_excl_from_incl): ordinary densities give the compositor's weights bit for bit.
//
// The alpha form's factors 1 - alpha and their running product are kept in DOUBLE.  1 - alpha is rounded in fp32 wherever alpha
// < 1/2, and a product of n fp32 factors carries n - 1 more roundings whatever the order of the multiplications, a wave scan as
// many as the sequential loop; the opaque sample behind a thin prefix takes the whole of that as the relative error of the ray's
// one heavy weight.  In double the factor is exact, the roundings are 2^-29 of an fp32 one and T is rounded once, when it is
// stored.  (12 more shuffles and 6 double multiplications per 64 samples, beside the memory traffic that bounds the kernel.)
//
// The reverse sums of the backward kernels are EXCLUSIVE as the inclusive value of the lane above (wave_excl_above), never
// `incl - v`: the alpha form divides the suffix by 1 - alpha_i, and a suffix that had the sample's own (1 / (1 - alpha_i) times
// larger) term added and taken away again keeps that term's rounding.
#include "common.h"
#include "wave.h"

namespace {

// reverse exclusive sum over the wave (the lanes above), and the wave's total in `total`
template <typename T>
__device__ __forceinline__ T vr_rev_excl_sum(T v, int lane, T &total) {
    const T rincl = wave_rev_incl_scan(v, lane);
    total = __shfl(rincl, 0);
    return wave_excl_above(rincl, lane);
}

// ------------------------------------------------------------------------------------------------------------ pack_info
// One thread per ray: the first packed position whose index is >= r and the first whose index is >= r + 1, by bisection of the
// non-decreasing index array.  A ray no sample names gets (position where it would stand, 0); indices outside [0, N) belong to no
// ray.  Every read is at a position in [0, M).
template <typename I>
__device__ __forceinline__ int64_t vr_lower_bound(const I *__restrict__ idx, int64_t M, int64_t r) {
    int64_t lo = 0, hi = M;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)idx[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <typename I>
__global__ __launch_bounds__(256) void pack_info_kernel(const I *__restrict__ idx, int64_t M, int N, int32_t *__restrict__ ray_start,
                                                        int32_t *__restrict__ ray_cnt) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    const int64_t a = vr_lower_bound(idx, M, (int64_t)r);
    const int64_t b = vr_lower_bound(idx, M, (int64_t)r + 1);
    ray_start[r] = (int32_t)a;
    ray_cnt[r] = (int32_t)(b - a);
}

// ------------------------------------------------------------------------------------------------- weights, forward
// density form: x = sigma (te - ts), alpha = -expm1f(-x), T = expf(-(exclusive sum of x))
// alpha form:   alpha = the value,   T = exclusive product of (1 - alpha)
template <bool ALPHA>
__global__ __launch_bounds__(256) void ray_weights_fwd_kernel(const float *__restrict__ val, const float *__restrict__ ts,
                                                              const float *__restrict__ te, const int32_t *__restrict__ ray_start,
                                                              const int32_t *__restrict__ ray_cnt, float *__restrict__ weights,
                                                              float *__restrict__ trans, float *__restrict__ alphas, int N) {
    const int lane = threadIdx.x & 63;
    const int ray = wave_ray();
    if (ray >= N) return;
    int64_t start;
    const int cnt = ray_range(ray_start, ray_cnt, ray, &start);
    float carry = 0.f;
    double carry_p = 1.0;
    for (int base = 0; base < cnt; base += 64) {
        const int k = base + lane;
        const bool on = k < cnt;
        const int64_t i = start + k;
        float T, alpha;
        if (ALPHA) {
            alpha = on ? val[i] : 0.f;
            const double incl = wave_incl_prod(1.0 - (double)alpha, lane);      // the factor itself is exact in double
            T = (float)(carry_p * wave_excl_below(incl, lane, 1.0));
            carry_p *= __shfl(incl, 63);
        } else {
            const float sd = on ? val[i] * (te[i] - ts[i]) : 0.f;
            const float incl = wave_incl_scan(sd, lane);
            T = expf(-(carry + wave_excl_from_incl(incl, sd, lane)));
            alpha = -expm1f(-sd);
            carry += __shfl(incl, 63);
        }
        if (on) {
            if (weights) weights[i] = T * alpha;
            if (trans) trans[i] = T;
            if (alphas) alphas[i] = alpha;
        }
    }
}

// ------------------------------------------------------------------------------------------------- weights, backward
// Density form, one reverse pass that reads the forward's saved transmittance:
//   dL/dx_i = (g_w_i T_i + g_a_i) (1 - alpha_i) - sum_{j>i} (g_w_j w_j + g_T_j T_j),   d_sigma_i = (te_i - ts_i) dL/dx_i
// with 1 - alpha_i = expf(-x_i) and w_j = T_j alpha_j as the forward formed it.
__global__ __launch_bounds__(256) void ray_weights_bwd_density_kernel(
    const float *__restrict__ sigma, const float *__restrict__ ts, const float *__restrict__ te, const int32_t *__restrict__ ray_start,
    const int32_t *__restrict__ ray_cnt, const float *__restrict__ trans, const float *__restrict__ g_w, const float *__restrict__ g_T,
    const float *__restrict__ g_a, float *__restrict__ d_sigma, int N) {
    const int lane = threadIdx.x & 63;
    const int ray = wave_ray();
    if (ray >= N) return;
    int64_t start;
    const int cnt = ray_range(ray_start, ray_cnt, ray, &start);
    float tail = 0.f;
    for (int c = (cnt + 63) / 64 - 1; c >= 0; c--) {
        const int k = c * 64 + lane;
        const bool on = k < cnt;
        const int64_t i = start + k;
        float dt = 0.f, own = 0.f, term = 0.f;
        if (on) {
            dt = te[i] - ts[i];
            const float sd = sigma[i] * dt;
            const float T = trans[i];
            const float keep = expf(-sd);                 // 1 - alpha
            const float gw = g_w ? g_w[i] : 0.f;
            own = (gw * T + (g_a ? g_a[i] : 0.f)) * keep;
            term = gw * (T * -expm1f(-sd)) + (g_T ? g_T[i] * T : 0.f);
        }
        float total;
        const float suffix = tail + vr_rev_excl_sum(term, lane, total);
        if (on) d_sigma[i] = dt * (own - suffix);
        tail += total;
    }
}

// Alpha form.  dL/dalpha_i = g_w_i T_i - sum_{j>i} (g_w_j alpha_j + g_T_j) prod_{k<j, k != i} (1 - alpha_k): the product with
// factor i LEFT OUT, finite at alpha_i = 1.  Pass 1 (forward) scans, exclusively, the product P of the non-zero factors and the
// count Z of the zero factors, and parks them as one signed number in d_alpha (each lane re-reads only what it wrote):
//   +P where Z = 0 (then T = P),  -P where Z = 1,  0 where Z >= 2 (no left-out product is non-zero there).
// Factors are taken as non-negative (alpha <= 1).  Pass 2 (reverse) forms two suffix sums of c_j P_j, c_j = g_w_j alpha_j + g_T_j,
// S0 over the samples with Z_j = 0 and S1 over those with Z_j = 1:
//   1 - alpha_i != 0:  d_i = g_w_i T_i - S0_i / (1 - alpha_i)      (every term of S0_i holds the factor once)
//   1 - alpha_i == 0:  d_i = g_w_i T_i - (Z_i == 0 ? S1_i : 0)     (the samples behind i up to the next opaque one)
__global__ __launch_bounds__(256) void ray_weights_bwd_alpha_kernel(const float *__restrict__ alphas,
                                                                    const int32_t *__restrict__ ray_start,
                                                                    const int32_t *__restrict__ ray_cnt, const float *__restrict__ g_w,
                                                                    const float *__restrict__ g_T, float *__restrict__ d_alpha, int N) {
    const int lane = threadIdx.x & 63;
    const int ray = wave_ray();
    if (ray >= N) return;
    int64_t start;
    const int cnt = ray_range(ray_start, ray_cnt, ray, &start);
    double carry_p = 1.0;
    int carry_z = 0;
    for (int base = 0; base < cnt; base += 64) {
        const int k = base + lane;
        const bool on = k < cnt;
        const int64_t i = start + k;
        const double f = on ? 1.0 - (double)alphas[i] : 1.0;      // exact
        const bool zero = f == 0.0;
        const double incl_p = wave_incl_prod(zero ? 1.0 : f, lane);
        const int incl_z = wave_incl_scan(zero ? 1 : 0, lane);
        const float P = (float)(carry_p * wave_excl_below(incl_p, lane, 1.0));
        const int Z = carry_z + incl_z - (zero ? 1 : 0);
        if (on) d_alpha[i] = Z == 0 ? P : (Z == 1 ? -P : 0.f);
        carry_p *= __shfl(incl_p, 63);
        carry_z += __shfl(incl_z, 63);
    }
    // the suffix sums and the last line in double as well: what is left of fp32 is the rounding of the parked P and of the result
    double tail0 = 0.0, tail1 = 0.0;
    for (int c = (cnt + 63) / 64 - 1; c >= 0; c--) {
        const int k = c * 64 + lane;
        const bool on = k < cnt;
        const int64_t i = start + k;
        float q = 0.f, gw = 0.f;
        double f = 1.0, t0 = 0.0, t1 = 0.0;
        if (on) {
            const float a = alphas[i];
            f = 1.0 - (double)a;
            q = d_alpha[i];
            gw = g_w ? g_w[i] : 0.f;
            const double cj = (double)gw * (double)a + (g_T ? (double)g_T[i] : 0.0);
            if (q > 0.f) t0 = cj * (double)q;
            if (q < 0.f) t1 = cj * -(double)q;
        }
        double tot0, tot1;
        const double s0 = tail0 + vr_rev_excl_sum(t0, lane, tot0);
        const double s1 = tail1 + vr_rev_excl_sum(t1, lane, tot1);
        if (on) {
            const double T = q > 0.f ? (double)q : 0.0;
            const double behind = f != 0.0 ? s0 / f : (q > 0.f ? s1 : 0.0);
            d_alpha[i] = (float)((double)gw * T - behind);
        }
        tail0 += tot0;
        tail1 += tot1;
    }
}

// ------------------------------------------------------------------------------------------------------- accumulate
// D <= 4: a lane per sample -- a chunk's 64 D values are one contiguous block -- D sums in registers, one wave reduction at the end.
template <int D, bool ONES>
__global__ __launch_bounds__(256) void accumulate_fwd_small_kernel(const float *__restrict__ weights, const float *__restrict__ values,
                                                                   const int32_t *__restrict__ ray_start,
                                                                   const int32_t *__restrict__ ray_cnt, float *__restrict__ out, int N) {
    const int lane = threadIdx.x & 63;
    const int ray = wave_ray();
    if (ray >= N) return;
    int64_t start;
    const int cnt = ray_range(ray_start, ray_cnt, ray, &start);
    float acc[D];
#pragma unroll
    for (int c = 0; c < D; c++) acc[c] = 0.f;
    for (int k = lane; k < cnt; k += 64) {
        const int64_t i = start + k;
        const float w = weights[i];
#pragma unroll
        for (int c = 0; c < D; c++) acc[c] += ONES ? w : w * values[i * D + c];
    }
#pragma unroll
    for (int c = 0; c < D; c++) {
        const float s = wave_sum(acc[c]);
        if (lane == 0) out[(int64_t)ray * D + c] = s;
    }
}

// D in 5 .. 256: G = the power of two >= D, at most 64, lanes per sample; lane (sub, ch) = (lane / G, lane % G) walks the samples
// sub, sub + 64 / G, ... and the channels ch, ch + 64, ... (more than one only when D > 64), so the wave reads 64 / G whole
// samples -- (64 / G) D contiguous floats -- per step.  Per-lane sums, then a butterfly across the sub-groups.
__global__ __launch_bounds__(256) void accumulate_fwd_wide_kernel(const float *__restrict__ weights, const float *__restrict__ values, int D,
                                                                  int G, const int32_t *__restrict__ ray_start,
                                                                  const int32_t *__restrict__ ray_cnt, float *__restrict__ out, int N) {
    const int lane = threadIdx.x & 63;
    const int ray = wave_ray();
    if (ray >= N) return;
    int64_t start;
    const int cnt = ray_range(ray_start, ray_cnt, ray, &start);
    const int sub = lane / G, ch = lane % G, step = 64 / G;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    // four steps' loads are issued before the first is used: with one load-use pair a step the D = 48 kernel ran at 0.41 of the
    // copy rate, each wave waiting out a memory latency per 192 bytes; this way at 0.75.  The sums are taken in the
    // order of the plain loop.
    for (int k0 = sub; k0 < cnt; k0 += 4 * step) {
        float w[4], v[4][4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int k = k0 + u * step;
            const bool on = k < cnt;
            const int64_t i = start + (on ? k : k0);
            w[u] = on ? weights[i] : 0.f;
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const int c = ch + s * 64;
                v[u][s] = (on && c < D) ? values[i * D + c] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
#pragma unroll
            for (int s = 0; s < 4; s++) acc[s] += w[u] * v[u][s];
        }
    }
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const float v = wave_sum_across(acc[s], G);
        const int c = ch + s * 64;
        if (sub == 0 && c < D) out[(int64_t)ray * D + c] = v;
    }
}

// backward, elementwise over the samples of a ray: d_weights_i = sum_c g[ray, c] v[i, c] (values NULL: g[ray, 0]),
// d_values[i, c] = w_i g[ray, c]
template <int D, bool ONES>
__global__ __launch_bounds__(256) void accumulate_bwd_small_kernel(const float *__restrict__ weights, const float *__restrict__ values,
                                                                   const int32_t *__restrict__ ray_start,
                                                                   const int32_t *__restrict__ ray_cnt, const float *__restrict__ g_out,
                                                                   float *__restrict__ d_weights, float *__restrict__ d_values, int N) {
    const int lane = threadIdx.x & 63;
    const int ray = wave_ray();
    if (ray >= N) return;
    int64_t start;
    const int cnt = ray_range(ray_start, ray_cnt, ray, &start);
    float g[D];
#pragma unroll
    for (int c = 0; c < D; c++) g[c] = g_out[(int64_t)ray * D + c];
    for (int k = lane; k < cnt; k += 64) {
        const int64_t i = start + k;
        if (d_weights) {
            float s = ONES ? g[0] : 0.f;
            if (!ONES) {
#pragma unroll
                for (int c = 0; c < D; c++) s += g[c] * values[i * D + c];
            }
            d_weights[i] = s;
        }
        if (!ONES && d_values) {
            const float w = weights[i];
#pragma unroll
            for (int c = 0; c < D; c++) d_values[i * D + c] = w * g[c];
        }
    }
}

__global__ __launch_bounds__(256) void accumulate_bwd_wide_kernel(const float *__restrict__ weights, const float *__restrict__ values, int D,
                                                                  int G, const int32_t *__restrict__ ray_start,
                                                                  const int32_t *__restrict__ ray_cnt, const float *__restrict__ g_out,
                                                                  float *__restrict__ d_weights, float *__restrict__ d_values, int N) {
    const int lane = threadIdx.x & 63;
    const int ray = wave_ray();
    if (ray >= N) return;
    int64_t start;
    const int cnt = ray_range(ray_start, ray_cnt, ray, &start);
    const int sub = lane / G, ch = lane % G, step = 64 / G;
    float g[4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const int c = ch + s * 64;
        g[s] = c < D ? g_out[(int64_t)ray * D + c] : 0.f;
    }
    // every lane of the wave takes every trip (the butterfly below needs all of them): the trip count is the wave's, not the lane's
    for (int base = 0; base < cnt; base += step) {
        const int k = base + sub;
        const bool on = k < cnt;
        const int64_t i = start + k;
        const float w = (on && d_values) ? weights[i] : 0.f;
        float s_gv = 0.f;
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const int c = ch + s * 64;
            if (on && c < D) {
                if (d_weights) s_gv += g[s] * values[i * D + c];
                if (d_values) d_values[i * D + c] = w * g[s];
            }
        }
        if (d_weights) {
            s_gv = wave_sum_within(s_gv, G);
            if (on && ch == 0) d_weights[i] = s_gv;
        }
    }
}

inline int vr_group(int D) {
    int G = 8;
    while (G < D && G < 64) G <<= 1;
    return G;
}

}  // namespace

extern "C" int mh_pack_info(const void *ray_indices, int32_t idx_is_i64, int64_t M, int32_t N, int32_t *ray_start, int32_t *ray_cnt,
                            void *stream) {
    if (N == 0) return MH_OK;
    if (N < 0 || M < 0 || M > 0x7fffffffLL || (M > 0 && !ray_indices) || !ray_start || !ray_cnt) return MH_ERR_ARG;
    const dim3 grid((N + 255) / 256), block(256);
    if (idx_is_i64)
        hipLaunchKernelGGL(pack_info_kernel<int64_t>, grid, block, 0, mh_stream(stream), (const int64_t *)ray_indices, M, (int)N, ray_start,
                           ray_cnt);
    else
        hipLaunchKernelGGL(pack_info_kernel<int32_t>, grid, block, 0, mh_stream(stream), (const int32_t *)ray_indices, M, (int)N, ray_start,
                           ray_cnt);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_ray_weights_fwd(const float *values, const float *t_starts, const float *t_ends, int32_t alpha_form,
                                  const int32_t *ray_start, const int32_t *ray_cnt, int32_t N, float *weights, float *trans,
                                  float *alphas, void *stream) {
    if (N == 0) return MH_OK;
    if (N < 0 || !values || !ray_start || !ray_cnt || (!alpha_form && (!t_starts || !t_ends)) || (!weights && !trans && !alphas))
        return MH_ERR_ARG;
    const dim3 grid((N + 3) / 4), block(256);
    if (alpha_form)
        hipLaunchKernelGGL(ray_weights_fwd_kernel<true>, grid, block, 0, mh_stream(stream), values, t_starts, t_ends, ray_start, ray_cnt,
                           weights, trans, alphas, (int)N);
    else
        hipLaunchKernelGGL(ray_weights_fwd_kernel<false>, grid, block, 0, mh_stream(stream), values, t_starts, t_ends, ray_start, ray_cnt,
                           weights, trans, alphas, (int)N);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_ray_weights_bwd(const float *values, const float *t_starts, const float *t_ends, int32_t alpha_form,
                                  const int32_t *ray_start, const int32_t *ray_cnt, int32_t N, const float *trans, const float *g_weights,
                                  const float *g_trans, const float *g_alphas, float *d_values, void *stream) {
    if (N == 0) return MH_OK;
    if (N < 0 || !values || !ray_start || !ray_cnt || !d_values) return MH_ERR_ARG;
    if (!alpha_form && (!t_starts || !t_ends || !trans)) return MH_ERR_ARG;
    if (alpha_form && g_alphas) return MH_ERR_ARG;      // the alpha form has no alphas output
    const dim3 grid((N + 3) / 4), block(256);
    if (alpha_form)
        hipLaunchKernelGGL(ray_weights_bwd_alpha_kernel, grid, block, 0, mh_stream(stream), values, ray_start, ray_cnt, g_weights, g_trans,
                           d_values, (int)N);
    else
        hipLaunchKernelGGL(ray_weights_bwd_density_kernel, grid, block, 0, mh_stream(stream), values, t_starts, t_ends, ray_start, ray_cnt,
                           trans, g_weights, g_trans, g_alphas, d_values, (int)N);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

#define VR_ACC_SMALL(KERNEL, ...)                                                                                   \
    do {                                                                                                            \
        if (!values) hipLaunchKernelGGL((KERNEL<1, true>), grid, block, 0, mh_stream(stream), __VA_ARGS__);          \
        else if (D == 1) hipLaunchKernelGGL((KERNEL<1, false>), grid, block, 0, mh_stream(stream), __VA_ARGS__);     \
        else if (D == 2) hipLaunchKernelGGL((KERNEL<2, false>), grid, block, 0, mh_stream(stream), __VA_ARGS__);     \
        else if (D == 3) hipLaunchKernelGGL((KERNEL<3, false>), grid, block, 0, mh_stream(stream), __VA_ARGS__);     \
        else hipLaunchKernelGGL((KERNEL<4, false>), grid, block, 0, mh_stream(stream), __VA_ARGS__);                 \
    } while (0)

extern "C" int mh_accumulate_fwd(const float *weights, const float *values, int32_t D, const int32_t *ray_start, const int32_t *ray_cnt,
                                 int32_t N, float *out, void *stream) {
    if (N < 0 || D < 1 || D > 256 || (!values && D != 1)) return MH_ERR_ARG;
    if (N == 0) return MH_OK;
    if (!weights || !ray_start || !ray_cnt || !out) return MH_ERR_ARG;
    const dim3 grid((N + 3) / 4), block(256);
    if (D <= 4)
        VR_ACC_SMALL(accumulate_fwd_small_kernel, weights, values, ray_start, ray_cnt, out, (int)N);
    else
        hipLaunchKernelGGL(accumulate_fwd_wide_kernel, grid, block, 0, mh_stream(stream), weights, values, (int)D, vr_group(D), ray_start,
                           ray_cnt, out, (int)N);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_accumulate_bwd(const float *weights, const float *values, int32_t D, const int32_t *ray_start, const int32_t *ray_cnt,
                                 int32_t N, const float *g_out, float *d_weights, float *d_values, void *stream) {
    if (N < 0 || D < 1 || D > 256 || (!values && D != 1)) return MH_ERR_ARG;
    if (N == 0) return MH_OK;
    if (!ray_start || !ray_cnt || !g_out || (!d_weights && !d_values)) return MH_ERR_ARG;
    if (d_values && (!values || !weights)) return MH_ERR_ARG;
    const dim3 grid((N + 3) / 4), block(256);
    if (D <= 4)
        VR_ACC_SMALL(accumulate_bwd_small_kernel, weights, values, ray_start, ray_cnt, g_out, d_weights, d_values, (int)N);
    else
        hipLaunchKernelGGL(accumulate_bwd_wide_kernel, grid, block, 0, mh_stream(stream), weights, values, (int)D, vr_group(D), ray_start,
                           ray_cnt, g_out, d_weights, d_values, (int)N);
    MH_CHECK_LAUNCH();
    return MH_OK;
}
