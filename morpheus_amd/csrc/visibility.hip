// Visibility pruning of packed samples: the keep mask of a density (or opacity) pass and the order-preserving compaction.
//
// Semantics: nerfacc 0.5.x's render_visibility_from_density / render_visibility_from_alpha as OccGridEstimator.sampling
// applies them (third-party, un-vendored; restated from recall in include/morpheus_hip.h, NOT verified).
// Design: one wavefront per ray, the compositor's scan (csrc/composite.hip): the ray's packed samples are walked in chunks of
// 64, the exclusive prefix of the optical depth is a 6-step wave scan plus a scalar carry.  The optical depth is clamped to
// >= 0, so the transmittance never rises along a ray: once the carry alone puts it under early_stop_eps the wavefront stops
// reading the ray and only zeroes the rest of its keep bytes.  The compaction is the marcher's: ballot + prefix popcount.
// No atomics, no LDS, no cross-ray sum.
#include "common.h"
#include "wave.h"

// exclusive wave scan that survives +inf terms (an opaque sample: alpha = 1, or sigma = inf): the "lane below" form, where the
// compositor's `incl - v` would form inf - inf
__device__ __forceinline__ float wave_excl_scan(float v, int lane, float *total) {
    const float incl = wave_incl_scan(v, lane);
    *total = __shfl(incl, 63);
    return wave_excl_below(incl, lane, 0.f);
}

template <bool ALPHA>
__global__ __launch_bounds__(256) void visibility_mask_kernel(const float *__restrict__ val, const float *__restrict__ ts,
                                                              const float *__restrict__ te,
                                                              const int32_t *__restrict__ ray_start,
                                                              const int32_t *__restrict__ ray_cnt, int N, int64_t M, float eps,
                                                              const float *__restrict__ alpha_thre,
                                                              uint8_t *__restrict__ keep, int32_t *__restrict__ kept_cnt) {
    const int lane = threadIdx.x & 63;
    const int ray = wave_ray();
    if (ray >= N) return;
    int64_t start;
    const int cnt = ray_range_clamped(ray_start, ray_cnt, ray, M, &start);
    const float thre = alpha_thre ? *alpha_thre : 0.f;
    float carry = 0.f;       // optical depth of the samples before this chunk: T = exp(-carry - prefix inside the chunk)
    int n = 0, base = 0;
    for (; base < cnt; base += 64) {
        const int k = base + lane;
        const bool on = k < cnt;
        const int64_t i = start + k;
        float x = 0.f, alpha = 0.f;
        bool ok = false;
        if (on) {
            const float v = val[i];
            ok = !(v != v);
            if (ALPHA) {
                alpha = fminf(fmaxf(v, 0.f), 1.f);
                x = -log1pf(-alpha);
            } else {
                x = v * (te[i] - ts[i]);
                ok = !(x != x);
                x = fmaxf(x, 0.f);
                alpha = -expm1f(-x);
            }
            if (!ok) x = 0.f;      // a NaN sample is dropped and adds nothing to the sum
        }
        float total;
        const float excl = carry + wave_excl_scan(x, lane, &total);
        const bool kp = ok && (expf(-excl) >= eps) && (alpha >= thre);
        if (on) keep[i] = kp ? 1 : 0;
        n += __popcll(__ballot(kp));
        carry += total;
        if (expf(-carry) < eps) {      // uniform over the wavefront: every later sample has T <= exp(-carry)
            base += 64;
            break;
        }
    }
    for (int k = base + lane; k < cnt; k += 64) keep[start + k] = 0;
    if (lane == 0) kept_cnt[ray] = n;
}

__global__ __launch_bounds__(256) void visibility_pack_kernel(const uint8_t *__restrict__ keep, const float *__restrict__ ts,
                                                              const float *__restrict__ te,
                                                              const int32_t *__restrict__ ray_start,
                                                              const int32_t *__restrict__ ray_cnt,
                                                              const int32_t *__restrict__ new_start, int N, int64_t M,
                                                              int64_t M_out, int32_t *__restrict__ out_ray_idx,
                                                              float *__restrict__ out_ts, float *__restrict__ out_te,
                                                              int32_t *__restrict__ src_index) {
    const int lane = threadIdx.x & 63;
    const int ray = wave_ray();
    if (ray >= N) return;
    int64_t start;
    const int cnt = ray_range_clamped(ray_start, ray_cnt, ray, M, &start);
    const int64_t dst0 = new_start[ray];
    int n = 0;
    for (int base = 0; base < cnt; base += 64) {
        const int k = base + lane;
        const int64_t i = start + k;
        const bool kp = k < cnt && keep[i] != 0;
        const unsigned long long mask = __ballot(kp);
        const int64_t dst = dst0 + n + wave_rank(mask, lane);
        if (kp && dst >= 0 && dst < M_out) {
            out_ray_idx[dst] = ray;
            out_ts[dst] = ts[i];
            out_te[dst] = te[i];
            src_index[dst] = (int32_t)i;
        }
        n += __popcll(mask);
    }
}

extern "C" int mh_visibility_mask(const float *values, int32_t alpha_form, const float *t_starts, const float *t_ends,
                                  const int32_t *ray_start, const int32_t *ray_cnt, int32_t N, int64_t M,
                                  float early_stop_eps, const float *alpha_thre, uint8_t *keep, int32_t *kept_cnt,
                                  void *stream) {
    if (N < 0 || M < 0 || M > 0x7fffffffLL || !(early_stop_eps >= 0.f) || !(early_stop_eps <= 1.f) ||
        (alpha_form != 0 && alpha_form != 1))
        return MH_ERR_ARG;
    if (N == 0 || M == 0) return MH_OK;
    if (!values || !ray_start || !ray_cnt || !keep || !kept_cnt) return MH_ERR_ARG;
    if (!alpha_form && (!t_starts || !t_ends)) return MH_ERR_ARG;
    if (alpha_form)
        hipLaunchKernelGGL(visibility_mask_kernel<true>, dim3((N + 3) / 4), dim3(256), 0, mh_stream(stream), values, t_starts,
                           t_ends, ray_start, ray_cnt, (int)N, M, early_stop_eps, alpha_thre, keep, kept_cnt);
    else
        hipLaunchKernelGGL(visibility_mask_kernel<false>, dim3((N + 3) / 4), dim3(256), 0, mh_stream(stream), values, t_starts,
                           t_ends, ray_start, ray_cnt, (int)N, M, early_stop_eps, alpha_thre, keep, kept_cnt);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_visibility_pack(const uint8_t *keep, const float *t_starts, const float *t_ends, const int32_t *ray_start,
                                  const int32_t *ray_cnt, const int32_t *new_start, int32_t N, int64_t M, int64_t M_out,
                                  int32_t *out_ray_idx, float *out_t_starts, float *out_t_ends, int32_t *src_index,
                                  void *stream) {
    if (N < 0 || M < 0 || M > 0x7fffffffLL || M_out < 0 || M_out > M) return MH_ERR_ARG;
    if (N == 0 || M == 0 || M_out == 0) return MH_OK;
    if (!keep || !t_starts || !t_ends || !ray_start || !ray_cnt || !new_start || !out_ray_idx || !out_t_starts ||
        !out_t_ends || !src_index)
        return MH_ERR_ARG;
    hipLaunchKernelGGL(visibility_pack_kernel, dim3((N + 3) / 4), dim3(256), 0, mh_stream(stream), keep, t_starts, t_ends,
                       ray_start, ray_cnt, new_start, (int)N, M, M_out, out_ray_idx, out_t_starts, out_t_ends, src_index);
    MH_CHECK_LAUNCH();
    return MH_OK;
}
