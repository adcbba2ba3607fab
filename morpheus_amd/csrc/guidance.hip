// The Zero-1-to-3 guidance shell: what models/guidance/zero123_utils.py:Zero123.train_step does around its three networks
// (morpheus_amd/guidance.py is the Python face; tests/guidance_oracle.py restates every statement).
//
//   mh_sds_view / mh_sds_view_bank   conditioning rows T, angles to the reference views, the SDS scale and the per-reference weights
//   mh_sds_angles                    Zero123.angle_between on [r, theta, phi] rows (radians in, radians out)
//   mh_sds_noise                     the DDIM add_noise, written twice (unconditional and conditional half of x_in)
//   mh_sds_grad                      classifier-free combination, weighted mean over the references, w(t), nan_to_num, 0.5 sum g^2 / B
// Each is ONE launch and nothing is read back by the host.
//
// The view arithmetic (:107-119, :129-134, :164-175, :191-197) runs in float64 from the fp32 inputs and is rounded to fp32 once
// per output: a handful of values per step, and the chain ends in an arccos whose fp32 form loses half its bits near a reference
// view (a dot product 4 ulp short of 1 is 0.06 degrees).  The statements and their order are the reference's:
//   v       = (r sin(theta) cos(phi), r sin(theta) sin(phi), r cos(theta)),  u = v / |v|
//   angle   = rad2deg(arccos(clip(u1 . u2, -1, 1)))
//   scale_b = (exp(min_k angle_bk / (180 / R)) - 1) * grad_scale
//   R > 1:  inv = 1 / angle, 100 where above 100, / its row maximum, 0 where below 0.1;  R = 1: inv = 1
//   ws      = user_w * inv, / its row maximum, 0 where below 0.1
//   T_kb    = (deg2rad(p), sin(deg2rad(a)), cos(deg2rad(a)), r),  p / a / r the view relative to reference k, a - 360 where a > 180
// deg2rad(x) = x * (pi / 180) and rad2deg(x) = x * (180 / pi), as torch states them.
//
// mh_sds_noise and mh_sds_grad are fp32, one rounded operation per statement (no contraction):
//   x      = sqrtf(a_t) * latents + sqrtf(1 - a_t) * noise
//   e_k    = u_k + s * (c_k - u_k);  e = (sum_k w_k e_k) / (sum_k w_k), k ascending;  g = (scale * (1 - a_t)) * (e - noise)
//   grad   = g, 0 for NaN, +-FLT_MAX for +-inf
// The loss is summed in float64: every thread its grid-stride share, a butterfly per wavefront, the block's four waves in order,
// the partials of the blocks in order by the block that finishes last -- a fixed association for a given size, the same bits on
// every run.  `ticket` counts finished blocks; the last block puts it back to 0.
#include "common.h"

#pragma clang fp contract(off)

#include <float.h>

#include "wave.h"

#define SDS_MAX_R 8
#define SDS_GRAD_BLOCKS 256
constexpr double SDS_PI = 3.14159265358979323846;

struct Sph {
    double x, y, z;
};
// [r, theta, phi] (radians) -> the unit vector
__device__ __forceinline__ Sph sph_unit(double r, double theta, double phi) {
    const double st = sin(theta);
    Sph v = {r * st * cos(phi), r * st * sin(phi), r * cos(theta)};
    const double n = sqrt(v.x * v.x + v.y * v.y + v.z * v.z);
    v.x /= n;
    v.y /= n;
    v.z /= n;
    return v;
}
__device__ __forceinline__ double sph_angle(const Sph &a, const Sph &b) {          // radians
    const double d = a.x * b.x + a.y * b.y + a.z * b.z;
    return acos(fmin(fmax(d, -1.0), 1.0));
}
__device__ __forceinline__ double deg2rad(double d) { return d * (SDS_PI / 180.0); }
__device__ __forceinline__ double rad2deg(double r) { return r * (180.0 / SDS_PI); }

// One view b against R references: everything the header lists.  p, a, r: the view's deltas to reference 0 (degrees, degrees, radius).
__device__ __forceinline__ void view_row(double p, double a, double r, const float *__restrict__ ref_p, const float *__restrict__ ref_a,
                                         const float *__restrict__ ref_r, const float *__restrict__ user_w, int R, int B, int b,
                                         float grad_scale, float *__restrict__ T, float *__restrict__ angles,
                                         float *__restrict__ scale, float *__restrict__ ws) {
    const Sph v1 = sph_unit(r + ref_r[0], deg2rad(p + ref_p[0]), deg2rad(a + ref_a[0]));
    double ang[SDS_MAX_R], w[SDS_MAX_R];
    double amin = 0.0, imax = 0.0;
#pragma unroll
    for (int k = 0; k < SDS_MAX_R; k++) {
        if (k >= R) break;
        ang[k] = rad2deg(sph_angle(v1, sph_unit(ref_r[k], deg2rad(ref_p[k]), deg2rad(ref_a[k]))));
        amin = k ? fmin(amin, ang[k]) : ang[k];
        w[k] = fmin(1.0 / ang[k], 100.0);                                // 1 / 0 = inf: 100
        imax = k ? fmax(imax, w[k]) : w[k];
        angles[b * R + k] = (float)ang[k];
    }
    scale[b] = (float)((exp(amin / (180.0 / (double)R)) - 1.0) * (double)grad_scale);
    double wmax = 0.0;
#pragma unroll
    for (int k = 0; k < SDS_MAX_R; k++) {
        if (k >= R) break;
        double inv = 1.0;
        if (R > 1) {
            inv = w[k] / imax;
            if (inv < 0.1) inv = 0.0;
        }
        w[k] = (double)user_w[k] * inv;
        wmax = k ? fmax(wmax, w[k]) : w[k];
    }
#pragma unroll
    for (int k = 0; k < SDS_MAX_R; k++) {
        if (k >= R) break;
        double v = w[k] / wmax;
        if (v < 0.1) v = 0.0;
        ws[b * R + k] = (float)v;
        const double pk = p + ref_p[0] - ref_p[k], rk = r + ref_r[0] - ref_r[k];
        double ak = a + ref_a[0] - ref_a[k];
        if (ak > 180.0) ak -= 360.0;
        float *row = T + ((int64_t)k * B + b) * 4;
        row[0] = (float)deg2rad(pk);
        row[1] = (float)sin(deg2rad(ak));
        row[2] = (float)cos(deg2rad(ak));
        row[3] = (float)rk;
    }
}

__global__ __launch_bounds__(64) void sds_view_kernel(const float *__restrict__ polar, const float *__restrict__ azimuth,
                                                      const float *__restrict__ radius, int B, const float *__restrict__ ref_p,
                                                      const float *__restrict__ ref_a, const float *__restrict__ ref_r,
                                                      const float *__restrict__ user_w, int R, float grad_scale,
                                                      float *__restrict__ T, float *__restrict__ angles, float *__restrict__ scale,
                                                      float *__restrict__ ws) {
    for (int b = threadIdx.x; b < B; b += 64)
        view_row(polar[b], azimuth[b], radius[b], ref_p, ref_a, ref_r, user_w, R, B, b, grad_scale, T, angles, scale, ws);
}

// The keyframe bank (R = 1): the nearest keyframe of *frame_id (lowest index on a tie, torch.argmin's answer on the CPU);
// target = 0: the view against that keyframe; target != 0: the view re-expressed against keyframe 0 (morpheus.py:1059-1070)
__global__ __launch_bounds__(64) void sds_view_bank_kernel(const float *__restrict__ polar, const float *__restrict__ azimuth,
                                                           const float *__restrict__ radius, int B, const int64_t *__restrict__ frame_id,
                                                           const int64_t *__restrict__ kf, int K, const float *__restrict__ ref_p,
                                                           const float *__restrict__ ref_a, const float *__restrict__ ref_r,
                                                           const float *__restrict__ user_w, int target, float grad_scale,
                                                           int64_t *__restrict__ chosen, float *__restrict__ T,
                                                           float *__restrict__ angles, float *__restrict__ scale,
                                                           float *__restrict__ ws) {
    const int64_t f = frame_id[0];
    int near = 0;
    int64_t best = kf[0] > f ? kf[0] - f : f - kf[0];
    for (int j = 1; j < K; j++) {
        const int64_t d = kf[j] > f ? kf[j] - f : f - kf[j];
        if (d < best) {
            best = d;
            near = j;
        }
    }
    const int sel = target ? 0 : near;
    if (threadIdx.x == 0) chosen[0] = sel;
    for (int b = threadIdx.x; b < B; b += 64) {
        double p = polar[b], a = azimuth[b], r = radius[b];
        if (target) {
            p = (p + ref_p[near]) - ref_p[0];
            a = (a + ref_a[near]) - ref_a[0];
            r = (r + ref_r[near]) - ref_r[0];
            if (a > 180.0) a -= 360.0;
        }
        view_row(p, a, r, ref_p + sel, ref_a + sel, ref_r + sel, user_w + sel, 1, B, b, grad_scale, T, angles, scale, ws);
    }
}

__global__ __launch_bounds__(256) void sds_angles_kernel(const float *__restrict__ v1, int N1, const float *__restrict__ v2, int N2,
                                                         float *__restrict__ out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= N1 * N2) return;
    const float *a = v1 + (p / N2) * 3, *b = v2 + (p % N2) * 3;
    out[p] = (float)sph_angle(sph_unit(a[0], a[1], a[2]), sph_unit(b[0], b[1], b[2]));
}

__device__ __forceinline__ float alpha_at(const float *__restrict__ alphas, int T, int64_t t) {
    return alphas[t < 0 ? 0 : t >= T ? T - 1 : t];                     // a step outside the table is held to its ends
}

__global__ __launch_bounds__(256) void sds_noise_kernel(const float *__restrict__ latents, const float *__restrict__ noise,
                                                        const int64_t *__restrict__ t, const float *__restrict__ alphas, int T, int B,
                                                        int64_t n, float *__restrict__ x_in) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B * n) return;
    const float a = alpha_at(alphas, T, t[p / n]);
    const float x = sqrtf(a) * latents[p] + sqrtf(1.0f - a) * noise[p];
    x_in[p] = x;
    x_in[B * n + p] = x;
}

// the sum of the block's 256 values, in every thread; waves in order
__device__ __forceinline__ double block_sum(double v) {
    __shared__ double s_w[4];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    const double total = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(256) void sds_grad_kernel(const float *__restrict__ noise_preds, const float *__restrict__ ws,
                                                       const float *__restrict__ noise, const int64_t *__restrict__ t,
                                                       const float *__restrict__ alphas, int T, const float *__restrict__ scale,
                                                       float guidance_scale, int R, int B, int64_t n, float *__restrict__ grad,
                                                       double *partials, uint32_t *__restrict__ ticket,
                                                       float *__restrict__ loss) {
    __shared__ bool s_last;
    double part = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < B * n; p += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(p / n);
        float acc = 0.f, wsum = 0.f;
        for (int k = 0; k < R; k++) {
            const float *np = noise_preds + (int64_t)k * 2 * B * n;
            const float u = np[p], c = np[B * n + p], w = ws[b * R + k];
            const float e = u + guidance_scale * (c - u);
            acc = k ? acc + w * e : w * e;
            wsum = k ? wsum + w : w;
        }
        const float wt = 1.0f - alpha_at(alphas, T, t[b]);
        float g = (scale[b] * wt) * (acc / wsum - noise[p]);
        if (g != g)
            g = 0.f;
        else if (g > FLT_MAX)
            g = FLT_MAX;
        else if (g < -FLT_MAX)
            g = -FLT_MAX;
        grad[p] = g;
        part += (double)g * (double)g;
    }
    part = block_sum(part);
    if (threadIdx.x == 0) {
        // the one lane that stores the partial also signals for it: store, agent release, the wait the compiler may not drop,
        // then the ticket; the block whose add came last is the reducer
        partials[blockIdx.x] = part;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    if (threadIdx.x == 0) {                                   // one agent acquire for the block (the L1 is the CU's), waited for
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    double v = threadIdx.x < gridDim.x ? partials[threadIdx.x] : 0.0;      // gridDim.x <= 256
    v = block_sum(v);
    if (threadIdx.x == 0) {
        loss[0] = (float)(0.5 * v / (double)B);
        *ticket = 0u;
    }
}

// ---- entry points ------------------------------------------------------------------------------------------------------------
static inline bool view_args_ok(const void *polar, const void *azimuth, const void *radius, const void *ref_p, const void *ref_a,
                                const void *ref_r, const void *w, const void *T, const void *angles, const void *scale, const void *ws) {
    return polar && azimuth && radius && ref_p && ref_a && ref_r && w && T && angles && scale && ws;
}

extern "C" int32_t mh_sds_max_refs(void) { return SDS_MAX_R; }
extern "C" int32_t mh_sds_grad_blocks(void) { return SDS_GRAD_BLOCKS; }

extern "C" int mh_sds_view(const float *polar, const float *azimuth, const float *radius, int32_t B, const float *ref_polars,
                           const float *ref_azimuths, const float *ref_radii, const float *user_ws, int32_t R, float grad_scale,
                           float *T, float *angles, float *scale, float *ws, void *stream) {
    if (B == 0) return MH_OK;
    if (!view_args_ok(polar, azimuth, radius, ref_polars, ref_azimuths, ref_radii, user_ws, T, angles, scale, ws) || B < 0 || R < 1 ||
        R > SDS_MAX_R)
        return MH_ERR_ARG;
    hipLaunchKernelGGL(sds_view_kernel, dim3(1), dim3(64), 0, mh_stream(stream), polar, azimuth, radius, (int)B, ref_polars,
                       ref_azimuths, ref_radii, user_ws, (int)R, grad_scale, T, angles, scale, ws);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_sds_view_bank(const float *polar, const float *azimuth, const float *radius, int32_t B, const int64_t *frame_id,
                                const int64_t *kf_index, int32_t K, const float *ref_polars, const float *ref_azimuths,
                                const float *ref_radii, const float *user_ws, int32_t target, float grad_scale, int64_t *chosen,
                                float *T, float *angles, float *scale, float *ws, void *stream) {
    if (!view_args_ok(polar, azimuth, radius, ref_polars, ref_azimuths, ref_radii, user_ws, T, angles, scale, ws) || !frame_id ||
        !kf_index || !chosen || B < 0 || K < 1)
        return MH_ERR_ARG;
    hipLaunchKernelGGL(sds_view_bank_kernel, dim3(1), dim3(64), 0, mh_stream(stream), polar, azimuth, radius, (int)B, frame_id,
                       kf_index, (int)K, ref_polars, ref_azimuths, ref_radii, user_ws, (int)target, grad_scale, chosen, T, angles,
                       scale, ws);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_sds_angles(const float *v1, int32_t N1, const float *v2, int32_t N2, float *out, void *stream) {
    if (N1 == 0 || N2 == 0) return MH_OK;
    if (!v1 || !v2 || !out || N1 < 0 || N2 < 0 || (int64_t)N1 * N2 > 0x7fffffffLL) return MH_ERR_ARG;
    hipLaunchKernelGGL(sds_angles_kernel, dim3((unsigned)(((int64_t)N1 * N2 + 255) / 256)), dim3(256), 0, mh_stream(stream), v1,
                       (int)N1, v2, (int)N2, out);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_sds_noise(const float *latents, const float *noise, const int64_t *t, const float *alphas_cumprod, int32_t T,
                            int32_t B, int64_t n, float *x_in, void *stream) {
    if (B == 0 || n == 0) return MH_OK;
    if (!latents || !noise || !t || !alphas_cumprod || !x_in || T < 1 || B < 0 || n < 0 || B * n > 0x3fffffffLL) return MH_ERR_ARG;
    hipLaunchKernelGGL(sds_noise_kernel, dim3((unsigned)((B * n + 255) / 256)), dim3(256), 0, mh_stream(stream), latents, noise, t,
                       alphas_cumprod, (int)T, (int)B, n, x_in);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_sds_grad(const float *noise_preds, const float *ws, const float *noise, const int64_t *t,
                           const float *alphas_cumprod, int32_t T, const float *scale, float guidance_scale, int32_t R, int32_t B,
                           int64_t n, float *grad, double *partials, uint32_t *ticket, float *loss, void *stream) {
    if (!noise_preds || !ws || !noise || !t || !alphas_cumprod || !scale || !grad || !partials || !ticket || !loss || T < 1 || R < 1 ||
        R > SDS_MAX_R || B < 1 || n < 1 || B * n > 0x3fffffffLL)
        return MH_ERR_ARG;
    int64_t blocks = (B * n + 255) / 256;
    if (blocks > SDS_GRAD_BLOCKS) blocks = SDS_GRAD_BLOCKS;
    hipLaunchKernelGGL(sds_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, mh_stream(stream), noise_preds, ws, noise, t,
                       alphas_cumprod, (int)T, scale, guidance_scale, (int)R, (int)B, n, grad, partials, ticket, loss);
    MH_CHECK_LAUNCH();
    return MH_OK;
}
