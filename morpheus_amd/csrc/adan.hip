// Adan over ONE flat fp32 parameter bucket: the step behind `train.optim: 'adan'`.
//
// Replaces Adan(model.get_params_all(5 lr), eps=1e-8, weight_decay=2e-5, max_grad_norm=5.0, foreach=False) of the reference
// (morpheus.py:146-150; the rule is models/optimizer.py:101-256): ~15 elementwise launches per parameter tensor plus a
// three-launch-per-tensor norm loop that ends in .item() there; here the layout of optim.hip -- parameters, gradients and the
// four states (exp_avg m, exp_avg_sq n, exp_avg_diff d, neg_pre_grad q) in six flat buffers -- and per step
//   prologue  one block (two above 80 segments): the segment table into the device workspace
//   norm      per-workgroup sums of g g in double over the segments that have a gradient, then one block that adds the partial
//             sums in a fixed order and leaves c = min(max_grad_norm / (sqrt(sum) + eps), 1) in the workspace: an fp32 value as
//             the reference's, rounded ONCE from the double quotient (the reference rounds the sum, the root and the quotient:
//             its c lies within those roundings of this one); no atomics: the same bits on every run; both launches only when
//             max_grad_norm > 0
//   step      one pass, float4 lanes:
//     first gradient of the parameter, or group step 1:  q = g (-c)
//     g' = g c;  q += g';  m = m b1 + (1 - b1) g';  d = d b2 + (1 - b2) q;  q = q b2 + g';  n = n b3 + ((1 - b3) q) q
//     den = sqrt(n) / sqrt(1 - b3^t) + eps
//     no_prox:    p = p (1 - lr wd);  p -= (ss m) / den;  p -= (sd d) / den         ss = lr / (1 - b1^t)
//     otherwise:  p -= (ss m) / den;  p -= (sd d) / den;  p = p / (1 + lr wd)       sd = lr b2 / (1 - b2^t)
//     q = -g';  with clipping g' is written back into the gradient bucket (the reference scales p.grad in place)
// -- every operator rounded on its own, in the reference's order (this file is built with -ffp-contract=off).  The host never
// reads c: a step makes no synchronisation.
#include "common.h"

#define ADAN_MAX_SEGS 160
#define ADAN_CHUNK 80            // segments per prologue launch: the table travels by value, 2 KB a launch
#define ADAN_NORM_BLOCKS 512
#define ADAN_SKIP 1              // flag bits of a segment
#define ADAN_FIRST 2

// A segment is ONE parameter tensor or a group's alignment pad (optim.hip): the group's step sizes, its decay factor, whether
// the parameter is skipped (gradient None: value and states keep their bits) and whether this is its first gradient.
struct AdanTable {
    int64_t end[ADAN_MAX_SEGS];
    float ss[ADAN_MAX_SEGS], sd[ADAN_MAX_SEGS], bc3s[ADAN_MAX_SEGS], decay[ADAN_MAX_SEGS];
    int32_t flag[ADAN_MAX_SEGS];
};
struct AdanWorkspace {
    float clip, sumsq, norm, pad;      // c of the last step; the sum of squares and the norm behind it (0 without clipping)
    AdanTable tab;
    double partial[ADAN_NORM_BLOCKS];
};
struct AdanChunk {
    int64_t end[ADAN_CHUNK];
    float ss[ADAN_CHUNK], sd[ADAN_CHUNK], bc3s[ADAN_CHUNK], decay[ADAN_CHUNK];
    uint8_t flag[ADAN_CHUNK];
    int32_t base, count;
};

// flag_dev / seen_dev: NULL (the flags of the chunk hold), or the data-parallel bookkeeping of adam_steps_kernel: a segment is
// stepped where its all-reduced has-gradient flag is > 0 (a NaN flag skips), its count of gradients seen goes up there, and a
// count of 0 before makes this its first gradient.
__global__ void adan_table_kernel(AdanWorkspace *__restrict__ ws, AdanChunk ch, const float *__restrict__ flag_dev,
                                  int64_t *__restrict__ seen_dev) {
    const int k = threadIdx.x;
    if (k == 0 && ch.base == 0) ws->clip = 1.0f, ws->sumsq = 0.0f, ws->norm = 0.0f, ws->pad = 0.0f;
    if (k >= ch.count) return;
    const int s = ch.base + k;
    int flag = ch.flag[k];
    if (flag_dev) {
        if (flag_dev[s] > 0.0f) {
            const int64_t seen = seen_dev[s];
            if (seen == 0) flag |= ADAN_FIRST;
            seen_dev[s] = seen + 1;
        } else {
            flag |= ADAN_SKIP;
        }
    }
    ws->tab.end[s] = ch.end[k];
    ws->tab.ss[s] = ch.ss[k], ws->tab.sd[s] = ch.sd[k], ws->tab.bc3s[s] = ch.bc3s[k], ws->tab.decay[s] = ch.decay[k];
    ws->tab.flag[s] = flag;
}

// first segment whose end is beyond i (binary search over <= 160 ends in LDS)
__device__ __forceinline__ int adan_seg_of(const int64_t *end, int n_segs, int64_t i) {
    int lo = 0, hi = n_segs - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (i >= end[mid]) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// sum over the block's 256 threads in a fixed order (a tree over LDS); the result is thread 0's
__device__ __forceinline__ double adan_block_sum(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void adan_norm_kernel(const float *__restrict__ g, AdanWorkspace *__restrict__ ws, int n_segs,
                                                        int64_t n) {
    __shared__ int64_t s_end[ADAN_MAX_SEGS];
    __shared__ int s_flag[ADAN_MAX_SEGS];
    __shared__ double red[256];
    if ((int)threadIdx.x < n_segs) s_end[threadIdx.x] = ws->tab.end[threadIdx.x], s_flag[threadIdx.x] = ws->tab.flag[threadIdx.x];
    __syncthreads();
    double acc = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
    for (int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i0 < n; i0 += stride) {
        const int cnt = (n - i0) < 4 ? (int)(n - i0) : 4;
        int seg = adan_seg_of(s_end, n_segs, i0);
        if ((i0 + cnt) <= s_end[seg] && (s_flag[seg] & ADAN_SKIP)) continue;
        float gv[4] = {0.f, 0.f, 0.f, 0.f};
        if (cnt == 4) {
            const f32x4 b = *reinterpret_cast<const f32x4 *>(g + i0);
#pragma unroll
            for (int k = 0; k < 4; k++) gv[k] = b[k];
        } else {
            for (int k = 0; k < cnt; k++) gv[k] = g[i0 + k];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (k < cnt) {
                while (seg < n_segs - 1 && i0 + k >= s_end[seg]) seg++;
                if (!(s_flag[seg] & ADAN_SKIP)) acc += (double)gv[k] * (double)gv[k];
            }
        }
    }
    const double sum = adan_block_sum(acc, red);
    if (threadIdx.x == 0) ws->partial[blockIdx.x] = sum;
}

__global__ __launch_bounds__(256) void adan_clip_kernel(AdanWorkspace *__restrict__ ws, int n_partials, double max_grad_norm, double eps) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += 256) acc += ws->partial[i];
    const double sum = adan_block_sum(acc, red);
    if (threadIdx.x == 0) {
        const double norm = sqrt(sum);
        const double q = max_grad_norm / (norm + eps);
        ws->sumsq = (float)sum, ws->norm = (float)norm;
        ws->clip = q > 1.0 ? 1.0f : (float)q;     // (a NaN norm stays NaN, as torch.clamp keeps it)
    }
}

struct AdanConst {
    float b1, b2, b3, omb1, omb2, omb3, eps;      // the betas and 1 - beta, each rounded to fp32 from double
    int32_t no_prox, write_g;
};

__global__ __launch_bounds__(256) void adan_kernel(float *__restrict__ p, float *__restrict__ g, float *__restrict__ m,
                                                   float *__restrict__ nn, float *__restrict__ d, float *__restrict__ q,
                                                   const AdanWorkspace *__restrict__ ws, int n_segs, AdanConst k, int64_t n) {
    __shared__ int64_t s_end[ADAN_MAX_SEGS];
    __shared__ float s_ss[ADAN_MAX_SEGS], s_sd[ADAN_MAX_SEGS], s_bc3s[ADAN_MAX_SEGS], s_decay[ADAN_MAX_SEGS];
    __shared__ int s_flag[ADAN_MAX_SEGS];
    const int t = threadIdx.x;
    if (t < n_segs) {
        s_end[t] = ws->tab.end[t], s_flag[t] = ws->tab.flag[t];
        s_ss[t] = ws->tab.ss[t], s_sd[t] = ws->tab.sd[t], s_bc3s[t] = ws->tab.bc3s[t], s_decay[t] = ws->tab.decay[t];
    }
    __syncthreads();
    const int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i0 >= n) return;
    const int cnt = (n - i0) < 4 ? (int)(n - i0) : 4;
    int seg = adan_seg_of(s_end, n_segs, i0);
    if ((i0 + cnt) <= s_end[seg] && (s_flag[seg] & ADAN_SKIP)) return;      // skipped parameter: nothing is read or written
    const float c = ws->clip;
    float pv[4], gv[4], mv[4], nv[4], dv[4], qv[4];
    if (cnt == 4) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(p + i0), b = *reinterpret_cast<const f32x4 *>(g + i0);
        const f32x4 e = *reinterpret_cast<const f32x4 *>(m + i0), f = *reinterpret_cast<const f32x4 *>(nn + i0);
        const f32x4 h = *reinterpret_cast<const f32x4 *>(d + i0), j = *reinterpret_cast<const f32x4 *>(q + i0);
#pragma unroll
        for (int i = 0; i < 4; i++) pv[i] = a[i], gv[i] = b[i], mv[i] = e[i], nv[i] = f[i], dv[i] = h[i], qv[i] = j[i];
    } else {
        for (int i = 0; i < cnt; i++)
            pv[i] = p[i0 + i], gv[i] = g[i0 + i], mv[i] = m[i0 + i], nv[i] = nn[i0 + i], dv[i] = d[i0 + i], qv[i] = q[i0 + i];
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (i < cnt) {
            while (seg < n_segs - 1 && i0 + i >= s_end[seg]) seg++;
            const int flag = s_flag[seg];
            if (!(flag & ADAN_SKIP)) {
                if (flag & ADAN_FIRST) qv[i] = gv[i] * (-c);
                const float gp = gv[i] * c;
                float qq = qv[i] + gp;
                mv[i] = mv[i] * k.b1 + k.omb1 * gp;
                dv[i] = dv[i] * k.b2 + k.omb2 * qq;
                qq = qq * k.b2 + gp;
                nv[i] = nv[i] * k.b3 + (k.omb3 * qq) * qq;
                const float den = sqrtf(nv[i]) / s_bc3s[seg] + k.eps;
                float pp = pv[i];
                if (k.no_prox) {
                    pp = pp * s_decay[seg];
                    pp = pp - (s_ss[seg] * mv[i]) / den;
                    pp = pp - (s_sd[seg] * dv[i]) / den;
                } else {
                    pp = pp - (s_ss[seg] * mv[i]) / den;
                    pp = pp - (s_sd[seg] * dv[i]) / den;
                    pp = pp / s_decay[seg];
                }
                pv[i] = pp, gv[i] = gp, qv[i] = -gp;
            }
        }
    }
    if (cnt == 4) {
        f32x4 a, b, e, f, h, j;
#pragma unroll
        for (int i = 0; i < 4; i++) a[i] = pv[i], b[i] = gv[i], e[i] = mv[i], f[i] = nv[i], h[i] = dv[i], j[i] = qv[i];
        *reinterpret_cast<f32x4 *>(p + i0) = a;
        *reinterpret_cast<f32x4 *>(m + i0) = e;
        *reinterpret_cast<f32x4 *>(nn + i0) = f;
        *reinterpret_cast<f32x4 *>(d + i0) = h;
        *reinterpret_cast<f32x4 *>(q + i0) = j;
        if (k.write_g) *reinterpret_cast<f32x4 *>(g + i0) = b;
    } else {
        for (int i = 0; i < cnt; i++) {
            p[i0 + i] = pv[i], m[i0 + i] = mv[i], nn[i0 + i] = nv[i], d[i0 + i] = dv[i], q[i0 + i] = qv[i];
            if (k.write_g) g[i0 + i] = gv[i];
        }
    }
}

extern "C" int64_t mh_adan_workspace_bytes(void) { return (int64_t)sizeof(AdanWorkspace); }

// both entry points: seg_flag_host NULL with device flags, seg_flag_dev / seg_seen_dev NULL with host flags
static int adan_step(float *params, float *grads, float *exp_avg, float *exp_avg_sq, float *exp_avg_diff, float *neg_pre_grad,
                     int64_t n, int32_t n_segs, const int64_t *seg_end_host, const double *seg_lr_host,
                     const int64_t *seg_step_host, const int32_t *seg_flag_host, const float *seg_flag_dev, int64_t *seg_seen_dev,
                     double beta1, double beta2, double beta3, double eps, double weight_decay, double max_grad_norm,
                     int32_t no_prox, void *workspace, hipStream_t stream) {
    if (n == 0) return MH_OK;
    if (!params || !grads || !exp_avg || !exp_avg_sq || !exp_avg_diff || !neg_pre_grad || !workspace || n < 0 || n_segs <= 0 ||
        n_segs > ADAN_MAX_SEGS || !seg_end_host || !seg_lr_host || !seg_step_host || !(beta1 >= 0.0 && beta1 < 1.0) ||
        !(beta2 >= 0.0 && beta2 < 1.0) || !(beta3 >= 0.0 && beta3 < 1.0) || !(eps >= 0.0) || !(weight_decay >= 0.0) ||
        !(max_grad_norm >= 0.0))
        return MH_ERR_ARG;
    if ((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)exp_avg_diff |
          (uintptr_t)neg_pre_grad | (uintptr_t)workspace) & 15) != 0)
        return MH_ERR_ARG;
    AdanChunk ch[(ADAN_MAX_SEGS + ADAN_CHUNK - 1) / ADAN_CHUNK];
    int64_t prev = 0;
    for (int s = 0; s < n_segs; s++) {
        const int flag = seg_flag_host ? seg_flag_host[s] : 0;
        if (seg_end_host[s] < prev || seg_end_host[s] > n || (flag & ~(ADAN_SKIP | ADAN_FIRST)) || !(seg_lr_host[s] >= 0.0)) return MH_ERR_ARG;
        const bool host_skip = flag & ADAN_SKIP;
        if (seg_step_host[s] < (host_skip ? 0 : 1)) return MH_ERR_ARG;
        AdanChunk &c = ch[s / ADAN_CHUNK];
        const int k = s % ADAN_CHUNK;
        prev = c.end[k] = seg_end_host[s];
        const double t = (double)(seg_step_host[s] < 1 ? 1 : seg_step_host[s]), lr = seg_lr_host[s];
        c.ss[k] = (float)(lr / (1.0 - pow(beta1, t)));
        c.sd[k] = (float)(lr * beta2 / (1.0 - pow(beta2, t)));
        c.bc3s[k] = (float)sqrt(1.0 - pow(beta3, t));
        c.decay[k] = (float)(no_prox ? 1.0 - lr * weight_decay : 1.0 + lr * weight_decay);
        c.flag[k] = (uint8_t)(flag | (seg_step_host[s] == 1 ? ADAN_FIRST : 0));
    }
    if (prev != n) return MH_ERR_ARG;
    AdanWorkspace *ws = reinterpret_cast<AdanWorkspace *>(workspace);
    for (int base = 0; base < n_segs; base += ADAN_CHUNK) {
        AdanChunk &c = ch[base / ADAN_CHUNK];
        c.base = base;
        c.count = n_segs - base < ADAN_CHUNK ? n_segs - base : ADAN_CHUNK;
        hipLaunchKernelGGL(adan_table_kernel, dim3(1), dim3(ADAN_CHUNK), 0, stream, ws, c, seg_flag_dev, seg_seen_dev);
        MH_CHECK_LAUNCH();
    }
    const int64_t threads = (n + 3) / 4;
    const int64_t blocks = (threads + 255) / 256;
    if (max_grad_norm > 0.0) {
        const int nb = blocks < ADAN_NORM_BLOCKS ? (int)blocks : ADAN_NORM_BLOCKS;
        hipLaunchKernelGGL(adan_norm_kernel, dim3(nb), dim3(256), 0, stream, (const float *)grads, ws, (int)n_segs, n);
        MH_CHECK_LAUNCH();
        hipLaunchKernelGGL(adan_clip_kernel, dim3(1), dim3(256), 0, stream, ws, nb, max_grad_norm, eps);
        MH_CHECK_LAUNCH();
    }
    AdanConst k;
    k.b1 = (float)beta1, k.b2 = (float)beta2, k.b3 = (float)beta3;
    k.omb1 = (float)(1.0 - beta1), k.omb2 = (float)(1.0 - beta2), k.omb3 = (float)(1.0 - beta3);
    k.eps = (float)eps, k.no_prox = no_prox ? 1 : 0, k.write_g = max_grad_norm > 0.0 ? 1 : 0;
    hipLaunchKernelGGL(adan_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, params, grads, exp_avg, exp_avg_sq, exp_avg_diff,
                       neg_pre_grad, (const AdanWorkspace *)ws, (int)n_segs, k, n);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_adan_step(float *params, float *grads, float *exp_avg, float *exp_avg_sq, float *exp_avg_diff,
                            float *neg_pre_grad, int64_t n, int32_t n_segs, const int64_t *seg_end_host, const double *seg_lr_host,
                            const int64_t *seg_step_host, const int32_t *seg_flag_host, double beta1, double beta2, double beta3,
                            double eps, double weight_decay, double max_grad_norm, int32_t no_prox, void *workspace, void *stream) {
    if (n != 0 && !seg_flag_host) return MH_ERR_ARG;
    return adan_step(params, grads, exp_avg, exp_avg_sq, exp_avg_diff, neg_pre_grad, n, n_segs, seg_end_host, seg_lr_host,
                     seg_step_host, seg_flag_host, nullptr, nullptr, beta1, beta2, beta3, eps, weight_decay, max_grad_norm, no_prox,
                     workspace, mh_stream(stream));
}

extern "C" int mh_adan_step_dev(float *params, float *grads, float *exp_avg, float *exp_avg_sq, float *exp_avg_diff,
                                float *neg_pre_grad, int64_t n, int32_t n_segs, const int64_t *seg_end_host,
                                const double *seg_lr_host, const int64_t *seg_step_host, const float *seg_flag_dev,
                                int64_t *seg_seen_dev, double beta1, double beta2, double beta3, double eps, double weight_decay,
                                double max_grad_norm, int32_t no_prox, void *workspace, void *stream) {
    if (n != 0 && (!seg_flag_dev || !seg_seen_dev)) return MH_ERR_ARG;
    return adan_step(params, grads, exp_avg, exp_avg_sq, exp_avg_diff, neg_pre_grad, n, n_segs, seg_end_host, seg_lr_host,
                     seg_step_host, nullptr, seg_flag_dev, seg_seen_dev, beta1, beta2, beta3, eps, weight_decay, max_grad_norm,
                     no_prox, workspace, mh_stream(stream));
}
