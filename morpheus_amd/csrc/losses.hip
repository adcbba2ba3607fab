// Caller-side glue of the hot path as single launches: the per-sample means of the training losses and the "displace along a
// random direction orthogonal to the normal" step of the normal-smoothness regularisers.
//
// The reference writes these as chains of elementwise torch operators (morpheus.py:518-528 get_ortho_normal_dir, :764-777 the
// in-render perturbation losses, :1090-1145 get_regularization_loss); on this path each chain was 8-25 launches forward and as
// many backward, ~300 of the ~700 launches of a real-view training step whose own kernels take 5.5 ms.
// Every function here is the same arithmetic in fp32, one launch forward (two for a mean: block partials, then one block that
// adds them in a fixed order -- deterministic, no atomics, nothing to zero) and one backward.
#include "common.h"
#include "wave.h"

#define MEAN_BLOCKS 512
#define MEAN_THREADS 256

enum MeanKind { MK_IDENTITY = 0, MK_SQUARE = 1, MK_ABS = 2, MK_ENTROPY = 3, MK_EIKONAL = 4, MK_ABSDIFF = 5, MK_SQDIFF = 6 };

__device__ __forceinline__ float sgnf(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

// f(a[, b]) of one element and its derivative with respect to a (d f / d b = -that for the two difference kinds)
template <bool GRAD>
__device__ __forceinline__ float mean_term(int kind, float a, float b) {
    switch (kind) {
    case MK_IDENTITY: return GRAD ? 1.f : a;
    case MK_SQUARE: return GRAD ? 2.f * a : a * a;
    case MK_ABS: return GRAD ? sgnf(a) : fabsf(a);
    case MK_ABSDIFF: return GRAD ? sgnf(a - b) : fabsf(a - b);
    case MK_SQDIFF: return GRAD ? 2.f * (a - b) : (a - b) * (a - b);
    case MK_ENTROPY: {   // -x log2 x - (1 - x) log2 (1 - x), x = clamp(a, 1e-5, 1 - 1e-5)   (morpheus.py:1093-1096)
        const float lo = 1e-5f, hi = 1.0f - 1e-5f;
        const float x = fminf(fmaxf(a, lo), hi);
        if (!GRAD) return -x * log2f(x) - (1.0f - x) * log2f(1.0f - x);
        // d/dx = -log2 x + log2 (1 - x) (the two 1/ln2 terms cancel); the clamp passes the gradient on [lo, hi]
        return (a >= lo && a <= hi) ? (log2f(1.0f - x) - log2f(x)) : 0.f;
    }
    default: return 0.f;
    }
}

// partial sums [2 * MEAN_BLOCKS]: (sum of f over the valid rows, sum of the row weights)
__global__ __launch_bounds__(MEAN_THREADS) void masked_mean_partial_kernel(int kind, const float *__restrict__ a,
                                                                           const float *__restrict__ b,
                                                                           const float *__restrict__ w_row, int64_t M, int C,
                                                                           const int32_t *__restrict__ n_valid,
                                                                           float *__restrict__ ws) {
    const int64_t rows = n_valid ? min((int64_t)max(*n_valid, 0), M) : M;
    float sf = 0.f, sw = 0.f;
    const int64_t stride = (int64_t)gridDim.x * MEAN_THREADS;
    if (kind == MK_EIKONAL) {   // one value per row of [M, 3]: (|row| - 1)^2   (morpheus.py:1117-1119)
        for (int64_t r = (int64_t)blockIdx.x * MEAN_THREADS + threadIdx.x; r < rows; r += stride) {
            const float x = a[3 * r], y = a[3 * r + 1], z = a[3 * r + 2];
            const float d = sqrtf(x * x + y * y + z * z) - 1.0f;
            const float w = w_row ? w_row[r] : 1.0f;
            sf += d * d * w;
            sw += w;
        }
    } else {
        const int64_t n = rows * C;
        for (int64_t i = (int64_t)blockIdx.x * MEAN_THREADS + threadIdx.x; i < n; i += stride) {
            const float f = mean_term<false>(kind, a[i], b ? b[i] : 0.f);
            if (w_row) {
                const int64_t r = i / C;
                const float w = w_row[r];
                sf += f * w;
                if (i - r * C == 0) sw += w;
            } else {
                sf += f;
            }
        }
    }
    __shared__ float red[2][MEAN_THREADS / 64];
    sf = wave_sum(sf);
    sw = wave_sum(sw);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = sf;
        red[1][threadIdx.x >> 6] = sw;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float f = 0.f, w = 0.f;
#pragma unroll
        for (int k = 0; k < MEAN_THREADS / 64; k++) {
            f += red[0][k];
            w += red[1][k];
        }
        ws[2 * blockIdx.x] = f;
        ws[2 * blockIdx.x + 1] = w;
    }
}

// out[0] = sum / den, out[1] = den.  den = per_row * max(n_valid, 1) without row weights (the reference's .mean() over the
// samples), max(per_row * sum of the weights, 1) with them (morpheus.py:556: `.sum() / (3 * keep.sum()).clamp(min=1)`)
__global__ __launch_bounds__(MEAN_THREADS) void masked_mean_final_kernel(const float *__restrict__ ws, int n_blocks, int64_t M,
                                                                         int per_row, bool weighted,
                                                                         const int32_t *__restrict__ n_valid,
                                                                         float *__restrict__ out) {
    float sf = 0.f, sw = 0.f;
    for (int k = threadIdx.x; k < n_blocks; k += MEAN_THREADS) {
        sf += ws[2 * k];
        sw += ws[2 * k + 1];
    }
    __shared__ float red[2][MEAN_THREADS / 64];
    sf = wave_sum(sf);
    sw = wave_sum(sw);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = sf;
        red[1][threadIdx.x >> 6] = sw;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float f = 0.f, w = 0.f;
#pragma unroll
        for (int k = 0; k < MEAN_THREADS / 64; k++) {
            f += red[0][k];
            w += red[1][k];
        }
        const int64_t rows = n_valid ? min((int64_t)max(*n_valid, 0), M) : M;
        const float den = weighted ? fmaxf((float)per_row * w, 1.0f) : (float)per_row * (float)max(rows, (int64_t)1);
        out[0] = f / den;
        out[1] = den;
    }
}

// g_a[i] = g * f'(a_i) * w_row / den inside the valid rows, 0 behind them; g_b = -g_a for the difference kinds
__global__ __launch_bounds__(256) void masked_mean_bwd_kernel(int kind, const float *__restrict__ a, const float *__restrict__ b,
                                                              const float *__restrict__ w_row, int64_t M, int C,
                                                              const int32_t *__restrict__ n_valid, const float *__restrict__ out,
                                                              const float *__restrict__ g, float *__restrict__ g_a,
                                                              float *__restrict__ g_b) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * C) return;
    const int64_t rows = n_valid ? min((int64_t)max(*n_valid, 0), M) : M;
    const int64_t r = i / C;
    float v = 0.f;
    if (r < rows) {
        const float scale = *g / out[1] * (w_row ? w_row[r] : 1.0f);
        if (kind == MK_EIKONAL) {
            const float x = a[3 * r], y = a[3 * r + 1], z = a[3 * r + 2];
            const float n = sqrtf(x * x + y * y + z * z);
            v = n > 0.f ? scale * 2.0f * (n - 1.0f) * a[i] / n : 0.f;
        } else {
            v = scale * mean_term<true>(kind, a[i], b ? b[i] : 0.f);
        }
    }
    if (g_a) g_a[i] = v;
    if (g_b) g_b[i] = -v;
}

extern "C" int64_t mh_masked_mean_workspace_floats(void) { return 2 * MEAN_BLOCKS; }

static inline bool mean_args_ok(int32_t kind, const float *a, const float *b, int64_t M, int32_t C) {
    if (kind < MK_IDENTITY || kind > MK_SQDIFF || M < 0 || C <= 0 || (M > 0 && !a)) return false;
    if ((kind == MK_ABSDIFF || kind == MK_SQDIFF) && M > 0 && !b) return false;
    if (kind == MK_EIKONAL && C != 3) return false;
    return true;
}

extern "C" int mh_masked_mean_fwd(int32_t kind, const float *a, const float *b, const float *w_row, int64_t M, int32_t C,
                                  const int32_t *n_valid, float *ws, float *out, void *stream) {
    if (!mean_args_ok(kind, a, b, M, C) || !ws || !out) return MH_ERR_ARG;
    const int64_t n = kind == MK_EIKONAL ? M : M * C;
    int blocks = (int)((n + 4 * MEAN_THREADS - 1) / (4 * MEAN_THREADS));
    blocks = blocks < 1 ? 1 : (blocks > MEAN_BLOCKS ? MEAN_BLOCKS : blocks);
    hipLaunchKernelGGL(masked_mean_partial_kernel, dim3(blocks), dim3(MEAN_THREADS), 0, mh_stream(stream), (int)kind, a, b, w_row, M,
                       (int)C, n_valid, ws);
    MH_CHECK_LAUNCH();
    hipLaunchKernelGGL(masked_mean_final_kernel, dim3(1), dim3(MEAN_THREADS), 0, mh_stream(stream), (const float *)ws, blocks, M,
                       kind == MK_EIKONAL ? 1 : (int)C, w_row != nullptr, n_valid, out);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_masked_mean_bwd(int32_t kind, const float *a, const float *b, const float *w_row, int64_t M, int32_t C,
                                  const int32_t *n_valid, const float *out, const float *g, float *g_a, float *g_b, void *stream) {
    if (!mean_args_ok(kind, a, b, M, C) || !out || !g || (!g_a && !g_b)) return MH_ERR_ARG;
    if (M == 0) return MH_OK;
    hipLaunchKernelGGL(masked_mean_bwd_kernel, dim3((unsigned)((M * C + 255) / 256)), dim3(256), 0, mh_stream(stream), (int)kind, a, b,
                       w_row, M, (int)C, n_valid, out, g, g_a, g_b);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

// ---- x + scale * (cos(phi) u + sin(phi) v),  u = normalize((n^_y, -n^_x, 0)),  v = n^ x u,  n^ = normalize(n)  -------------
// (morpheus.py:518-528; torch.nn.functional.normalize divides by max(|.|, 1e-12))
struct Ortho {
    float nh[3], u[3], v[3], m, r;
};

__device__ __forceinline__ Ortho ortho_frame(const float *__restrict__ n) {
    Ortho o;
    o.m = fmaxf(sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), 1e-12f);
    o.nh[0] = n[0] / o.m;
    o.nh[1] = n[1] / o.m;
    o.nh[2] = n[2] / o.m;
    const float ur0 = o.nh[1], ur1 = -o.nh[0];
    o.r = fmaxf(sqrtf(ur0 * ur0 + ur1 * ur1), 1e-12f);
    o.u[0] = ur0 / o.r;
    o.u[1] = ur1 / o.r;
    o.u[2] = 0.f;
    o.v[0] = o.nh[1] * o.u[2] - o.nh[2] * o.u[1];
    o.v[1] = o.nh[2] * o.u[0] - o.nh[0] * o.u[2];
    o.v[2] = o.nh[0] * o.u[1] - o.nh[1] * o.u[0];
    return o;
}

__global__ __launch_bounds__(256) void ortho_perturb_kernel(const float *__restrict__ x, const float *__restrict__ n,
                                                            const float *__restrict__ phi, float scale, int64_t M,
                                                            float *__restrict__ out) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const Ortho o = ortho_frame(n + 3 * m);
    const float c = cosf(phi[m]), s = sinf(phi[m]);
#pragma unroll
    for (int d = 0; d < 3; d++) out[3 * m + d] = x[3 * m + d] + (c * o.u[d] + s * o.v[d]) * scale;
}

__global__ __launch_bounds__(256) void ortho_perturb_bwd_kernel(const float *__restrict__ n, const float *__restrict__ phi,
                                                                const float *__restrict__ g_out, float scale, int64_t M,
                                                                float *__restrict__ g_n) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const float *nn = n + 3 * m;
    const Ortho o = ortho_frame(nn);
    const float c = cosf(phi[m]), s = sinf(phi[m]);
    const float g[3] = {g_out[3 * m] * scale, g_out[3 * m + 1] * scale, g_out[3 * m + 2] * scale};   // d L / d w
    // w = c u + s (n^ x u):  dL/du = c g + s (g x n^),  dL/dn^ = s (u x g)
    float gu[3] = {c * g[0] + s * (g[1] * o.nh[2] - g[2] * o.nh[1]), c * g[1] + s * (g[2] * o.nh[0] - g[0] * o.nh[2]),
                   c * g[2] + s * (g[0] * o.nh[1] - g[1] * o.nh[0])};
    float gn[3] = {s * (o.u[1] * g[2] - o.u[2] * g[1]), s * (o.u[2] * g[0] - o.u[0] * g[2]), s * (o.u[0] * g[1] - o.u[1] * g[0])};
    // u = u_raw / max(|u_raw|, eps), u_raw = (n^_y, -n^_x, 0 * n^_z)
    const float ur0 = o.nh[1], ur1 = -o.nh[0];
    float gur0, gur1;
    if (sqrtf(ur0 * ur0 + ur1 * ur1) > 1e-12f) {
        const float dot = o.u[0] * gu[0] + o.u[1] * gu[1];
        gur0 = (gu[0] - o.u[0] * dot) / o.r;
        gur1 = (gu[1] - o.u[1] * dot) / o.r;
    } else {
        gur0 = gu[0] / o.r;
        gur1 = gu[1] / o.r;
    }
    gn[1] += gur0;
    gn[0] -= gur1;
    // n^ = n / max(|n|, eps)
    if (sqrtf(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]) > 1e-12f) {
        const float dot = o.nh[0] * gn[0] + o.nh[1] * gn[1] + o.nh[2] * gn[2];
#pragma unroll
        for (int d = 0; d < 3; d++) g_n[3 * m + d] = (gn[d] - o.nh[d] * dot) / o.m;
    } else {
#pragma unroll
        for (int d = 0; d < 3; d++) g_n[3 * m + d] = gn[d] / o.m;
    }
}

extern "C" int mh_ortho_perturb_fwd(const float *x, const float *n, const float *phi, float scale, int64_t M, float *out,
                                    void *stream) {
    if (M == 0) return MH_OK;
    if (M < 0 || !x || !n || !phi || !out) return MH_ERR_ARG;
    hipLaunchKernelGGL(ortho_perturb_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, mh_stream(stream), x, n, phi, scale, M, out);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_ortho_perturb_bwd(const float *n, const float *phi, const float *g_out, float scale, int64_t M, float *g_n,
                                    void *stream) {
    if (M == 0) return MH_OK;
    if (M < 0 || !n || !phi || !g_out || !g_n) return MH_ERR_ARG;
    hipLaunchKernelGGL(ortho_perturb_bwd_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, mh_stream(stream), n, phi, g_out, scale,
                       M, g_n);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

// ---- per-frame pose correction of a batch of rays: o' = o + t_f, d' = R(a, b, g)_f d  (models/pose.py:4-64, model.py:335-346) ------
// The batch is B rows of n rays, one frame per row.  As torch operators this is ~60 launches forward (six
// sin/cos, twenty products, four stacks, two gathers) and ~100 backward for 3 x 3 numbers per frame; here: one launch forward,
// two backward (per-block partial sums of dL/dR = sum_rays g_d' d^T and dL/dt = sum_rays g_o', then one block that adds them in a
// fixed order, applies dR/d(angles) and adds the rows' results into the zeroed [F,6] gradient: deterministic, no atomics).
#define POSE_RAYS_PER_BLOCK 1024

struct PoseR {
    float r[3][3];
};

__device__ __forceinline__ PoseR pose_matrix(float a, float b, float g) {
    const float ca = cosf(a), cb = cosf(b), cg = cosf(g), sa = sinf(a), sb = sinf(b), sg = sinf(g);
    // every product and sum rounded on its own, left to right (this file is compiled with -ffp-contract=off, morpheus_amd/build.py:
    // HIP's __fmul_rn / __fadd_rn are plain operators the compiler would otherwise fuse): the values the reference's operator chain
    // (models/pose.py:44-53) produces -- a one-ulp difference in R moves sample positions enough to show in SDF values next to 0
    PoseR m;
    const float casb = __fmul_rn(ca, sb), sasb = __fmul_rn(sa, sb);
    m.r[0][0] = __fmul_rn(ca, cb);  m.r[1][0] = __fmul_rn(sa, cb);  m.r[2][0] = -sb;
    m.r[0][1] = __fsub_rn(__fmul_rn(casb, sg), __fmul_rn(sa, cg));
    m.r[1][1] = __fadd_rn(__fmul_rn(sasb, sg), __fmul_rn(ca, cg));
    m.r[2][1] = __fmul_rn(cb, sg);
    m.r[0][2] = __fadd_rn(__fmul_rn(casb, cg), __fmul_rn(sa, sg));
    m.r[1][2] = __fsub_rn(__fmul_rn(sasb, cg), __fmul_rn(ca, sg));
    m.r[2][2] = __fmul_rn(cb, cg);
    return m;
}

__global__ __launch_bounds__(256) void pose_apply_kernel(const float *__restrict__ o, const float *__restrict__ d,
                                                         const float *__restrict__ pose, const int64_t *__restrict__ frame_of_row,
                                                         int64_t n_per_row, int64_t N, float *__restrict__ o_out,
                                                         float *__restrict__ d_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float *p = pose + 6 * frame_of_row[i / n_per_row];
    const PoseR m = pose_matrix(p[0], p[1], p[2]);
    const float x = d[3 * i], y = d[3 * i + 1], z = d[3 * i + 2];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        o_out[3 * i + r] = o[3 * i + r] + p[3 + r];
        // (rays_d[..., None, :] * R).sum(-1) (model.py:346): three rounded products, added in the order PyTorch's reduction over a
        // length-3 axis adds them on this device ((p0 + p2) + p1; tools/gpu/pose_probe.py) -- bit for bit the operator chain
        d_out[3 * i + r] = __fadd_rn(__fadd_rn(__fmul_rn(x, m.r[r][0]), __fmul_rn(z, m.r[r][2])), __fmul_rn(y, m.r[r][1]));
    }
}

// ws[(row * blocks_per_row + blk) * 12 + k]: k < 9 -> sum g_d'[r] * d[c] (k = 3 r + c), k >= 9 -> sum g_o'[k - 9]
__global__ __launch_bounds__(256) void pose_bwd_partial_kernel(const float *__restrict__ d, const float *__restrict__ g_o,
                                                               const float *__restrict__ g_d, int64_t n_per_row,
                                                               int blocks_per_row, float *__restrict__ ws) {
    const int row = blockIdx.y, blk = blockIdx.x;
    float acc[12];
#pragma unroll
    for (int k = 0; k < 12; k++) acc[k] = 0.f;
    const int64_t lo = (int64_t)blk * POSE_RAYS_PER_BLOCK, hi = min(lo + POSE_RAYS_PER_BLOCK, n_per_row);
    for (int64_t j = lo + threadIdx.x; j < hi; j += 256) {
        const int64_t i = (int64_t)row * n_per_row + j;
        const float x = d[3 * i], y = d[3 * i + 1], z = d[3 * i + 2];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const float gd = g_d ? g_d[3 * i + r] : 0.f;
            acc[3 * r] += gd * x;
            acc[3 * r + 1] += gd * y;
            acc[3 * r + 2] += gd * z;
            acc[9 + r] += g_o ? g_o[3 * i + r] : 0.f;
        }
    }
    __shared__ float red[4][12];
#pragma unroll
    for (int k = 0; k < 12; k++) {
        acc[k] = wave_sum(acc[k]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < 12)
        ws[((int64_t)row * blocks_per_row + blk) * 12 + threadIdx.x] =
            red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

__global__ __launch_bounds__(256) void pose_bwd_final_kernel(const float *__restrict__ ws, const float *__restrict__ pose,
                                                             const int64_t *__restrict__ frame_of_row, int B, int blocks_per_row,
                                                             int64_t n_frames, float *__restrict__ g_pose) {
    for (int64_t i = threadIdx.x; i < n_frames * 6; i += 256) g_pose[i] = 0.f;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int row = 0; row < B; row++) {                     // rows of the same frame add up in row order
        float s[12];
        for (int k = 0; k < 12; k++) {
            float t = 0.f;
            for (int blk = 0; blk < blocks_per_row; blk++) t += ws[((int64_t)row * blocks_per_row + blk) * 12 + k];
            s[k] = t;
        }
        const int64_t f = frame_of_row[row];
        const float *p = pose + 6 * f;
        const float ca = cosf(p[0]), cb = cosf(p[1]), cg = cosf(p[2]), sa = sinf(p[0]), sb = sinf(p[1]), sg = sinf(p[2]);
        // dR/da, dR/db, dR/dg of pose_matrix, contracted with G = s[3 r + c]
        const float Ga = s[0] * (-sa * cb) + s[3] * (ca * cb) + s[1] * (-sa * sb * sg - ca * cg) + s[4] * (ca * sb * sg - sa * cg) +
                         s[2] * (-sa * sb * cg + ca * sg) + s[5] * (ca * sb * cg + sa * sg);
        const float Gb = s[0] * (-ca * sb) + s[3] * (-sa * sb) + s[6] * (-cb) + s[1] * (ca * cb * sg) + s[4] * (sa * cb * sg) +
                         s[7] * (-sb * sg) + s[2] * (ca * cb * cg) + s[5] * (sa * cb * cg) + s[8] * (-sb * cg);
        const float Gg = s[1] * (ca * sb * cg + sa * sg) + s[4] * (sa * sb * cg - ca * sg) + s[7] * (cb * cg) +
                         s[2] * (-ca * sb * sg + sa * cg) + s[5] * (-sa * sb * sg - ca * cg) + s[8] * (-cb * sg);
        g_pose[6 * f + 0] += Ga;
        g_pose[6 * f + 1] += Gb;
        g_pose[6 * f + 2] += Gg;
        g_pose[6 * f + 3] += s[9];
        g_pose[6 * f + 4] += s[10];
        g_pose[6 * f + 5] += s[11];
    }
}

static inline int pose_blocks_per_row(int64_t n_per_row) { return (int)((n_per_row + POSE_RAYS_PER_BLOCK - 1) / POSE_RAYS_PER_BLOCK); }

extern "C" int64_t mh_pose_bwd_workspace_floats(int64_t B, int64_t n_per_row) { return B * pose_blocks_per_row(n_per_row) * 12; }

extern "C" int mh_pose_apply_fwd(const float *rays_o, const float *rays_d, const float *pose, const int64_t *frame_of_row, int64_t B,
                                 int64_t n_per_row, float *o_out, float *d_out, void *stream) {
    const int64_t N = B * n_per_row;
    if (N == 0) return MH_OK;
    if (B < 0 || n_per_row < 0 || !rays_o || !rays_d || !pose || !frame_of_row || !o_out || !d_out) return MH_ERR_ARG;
    hipLaunchKernelGGL(pose_apply_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, mh_stream(stream), rays_o, rays_d, pose,
                       frame_of_row, n_per_row, N, o_out, d_out);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_pose_apply_bwd(const float *rays_d, const float *pose, const int64_t *frame_of_row, int64_t B, int64_t n_per_row,
                                 int64_t n_frames, const float *g_o, const float *g_d, float *ws, float *g_pose, void *stream) {
    if (B < 0 || n_per_row < 0 || n_frames <= 0 || B > 65535 || !pose || !frame_of_row || !ws || !g_pose || (B * n_per_row > 0 && !rays_d))
        return MH_ERR_ARG;
    const int bpr = pose_blocks_per_row(n_per_row);
    if (B * n_per_row > 0) {
        hipLaunchKernelGGL(pose_bwd_partial_kernel, dim3(bpr, (unsigned)B), dim3(256), 0, mh_stream(stream), rays_d, g_o, g_d, n_per_row,
                           bpr, ws);
        MH_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(pose_bwd_final_kernel, dim3(1), dim3(256), 0, mh_stream(stream), (const float *)ws, pose, frame_of_row,
                       (int)(B * n_per_row > 0 ? B : 0), bpr, n_frames, g_pose);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

// ---- the real-view render loss (morpheus.py:930-983: get_gt_from_data + get_real_view_render_loss) as one launch each way ---------
// Per ray: m = mask > 0.5; gt_rgb = image * m + bg * (1 - m); valid = depth > 0 and |o + depth d| <= 1.1 and m;
//   rgb   = mean over rays and channels of (pred_rgb - gt_rgb)^2
//   mask  = mean of -(m log p + (1 - m) log (1 - p)),  p = clip(opacity, 1e-5, 1 - 1e-5)
//   depth = mean of (valid (pred_depth - depth))^2
// out[0] = w_rgb rgb + w_mask mask + w_depth depth, out[1..3] = the three terms; gt_rgb [3,N] (channel-major, the layout the
// caller's [B,3,H,W] view has) and valid [N] go back to the caller for the surface-point loss (:1001-1026).
// ONE workgroup of 1024 threads walks the rays (a training batch is a few thousand rays): deterministic, nothing to zero.
struct RenderLossW {
    float rgb, mask, depth;
};

__global__ __launch_bounds__(1024) void render_loss_kernel(const float *__restrict__ pred_rgb /*[N,3]*/,
                                                           const float *__restrict__ pred_depth, const float *__restrict__ opacity,
                                                           const float *__restrict__ image /*[3,N]*/, const float *__restrict__ depth,
                                                           const float *__restrict__ mask, const float *__restrict__ bg /*[N,3]*/,
                                                           const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                           int64_t N, RenderLossW w, float *__restrict__ gt_rgb /*[3,N]*/,
                                                           float *__restrict__ valid, float *__restrict__ out /*[4]*/) {
    float s_rgb = 0.f, s_mask = 0.f, s_depth = 0.f;
    for (int64_t i = threadIdx.x; i < N; i += 1024) {
        const float m = mask[i] > 0.5f ? 1.0f : 0.0f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float g = image[c * N + i] * m + bg[3 * i + c] * (1.0f - m);
            gt_rgb[c * N + i] = g;
            const float d = pred_rgb[3 * i + c] - g;
            s_rgb += d * d;
        }
        const float p = fminf(fmaxf(opacity[i], 1e-5f), 1.0f - 1e-5f);
        s_mask -= m * logf(p) + (1.0f - m) * logf(1.0f - p);
        const float gd = depth[i];
        const float x = rays_o[3 * i] + gd * rays_d[3 * i], y = rays_o[3 * i + 1] + gd * rays_d[3 * i + 1],
                    z = rays_o[3 * i + 2] + gd * rays_d[3 * i + 2];
        const float v = (gd > 0.f && sqrtf(x * x + y * y + z * z) <= 1.1f && m > 0.5f) ? 1.0f : 0.0f;
        valid[i] = v;
        const float dd = pred_depth[i] * v - gd * v;
        s_depth += dd * dd;
    }
    __shared__ float red[3][16];
    s_rgb = wave_sum(s_rgb);
    s_mask = wave_sum(s_mask);
    s_depth = wave_sum(s_depth);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = s_rgb;
        red[1][threadIdx.x >> 6] = s_mask;
        red[2][threadIdx.x >> 6] = s_depth;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f, b = 0.f, c = 0.f;
        for (int k = 0; k < 16; k++) {
            a += red[0][k];
            b += red[1][k];
            c += red[2][k];
        }
        const float n = (float)(N > 0 ? N : 1);
        a /= 3.0f * n;
        b /= n;
        c /= n;
        out[0] = w.rgb * a + w.mask * b + w.depth * c;
        out[1] = a;
        out[2] = b;
        out[3] = c;
    }
}

__global__ __launch_bounds__(256) void render_loss_bwd_kernel(const float *__restrict__ pred_rgb, const float *__restrict__ pred_depth,
                                                              const float *__restrict__ opacity, const float *__restrict__ gt_rgb,
                                                              const float *__restrict__ depth, const float *__restrict__ mask,
                                                              const float *__restrict__ valid, int64_t N, RenderLossW w,
                                                              const float *__restrict__ g, float *__restrict__ g_rgb,
                                                              float *__restrict__ g_depth, float *__restrict__ g_opacity) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float gg = *g, n = (float)N;
    if (g_rgb) {
#pragma unroll
        for (int c = 0; c < 3; c++) g_rgb[3 * i + c] = gg * w.rgb * 2.0f * (pred_rgb[3 * i + c] - gt_rgb[c * N + i]) / (3.0f * n);
    }
    if (g_depth) {
        const float v = valid[i];
        g_depth[i] = gg * w.depth * 2.0f * (pred_depth[i] * v - depth[i] * v) * v / n;
    }
    if (g_opacity) {
        const float o = opacity[i], m = mask[i] > 0.5f ? 1.0f : 0.0f;
        const float p = fminf(fmaxf(o, 1e-5f), 1.0f - 1e-5f);
        g_opacity[i] = (o >= 1e-5f && o <= 1.0f - 1e-5f) ? gg * w.mask * (-(m / p) + (1.0f - m) / (1.0f - p)) / n : 0.f;
    }
}

extern "C" int mh_render_loss_fwd(const float *pred_rgb, const float *pred_depth, const float *opacity, const float *image,
                                  const float *depth, const float *mask, const float *bg, const float *rays_o, const float *rays_d,
                                  int64_t N, float w_rgb, float w_mask, float w_depth, float *gt_rgb, float *valid, float *out,
                                  void *stream) {
    if (N < 0 || !out || (N > 0 && (!pred_rgb || !pred_depth || !opacity || !image || !depth || !mask || !bg || !rays_o || !rays_d ||
                                    !gt_rgb || !valid)))
        return MH_ERR_ARG;
    RenderLossW w = {w_rgb, w_mask, w_depth};
    hipLaunchKernelGGL(render_loss_kernel, dim3(1), dim3(1024), 0, mh_stream(stream), pred_rgb, pred_depth, opacity, image, depth, mask,
                       bg, rays_o, rays_d, N, w, gt_rgb, valid, out);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_render_loss_bwd(const float *pred_rgb, const float *pred_depth, const float *opacity, const float *gt_rgb,
                                  const float *depth, const float *mask, const float *valid, int64_t N, float w_rgb, float w_mask,
                                  float w_depth, const float *g, float *g_rgb, float *g_depth, float *g_opacity, void *stream) {
    if (N == 0) return MH_OK;
    if (N < 0 || !pred_rgb || !pred_depth || !opacity || !gt_rgb || !depth || !mask || !valid || !g) return MH_ERR_ARG;
    RenderLossW w = {w_rgb, w_mask, w_depth};
    hipLaunchKernelGGL(render_loss_bwd_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, mh_stream(stream), pred_rgb, pred_depth,
                       opacity, gt_rgb, depth, mask, valid, N, w, g, g_rgb, g_depth, g_opacity);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

// ---- the points of get_normal_smoothness_loss (morpheus.py:530-547) and the background blend of render_rays (:686-694) -------------
// Round 6: what was left of the reference's operator chains inside the boundary.  Both are the chain's arithmetic operator for
// operator (this file is compiled without FMA contraction): every product and sum rounded on its own, in the chain's order.
//   pts[k, n, :] = (depth[n] + off[k]) * d[n, :] + o[n, :]     keep[k, n] = |pts| < 1.1        (12 torch launches forward, 8 back)
__global__ __launch_bounds__(256) void smooth_points_kernel(const float *__restrict__ depth, const float *__restrict__ off,
                                                            const float *__restrict__ o, const float *__restrict__ d, int64_t N, int K,
                                                            float *__restrict__ pts, float *__restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N * K) return;
    const int64_t n = i % N;
    const int k = (int)(i / N);
    const float t = depth[n] + off[k];
    const float x = t * d[3 * n] + o[3 * n], y = t * d[3 * n + 1] + o[3 * n + 1], z = t * d[3 * n + 2] + o[3 * n + 2];
    pts[3 * i] = x;
    pts[3 * i + 1] = y;
    pts[3 * i + 2] = z;
    keep[i] = sqrtf(x * x + y * y + z * z) < 1.1f ? 1.0f : 0.0f;
}

// g_depth[n] = sum_k g[k, n, :] . d[n, :];  g_o[n, :] = sum_k g[k, n, :];  g_d[n, :] = sum_k g[k, n, :] (depth[n] + off[k]) -- one lane per
// ray, the K points added in index order (deterministic)
__global__ __launch_bounds__(256) void smooth_points_bwd_kernel(const float *__restrict__ g, const float *__restrict__ depth,
                                                                const float *__restrict__ off, const float *__restrict__ d, int64_t N,
                                                                int K, float *__restrict__ g_depth, float *__restrict__ g_o,
                                                                float *__restrict__ g_d) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float s[3] = {0.f, 0.f, 0.f}, st[3] = {0.f, 0.f, 0.f};
    const float dn = depth[n];
    for (int k = 0; k < K; k++) {
        const float t = dn + off[k];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float gv = g[3 * ((int64_t)k * N + n) + c];
            s[c] += gv;
            st[c] += gv * t;
        }
    }
    if (g_depth) g_depth[n] = s[0] * d[3 * n] + s[1] * d[3 * n + 1] + s[2] * d[3 * n + 2];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (g_o) g_o[3 * n + c] = s[c];
        if (g_d) g_d[3 * n + c] = st[c];
    }
}

extern "C" int mh_smooth_points_fwd(const float *depth, const float *off, const float *rays_o, const float *rays_d, int64_t N, int32_t K,
                                    float *pts, float *keep, void *stream) {
    if (N == 0 || K == 0) return MH_OK;
    if (N < 0 || K < 0 || !depth || !off || !rays_o || !rays_d || !pts || !keep || N * K > 0x7fffffffLL * 256) return MH_ERR_ARG;
    hipLaunchKernelGGL(smooth_points_kernel, dim3((unsigned)((N * K + 255) / 256)), dim3(256), 0, mh_stream(stream), depth, off, rays_o,
                       rays_d, N, (int)K, pts, keep);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_smooth_points_bwd(const float *g_pts, const float *depth, const float *off, const float *rays_d, int64_t N, int32_t K,
                                    float *g_depth, float *g_o, float *g_d, void *stream) {
    if (N == 0) return MH_OK;
    if (N < 0 || K < 0 || !g_pts || !depth || !off || !rays_d) return MH_ERR_ARG;
    hipLaunchKernelGGL(smooth_points_bwd_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, mh_stream(stream), g_pts, depth, off,
                       rays_d, N, (int)K, g_depth, g_o, g_d);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

//   image = color + (1 - opacity) * bg          (3 torch launches forward, 4 back)
__global__ __launch_bounds__(256) void bg_blend_kernel(const float *__restrict__ color, const float *__restrict__ opacity,
                                                       const float *__restrict__ bg, int64_t N, float *__restrict__ image) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float t = 1.0f - opacity[n];
#pragma unroll
    for (int c = 0; c < 3; c++) image[3 * n + c] = color[3 * n + c] + t * bg[3 * n + c];
}

// g_color = g_image (no launch);  g_opacity[n] = -sum_c g_image[n, c] bg[n, c];  g_bg = (1 - opacity) g_image (NULL: not wanted)
__global__ __launch_bounds__(256) void bg_blend_bwd_kernel(const float *__restrict__ g_image, const float *__restrict__ opacity,
                                                           const float *__restrict__ bg, int64_t N, float *__restrict__ g_opacity,
                                                           float *__restrict__ g_bg) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float g0 = g_image[3 * n], g1 = g_image[3 * n + 1], g2 = g_image[3 * n + 2];
    if (g_opacity) g_opacity[n] = -((g0 * bg[3 * n] + g1 * bg[3 * n + 1]) + g2 * bg[3 * n + 2]);
    if (g_bg) {
        const float t = 1.0f - opacity[n];
        g_bg[3 * n] = t * g0;
        g_bg[3 * n + 1] = t * g1;
        g_bg[3 * n + 2] = t * g2;
    }
}

extern "C" int mh_bg_blend_fwd(const float *color, const float *opacity, const float *bg, int64_t N, float *image, void *stream) {
    if (N == 0) return MH_OK;
    if (N < 0 || !color || !opacity || !bg || !image) return MH_ERR_ARG;
    hipLaunchKernelGGL(bg_blend_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, mh_stream(stream), color, opacity, bg, N, image);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_bg_blend_bwd(const float *g_image, const float *opacity, const float *bg, int64_t N, float *g_opacity, float *g_bg,
                               void *stream) {
    if (N == 0) return MH_OK;
    if (N < 0 || !g_image || !opacity || !bg) return MH_ERR_ARG;
    hipLaunchKernelGGL(bg_blend_bwd_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, mh_stream(stream), g_image, opacity, bg, N,
                       g_opacity, g_bg);
    MH_CHECK_LAUNCH();
    return MH_OK;
}
