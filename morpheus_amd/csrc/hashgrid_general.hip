// The multiresolution grid encoder in full: every switch of the reference operator that hashgrid.hip's one instantiation
// (C = 2, hash, linear, align_corners = False) leaves out, plus its two regularisers.
//
// Semantics: reference external/encoders/gridencoder/src/gridencoder.cu
//   smoothstep :35-42, fast_hash :45-58, get_grid_index :61-79, kernel_grid :83-249, kernel_grid_backward :253-349,
//   kernel_input_backward :353-378, kernel_grad_tv :526-631, kernel_grad_wd :671-703; host logic grid.py:28-96, :157, :173-206.
// D = 3; C in {1, 2, 4, 8}; gridtype 0 hash / 1 tiled; align_corners 0 / 1; interp 0 linear / 1 smoothstep.
//
// Shape: one lane per point, one LEVEL per wave (blockIdx.y, or a wave-uniform loop in the d/dx kernel), so that the level's
// resolution, table size, index strides and table offset are scalars; a table row is one C-wide vector load (16 bytes at most
// per instruction) whenever the buffers are aligned for it.  The backward recomputes cells and weights, as hashgrid.hip does.
// Every sum into a table-shaped buffer (table gradient, total variation) goes through 64-bit fixed point: integer adds commute,
// so the result is the same from run to run whatever order the waves arrive in, which float atomics cannot give.
// This is the plain path: no brick staging.  The default configuration keeps hashgrid.hip's kernels.
// The cell rule (grid_locate), the level table's validation (grid_fill_meta) and the fixed-point rule (fx_scales, fx_quantize, the
// absmax and finalize kernels) are grid.h's, shared with hashgrid.hip; the row index of every grid type (gg_row) is this file's.
#include "common.h"
#include "wave.h"
#include "grid.h"
#include <algorithm>
#include <cmath>

// what is written is what runs: the explicit fmaf calls below are the single-rounding operations oracle/hashgrid.c makes
// (`+= w * value`, as nvcc -fmad=true fuses it), nothing else is contracted, so the fp32 restatement of the tests
// (tests/grid_general_oracle.py) takes the same cells as these kernels
#pragma clang fp contract(off)

struct GGMeta : GridMeta {
    uint32_t my[MH_MAX_LEVELS], mz[MH_MAX_LEVELS];   // get_grid_index's strides of y and z; 0 where its loop stopped before the axis
    int32_t hashed[MH_MAX_LEVELS];                   // gridtype == 0 and the running stride outgrew the table
};

struct GGLevel {
    uint32_t res, T, my, mz, off;
    bool hashed, pow2;
};

__device__ __forceinline__ GGLevel gg_level(const GGMeta &m, int l) {
    GGLevel v;
    v.res = (uint32_t)m.res[l];
    v.off = (uint32_t)m.offsets[l];
    v.T = (uint32_t)(m.offsets[l + 1] - m.offsets[l]);
    v.my = m.my[l], v.mz = m.mz[l];
    v.hashed = m.hashed[l] != 0;
    v.pow2 = (v.T & (v.T - 1)) == 0;
    return v;
}

// get_grid_index (gridencoder.cu:61-79) without its channel term: the partial sum over the axes the stride loop accepted, replaced
// by the xor hash on a hashed level, modulo the table size in both cases.  Coordinates may exceed res - 1 (total variation's right
// neighbour): nothing here assumes otherwise.
__device__ __forceinline__ uint32_t gg_row(uint32_t cx, uint32_t cy, uint32_t cz, const GGLevel &v) {
    const uint32_t idx = v.hashed ? (cx ^ (cy * 2654435761u) ^ (cz * 805459861u)) : (cx + cy * v.my + cz * v.mz);
    return v.pow2 ? (idx & (v.T - 1)) : (idx % v.T);
}

__device__ __forceinline__ float gg_smoothstep(float v) { return v * v * (3.0f - 2.0f * v); }
__device__ __forceinline__ float gg_smoothstep_d(float v) { return 6.0f * v * (1.0f - v); }

// C consecutive floats as one vector access where the buffer is aligned for it (VEC), 16 bytes per instruction at most
template <int C, bool VEC>
__device__ __forceinline__ void gg_load(const float *__restrict__ p, float (&v)[C]) {
    if constexpr (VEC && C == 2) {
        const float2 t = *reinterpret_cast<const float2 *>(p);
        v[0] = t.x, v[1] = t.y;
    } else if constexpr (VEC && C >= 4) {
#pragma unroll
        for (int k = 0; k < C; k += 4) {
            const f32x4 t = *reinterpret_cast<const f32x4 *>(p + k);
            v[k] = t[0], v[k + 1] = t[1], v[k + 2] = t[2], v[k + 3] = t[3];
        }
    } else {
#pragma unroll
        for (int k = 0; k < C; k++) v[k] = p[k];
    }
}

template <int C, bool VEC>
__device__ __forceinline__ void gg_store(float *__restrict__ p, const float (&v)[C]) {
    if constexpr (VEC && C == 2) {
        *reinterpret_cast<float2 *>(p) = make_float2(v[0], v[1]);
    } else if constexpr (VEC && C >= 4) {
#pragma unroll
        for (int k = 0; k < C; k += 4) {
            f32x4 t;
            t[0] = v[k], t[1] = v[k + 1], t[2] = v[k + 2], t[3] = v[k + 3];
            *reinterpret_cast<f32x4 *>(p + k) = t;
        }
    } else {
#pragma unroll
        for (int k = 0; k < C; k++) p[k] = v[k];
    }
}

// the eight corner rows (corner c: bit d -> axis d at g + 1, clamped to res - 1, gridencoder.cu:182) and weights (:171-184)
__device__ __forceinline__ void gg_corners(const uint32_t (&g)[3], const float (&f)[3], const GGLevel &lv, uint32_t (&row)[8],
                                           float (&w)[8]) {
    const uint32_t g1[3] = {min(g[0] + 1, lv.res - 1), min(g[1] + 1, lv.res - 1), min(g[2] + 1, lv.res - 1)};
#pragma unroll
    for (int c = 0; c < 8; c++) {
        row[c] = gg_row((c & 1) ? g1[0] : g[0], (c & 2) ? g1[1] : g[1], (c & 4) ? g1[2] : g[2], lv);
        w[c] = ((c & 1) ? f[0] : 1.f - f[0]) * ((c & 2) ? f[1] : 1.f - f[1]) * ((c & 4) ? f[2] : 1.f - f[2]);
    }
}

template <int C, bool VEC>
__global__ __launch_bounds__(256) void gg_fwd_kernel(const float *__restrict__ x, const float *__restrict__ emb, GGMeta meta,
                                                     float *__restrict__ out, int64_t M, int L, int n_levels, int align, int interp,
                                                     float bound, float two_bound) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int l = blockIdx.y;
    if (p >= M) return;
    float r[C];
#pragma unroll
    for (int k = 0; k < C; k++) r[k] = 0.f;
    if (l < n_levels) {
        const GGLevel lv = gg_level(meta, l);
        uint32_t g[3];
        float f[3];
        if (grid_locate(x, p, bound, two_bound, lv.res, g, f, align)) {
            if (interp) {
#pragma unroll
                for (int d = 0; d < 3; d++) f[d] = gg_smoothstep(f[d]);
            }
            uint32_t row[8];
            float w[8];
            gg_corners(g, f, lv, row, w);
            const float *tab = emb + (size_t)lv.off * C;
            float v[8][C];
#pragma unroll
            for (int c = 0; c < 8; c++) gg_load<C, VEC>(tab + (size_t)row[c] * C, v[c]);
#pragma unroll
            for (int c = 0; c < 8; c++)
#pragma unroll
                for (int k = 0; k < C; k++) r[k] = fmaf(w[c], v[c][k], r[k]);
        }
    }
    gg_store<C, VEC>(out + (p * L + l) * C, r);
}

// ---- table gradient: 64-bit fixed point ----------------------------------------------------------------------------------------
// A term w * g is rounded ONCE onto the grid 2^-(40 - shift) G, G the power of two above max |grad| (grid.h), from the exact double
// product; the integer sums are exact and order-independent; one conversion to fp32 per table entry (grid_acc_finalize_kernel).
template <int C, bool VEC>
__global__ __launch_bounds__(256) void gg_bwd_emb_kernel(const float *__restrict__ grad, const float *__restrict__ x, GGMeta meta,
                                                         long long *__restrict__ acc, int acc_shift, int64_t M, int L, int align,
                                                         int interp, float bound, float two_bound,
                                                         const uint32_t *__restrict__ gmax_bits) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int l = blockIdx.y;            // < n_levels: the launch has no other rows
    if (p >= M) return;
    const GGLevel lv = gg_level(meta, l);
    uint32_t g[3];
    float f[3];
    if (!grid_locate(x, p, bound, two_bound, lv.res, g, f, align)) return;     // gridencoder.cu:279-284
    if (interp) {
#pragma unroll
        for (int d = 0; d < 3; d++) f[d] = gg_smoothstep(f[d]);                 // :301-304
    }
    float to_fx, from_fx;
    fx_scales(*gmax_bits, to_fx, from_fx);
    to_fx = ldexpf(to_fx, -acc_shift);
    const float lim = ldexpf(FX_LIMIT, -acc_shift);
    float gr[C];
    gg_load<C, VEC>(grad + (p * L + l) * C, gr);
    double gd[C];
#pragma unroll
    for (int k = 0; k < C; k++) gd[k] = (double)gr[k] * (double)to_fx;          // exact: a power-of-two scale
    uint32_t row[8];
    float w[8];
    gg_corners(g, f, lv, row, w);
    unsigned long long *a = reinterpret_cast<unsigned long long *>(acc) + (size_t)lv.off * C;
#pragma unroll
    for (int c = 0; c < 8; c++)
#pragma unroll
        for (int k = 0; k < C; k++)
            atomicAdd(a + (size_t)row[c] * C + k, (unsigned long long)fx_quantize((double)w[c] * gd[k], lim));
}

// ---- d(loss)/dx -----------------------------------------------------------------------------------------------------------------
// One lane per point walks the levels (wave-uniform loop): dy_dx of a level (gridencoder.cu:205-247) per axis and channel, in the
// reference's order -- w = scale, times the weights of the other two axes, times (right - left), times the interpolation's derivative
// factor, summed over the four corner pairs -- then contracted with the level's gradient in kernel_input_backward's order (:353-378:
// levels ascending, channels ascending, one running sum per axis).  The border clamp is ignored, as the reference ignores it.
template <int C, bool VEC>
__global__ __launch_bounds__(256) void gg_bwd_dx_kernel(const float *__restrict__ grad, const float *__restrict__ x,
                                                        const float *__restrict__ emb, GGMeta meta, float *__restrict__ grad_x,
                                                        int64_t M, int L, int n_levels, int align, int interp, float bound,
                                                        float two_bound) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= M) return;
    float res3[3] = {0.f, 0.f, 0.f};
    for (int l = 0; l < n_levels; l++) {
        const GGLevel lv = gg_level(meta, l);
        uint32_t g[3];
        float f[3], df[3] = {1.f, 1.f, 1.f};
        if (!grid_locate(x, p, bound, two_bound, lv.res, g, f, align)) break;      // outside at one level = outside at all: zero
        if (interp) {
#pragma unroll
            for (int d = 0; d < 3; d++) df[d] = gg_smoothstep_d(f[d]), f[d] = gg_smoothstep(f[d]);
        }
        const uint32_t g1[3] = {min(g[0] + 1, lv.res - 1), min(g[1] + 1, lv.res - 1), min(g[2] + 1, lv.res - 1)};
        const float *tab = emb + (size_t)lv.off * C;
        float v[8][C];
#pragma unroll
        for (int c = 0; c < 8; c++)
            gg_load<C, VEC>(tab + (size_t)gg_row((c & 1) ? g1[0] : g[0], (c & 2) ? g1[1] : g[1], (c & 4) ? g1[2] : g[2], lv) * C, v[c]);
        float gr[C];
        gg_load<C, VEC>(grad + (p * L + l) * C, gr);
        const float scale = (float)(align ? lv.res - 1 : lv.res);
#pragma unroll
        for (int gd = 0; gd < 3; gd++) {
            float dy[C];
#pragma unroll
            for (int k = 0; k < C; k++) dy[k] = 0.f;
#pragma unroll
            for (int idx = 0; idx < 4; idx++) {
                float w = scale;
                int lo_c = 0;
#pragma unroll
                for (int nd = 0; nd < 2; nd++) {
                    const int d = (nd >= gd) ? nd + 1 : nd;
                    const bool up = (idx >> nd) & 1;
                    w *= up ? f[d] : 1.f - f[d];
                    lo_c |= up ? (1 << d) : 0;
                }
                const int hi_c = lo_c | (1 << gd);
#pragma unroll
                for (int k = 0; k < C; k++) dy[k] += w * (v[hi_c][k] - v[lo_c][k]) * df[gd];
            }
#pragma unroll
            for (int k = 0; k < C; k++) res3[gd] += gr[k] * dy[k];
        }
    }
    const float inv = 1.0f / two_bound;       // chain factor of u = (x + bound) / (2 bound), applied once per point
#pragma unroll
    for (int d = 0; d < 3; d++) grad_x[p * 3 + d] = res3[d] * inv;
}

// ---- total variation (gridencoder.cu:526-631) -----------------------------------------------------------------------------------
// Per (point, level): the cell's row against its right neighbour at g + 1 on every axis (ALWAYS: :595 tests cur_d < resolution, which
// holds for every cell; the coordinate may equal res and goes through the index unclamped) and its left neighbour at g - 1 where
// g > 0; per channel r = sum (v - v_nb), q = sum (v - v_nb)^2, addend (weight / 6) r / sqrt(q + 1e-9) to the cell's row.  1 / sqrt is
// a square root and a division, both correctly rounded.  The addend is at most |weight| sqrt(6) / 6 (Cauchy-Schwarz) < G, the power
// of two at or above |weight|: the fixed-point grid is 2^-(40 - shift) G, sized by the host for M addends per row.
template <int C, bool VEC>
__global__ __launch_bounds__(256) void gg_tv_kernel(const float *__restrict__ x, const float *__restrict__ emb, GGMeta meta,
                                                    long long *__restrict__ acc, float w6, float to_fx, float lim, int64_t M, int align,
                                                    int normalized, float bound, float two_bound) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int l = blockIdx.y;
    if (p >= M) return;
    const GGLevel lv = gg_level(meta, l);
    uint32_t g[3];
    float f[3];
    if (!grid_locate(x, p, bound, two_bound, lv.res, g, f, align, normalized)) return;
    const float *tab = emb + (size_t)lv.off * C;
    const uint32_t row = gg_row(g[0], g[1], g[2], lv);
    float v[C], r[C], q[C];
    gg_load<C, VEC>(tab + (size_t)row * C, v);
#pragma unroll
    for (int k = 0; k < C; k++) r[k] = 0.f, q[k] = 0.f;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        uint32_t c[3] = {g[0], g[1], g[2]};
        float nb[C];
        c[d] = g[d] + 1;
        gg_load<C, VEC>(tab + (size_t)gg_row(c[0], c[1], c[2], lv) * C, nb);
#pragma unroll
        for (int k = 0; k < C; k++) {
            const float gv = v[k] - nb[k];
            r[k] += gv;
            q[k] += gv * gv;
        }
        if (g[d] > 0) {
            c[d] = g[d] - 1;
            gg_load<C, VEC>(tab + (size_t)gg_row(c[0], c[1], c[2], lv) * C, nb);
#pragma unroll
            for (int k = 0; k < C; k++) {
                const float gv = v[k] - nb[k];
                r[k] += gv;
                q[k] += gv * gv;
            }
        }
    }
    unsigned long long *a = reinterpret_cast<unsigned long long *>(acc) + ((size_t)lv.off + row) * C;
#pragma unroll
    for (int k = 0; k < C; k++) {
        const float addend = (w6 * r[k]) / sqrtf(q[k] + 1e-9f);
        const long long t = fx_quantize((double)addend * (double)to_fx, lim);
        if (t != 0) atomicAdd(a + k, (unsigned long long)t);
    }
}

// ---- weight decay (gridencoder.cu:671-703): grad[i] += 2 weight emb[i] / rows(level of i); the level is the launch's row ---------
__global__ __launch_bounds__(256) void gg_wd_kernel(const float *__restrict__ emb, float *__restrict__ grad, GGMeta meta, int C,
                                                    float two_w) {
    const int l = blockIdx.y;
    const int64_t a = (int64_t)meta.offsets[l] * C, n = (int64_t)(meta.offsets[l + 1] - meta.offsets[l]) * C;
    const float T = (float)(uint32_t)(meta.offsets[l + 1] - meta.offsets[l]);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        grad[a + i] += two_w * emb[a + i] / T;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
static int gg_fill_meta(GGMeta &m, const int32_t *offsets_host, const int32_t *res_host, int L, int gridtype) {
    if (int st = grid_fill_meta(m, offsets_host, res_host, L)) return st;
    for (int i = 0; i < L; i++) {
        const uint32_t res = (uint32_t)res_host[i], T = (uint32_t)(offsets_host[i + 1] - offsets_host[i]);
        // the stride loop of get_grid_index in its own uint32 arithmetic: axis 0 always (stride 1 <= T), then while stride <= T
        uint32_t stride = res;
        m.my[i] = m.mz[i] = 0;
        if (stride <= T) {
            m.my[i] = stride;
            stride *= res;
            if (stride <= T) {
                m.mz[i] = stride;
                stride *= res;
            }
        }
        m.hashed[i] = (gridtype == 0 && stride > T) ? 1 : 0;
    }
    return MH_OK;
}

static inline bool gg_channels_ok(int C) { return C == 1 || C == 2 || C == 4 || C == 8; }
// one C-wide vector access per row needs every row address aligned to min(4 C, 16) bytes
static inline bool gg_aligned(const void *p, int C) { return ((uintptr_t)p % (size_t)(C * 4 < 16 ? C * 4 : 16)) == 0; }

#define GG_DISPATCH(C, vec, LAUNCH)                 \
    switch (C) {                                    \
    case 1: { LAUNCH(1, false); } break;            \
    case 2: if (vec) { LAUNCH(2, true); } else { LAUNCH(2, false); } break; \
    case 4: if (vec) { LAUNCH(4, true); } else { LAUNCH(4, false); } break; \
    default: if (vec) { LAUNCH(8, true); } else { LAUNCH(8, false); } break; \
    }

extern "C" int mh_grid_general_fwd(const float *x, const float *emb, const int32_t *offsets_host, const int32_t *res_host,
                                   float *out, int64_t M, int32_t L, int32_t n_levels, int32_t C, int32_t gridtype,
                                   int32_t align_corners, int32_t interp, float bound, void *stream) {
    if (M == 0) return MH_OK;
    if (!x || !emb || !out || M < 0 || n_levels < 0 || n_levels > L || !(bound > 0.f) || !gg_channels_ok(C) || gridtype < 0 ||
        gridtype > 1 || align_corners < 0 || align_corners > 1 || interp < 0 || interp > 1)
        return MH_ERR_ARG;
    GGMeta meta;
    int st = gg_fill_meta(meta, offsets_host, res_host, L, gridtype);
    if (st) return st;
    const int64_t blocks = (M + 255) / 256;
    if (blocks > 0x7fffffffLL) return MH_ERR_ARG;
    const bool vec = gg_aligned(emb, C) && gg_aligned(out, C);
#define GG_FWD(CC, VV)                                                                                                        \
    hipLaunchKernelGGL((gg_fwd_kernel<CC, VV>), dim3((unsigned)blocks, (unsigned)L), dim3(256), 0, mh_stream(stream), x, emb, meta, \
                       out, M, (int)L, (int)n_levels, (int)align_corners, (int)interp, bound, 2.0f * bound)
    GG_DISPATCH(C, vec, GG_FWD)
#undef GG_FWD
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_grid_general_bwd(const float *grad, const float *x, const float *emb, const int32_t *offsets_host,
                                   const int32_t *res_host, float *grad_emb, int64_t *emb_acc, float *grad_x, int64_t M, int32_t L,
                                   int32_t n_levels, int32_t C, int32_t gridtype, int32_t align_corners, int32_t interp, float bound,
                                   void *stream) {
    if (M == 0) return MH_OK;
    if (!grad || !x || !emb || !grad_emb || !emb_acc || M < 0 || n_levels < 0 || n_levels > L || !(bound > 0.f) ||
        !gg_channels_ok(C) || gridtype < 0 || gridtype > 1 || align_corners < 0 || align_corners > 1 || interp < 0 || interp > 1)
        return MH_ERR_ARG;
    GGMeta meta;
    int st = gg_fill_meta(meta, offsets_host, res_host, L, gridtype);
    if (st) return st;
    const int64_t blocks = (M + 255) / 256;
    if (blocks > 0x7fffffffLL) return MH_ERR_ARG;
    const int64_t n_acc = (int64_t)offsets_host[L] * C;
    hipStream_t s = mh_stream(stream);
    // emb_acc: n_acc sums and, behind them, the word that receives max |grad|
    if (!mh_zero_async(emb_acc, sizeof(int64_t) * (size_t)(n_acc + 1), s)) return MH_ERR_LAUNCH;
    uint32_t *gmax = reinterpret_cast<uint32_t *>(emb_acc + n_acc);
    grid_absmax_launch(grad, M * (int64_t)L * C, gmax, s);
    MH_CHECK_LAUNCH();
    const int acc_shift = grid_acc_shift(M, 8);
    const bool vec = gg_aligned(emb, C) && gg_aligned(grad, C);
    if (n_levels > 0) {
#define GG_BWD(CC, VV)                                                                                                             \
    hipLaunchKernelGGL((gg_bwd_emb_kernel<CC, VV>), dim3((unsigned)blocks, (unsigned)n_levels), dim3(256), 0, s, grad, x, meta,   \
                       reinterpret_cast<long long *>(emb_acc), acc_shift, M, (int)L, (int)align_corners, (int)interp, bound,      \
                       2.0f * bound, gmax)
        GG_DISPATCH(C, vec, GG_BWD)
#undef GG_BWD
        MH_CHECK_LAUNCH();
        hipLaunchKernelGGL(grid_acc_finalize_kernel, dim3((unsigned)std::min<int64_t>((n_acc + 255) / 256, 4096)), dim3(256), 0, s,
                           reinterpret_cast<const long long *>(emb_acc), grad_emb, n_acc, acc_shift, gmax, 0.0);
        MH_CHECK_LAUNCH();
    }
    if (grad_x) {
#define GG_DX(CC, VV)                                                                                                          \
    hipLaunchKernelGGL((gg_bwd_dx_kernel<CC, VV>), dim3((unsigned)blocks), dim3(256), 0, s, grad, x, emb, meta, grad_x, M, (int)L, \
                       (int)n_levels, (int)align_corners, (int)interp, bound, 2.0f * bound)
        GG_DISPATCH(C, vec, GG_DX)
#undef GG_DX
        MH_CHECK_LAUNCH();
    }
    return MH_OK;
}

extern "C" int mh_grid_grad_tv(const float *x, const float *emb, const int32_t *offsets_host, const int32_t *res_host,
                               float *grad_emb, int64_t *emb_acc, float weight, int64_t M, int32_t L, int32_t C, int32_t gridtype,
                               int32_t align_corners, int32_t normalized, float bound, void *stream) {
    if (M == 0) return MH_OK;
    if (!x || !emb || !grad_emb || !emb_acc || M < 0 || !std::isfinite(weight) || !gg_channels_ok(C) || gridtype < 0 ||
        gridtype > 1 || align_corners < 0 || align_corners > 1 || normalized < 0 || normalized > 1 || (!normalized && !(bound > 0.f)))
        return MH_ERR_ARG;
    GGMeta meta;
    int st = gg_fill_meta(meta, offsets_host, res_host, L, gridtype);
    if (st) return st;
    const int64_t blocks = (M + 255) / 256;
    if (blocks > 0x7fffffffLL) return MH_ERR_ARG;
    const int64_t n_acc = (int64_t)offsets_host[L] * C;
    hipStream_t s = mh_stream(stream);
    if (!mh_zero_async(emb_acc, sizeof(int64_t) * (size_t)n_acc, s)) return MH_ERR_LAUNCH;
    // G: the power of two at or above |weight| (an addend is below 0.41 |weight|); weight 0 adds nothing whatever the scale
    int e = 0;
    if (weight != 0.f) {
        std::frexp(std::fabs(weight), &e);          // |weight| = m 2^e, 0.5 <= m < 1: 2^e > |weight|
        e = std::max(e, -60);
    }
    const int acc_shift = grid_acc_shift(M, 1);
    const float to_fx = std::ldexp(1.0f, FX_BITS - acc_shift - e), lim = std::ldexp(1.0f, FX_BITS - acc_shift);
    const double from_fx = std::ldexp(1.0, e + acc_shift - FX_BITS);
    const float w6 = weight / 6.0f;                 // `weight / (2 * D)`, gridencoder.cu:586
    const float b = normalized ? 1.0f : bound;
    const bool vec = gg_aligned(emb, C);
#define GG_TV(CC, VV)                                                                                                         \
    hipLaunchKernelGGL((gg_tv_kernel<CC, VV>), dim3((unsigned)blocks, (unsigned)L), dim3(256), 0, s, x, emb, meta,             \
                       reinterpret_cast<long long *>(emb_acc), w6, to_fx, lim, M, (int)align_corners, (int)normalized, b, 2.0f * b)
    GG_DISPATCH(C, vec, GG_TV)
#undef GG_TV
    MH_CHECK_LAUNCH();
    hipLaunchKernelGGL(grid_acc_finalize_kernel, dim3((unsigned)std::min<int64_t>((n_acc + 255) / 256, 4096)), dim3(256), 0, s,
                       reinterpret_cast<const long long *>(emb_acc), grad_emb, n_acc, 0, (const uint32_t *)nullptr, from_fx);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_grid_grad_wd(const float *emb, const int32_t *offsets_host, float *grad_emb, float weight, int32_t L, int32_t C,
                               void *stream) {
    if (!emb || !grad_emb || !offsets_host || L < 1 || L > MH_MAX_LEVELS || !gg_channels_ok(C) || !std::isfinite(weight) ||
        offsets_host[0] < 0)
        return MH_ERR_ARG;
    GGMeta meta = {};
    int64_t widest = 0;
    for (int i = 0; i <= L; i++) meta.offsets[i] = offsets_host[i];
    for (int i = 0; i < L; i++) {
        if (offsets_host[i + 1] <= offsets_host[i]) return MH_ERR_ARG;
        widest = std::max<int64_t>(widest, (int64_t)(offsets_host[i + 1] - offsets_host[i]) * C);
    }
    const unsigned blocks = (unsigned)std::min<int64_t>((widest + 255) / 256, 2048);
    hipLaunchKernelGGL(gg_wd_kernel, dim3(blocks, (unsigned)L), dim3(256), 0, mh_stream(stream), emb, grad_emb, meta, (int)C,
                       2.0f * weight);
    MH_CHECK_LAUNCH();
    return MH_OK;
}
