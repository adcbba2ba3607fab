// The multiresolution grid's rules, written once: where a point lies in a level (grid_unit, grid_locate), what a legal level
// table is (GridMeta, grid_fill_meta), and the 64-bit fixed point that every sum into a table-shaped buffer goes through
// (fx_scales, fx_quantize, grid_acc_shift, absmax_kernel, grid_acc_finalize_kernel).  hashgrid.hip (C = 2, hash, linear,
// align_corners = False: the training step's kernels) and hashgrid_general.hip (the reference operator in full) both take them
// from here -- the two files are switched between per call and compared bit for bit by the tests, so a new grid kernel file
// includes this header; it does not copy a rule from a neighbour.
//
// Semantics: reference external/encoders/gridencoder/src/gridencoder.cu (kernel_grid :83-249), host logic grid.py:157.
//
// Contraction: the including files set `#pragma clang fp contract(off)` BELOW their includes, so this header is compiled with
// hipcc's default (fast) mode, and a file-scope pragma here would reach the rest of the including file (wave.h).  Every function
// below that holds a multiply and an add therefore opens its body with the pragma: what is written is what runs, wherever the
// header is included (a fused `u * (res - 1) - c` moves the position inside the cell by an ulp).  The explicit fmaf calls are the
// single-rounding operations oracle/hashgrid.c makes (`u * res - 0.5`, as nvcc -fmad=true fuses it in the reference).
#pragma once
#include "common.h"
#include "wave.h"
#include <cmath>

// ---- the level table ---------------------------------------------------------------------------------------------------------------
// offsets (rows, not floats) and resolutions travel by value in the kernarg segment (SGPRs); resolutions are host-computed float32
// ceil(exp2f(l * S) * H), so oracle and kernel agree
struct GridMeta {
    int32_t offsets[MH_MAX_LEVELS + 1];
    int32_t res[MH_MAX_LEVELS];
};

// a legal table: 1 .. MH_MAX_LEVELS levels, a non-negative first offset, every level at least one row and two vertices per axis
static inline int grid_fill_meta(GridMeta &m, const int32_t *offsets_host, const int32_t *res_host, int L) {
    if (!offsets_host || !res_host || L < 1 || L > MH_MAX_LEVELS) return MH_ERR_ARG;
    if (offsets_host[0] < 0) return MH_ERR_ARG;
    for (int i = 0; i <= L; i++) m.offsets[i] = offsets_host[i];
    for (int i = 0; i < L; i++) {
        m.res[i] = res_host[i];
        if (res_host[i] < 2 || offsets_host[i + 1] <= offsets_host[i]) return MH_ERR_ARG;
    }
    return MH_OK;
}

// ---- cell location -----------------------------------------------------------------------------------------------------------------
// n / d, correctly rounded (what the reference's fp32 `/` gives), for a divisor that stays the same over many quotients: hipcc
// expands an IEEE division into ~14 VALU instructions (scale, reciprocal, two refinements, fix-up), and every (point, level) lane
// of the grid kernels did three of them -- a tenth of the brick backward's instruction stream.  With r = RN(1 / d) (ONE division,
// hoisted out of the loops: d = 2 bound is a kernel argument) two residual corrections give the correctly rounded quotient
// (Markstein: q' = RN(q + RN(n - d q) r) is correctly rounded once q is within an ulp and r is the correctly rounded reciprocal);
// checked against exact rational arithmetic on 2.2e5 numerators for seven divisors (tools/micro/README.md).  No scaling: the
// operands here are O(1), far from the subnormal / overflow ranges the compiler's fix-up instructions exist for.
__device__ __forceinline__ float exact_div(float n, float d, float r) {
#pragma clang fp contract(off)
    const float q0 = n * r;
    const float q1 = fmaf(fmaf(-d, q0, n), r, q0);
    return fmaf(fmaf(-d, q1, n), r, q1);
}

// u = (x + bound) / (2 bound) of one coordinate (grid.py:157, fp32 add then IEEE divide), inv = 1 / two_bound; normalized: the
// coordinate is u already (grad_total_variation's own random points, grid.py:184).  Inside the box <=> grid_in_box(u).
// (an infinite coordinate makes exact_div's residual inf - inf = NaN where the IEEE quotient is +-inf: the ordered comparison sends
//  both -- and a NaN coordinate -- out of the box, as `u < 0 || u > 1` does for the reference's +-inf)
__device__ __forceinline__ float grid_unit(float x, float bound, float two_bound, float inv, int normalized = 0) {
    return normalized ? x : exact_div(x + bound, two_bound, inv);
}
__device__ __forceinline__ bool grid_in_box(float u) { return u >= 0.0f && u <= 1.0f; }

// cell g and position f inside it at a level of resolution res (gridencoder.cu:105-111, :143-151); false for a point outside
// [0,1]^3 (or not finite).  align_corners and normalized are the reference operator's switches; the specialised kernels leave
// them at 0 and the other branches fold away.
__device__ __forceinline__ bool grid_locate(const float (&xv)[3], float bound, float two_bound, uint32_t res, uint32_t g[3],
                                            float f[3], int align_corners = 0, int normalized = 0) {
#pragma clang fp contract(off)
    bool inb = true;
    const float inv = 1.0f / two_bound;                // loop-invariant in every caller
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const float u = grid_unit(xv[d], bound, two_bound, inv, normalized);
        inb = inb && grid_in_box(u);
        float pos, fl;                                  // position in cells, and the cell as a float
        if (align_corners) {
            pos = u * (float)(res - 1);
            g[d] = min((uint32_t)floorf(pos), res - 2);
            fl = (float)g[d];
        } else {
            pos = fminf(fmaxf(fmaf(u, (float)res, -0.5f), 0.0f), (float)(res - 1));
            fl = floorf(pos);
            g[d] = (uint32_t)fl;
        }
        f[d] = pos - fl;
    }
    return inb;
}

__device__ __forceinline__ bool grid_locate(const float *__restrict__ x, int64_t p, float bound, float two_bound, uint32_t res,
                                            uint32_t g[3], float f[3], int align_corners = 0, int normalized = 0) {
    const float xv[3] = {x[p * 3 + 0], x[p * 3 + 1], x[p * 3 + 2]};
    return grid_locate(xv, bound, two_bound, res, g, f, align_corners, normalized);
}

// ---- 64-bit fixed point --------------------------------------------------------------------------------------------------------------
// Sums into a table-shaped buffer are integer: q = (int64) (v * 2^40 / G), G = the power of two above the call's max |v| (or at or
// above a regulariser's |weight|).  Every fp32 term is represented to 2^-40 G, integer addition commutes, so the sums are exact and
// the same from run to run whatever order the waves arrive in -- which float atomics cannot give; one conversion to fp32 per table
// entry ends it.  acc_shift (grid_acc_shift) takes the bits of headroom a call needs out of the scale.
#define FX_BITS 40
#define FX_LIMIT 1099511627776.0f                   // 2^40: the fixed-point range a scaled term is clamped to
__device__ __forceinline__ void fx_scales(uint32_t maxbits, float &to_fx, float &from_fx) {
    int e = (int)(maxbits >> 23) + 1;   // biased exponent of the power of two above max|grad|
    e = max(e, 60);                     // gradients below 2^-67 are accumulated with a fixed (coarser) scale
    e = min(e, 254);
    to_fx = __uint_as_float((uint32_t)(127 + FX_BITS + 127 - e) << 23);    // 2^(40 - (e-127))
    from_fx = __uint_as_float((uint32_t)(127 - FX_BITS - 127 + e) << 23);  // 2^((e-127) - 40)
}

// a value already scaled to fixed point, rounded to the nearest integer and saturated inside the headroom (a NaN gives the lower
// limit: fmax(NaN, -lim) = -lim -- one bounded contribution, not an arbitrary bit pattern)
__device__ __forceinline__ long long fx_quantize(double v, float lim) {
    const double c = fmin(fmax(v, (double)-lim), (double)lim);
    return __double2ll_rn(c);
}

// headroom of a call's int64 sums: a row receives at most terms_per_point * M terms of at most 2^(FX_BITS - shift) each (hash
// collisions included); the shift keeps their sum inside +-2^62
static inline int grid_acc_shift(int64_t M, int terms_per_point) {
    int s = 0;
    while (s < 40 && (double)M * terms_per_point > std::ldexp(1.0, 62 - FX_BITS + s)) s++;
    return s;
}

// max |g| over n floats, as the raw bits of a non-negative float (monotone in the value, so an integer atomicMax does the
// reduction).  VEC4: g is 16-byte aligned and is read as whole float4s (the tail loop covers n % 4); a caller that does not know
// its pointer to be aligned -- a contiguous gradient may start anywhere inside an allocation -- takes the scalar form.
template <bool VEC4>
static __global__ __launch_bounds__(256) void absmax_kernel(const float *__restrict__ g, int64_t n, uint32_t *__restrict__ out) {
    uint32_t m = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t n4 = VEC4 ? n >> 2 : 0;
    if (VEC4) {
        const f32x4 *g4 = reinterpret_cast<const f32x4 *>(g);
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
            const f32x4 v = g4[i];
            m = max(max(m, __float_as_uint(fabsf(v[0]))), __float_as_uint(fabsf(v[1])));
            m = max(max(m, __float_as_uint(fabsf(v[2]))), __float_as_uint(fabsf(v[3])));
        }
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) m = max(m, __float_as_uint(fabsf(g[i])));
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// (the launch of a call's pre-pass: `out` zeroed by the caller; the error, if any, is left for the caller's MH_CHECK_LAUNCH)
static inline void grid_absmax_launch(const float *g, int64_t n, uint32_t *out, hipStream_t s) {
    if ((uintptr_t)g % 16 == 0) hipLaunchKernelGGL(absmax_kernel<true>, dim3(1024), dim3(256), 0, s, g, n, out);
    else hipLaunchKernelGGL(absmax_kernel<false>, dim3(1024), dim3(256), 0, s, g, n, out);
}

// out[i] += acc[i] * scale, one rounding per entry; entries nothing was added to are not written.  The scale is the call's
// (from_fx of its max |grad| word, times 2^acc_shift) where gmax_bits is given, fixed_scale otherwise.
static __global__ __launch_bounds__(256) void grid_acc_finalize_kernel(const long long *__restrict__ acc, float *__restrict__ out,
                                                                       int64_t n, int acc_shift,
                                                                       const uint32_t *__restrict__ gmax_bits, double fixed_scale) {
#pragma clang fp contract(off)
    double scale = fixed_scale;
    if (gmax_bits) {
        float to_fx, from_fx;
        fx_scales(*gmax_bits, to_fx, from_fx);
        scale = (double)from_fx * (double)(1LL << acc_shift);
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const long long a = acc[i];
        if (a != 0) out[i] += (float)((double)a * scale);
    }
}
