// Wavefront (64 lanes) primitives: reductions, scans, ballot ranks and the wave-per-ray index, written once.
// A new kernel file includes this header; it does not copy a loop from a neighbour.
//
// Every function must be reached by all 64 lanes of the wavefront (the shuffles read lanes, they do not wait for them).  The
// association order of each reduction and scan is part of its definition -- results are pinned bit for bit by the tests of the
// callers -- and is stated with the function.  Several values are reduced by several calls: each value sees the same sequence
// of operations as in a joint loop.
//
// No `#pragma clang fp contract` here: a file-scope pragma in a header would reach the rest of the including file, and the
// including files differ in their contraction mode.  No function below holds a multiply next to an add, so none needs one.
#pragma once
#include "common.h"

// ---- butterfly reductions, offsets 32 down to 1: every lane holds the result, the same bits in every lane ---------------
// lane i's value after the step of offset o is v[i] (op) v[i ^ o]
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}
// signed: the order-preserving integer image of floats (tsdf_ordered) is reduced this way
__device__ __forceinline__ int32_t wave_min(int32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int32_t wave_max(int32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// Butterflies over a part of the offsets, for a wave split into 64 / G sub-groups of G consecutive lanes (G a power of two):
// wave_sum_across adds the lanes of equal position in every sub-group (offsets G up to 32; every lane holds the result),
// wave_sum_within adds the G lanes of a sub-group (offsets 1 up to G / 2; every lane holds its own sub-group's result).
__device__ __forceinline__ float wave_sum_across(float v, int G) {
    for (int o = G; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_sum_within(float v, int G) {
    for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- inclusive scans, offsets 1 up to 32 (Hillis-Steele): lane i holds v[0] (op) ... (op) v[i], every lane valid ---------
__device__ __forceinline__ float wave_incl_scan(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        float n = __shfl_up(v, o);
        if (lane >= o) v += n;
    }
    return v;
}
__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        int n = __shfl_up(v, o);
        if (lane >= o) v += n;
    }
    return v;
}
__device__ __forceinline__ double wave_incl_scan(double v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        double n = __shfl_up(v, o);
        if (lane >= o) v += n;
    }
    return v;
}
// running maximum: exact, so lane i's value is >= lane i - 1's whatever the terms are (fmaxf drops a NaN term)
__device__ __forceinline__ float wave_incl_max(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        float n = __shfl_up(v, o);
        if (lane >= o) v = fmaxf(v, n);
    }
    return v;
}
// running product in double (the alpha form of volrend.hip, which says why it is double)
__device__ __forceinline__ double wave_incl_prod(double v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        double n = __shfl_up(v, o);
        if (lane >= o) v *= n;
    }
    return v;
}

// reverse inclusive scan: lane i holds v[i] + ... + v[63], every lane valid
__device__ __forceinline__ float wave_rev_incl_scan(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        float n = __shfl_down(v, o);
        if (lane + o < 64) v += n;
    }
    return v;
}
__device__ __forceinline__ double wave_rev_incl_scan(double v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        double n = __shfl_down(v, o);
        if (lane + o < 64) v += n;
    }
    return v;
}

// ---- exclusive values from an inclusive scan, every lane valid ----------------------------------------------------------
// The "lane below" form: the inclusive value of the lane below, `identity` at lane 0.  It never contains the lane's own term, so
// it survives +inf terms (`incl - v` would form inf - inf) and keeps nothing of the own term's rounding.
__device__ __forceinline__ float wave_excl_below(float incl, int lane, float identity) {
    const float below = __shfl_up(incl, 1);
    return lane ? below : identity;
}
__device__ __forceinline__ double wave_excl_below(double incl, int lane, double identity) {
    const double below = __shfl_up(incl, 1);
    return lane ? below : identity;
}
// the same from the other end: the reverse-inclusive value of the lane above, 0 at lane 63
__device__ __forceinline__ float wave_excl_above(float rincl, int lane) {
    const float above = __shfl_down(rincl, 1);
    return lane < 63 ? above : 0.f;
}
__device__ __forceinline__ double wave_excl_above(double rincl, int lane) {
    const double above = __shfl_down(rincl, 1);
    return lane < 63 ? above : 0.0;
}

// The compositor's rule for the exclusive prefix of sigma*dt.  `incl - v` returns the prefix with an absolute error of
// ulp(incl) / 2, which the weight takes as a relative error.  While the sample's own v = sigma*dt is below 1 that is at most
// 2^-24 x the transmittance-weighted share of the sample (a prefix large enough to raise ulp(incl) has already taken the weight
// away), and the subtraction stays, so that results for ordinary densities are bit for bit what they were.  For an opaque sample
// -- the first one of a ray carries most of the ray's weight -- incl is rounded at ulp(v): 4e-6 of the weight at v = 100, 5e-4 at
// 1e4, and inf - inf = NaN at sigma = +inf, where the definition gives w = T for the sample and 0 behind it.  There the exclusive
// value is the inclusive value of the lane below, 0 at lane 0, which never contains the sample's own term.
constexpr float WAVE_OPAQUE_SD = 1.0f;
__device__ __forceinline__ float wave_excl_from_incl(float incl, float v, int lane) {
    const float below = __shfl_up(incl, 1);
    return v >= WAVE_OPAQUE_SD ? (lane ? below : 0.f) : incl - v;
}

// ---- workgroup exclusive scan of ints, built from the wave scan ------------------------------------------------------------
// The sum of v over the threads below this one, in thread order, for a workgroup of NW whole wavefronts; *total = the sum over
// the workgroup, the same in every thread.  Every thread of the workgroup must reach the call (two barriers; `lds`, NW ints
// of shared memory, is free again when it returns).  Integer sums: no association order to state.
template <int NW>
__device__ __forceinline__ int block_excl_scan(int v, int *lds, int *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_incl_scan(v, lane);
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    int below = 0, sum = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const int s = lds[i];
        if (i < wave) below += s;
        sum += s;
    }
    __syncthreads();
    *total = sum;
    return below + incl - v;
}

// ---- ballot rank: the number of set bits of `mask` below `lane`, valid in every lane ------------------------------------
__device__ __forceinline__ int wave_rank(unsigned long long mask, int lane) {
    return __popcll(mask & ((1ull << lane) - 1ull));
}

// ---- broadcast: lane `src`'s value in every lane; `src` (0 .. 63) must be the same in every lane ------------------------
// a v_readlane, not a shuffle: the result is wave-uniform to the compiler as well, so what is computed from it stays scalar
__device__ __forceinline__ float wave_read(float v, int src) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// ---- one wavefront per ray, four rays per 256-thread block --------------------------------------------------------------
// the ray (row, chunk) of this wavefront; the caller returns when it is past the end, the whole wavefront together
__device__ __forceinline__ int wave_ray() { return blockIdx.x * 4 + (threadIdx.x >> 6); }

// the ray's packed sample range as stored: the count is returned, the first position goes to *start
__device__ __forceinline__ int ray_range(const int32_t *__restrict__ ray_start, const int32_t *__restrict__ ray_cnt, int ray,
                                         int64_t *start) {
    *start = ray_start[ray];
    return ray_cnt[ray];
}
// the same, held inside the packed arrays of length M whatever ray_start / ray_cnt say
__device__ __forceinline__ int ray_range_clamped(const int32_t *__restrict__ ray_start, const int32_t *__restrict__ ray_cnt,
                                                 int ray, int64_t M, int64_t *start) {
    const int64_t s = ray_start[ray];
    int64_t c = ray_cnt[ray];
    if (s < 0 || s >= M || c < 0) c = 0;
    if (s + c > M) c = M - s;
    *start = s;
    return (int)c;
}
