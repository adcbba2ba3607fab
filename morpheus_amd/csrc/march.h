// The occupancy-grid ray marcher, once: the box clip, the cell lookup and the slot-row trip loop behind both
// march_wave_kernel (csrc/sampler.hip, OccupancyGrid: one level, the cube [-bound, bound]^3, no planes, no cone steps) and
// est_march_kernel (csrc/estimator.hip, OccGridEstimator: levels, per-axis boxes, planes, per-ray limits, cone steps).
//
// The definition of the intervals stands in csrc/estimator.hip's header comment (points 1 - 7) and, for the cube, above
// march_wave_kernel.  The cube is marched AS the box lo = (-bound) x 3, hi = (+bound) x 3, and that is the same rounded
// arithmetic as the scalar form it replaces, operation by operation:
//   clip   (lo - o) / d  with lo = -bound  is  (-bound - o) / d  itself (negation is exact);  (hi - o) / d  is  (bound - o) / d;
//   cell   x - lo = x - (-bound)  is the IEEE operation  x + bound  (subtracting is adding the negated operand, one rounding);
//          hi - lo = bound - (-bound) = bound + bound = 2.0f * bound  exactly (a doubling is exact; both overflow to +inf alike);
//          one level: the level search is empty, level 0's stride is 0, the index is (c0 * R + c1) * R + c2;
//   steps  t0 + (float)k * step, min(ts + step, t_far), the midpoint (ts + te) / 2.0f and o + d * tm are the same statements.
// tests/test_gpu_estimator.py::test_one_level_defaults_equal_occupancy_grid and tests/test_gpu_sampler_cases.py hold both
// kernels to it bit for bit.
#pragma once

// No FMA contraction: every mul / add / div below is one IEEE round-to-nearest operation.  Both including files state the
// same pragma at file scope before their includes; it is repeated here, as in rays.h, so that the arithmetic does not
// depend on where the header is included.
#pragma clang fp contract(off)

#include "wave.h"

#define MARCH_MAX_LEVELS 16

struct GridRes {
    int x, y, z;
};

// Slab clip of one ray to the box lo = box[0..2], hi = box[3..5] -> [*t_near >= 0, *t_far]; a MISS gives t_near = t_far = 0.
// A ray is a miss when the clipped segment is empty, when one of its six slab quotients is NaN (fmaxf / fminf would drop
// the NaN and clip on the remaining axes; the oracle's minimum / maximum propagate it) or when the clipped t_far is not
// finite (d = 0 inside the box: nothing bounds the walk).
__device__ __forceinline__ void slab_clip(const float *o, const float *d, const float *box, float *t_near, float *t_far) {
    float tmin = -INFINITY, tmax = INFINITY;
    bool nan = false;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float ta = (box[a] - o[a]) / d[a];
        const float tb = (box[3 + a] - o[a]) / d[a];
        nan = nan || ta != ta || tb != tb;
        tmin = fmaxf(tmin, fminf(ta, tb));
        tmax = fminf(tmax, fmaxf(ta, tb));
    }
    tmin = fmaxf(tmin, 0.0f);
    // tmax > tmin >= 0 leaves +inf as the only non-finite t_far; a non-finite t_near never passes tmax > tmin
    if (nan || !(tmax > tmin) || !(tmax < INFINITY)) {
        tmin = 0.f;
        tmax = 0.f;
    }
    *t_near = tmin;
    *t_far = tmax;
}

// the cube [-bound, bound]^3 as a box (in registers: a kernel that clips to the cube reads no box from memory)
struct CubeBox {
    float b[6];
    __device__ __forceinline__ explicit CubeBox(float bound) : b{-bound, -bound, -bound, bound, bound, bound} {}
};

// Is the cell of the step's midpoint occupied?  The finest level whose box holds the midpoint (lo <= x < hi on the three axes;
// none: the coarsest, L - 1), cell = clamp(floor((x - lo) / (hi - lo) * R), 0, R - 1) per axis.
__device__ __forceinline__ bool march_occupied(const float *o, const float *d, float ts, float te, const float *boxes, int L,
                                               GridRes R, const uint8_t *__restrict__ binary) {
    const float tm = (ts + te) / 2.0f;
    float x[3];
#pragma unroll
    for (int a = 0; a < 3; a++) x[a] = o[a] + d[a] * tm;
    int lvl = L - 1;
    for (int l = 0; l < L - 1; l++) {
        const float *b = boxes + l * 6;
        if (b[0] <= x[0] && x[0] < b[3] && b[1] <= x[1] && x[1] < b[4] && b[2] <= x[2] && x[2] < b[5]) {
            lvl = l;
            break;
        }
    }
    const float *b = boxes + lvl * 6;
    const int res[3] = {R.x, R.y, R.z};
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float u = (x[a] - b[a]) / (b[3 + a] - b[a]);
        c[a] = min(max((int)floorf(u * (float)res[a]), 0), res[a] - 1);
    }
    return binary[(((int64_t)lvl * R.x + c[0]) * R.y + c[1]) * R.z + c[2]] != 0;
}

// What only the estimator's march has; the grid's instantiation compiles none of it.
struct MarchLimits {
    const float *t_min, *t_max;      // per-ray limits, either may be NULL
    float near_plane, far_plane;
    float cone;                      // cone_angle; > 0: the step grows along the ray
};

// Wave-per-ray march of ray wave_ray() into its slot row: one wavefront walks one ray, 64 consecutive steps a trip (a lane =
// one step: setup once, one occupancy byte per lane in flight instead of a dependent-load loop per thread), ballot + rank
// compacts the occupied steps into the ray's slot row [cap].  A second launch (march_pack_kernel) copies the slot rows to
// their packed positions once the exclusive scan of the counts is known -- the march itself runs ONCE.
// `boxes`: L boxes of six floats, the clip box last (the coarsest); registers or LDS, the caller's choice.
// LIMITS = false: near plane 0 and no far plane (after the clip 0 > t_near and inf < t_far are never true), no per-ray
// limits, constant steps in closed form.  LIMITS = true adds `lim`.  Cone steps are a recurrence (each rounds on the one
// before), so a lane cannot jump to its step: every lane walks the 64 steps of the trip in lockstep -- three VALU operations
// a step, against the latency of the occupancy byte -- and keeps its own; the value behind the 64th is the next trip's start.
template <bool LIMITS>
__device__ __forceinline__ void march_slots(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                            const float *__restrict__ jitter, int N, float step, const MarchLimits &lim,
                                            const float *boxes, int L, GridRes R, const uint8_t *__restrict__ binary, int cap,
                                            int32_t *__restrict__ ray_cnt, float *__restrict__ slot_ts,
                                            float *__restrict__ slot_te, int32_t *__restrict__ overflow) {
    const int lane = threadIdx.x & 63;
    const int r = wave_ray();
    if (r >= N) return;
    float o[3], d[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        o[a] = rays_o[r * 3 + a];
        d[a] = rays_d[r * 3 + a];
    }
    float tn, tf;
    slab_clip(o, d, boxes + (L - 1) * 6, &tn, &tf);
    if (LIMITS) {
        if (lim.near_plane > tn) tn = lim.near_plane;
        if (lim.t_min) {
            const float v = lim.t_min[r];
            if (v > tn) tn = v;
        }
        if (lim.far_plane < tf) tf = lim.far_plane;
        if (lim.t_max) {
            const float v = lim.t_max[r];
            if (v < tf) tf = v;
        }
    }
    const float t0 = tn + (jitter ? jitter[r] : 0.0f) * step;
    float *row_s = slot_ts + (int64_t)r * cap, *row_e = slot_te + (int64_t)r * cap;
    const bool coned = LIMITS && lim.cone > 0.f;
    float carry = t0;      // cone marching: ts of step k0, the same value in every lane
    int n = 0, k0 = 0;
    for (; k0 < cap; k0 += 64) {
        float ts, dt = step;
        if (coned) {
            float t = carry;
            ts = t;
            for (int j = 0; j < 64; j++) {
                const float dj = fminf(fmaxf(t * lim.cone, step), 1e10f);
                if (j == lane) {
                    ts = t;
                    dt = dj;
                }
                t = t + dj;
            }
            carry = t;
        } else {
            ts = t0 + (float)(k0 + lane) * step;
        }
        const bool in = ts < tf;
        if (__ballot(in) == 0ull) break;
        const float te = fminf(ts + dt, tf);
        const bool occ = in && march_occupied(o, d, ts, te, boxes, L, R, binary);
        const unsigned long long mask = __ballot(occ);
        const int pos = n + wave_rank(mask, lane);
        if (occ && pos < cap) {
            row_s[pos] = ts;
            row_e[pos] = te;
        }
        n += __popcll(mask);
    }
    if (lane == 0) {
        ray_cnt[r] = n < cap ? n : cap;
        // more kept steps than the slot row holds, or steps left unwalked (directions much shorter than unit length): tell the
        // host, which marches again with a longer slot row
        const float next = coned ? carry : t0 + (float)k0 * step;
        if (n > cap || next < tf) atomicOr(overflow, 1);
    }
}
