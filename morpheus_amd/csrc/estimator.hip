// Occupancy estimator in full (morpheus_amd/estimator.py:OccGridEstimator): multi-level marcher with cone steps and planes,
// the occupancy update without a device->host read, and mark_invisible_cells.
//
// Stands where nerfacc 0.5.x's OccGridEstimator stands for a render loop written against it.  nerfacc is third-party and
// un-vendored: names, buffers and the update rule are recalled from its public source, agreement unverified.  The interval
// placement is this build's definition (csrc/march.h:march_slots, one body for this file and csrc/sampler.hip), restated in fp32, one
// rounding per operation, by tests/estimator_oracle.py -- every kernel below is held to it bit for bit.
//   1. clip the ray to the COARSEST level's stored box (slab_clip's operations and order, per-axis lo / hi);
//   2. a MISS (empty clip, NaN quotient, non-finite t_far) is decided on that clip alone and has no interval;
//   3. t_near = near_plane if near_plane > t_near, then t_min[r] alike; t_far = far_plane if far_plane < t_far, then t_max[r];
//   4. t0 = t_near + u * step;
//   5. cone_angle == 0: ts_k = t0 + k * step, te_k = min(ts_k + step, t_far), kept while ts_k < t_far (the closed form);
//   6. cone_angle > 0: ts_0 = t0, dt_k = min(max(ts_k * cone_angle, step), 1e10f), te_k = min(ts_k + dt_k, t_far),
//      ts_{k+1} = ts_k + dt_k, kept while ts_k < t_far;
//   7. a step is a sample iff the cell of its midpoint (ts + te) / 2 is occupied in the finest level whose stored box holds the
//      midpoint (lo <= x < hi on the three axes; none: the coarsest), cell = clamp(floor((x - lo) / (hi - lo) * R), 0, R - 1).
// With one level, a centred cubic box and default planes these are the operations of march_wave_kernel (csrc/sampler.hip), bit
// for bit: both kernels run csrc/march.h's march_slots, which says why the cube marched as a box rounds the same.
// The opt-in second placement, the cell-by-cell traversal, shares points 1 - 3 and is stated above est_traverse_kernel.
#include "common.h"

// no FMA contraction: every mul / add / div below is one IEEE round-to-nearest operation (see csrc/sampler.hip)
#pragma clang fp contract(off)

#include "march.h"      // slab_clip, march_occupied, march_slots: shared with sampler.hip
#include "wave.h"

#define EST_MAX_LEVELS MARCH_MAX_LEVELS
#define EST_CHUNK 2048          // cells one wavefront scans in the occupied-list kernels
#define EST_MAX_PARTIALS 1024   // blocks of the mean's first pass

typedef GridRes EstRes;

// march_slots with everything on: the boxes are copied to LDS once per block (the level search reads them per step)
__global__ __launch_bounds__(256) void est_march_kernel(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                        const float *__restrict__ jitter, const float *__restrict__ t_min,
                                                        const float *__restrict__ t_max, int N, float step, float cone,
                                                        float near_plane, float far_plane, const float *__restrict__ aabbs,
                                                        int L, EstRes R, const uint8_t *__restrict__ binary, int cap,
                                                        int32_t *__restrict__ ray_cnt, float *__restrict__ slot_ts,
                                                        float *__restrict__ slot_te, int32_t *__restrict__ overflow) {
    __shared__ float boxes[EST_MAX_LEVELS * 6];
    if ((int)threadIdx.x < L * 6) boxes[threadIdx.x] = aabbs[threadIdx.x];
    __syncthreads();
    march_slots<true>(rays_o, rays_d, jitter, N, step, MarchLimits{t_min, t_max, near_plane, far_plane, cone}, boxes, L, R, binary,
                      cap, ray_cnt, slot_ts, slot_te, overflow);
}

// ---- cell-by-cell traversal: the opt-in second placement (OccGridEstimator(traversal = "dda")) ---------------------------
// The definition is points 1 - 5 under mh_est_traverse_slots in include/morpheus_hip.h, restated in fp32 by
// tests/traverse_oracle.py; this build's statement of nerfacc 0.5.x's traverse_grids as recalled, agreement unverified, with one
// deliberate departure (a run's samples start at max(run start, the ray's last te), so that samples never overlap).
// One wavefront per ray, the slot-row contract of march_slots.  A trip is 64 cell spans.  The walk from span to span is a
// recurrence (which axis steps depends on the exits before), so -- as march_slots does for cone steps -- every lane walks the
// trip's 64 spans in lockstep and keeps its own: the walk's state is wave-uniform (the ray is read through readfirstlane, the
// segment boundaries through wave_read).  A step needs one new exit, of the stepped axis; exits are closed form in the cell
// index, so once a trip and segment lane i forms the exit of the i-th next cell of every axis and the walk only reads them: no
// division sits in the chain.  The 64 occupancy bytes of a trip are then in flight at once, one a lane, not a dependent-load
// chain.  Two ballots (spans wider than zero, occupied spans) give the runs; a run is closed by the first empty span behind it,
// in this trip or a later one (the open run's start and end, the last te, the segment and the cell carry over).  A closed run's
// samples are written a lane a sample, 64 a round: the closed form for cone_angle == 0, march_slots' lockstep recurrence
// otherwise; the kept ones are a prefix (midpoints do not decrease), compacted by ballot + rank behind the n samples the ray
// already has.
__device__ __forceinline__ float trav_exit(int c, float o, float d, float lo, float ext, int res) {
    if (d == 0.f) return INFINITY;
    const int k = c + (d > 0.f ? 1 : 0);
    const float plane = lo + ((float)k / (float)res) * ext;      // closed form from the integer index
    return (plane - o) / d;
}

__global__ __launch_bounds__(256) void est_traverse_kernel(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                           const float *__restrict__ jitter, const float *__restrict__ t_min,
                                                           const float *__restrict__ t_max, int N, float step, float cone,
                                                           float near_plane, float far_plane, const float *__restrict__ aabbs,
                                                           int L, EstRes R, const uint8_t *__restrict__ binary, int cap,
                                                           int32_t *__restrict__ ray_cnt, float *__restrict__ slot_ts,
                                                           float *__restrict__ slot_te, int32_t *__restrict__ overflow) {
    __shared__ float boxes[EST_MAX_LEVELS * 6];
    if ((int)threadIdx.x < L * 6) boxes[threadIdx.x] = aabbs[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int r = __builtin_amdgcn_readfirstlane(wave_ray());
    if (r >= N) return;
    float o[3], d[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        o[a] = rays_o[r * 3 + a];
        d[a] = rays_d[r * 3 + a];
    }
    // 1. clip, miss rule, planes, per-ray limits: march_slots' statements; the jitter moves the near end only
    float tn, tf;
    slab_clip(o, d, boxes + (L - 1) * 6, &tn, &tf);
    if (near_plane > tn) tn = near_plane;
    if (t_min) {
        const float v = t_min[r];
        if (v > tn) tn = v;
    }
    if (far_plane < tf) tf = far_plane;
    if (t_max) {
        const float v = t_max[r];
        if (v < tf) tf = v;
    }
    tn = tn + (jitter ? jitter[r] : 0.0f) * step;
    // 2. level segments: lane i holds boundary T_i of (a_{L-1}, ..., a_0, b_0, ..., b_{L-1}); segment j = [T_j, T_{j+1}] at level
    // |L - 1 - j|
    const int nseg = 2 * L - 1;
    float T = 0.f;
    {
        float a_up = tn, b_up = tf;
        if (lane == 0) T = tn;
        if (lane == nseg) T = tf;
        for (int l = L - 2; l >= 0; l--) {
            float ca, cb;
            slab_clip(o, d, boxes + l * 6, &ca, &cb);
            float al = b_up, bl = b_up;                              // a miss (a hit has t_far > t_near >= 0)
            if (cb != 0.f) {
                al = fminf(fmaxf(ca, a_up), b_up);
                bl = fmaxf(fminf(cb, b_up), al);
            }
            if (lane == L - 1 - l) T = al;
            if (lane == L + l) T = bl;
            a_up = al;
            b_up = bl;
        }
    }
    const int res[3] = {R.x, R.y, R.z};
    const int span_max = R.x + R.y + R.z + 3;
    float *row_s = slot_ts + (int64_t)r * cap, *row_e = slot_te + (int64_t)r * cap;
    const bool coned = cone > 0.f;
    // the walk (wave-uniform): segment j, `fresh`: its first span is still to be set up; cell c, exits t, span start cur, segment
    // end e, spans the segment may still take
    int j = 0, lvl = 0, left = 0, c[3] = {0, 0, 0};
    bool fresh = true;
    float t[3] = {INFINITY, INFINITY, INFINITY}, lo[3] = {0.f, 0.f, 0.f}, ext[3] = {0.f, 0.f, 0.f}, cur = 0.f, e = 0.f;
    // The exit of a cell is closed form in its index, so the two divisions need not sit in the walk's chain: lane i holds, per
    // axis, the exit of the i-th next cell from the table's base cell (the same statement on the same integer index, so the same
    // bits), `ahead` counts the steps taken on the axis since, and the walk reads its next exit with wave_read.  A trip takes at
    // most 64 steps; the tables are formed again at every trip and at every segment.
    const int dir[3] = {d[0] > 0.f ? 1 : -1, d[1] > 0.f ? 1 : -1, d[2] > 0.f ? 1 : -1};
    float tab[3] = {INFINITY, INFINITY, INFINITY};
    int ahead[3] = {0, 0, 0};
    auto exits_from_here = [&]() {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            tab[a] = trav_exit(c[a] + lane * dir[a], o[a], d[a], lo[a], ext[a], res[a]);
            ahead[a] = 0;
            t[a] = wave_read(tab[a], 0);
        }
    };
    // the samples (wave-uniform): n so far, the last te, the open run [run_a, run_b]
    int n = 0;
    bool open = false, over = false;
    float last_te = -INFINITY, run_a = 0.f, run_b = 0.f;

    // 5. the samples of the closed run [run_a, run_b]
    auto emit = [&]() {
        const float a1 = fmaxf(run_a, last_te);
        float carry = a1;                                            // cone steps: ts of the round's first sample
        for (int k0 = 0;; k0 += 64) {
            float ts, te;
            if (coned) {
                float tt = carry, dt = step;
                ts = tt;
                for (int i = 0; i < 64; i++) {
                    const float di = fminf(fmaxf(tt * cone, step), 1e10f);
                    if (i == lane) {
                        ts = tt;
                        dt = di;
                    }
                    tt = tt + di;
                }
                carry = tt;
                te = ts + dt;
            } else {
                ts = a1 + (float)(k0 + lane) * step;
                te = a1 + (float)(k0 + lane + 1) * step;
            }
            const bool keep = (ts + te) / 2.0f < run_b;
            const unsigned long long mask = __ballot(keep);
            const int pos = n + wave_rank(mask, lane), kept = __popcll(mask);
            if (keep && pos < cap) {
                row_s[pos] = ts;
                row_e[pos] = te;
            }
            if (kept) last_te = wave_read(te, kept - 1);             // the kept ones are lanes 0 .. kept - 1
            n += kept;
            if (n > cap) over = true;                                // the slot row is full: the host marches again
            if (over || mask != ~0ull) break;
        }
    };

    while (j < nseg && !over) {
        // 3. the trip's 64 spans in lockstep; a lane keeps span `lane` (sp_e <= sp_s: no span, or one of no width)
        float sp_s = 0.f, sp_e = 0.f;
        int sp_cell = 0;
        if (!fresh) exits_from_here();
        for (int i = 0; i < 64; i++) {
            if (fresh) {
                float s = 0.f;
                for (; j < nseg; j++) {                              // a segment with e <= s is skipped
                    s = wave_read(T, j);
                    e = wave_read(T, j + 1);
                    if (e > s) break;
                }
                if (j >= nseg) break;
                lvl = j < L - 1 ? L - 1 - j : j - (L - 1);
                const float *b = boxes + lvl * 6;
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    lo[a] = b[a];
                    ext[a] = b[3 + a] - b[a];
                    const float x = o[a] + d[a] * s;
                    const float u = (x - lo[a]) / ext[a];
                    c[a] = min(max((int)floorf(u * (float)res[a]), 0), res[a] - 1);
                }
                exits_from_here();
                cur = s;
                left = span_max;
                fresh = false;
            }
            const float m = fminf(fminf(t[0], t[1]), t[2]);
            const float x = fmaxf(fminf(m, e), cur);
            if (i == lane) {
                sp_s = cur;
                sp_e = x;
                sp_cell = ((lvl * R.x + c[0]) * R.y + c[1]) * R.z + c[2];
            }
            left--;
            if (x >= e) {
                fresh = true;
            } else {
                const int ax = t[0] == m ? 0 : (t[1] == m ? 1 : 2);  // the first axis whose exit is the minimum
#pragma unroll
                for (int a = 0; a < 3; a++)
                    if (a == ax) {
                        c[a] += dir[a];
                        ahead[a]++;
                        if (c[a] < 0 || c[a] >= res[a] || left == 0)
                            fresh = true;
                        else
                            t[a] = wave_read(tab[a], ahead[a] & 63);     // 64 only behind the trip's last span: formed again
                    }
            }
            if (fresh) j++;
            cur = x;
        }
        // 4. runs: the occupied spans among those wider than zero
        const bool wide = sp_e > sp_s;
        const bool occ = wide && binary[sp_cell] != 0;
        unsigned long long v = __ballot(wide), oc = __ballot(occ);
        while (v && !over) {
            if (!open) {
                if (!oc) break;
                const int i = __builtin_ctzll(oc);
                run_a = wave_read(sp_s, i);
                run_b = wave_read(sp_e, i);
                open = true;
                const unsigned long long upto = (2ull << i) - 1ull;  // lanes 0 .. i
                v &= ~upto;
                oc &= ~upto;
            } else {
                const unsigned long long empty = v & ~oc;
                const unsigned long long more = empty ? v & ((1ull << __builtin_ctzll(empty)) - 1ull) : v;
                if (more) run_b = wave_read(sp_e, 63 - __builtin_clzll(more));
                if (!empty) break;                                   // still open behind the trip's last span
                emit();
                open = false;
                const unsigned long long upto = (2ull << __builtin_ctzll(empty)) - 1ull;
                v &= ~upto;
                oc &= ~upto;
            }
        }
    }
    if (open && !over) emit();
    if (lane == 0) {
        ray_cnt[r] = n < cap ? n : cap;
        if (n > cap) atomicOr(overflow, 1);
    }
}

// ---- occupied list: each level's occupied cells in index order, count on the device -------------------------------------
// The scan-and-pack of csrc/visibility.hip: one wavefront per chunk of EST_CHUNK cells counts, the caller scans the chunk counts
// (a cumsum on the device, no host read), the same walk packs.
template <bool PACK>
__global__ __launch_bounds__(256) void est_occ_list_kernel(const uint8_t *__restrict__ binary, int L, int64_t cells,
                                                           int n_chunks, int32_t *__restrict__ chunk_cnt,
                                                           const int32_t *__restrict__ chunk_start,
                                                           int32_t *__restrict__ occ_list) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (int64_t)L * n_chunks) return;
    const int l = (int)(w / n_chunks);
    const int64_t base = (w - (int64_t)l * n_chunks) * EST_CHUNK;
    const uint8_t *row = binary + (int64_t)l * cells;
    int n = 0;
    for (int i = lane; i < EST_CHUNK; i += 64) {
        const int64_t idx = base + i;
        const bool occ = idx < cells && row[idx] != 0;
        const unsigned long long mask = __ballot(occ);
        if (PACK) {
            const int64_t dst = (int64_t)chunk_start[w] + n + wave_rank(mask, lane);
            if (occ && dst >= 0 && dst < cells) occ_list[(int64_t)l * cells + dst] = (int32_t)idx;
        }
        n += __popcll(mask);
    }
    if (!PACK && lane == 0) chunk_cnt[w] = n;
}

// ---- cell selection and the points to evaluate, one launch --------------------------------------------------------------
// Entry i of level l.  Warm-up: cell i.  Afterwards n = 2 k, k = cells / 4: i < k the uniform draw uni[l, i]; behind them the
// occupied draws, with c = occ_cnt[l]: c > k -> the min((int)(u * (float)c), c - 1)-th occupied cell, else the (i - k)-th while
// i - k < c and padding (-1) behind.  Point: x = lo + ((ijk + u) / R) * (hi - lo); padding gets cell 0's.
__global__ __launch_bounds__(256) void est_select_kernel(int warm, int L, int64_t cells, int64_t n, int64_t k,
                                                         const int32_t *__restrict__ uni, const float *__restrict__ u_occ,
                                                         const float *__restrict__ u_pt, const int32_t *__restrict__ occ_list,
                                                         const int32_t *__restrict__ occ_cnt, const float *__restrict__ aabbs,
                                                         EstRes R, int32_t *__restrict__ ids, float *__restrict__ pts) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (int64_t)L * n) return;
    const int l = (int)(gid / n);
    const int64_t i = gid - (int64_t)l * n;
    int64_t id;
    if (warm) {
        id = i;
    } else if (i < k) {
        id = uni[(int64_t)l * k + i];
        if (id < 0 || id >= cells) id = -1;
    } else {
        const int64_t j = i - k;
        int64_t c = occ_cnt[l];
        c = c < 0 ? 0 : (c > cells ? cells : c);
        if (c > k) {
            int64_t p = (int64_t)(int)(u_occ[(int64_t)l * k + j] * (float)c);
            p = p > c - 1 ? c - 1 : p;
            p = p < 0 ? 0 : p;
            id = occ_list[(int64_t)l * cells + p];
        } else {
            id = j < c ? occ_list[(int64_t)l * cells + j] : -1;
        }
        if (id < 0 || id >= cells) id = -1;
    }
    ids[gid] = (int32_t)id;
    const int64_t cell = id < 0 ? 0 : id;
    const int ijk[3] = {(int)(cell / ((int64_t)R.y * R.z)), (int)((cell / R.z) % R.y), (int)(cell % R.z)};
    const int res[3] = {R.x, R.y, R.z};
    const float *b = aabbs + l * 6;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float u = ((float)ijk[a] + u_pt[gid * 3 + a]) / (float)res[a];
        pts[gid * 3 + a] = b[a] + u * (b[3 + a] - b[a]);
    }
}

// ---- EMA-max: occs[cell] = max over the entries naming it of max(old * decay, occ), old not part of the max -------------
// Two passes over the entries: the reset writes old * decay (every duplicate writes the same value), then an integer atomic
// max of the clamped evaluations -- non-negative floats order as their bit patterns.  Padding and invisible cells (old < 0)
// are skipped.  `old` is the caller's copy of occs from before the update.
template <bool MAX>
__global__ __launch_bounds__(256) void est_ema_kernel(const int32_t *__restrict__ ids, const float *__restrict__ occ, int L,
                                                      int64_t n, int64_t cells, const float *__restrict__ old, float decay,
                                                      float *__restrict__ occs) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (int64_t)L * n) return;
    const int64_t id = ids[gid];
    if (id < 0 || id >= cells) return;
    const int64_t idx = (gid / n) * cells + id;
    const float o = old[idx];
    if (!(o >= 0.f)) return;
    if (MAX) {
        float v = occ[gid];
        v = v > 0.f ? v : 0.f;
        atomicMax(reinterpret_cast<int *>(occs + idx), __float_as_int(v));
    } else {
        occs[idx] = o * decay;
    }
}

// ---- threshold and binaries: thre = min(mean(occs[occs >= 0]), cap), the mean summed in float64 in a fixed order --------
__device__ __forceinline__ void est_block_sum(double &s, double &c, double *sh) {
    // only lane 0 is used: the down form this replaces gave lane 0 the butterfly's association (at every step lane 0 adds
    // lane o, whose partner 2 o exists)
    s = wave_sum(s);
    c = wave_sum(c);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sh[wave * 2] = s;
        sh[wave * 2 + 1] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        s = (sh[0] + sh[2]) + (sh[4] + sh[6]);
        c = (sh[1] + sh[3]) + (sh[5] + sh[7]);
    }
}

__global__ __launch_bounds__(256) void est_mean_partial_kernel(const float *__restrict__ occs, int64_t n,
                                                               double *__restrict__ part) {
    __shared__ double sh[8];
    double s = 0.0, c = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = occs[i];
        if (v >= 0.f) {
            s += (double)v;
            c += 1.0;
        }
    }
    est_block_sum(s, c, sh);
    if (threadIdx.x == 0) {
        part[blockIdx.x * 2] = s;
        part[blockIdx.x * 2 + 1] = c;
    }
}

__global__ __launch_bounds__(256) void est_thre_kernel(const double *__restrict__ part, int n_part, float cap,
                                                       float *__restrict__ thre) {
    __shared__ double sh[8];
    double s = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < n_part; i += blockDim.x) {
        s += part[i * 2];
        c += part[i * 2 + 1];
    }
    est_block_sum(s, c, sh);
    if (threadIdx.x == 0) {
        const float mean = c > 0.0 ? (float)(s / c) : NAN;       // no visible cell: the cap alone
        *thre = mean < cap ? mean : cap;
    }
}

__global__ __launch_bounds__(256) void est_binaries_kernel(const float *__restrict__ occs, int64_t n,
                                                           const float *__restrict__ thre, uint8_t *__restrict__ binary) {
    const float t = *thre;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        binary[i] = occs[i] > t ? 1 : 0;
}

// ---- mark_invisible_cells: one thread per cell, every camera in turn (OpenCV convention) --------------------------------
// x = lo + ijk / (R - 1) * (hi - lo);  x_c = R^T x - R^T t;  uvd = K x_c;  in the image iff d >= 0, 0 <= u / d < width and
// 0 <= v / d < height.  Visible iff some camera has the cell in the image with d >= near_plane and none has it in the image
// with d < near_plane.  Sums of three products are (p0 + p1) + p2.
__global__ __launch_bounds__(256) void est_mark_invisible_kernel(const float *__restrict__ K, const float *__restrict__ c2w,
                                                                 int C, float width, float height, float near_plane,
                                                                 const float *__restrict__ aabbs, int L, int64_t cells,
                                                                 EstRes R, float *__restrict__ occs) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (int64_t)L * cells) return;
    const int l = (int)(gid / cells);
    const int64_t cell = gid - (int64_t)l * cells;
    const int ijk[3] = {(int)(cell / ((int64_t)R.y * R.z)), (int)((cell / R.z) % R.y), (int)(cell % R.z)};
    const int res[3] = {R.x, R.y, R.z};
    const float *b = aabbs + l * 6;
    float x[3];
#pragma unroll
    for (int a = 0; a < 3; a++) x[a] = b[a] + ((float)ijk[a] / (float)(res[a] - 1)) * (b[3 + a] - b[a]);
    bool seen = false, too_near = false;
    for (int cam = 0; cam < C; cam++) {
        const float *m = c2w + (int64_t)cam * 12;      // [3,4] row-major: m[4 i + j], translation m[4 i + 3]
        const float *k = K + (int64_t)cam * 9;
        float xc[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float rx = (m[a] * x[0] + m[4 + a] * x[1]) + m[8 + a] * x[2];
            const float rt = (m[a] * m[3] + m[4 + a] * m[7]) + m[8 + a] * m[11];
            xc[a] = rx - rt;
        }
        float uvd[3];
#pragma unroll
        for (int a = 0; a < 3; a++) uvd[a] = (k[3 * a] * xc[0] + k[3 * a + 1] * xc[1]) + k[3 * a + 2] * xc[2];
        const float dd = uvd[2], u = uvd[0] / dd, v = uvd[1] / dd;
        const bool in = dd >= 0.f && u >= 0.f && u < width && v >= 0.f && v < height;
        seen = seen || (in && dd >= near_plane);
        too_near = too_near || (in && dd < near_plane);
    }
    occs[gid] = (seen && !too_near) ? 0.f : -1.f;
}

// ------------------------------------------------------------------------------------------------------------ C ABI
static inline bool est_grid_ok(int32_t L, int32_t Rx, int32_t Ry, int32_t Rz) {
    if (L < 1 || L > EST_MAX_LEVELS || Rx <= 0 || Ry <= 0 || Rz <= 0) return false;
    return (int64_t)L * Rx * Ry * Rz <= 0x7fffffffLL;
}

extern "C" int32_t mh_est_occ_chunk(void) { return EST_CHUNK; }
extern "C" int32_t mh_est_max_partials(void) { return EST_MAX_PARTIALS; }

// steps a ray of unit-or-longer direction can take: every step is at least `step` long and lies inside both the coarsest
// box (its longest chord is the diagonal) and [near_plane, far_plane].
// The same bound holds the traversal's slot row (mh_est_traverse_slots): its samples are at least `step` long as well, they are
// disjoint (a run starts at max(run start, the last te)), every ts >= t_near and every ts < t_far (a kept sample's midpoint lies
// before its run's end <= t_far), so at most (t_far - t_near) / step + 1 of them fit -- inside the + 4.
extern "C" int32_t mh_est_march_cap(float step, float diagonal, float near_plane, float far_plane) {
    if (!(step > 0.f) || !(diagonal > 0.f)) return 0;
    double len = (double)diagonal;
    const double planes = (double)far_plane - (double)near_plane;
    if (planes < len) len = planes > 0.0 ? planes : 0.0;
    const double n = len / (double)step;
    if (!(n < 1073741824.0)) return 0;
    return (int32_t)n + 4;
}

// the two placements share the argument list, the argument rules and the launch shape
template <typename Kernel>
static inline int est_slots_launch(Kernel kernel, const float *rays_o, const float *rays_d, const float *jitter, const float *t_min,
                                   const float *t_max, int32_t N, float step, float cone_angle, float near_plane, float far_plane,
                                   const float *aabbs, int32_t L, int32_t Rx, int32_t Ry, int32_t Rz, const uint8_t *binary,
                                   int32_t cap, int32_t *ray_cnt, float *slot_ts, float *slot_te, int32_t *overflow, void *stream) {
    if (N == 0) return MH_OK;
    if (!rays_o || !rays_d || !aabbs || !binary || !ray_cnt || !slot_ts || !slot_te || !overflow || N < 0 ||
        !est_grid_ok(L, Rx, Ry, Rz) || !(step > 0.f) || !(cone_angle >= 0.f) || cap <= 0 || near_plane != near_plane ||
        far_plane != far_plane)
        return MH_ERR_ARG;
    const EstRes R = {Rx, Ry, Rz};
    hipLaunchKernelGGL(kernel, dim3((N + 3) / 4), dim3(256), 0, mh_stream(stream), rays_o, rays_d, jitter, t_min, t_max, (int)N,
                       step, cone_angle, near_plane, far_plane, aabbs, (int)L, R, binary, (int)cap, ray_cnt, slot_ts, slot_te,
                       overflow);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_est_march_slots(const float *rays_o, const float *rays_d, const float *jitter, const float *t_min,
                                  const float *t_max, int32_t N, float step, float cone_angle, float near_plane,
                                  float far_plane, const float *aabbs, int32_t L, int32_t Rx, int32_t Ry, int32_t Rz,
                                  const uint8_t *binary, int32_t cap, int32_t *ray_cnt, float *slot_ts, float *slot_te,
                                  int32_t *overflow, void *stream) {
    return est_slots_launch(est_march_kernel, rays_o, rays_d, jitter, t_min, t_max, N, step, cone_angle, near_plane, far_plane,
                            aabbs, L, Rx, Ry, Rz, binary, cap, ray_cnt, slot_ts, slot_te, overflow, stream);
}

extern "C" int mh_est_traverse_slots(const float *rays_o, const float *rays_d, const float *jitter, const float *t_min,
                                     const float *t_max, int32_t N, float step, float cone_angle, float near_plane,
                                     float far_plane, const float *aabbs, int32_t L, int32_t Rx, int32_t Ry, int32_t Rz,
                                     const uint8_t *binary, int32_t cap, int32_t *ray_cnt, float *slot_ts, float *slot_te,
                                     int32_t *overflow, void *stream) {
    return est_slots_launch(est_traverse_kernel, rays_o, rays_d, jitter, t_min, t_max, N, step, cone_angle, near_plane, far_plane,
                            aabbs, L, Rx, Ry, Rz, binary, cap, ray_cnt, slot_ts, slot_te, overflow, stream);
}

static inline unsigned est_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

extern "C" int mh_est_occ_count(const uint8_t *binary, int32_t L, int64_t cells, int32_t *chunk_cnt, void *stream) {
    if (!binary || !chunk_cnt || L < 1 || L > EST_MAX_LEVELS || cells <= 0 || (int64_t)L * cells > 0x7fffffffLL) return MH_ERR_ARG;
    const int n_chunks = (int)((cells + EST_CHUNK - 1) / EST_CHUNK);
    hipLaunchKernelGGL(est_occ_list_kernel<false>, dim3((unsigned)(((int64_t)L * n_chunks + 3) / 4)), dim3(256), 0,
                       mh_stream(stream), binary, (int)L, cells, n_chunks, chunk_cnt, (const int32_t *)nullptr,
                       (int32_t *)nullptr);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_est_occ_pack(const uint8_t *binary, int32_t L, int64_t cells, const int32_t *chunk_start,
                               int32_t *occ_list, void *stream) {
    if (!binary || !chunk_start || !occ_list || L < 1 || L > EST_MAX_LEVELS || cells <= 0 || (int64_t)L * cells > 0x7fffffffLL)
        return MH_ERR_ARG;
    const int n_chunks = (int)((cells + EST_CHUNK - 1) / EST_CHUNK);
    hipLaunchKernelGGL(est_occ_list_kernel<true>, dim3((unsigned)(((int64_t)L * n_chunks + 3) / 4)), dim3(256), 0,
                       mh_stream(stream), binary, (int)L, cells, n_chunks, (int32_t *)nullptr, chunk_start, occ_list);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_est_select(int32_t warmup, int32_t L, int32_t Rx, int32_t Ry, int32_t Rz, int64_t n, const int32_t *uniform,
                             const float *u_occ, const float *u_point, const int32_t *occ_list, const int32_t *occ_cnt,
                             const float *aabbs, int32_t *ids, float *points, void *stream) {
    if (!est_grid_ok(L, Rx, Ry, Rz) || n < 0) return MH_ERR_ARG;
    if (n == 0) return MH_OK;
    const int64_t cells = (int64_t)Rx * Ry * Rz, k = cells / 4;
    if (!u_point || !aabbs || !ids || !points || (int64_t)L * n > 0x7fffffffLL / 3) return MH_ERR_ARG;
    if (warmup ? n != cells : (n != 2 * k || !uniform || !u_occ || !occ_list || !occ_cnt)) return MH_ERR_ARG;
    const EstRes R = {Rx, Ry, Rz};
    hipLaunchKernelGGL(est_select_kernel, dim3(est_blocks((int64_t)L * n)), dim3(256), 0, mh_stream(stream), warmup ? 1 : 0,
                       (int)L, cells, n, k, uniform, u_occ, u_point, occ_list, occ_cnt, aabbs, R, ids, points);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_est_ema(const int32_t *ids, const float *occ, int32_t L, int64_t n, int64_t cells, const float *old_occs,
                          float decay, float *occs, void *stream) {
    if (L < 1 || L > EST_MAX_LEVELS || n < 0 || cells <= 0 || (int64_t)L * cells > 0x7fffffffLL || !(decay >= 0.f)) return MH_ERR_ARG;
    if (n == 0) return MH_OK;
    if (!ids || !occ || !old_occs || !occs || old_occs == occs || (int64_t)L * n > 0x7fffffffLL) return MH_ERR_ARG;
    hipLaunchKernelGGL(est_ema_kernel<false>, dim3(est_blocks((int64_t)L * n)), dim3(256), 0, mh_stream(stream), ids, occ, (int)L,
                       n, cells, old_occs, decay, occs);
    MH_CHECK_LAUNCH();
    hipLaunchKernelGGL(est_ema_kernel<true>, dim3(est_blocks((int64_t)L * n)), dim3(256), 0, mh_stream(stream), ids, occ, (int)L,
                       n, cells, old_occs, decay, occs);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_est_threshold(const float *occs, int64_t n, float cap, double *partials, float *thre, uint8_t *binaries,
                                void *stream) {
    if (!occs || !partials || !thre || n <= 0 || n > 0x7fffffffLL || cap != cap) return MH_ERR_ARG;
    int64_t blocks = (n + 2047) / 2048;
    if (blocks > EST_MAX_PARTIALS) blocks = EST_MAX_PARTIALS;
    hipLaunchKernelGGL(est_mean_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, mh_stream(stream), occs, n, partials);
    MH_CHECK_LAUNCH();
    hipLaunchKernelGGL(est_thre_kernel, dim3(1), dim3(256), 0, mh_stream(stream), (const double *)partials, (int)blocks, cap, thre);
    MH_CHECK_LAUNCH();
    if (binaries) {
        int64_t bb = (n + 255) / 256;
        if (bb > 4096) bb = 4096;
        hipLaunchKernelGGL(est_binaries_kernel, dim3((unsigned)bb), dim3(256), 0, mh_stream(stream), occs, n, (const float *)thre,
                           binaries);
        MH_CHECK_LAUNCH();
    }
    return MH_OK;
}

extern "C" int mh_est_mark_invisible(const float *K, const float *c2w, int32_t C, float width, float height, float near_plane,
                                     const float *aabbs, int32_t L, int32_t Rx, int32_t Ry, int32_t Rz, float *occs,
                                     void *stream) {
    if (!est_grid_ok(L, Rx, Ry, Rz) || C < 0 || (C > 0 && (!K || !c2w)) || !aabbs || !occs || !(width > 0.f) || !(height > 0.f) ||
        near_plane != near_plane)
        return MH_ERR_ARG;
    const int64_t cells = (int64_t)Rx * Ry * Rz;
    const EstRes R = {Rx, Ry, Rz};
    hipLaunchKernelGGL(est_mark_invisible_kernel, dim3(est_blocks((int64_t)L * cells)), dim3(256), 0, mh_stream(stream), K, c2w,
                       (int)C, width, height, near_plane, aabbs, (int)L, cells, R, occs);
    MH_CHECK_LAUNCH();
    return MH_OK;
}
