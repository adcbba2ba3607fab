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
// box (its longest chord is the diagonal) and [near_plane, far_plane]
extern "C" int32_t mh_est_march_cap(float step, float diagonal, float near_plane, float far_plane) {
    if (!(step > 0.f) || !(diagonal > 0.f)) return 0;
    double len = (double)diagonal;
    const double planes = (double)far_plane - (double)near_plane;
    if (planes < len) len = planes > 0.0 ? planes : 0.0;
    const double n = len / (double)step;
    if (!(n < 1073741824.0)) return 0;
    return (int32_t)n + 4;
}

extern "C" int mh_est_march_slots(const float *rays_o, const float *rays_d, const float *jitter, const float *t_min,
                                  const float *t_max, int32_t N, float step, float cone_angle, float near_plane,
                                  float far_plane, const float *aabbs, int32_t L, int32_t Rx, int32_t Ry, int32_t Rz,
                                  const uint8_t *binary, int32_t cap, int32_t *ray_cnt, float *slot_ts, float *slot_te,
                                  int32_t *overflow, void *stream) {
    if (N == 0) return MH_OK;
    if (!rays_o || !rays_d || !aabbs || !binary || !ray_cnt || !slot_ts || !slot_te || !overflow || N < 0 ||
        !est_grid_ok(L, Rx, Ry, Rz) || !(step > 0.f) || !(cone_angle >= 0.f) || cap <= 0 || near_plane != near_plane ||
        far_plane != far_plane)
        return MH_ERR_ARG;
    const EstRes R = {Rx, Ry, Rz};
    hipLaunchKernelGGL(est_march_kernel, dim3((N + 3) / 4), dim3(256), 0, mh_stream(stream), rays_o, rays_d, jitter, t_min,
                       t_max, (int)N, step, cone_angle, near_plane, far_plane, aabbs, (int)L, R, binary, (int)cap, ray_cnt,
                       slot_ts, slot_te, overflow);
    MH_CHECK_LAUNCH();
    return MH_OK;
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
