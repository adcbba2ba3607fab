// What the dense marching cubes (mesh.hip) and the one over the block-sparse TSDF store (tsdf_sparse.hip) share: the case table,
// the edge numbering, the workgroup scans and the vertex formula.  Conventions: include/morpheus_hip.h (marching cubes).
#pragma once
#include "common.h"
#include "wave.h"

#define MC_THREADS 256
#define MC_WAVES (MC_THREADS / MH_WAVE)
#define MC_SCAN_THREADS 1024

// one word per cube case: edge nibbles from bit 0, triangle count in bits 60-63 (tools/gen_mc_table.py)
static __constant__ uint64_t kMcTable[256] = {
#include "mc_table.inc"
};

// edge e of the cell at p: owner corner (dx | dy << 1 | dz << 2) and axis (0 x, 1 y, 2 z) -- Bourke's edge numbering
static __constant__ uint8_t kMcEdgeOwner[12] = {0, 1, 2, 0, 4, 5, 6, 4, 0, 1, 3, 2};
static __constant__ uint8_t kMcEdgeAxis[12] = {0, 1, 0, 1, 0, 1, 0, 1, 2, 2, 2, 2};

static inline int64_t mc_align(int64_t b) { return (b + 255) & ~(int64_t)255; }

// exclusive prefix of a small count (< 8) over the workgroup: three ballots per wave, wave totals through LDS.  Returns the
// thread's offset; *total = the workgroup's sum.  `red` holds MC_WAVES ints; one barrier pair per call.
__device__ __forceinline__ int mc_block_scan(int v, int *red, int *total) {
    const int lane = mh_lane(), wave = threadIdx.x >> 6;
    int pre = 0, wsum = 0;
#pragma unroll
    for (int b = 0; b < 3; b++) {
        const uint64_t bal = __ballot((v >> b) & 1);
        pre += wave_rank(bal, lane) << b;
        wsum += __popcll(bal) << b;
    }
    if (lane == 0) red[wave] = wsum;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < MC_WAVES; w++) {
        const int t = red[w];
        before += (w < wave) ? t : 0;
        all += t;
    }
    __syncthreads();                                           // red is reused by the next call
    *total = all;
    return before + pre;
}

// one workgroup: tile_off[2t + c] = sum of tile_tot[2u + c] over u < t (t = 0..tiles), counts = the grand totals.  Thread
// r takes a contiguous run of tiles: sum, scan of the run sums through LDS, then the run again with its offset.
static __global__ __launch_bounds__(MC_SCAN_THREADS) void mc_scan_kernel(const int64_t *__restrict__ tile_tot, int64_t tiles,
                                                                  int64_t *__restrict__ tile_off, int64_t *__restrict__ counts) {
    __shared__ int64_t part[2][MC_SCAN_THREADS];
    const int64_t run = (tiles + MC_SCAN_THREADS - 1) / MC_SCAN_THREADS;
    const int64_t lo = min(tiles, (int64_t)threadIdx.x * run), hi = min(tiles, lo + run);
    int64_t sv = 0, st = 0;
    for (int64_t u = lo; u < hi; u++) {
        sv += tile_tot[2 * u];
        st += tile_tot[2 * u + 1];
    }
    part[0][threadIdx.x] = sv;
    part[1][threadIdx.x] = st;
    __syncthreads();
    // Hillis-Steele inclusive scan of the run sums (1024 entries, 10 steps)
    for (int o = 1; o < MC_SCAN_THREADS; o <<= 1) {
        const int64_t av = threadIdx.x >= o ? part[0][threadIdx.x - o] : 0;
        const int64_t at = threadIdx.x >= o ? part[1][threadIdx.x - o] : 0;
        __syncthreads();
        part[0][threadIdx.x] += av;
        part[1][threadIdx.x] += at;
        __syncthreads();
    }
    int64_t ov = part[0][threadIdx.x] - sv, ot = part[1][threadIdx.x] - st;
    for (int64_t u = lo; u < hi; u++) {
        tile_off[2 * u] = ov;
        tile_off[2 * u + 1] = ot;
        ov += tile_tot[2 * u];
        ot += tile_tot[2 * u + 1];
    }
    if (threadIdx.x == MC_SCAN_THREADS - 1) {
        tile_off[2 * tiles] = part[0][threadIdx.x];
        tile_off[2 * tiles + 1] = part[1][threadIdx.x];
        counts[0] = part[0][threadIdx.x];
        counts[1] = part[1][threadIdx.x];
    }
}

// vertex on the edge from p (value f0) to p + e_axis (value f1): coord_axis = p_axis + t, t = (iso - f0) / (f1 - f0), 0.5
// when that is not in [0, 1] (NaN / inf corners).  One IEEE division and one addition (the file is built without FP
// contraction).
__device__ __forceinline__ float mc_t(float iso, float f0, float f1) {
    float t = (iso - f0) / (f1 - f0);
    if (!(t >= 0.f && t <= 1.f)) t = 0.5f;
    return t;
}
