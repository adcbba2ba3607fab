// Multiresolution hash-grid encoder, forward + backward, for gfx950.
//
// Semantics: reference external/encoders/gridencoder/src/gridencoder.cu
//   kernel_grid :83-249, kernel_grid_backward :253-349, kernel_input_backward :353-378,
//   get_grid_index :61-79, fast_hash :45-58; host logic grid.py:28-96, :157.
// Design (MI355X-first, not the reference's launch shape):
//   * one lane per (point, level); a wavefront = 4 points x 16 levels, level fastest.  A point's
//     32 features are produced by 16 adjacent lanes -> every store instruction writes 4 x 128 B
//     contiguous rows of the point-major [M, L*2] output (what the MFMA field kernel consumes);
//     no [L,B,C] intermediate and no permute.
//   * level metadata (offsets, resolutions) travels by value in the kernarg segment (SGPRs);
//     resolutions are host-computed float32 ceil(exp2f(l*S)*H) so oracle and kernel agree.
//   * backward recomputes corner indices/weights (no [M, L*3*2] dy_dx tensor: 805 MB at
//     M = 2.1M in the reference); d/dx is reduced over the 16 level-lanes of a point with DPP
//     row operations, embedding gradients go out as fp32 atomics (same as the reference).
//   * both tables (3.2 MB each) are L2-resident per XCD; gathers are 8-byte float2 loads.
// The cell rule (grid_locate), the level table (GridMeta) and the fixed-point rule of the table gradient (fx_scales, the absmax
// and finalize kernels) are grid.h's, shared with hashgrid_general.hip; the row former of this instantiation (grid_rows8) and the
// brick kernels' own rounding trick (FX_MAGIC) are here.
#include "common.h"
#include "wave.h"
#include "grid.h"
#include <stdlib.h>
#include <algorithm>
#include <atomic>
#include <cmath>

// explicit fmaf where the reference kernel (nvcc -fmad=true) fuses, nothing else contracted:
// the CPU oracle does the same, so features agree to the last bit of the interpolation.
#pragma clang fp contract(off)

// the rows of a cell's eight corners (corner c: bit 0 -> x + 1, bit 1 -> y + 1, bit 2 -> z + 1) by get_grid_index
// (gridencoder.cu:61-79): dense x + y*res + z*res^2 (< res^3 <= T: the modulo is the identity) while the running stride fits, else
// the xor-prime hash modulo T; for D=3 "stride > T after the loop" <=> res^3 > T.  The per-axis terms are formed ONCE for the two
// y and the two z values -- four 32-bit multiplies (v_mul_lo_u32: quarter rate) per cell instead of two or three per corner
__device__ __forceinline__ void grid_rows8(const uint32_t (&g)[3], const uint32_t (&g1)[3], uint32_t res, uint32_t T, bool dense,
                                           bool pow2, uint32_t (&row)[8]) {
    // branch-free over the lanes of a wave (its 16 level-lanes mix dense and hashed levels, and a divergent branch per corner cost
    // ~100 scalar instructions and 30 taken branches per point): the axis multipliers are selected once, both combinations are
    // formed (two adds / two xors per corner pair) and one select keeps the lane's.  A hashed level whose table size is NOT a
    // power of two (no shipped geometry has one: a hashed level's size is the 2^k cap) takes the modulo in ONE rarely entered
    // branch for all eight corners.
    const uint32_t my = dense ? res : 2654435761u, mz = dense ? res * res : 805459861u;
    const uint32_t ay[2] = {g[1] * my, g1[1] * my}, az[2] = {g[2] * mz, g1[2] * mz};
    // (the select is a bit merge, v_bfi_b32, on a per-lane all-ones / all-zeros word: written as `dense ? a : b` hipcc turns it
    //  back into eight divergent branches)
    const uint32_t mask = pow2 ? T - 1 : 0xffffffffu, sel = dense ? 0xffffffffu : 0u;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const uint32_t cx = (c & 1) ? g1[0] : g[0], y = ay[(c >> 1) & 1], z = az[(c >> 2) & 1];
        row[c] = ((cx + y + z) & sel) | ((cx ^ y ^ z) & mask & ~sel);
    }
    if (__builtin_expect(!dense && !pow2, 0)) {
#pragma unroll
        for (int c = 0; c < 8; c++) row[c] %= T;
    }
}

__global__ __launch_bounds__(256) void grid_fwd_kernel(const float *__restrict__ x, const float2 *__restrict__ emb, GridMeta meta,
                                                       float2 *__restrict__ out, int64_t M, int L, int n_levels, float bound,
                                                       float two_bound) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = gid / L;
    const int l = (int)(gid - p * L);
    if (p >= M) return;
    float2 r = make_float2(0.f, 0.f);
    if (l < n_levels) {
        const uint32_t res = (uint32_t)meta.res[l];
        const uint32_t T = (uint32_t)(meta.offsets[l + 1] - meta.offsets[l]);
        const bool dense = (uint64_t)res * res * res <= (uint64_t)T;
        const bool pow2 = (T & (T - 1)) == 0;
        uint32_t g[3];
        float f[3];
        if (grid_locate(x, p, bound, two_bound, res, g, f)) {
            const float2 *tab = emb + meta.offsets[l];
            const uint32_t g1[3] = {min(g[0] + 1, res - 1), min(g[1] + 1, res - 1), min(g[2] + 1, res - 1)};
            uint32_t row[8];
            grid_rows8(g, g1, res, T, dense, pow2, row);
            float2 v[8];
#pragma unroll
            for (int c = 0; c < 8; c++) v[c] = tab[row[c]];
#pragma unroll
            for (int c = 0; c < 8; c++) {
                float w = ((c & 1) ? f[0] : 1.f - f[0]) * ((c & 2) ? f[1] : 1.f - f[1]) * ((c & 4) ? f[2] : 1.f - f[2]);
                r.x = fmaf(w, v[c].x, r.x);
                r.y = fmaf(w, v[c].y, r.y);
            }
        }
    }
    out[gid] = r;
}

// Grouped forward: every G consecutive points are known to lie close together (the six finite-difference taps of one
// sample, models/model.py:367-385, laid out point-major) -- a lane walks the G points of its (group, level) and keeps the
// last cell's eight corner values in registers, so taps that share a cell (94 % of them on average: the tap offset is
// 0.13 of the finest cell) cost no gathers.  Per-point arithmetic is the ungrouped kernel's: results are bit-identical.
template <int G>
__global__ __launch_bounds__(256) void grid_fwd_grouped_kernel(const float *__restrict__ x, const float2 *__restrict__ emb,
                                                               GridMeta meta, float2 *__restrict__ out, int64_t n_groups,
                                                               int L, int n_levels, float bound, float two_bound) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t grp = gid / L;
    const int l = (int)(gid - grp * L);
    if (grp >= n_groups) return;
    if (l >= n_levels) {
#pragma unroll
        for (int i = 0; i < G; i++) out[(grp * G + i) * L + l] = make_float2(0.f, 0.f);
        return;
    }
    const uint32_t res = (uint32_t)meta.res[l];
    const uint32_t T = (uint32_t)(meta.offsets[l + 1] - meta.offsets[l]);
    const bool dense = (uint64_t)res * res * res <= (uint64_t)T;
    const bool pow2 = (T & (T - 1)) == 0;
    const float2 *tab = emb + meta.offsets[l];
    float2 v[8];
    uint32_t cg[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};  // cached cell
#pragma unroll
    for (int i = 0; i < G; i++) {
        const int64_t p = grp * G + i;
        uint32_t g[3];
        float f[3];
        float2 r = make_float2(0.f, 0.f);
        if (grid_locate(x, p, bound, two_bound, res, g, f)) {
            if (g[0] != cg[0] || g[1] != cg[1] || g[2] != cg[2]) {
                const uint32_t g1[3] = {min(g[0] + 1, res - 1), min(g[1] + 1, res - 1), min(g[2] + 1, res - 1)};
                uint32_t row[8];
                grid_rows8(g, g1, res, T, dense, pow2, row);
#pragma unroll
                for (int c = 0; c < 8; c++) v[c] = tab[row[c]];
                cg[0] = g[0], cg[1] = g[1], cg[2] = g[2];
            }
#pragma unroll
            for (int c = 0; c < 8; c++) {
                float w = ((c & 1) ? f[0] : 1.f - f[0]) * ((c & 2) ? f[1] : 1.f - f[1]) * ((c & 4) ? f[2] : 1.f - f[2]);
                r.x = fmaf(w, v[c].x, r.x);
                r.y = fmaf(w, v[c].y, r.y);
            }
        }
        out[p * L + l] = r;
    }
}

// d(loss)/d(pos) of one (point, level): dy_dx (gridencoder.cu:205-247) is res * the sum over the 4 corners of the other two axes
// of w_other * (table[right] - table[left]) per channel (the border clamp ignored on purpose), and the loss gradient contracts the
// two channels.  The contraction goes FIRST here -- s_c = gr . table[corner c], eight dot products -- so the three axis sums run on
// one scalar per corner instead of two channels: 55 VALU instructions instead of 134 for the same sum of the same products
// (associated differently: fp32 rounding-level differences to the channel-wise form, and to the reference's, which sums the
// per-level rows in a torch reduction of unspecified order anyway).
__device__ __forceinline__ void grid_ddx(const float2 (&v)[8], const float (&f)[3], float2 gr, float s, float (&dx)[3]) {
    float sc[8];
#pragma unroll
    for (int c = 0; c < 8; c++) sc[c] = fmaf(gr.y, v[c].y, gr.x * v[c].x);
    const float p[3][2] = {{1.f - f[0], f[0]}, {1.f - f[1], f[1]}, {1.f - f[2], f[2]}};
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const int a = (d + 1) % 3, b = (d + 2) % 3;
        float acc = 0.f;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int ba = q & 1, bb = (q >> 1) & 1;
            const int lo_c = (ba << a) | (bb << b), hi_c = lo_c | (1 << d);
            const float w = p[a][ba] * p[b][bb], diff = sc[hi_c] - sc[lo_c];
            acc = q ? fmaf(w, diff, acc) : w * diff;
        }
        dx[d] = s * acc;
    }
}

// sum over the 16 level-lanes of a point (an aligned group of 16 lanes = one DPP row), every lane gets the total.  The butterfly
// v += v[lane ^ 1], ^ 2, ^ 4, ^ 8 written as DPP operands of the adds: quad_perm [1,0,3,2], quad_perm [2,3,0,1], then
// row_half_mirror (lane i <-> 7 - i: after the first two steps a quad's lanes agree, and 7 - i lies in the other quad of the half
// row -- the value lane i ^ 4 holds) and row_mirror (i <-> 15 - i, the other half row).  The same additions in the same order as the
// __shfl_xor form, which hipcc turns into twelve ds_bpermute_b32 per point: LDS-pipe instructions with a round trip each, in the
// middle of the brick backward's dependent chain.
#define DPP_ADD(v, ctrl) ((v) + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), (ctrl), 0xf, 0xf, true)))
__device__ __forceinline__ float sum16(float v) {
    v = DPP_ADD(v, 0xB1);    // quad_perm:[1,0,3,2]
    v = DPP_ADD(v, 0x4E);    // quad_perm:[2,3,0,1]
    v = DPP_ADD(v, 0x141);   // row_half_mirror
    v = DPP_ADD(v, 0x140);   // row_mirror
    return v;
}

template <bool NEED_DX>
__global__ __launch_bounds__(256) void grid_bwd_kernel(const float2 *__restrict__ grad, const float *__restrict__ x,
                                                       const float2 *__restrict__ emb, GridMeta meta,
                                                       float *__restrict__ grad_emb, float *__restrict__ grad_x,
                                                       int64_t M, int L, int n_levels, float bound, float two_bound) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t p = gid / L;
    const int l = (int)(gid - p * L);
    const bool live = p < M;
    if (!live) p = M - 1;  // keep whole 16-lane groups converged for the shuffles
    float dx[3] = {0.f, 0.f, 0.f};
    if (live && l < n_levels) {
        const uint32_t res = (uint32_t)meta.res[l];
        const uint32_t T = (uint32_t)(meta.offsets[l + 1] - meta.offsets[l]);
        const bool dense = (uint64_t)res * res * res <= (uint64_t)T;
        const bool pow2 = (T & (T - 1)) == 0;
        uint32_t g[3];
        float f[3];
        if (grid_locate(x, p, bound, two_bound, res, g, f)) {
            const float2 gr = grad[gid];
            const uint32_t g1[3] = {min(g[0] + 1, res - 1), min(g[1] + 1, res - 1), min(g[2] + 1, res - 1)};
            uint32_t row[8];
            grid_rows8(g, g1, res, T, dense, pow2, row);
            float *ge = grad_emb + (size_t)meta.offsets[l] * 2;
#pragma unroll
            for (int c = 0; c < 8; c++) {
                float w = ((c & 1) ? f[0] : 1.f - f[0]) * ((c & 2) ? f[1] : 1.f - f[1]) * ((c & 4) ? f[2] : 1.f - f[2]);
                atomicAdd(ge + (size_t)row[c] * 2 + 0, w * gr.x);
                atomicAdd(ge + (size_t)row[c] * 2 + 1, w * gr.y);
            }
            if (NEED_DX) {
                // dy_dx (gridencoder.cu:205-247): res * sum over the 4 corners of the other two axes of
                // w_other * (table[right] - table[left]); ignores the border clamp on purpose.
                const float2 *tab = emb + meta.offsets[l];
                float2 v[8];
#pragma unroll
                for (int c = 0; c < 8; c++) v[c] = tab[row[c]];
                grid_ddx(v, f, gr, (float)res, dx);
            }
        }
    }
    if (NEED_DX) {
        // L == 16: the point's levels are one aligned 16-lane group
        float sx = sum16(dx[0]), sy = sum16(dx[1]), sz = sum16(dx[2]);
        if (live && l == 0) {
            const float inv = 1.0f / two_bound;  // chain factor of u = (x + bound) / (2 bound)
            grad_x[p * 3 + 0] = sx * inv;
            grad_x[p * 3 + 1] = sy * inv;
            grad_x[p * 3 + 2] = sz * inv;
        }
    }
}


// =====================================================================================
// Brick-binned backward.
// Device-scope float atomics on MI355X execute memory-side (the per-XCD L2s are not coherent), at
// ~12 G transactions/s: the reference's formulation -- 16 atomics per (point, level) -- costs 43 ms
// for 2.1 M points.  Here the points are counting-sorted into 16^3 spatial bricks once per step
// (shared by both encoders); one workgroup owns one brick, accumulates every level's vertex
// gradients of its points in LDS (73 KB: sum over levels of (ceil(res/16)+2)^3 vertices x 2 channels
// of int64 fixed point), and only the touched vertices are flushed with global atomics -- the 8
// corner contributions of neighbouring samples collapse on-chip first.  (The on-chip accumulation is
// 64-bit fixed point, see fx_scales in grid.h.)
// =====================================================================================
#define BRK 16
#define NBRK (BRK * BRK * BRK)
#define BRK_NODES_MAX 4608   // >= sum_l (ceil(res_l/16)+2)^3 for the 16-level 16..128 pyramid (4558)

#define BRK_ACC_ROWS 1152    // the staged backward's accumulator: rows of 128 bytes = 16 words of 8 (144 KB; with flush_par and item < 160 KB)

struct BrickMeta {
    int32_t n[MH_MAX_LEVELS];        // LDS vertices per axis at level l
    int32_t lds_off[MH_MAX_LEVELS];  // first LDS vertex of level l
    // the staged backward's accumulator (brick_layout): word k {sum x, sum y, table row} of vertex li of level l is at byte
    // cbase[k][l] + li * stride
    int32_t cbase[3][16];
    int32_t stride;
};

__device__ __forceinline__ int brick_of(const float *__restrict__ x, int64_t p, float bound, float two_bound) {
    int b[3];
    const float inv = 1.0f / two_bound;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const float u = grid_unit(x[p * 3 + d], bound, two_bound, inv);
        if (!grid_in_box(u)) return NBRK;  // out of range (or not finite): no gradient (gridencoder.cu:279-284)
        b[d] = min((int)floorf(u * (float)BRK), BRK - 1);
    }
    return (b[2] * BRK + b[1]) * BRK + b[0];
}

__global__ __launch_bounds__(256) void bin_hist_kernel(const float *__restrict__ x, int64_t M, int64_t chunk, float bound,
                                                       float two_bound, int32_t *__restrict__ block_hist) {
    __shared__ int hist[NBRK + 1];
    for (int i = threadIdx.x; i <= NBRK; i += 256) hist[i] = 0;
    __syncthreads();
    const int64_t p0 = (int64_t)blockIdx.x * chunk, p1 = min(p0 + chunk, M);
    for (int64_t p = p0 + threadIdx.x; p < p1; p += 256) atomicAdd(&hist[brick_of(x, p, bound, two_bound)], 1);
    __syncthreads();
    for (int i = threadIdx.x; i <= NBRK; i += 256) block_hist[(int64_t)blockIdx.x * (NBRK + 1) + i] = hist[i];
}

// one thread per brick: exclusive scan of its counts over the G blocks
__global__ __launch_bounds__(256) void bin_colscan_kernel(int32_t *__restrict__ block_hist, int G,
                                                          int32_t *__restrict__ brick_cnt) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b > NBRK) return;
    int run = 0, g = 0;
    // 8 loads in flight per round trip (a plain in-place loop is one dependent L2 round trip per block row)
    for (; g + 8 <= G; g += 8) {
        int c[8];
#pragma unroll
        for (int k = 0; k < 8; k++) c[k] = block_hist[(int64_t)(g + k) * (NBRK + 1) + b];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            block_hist[(int64_t)(g + k) * (NBRK + 1) + b] = run;
            run += c[k];
        }
    }
    for (; g < G; g++) {
        const int c = block_hist[(int64_t)g * (NBRK + 1) + b];
        block_hist[(int64_t)g * (NBRK + 1) + b] = run;
        run += c;
    }
    brick_cnt[b] = run;
}

// single block: exclusive scans over the NBRK+1 brick totals -> brick_start[NBRK+2], and over the
// per-brick work-item counts ceil(cnt/chunk) -> work_start[NBRK+1] (stored behind brick_start)
// points per work item.  Every item flushes its brick's touched vertices -- ~9000 global float atomics whatever its size, a
// fifth of the staged backward at cfg3 (with the flush taken out: 1.16 -> 0.94 ms, profiles/r05_ab_hashgrid.txt) -- so large calls take larger items (cfg3: 1.16 ->
// 1.08 ms, the binned forward 0.36 -> 0.34); the small calls of a training step lose balance with them (real-view step 0.78 ->
// 0.92 ms at 2048, 1.15 at 4096).  The binning writes its choice behind the work-item table; the kernels read it there.
#define BRK_CHUNK_SMALL 1024
constexpr int BRK_CHUNK_LARGE = 2048;
#define BRK_CHUNK_WORD (2 * NBRK + 5)
__global__ __launch_bounds__(1024) void bin_rowscan_kernel(const int32_t *__restrict__ brick_cnt,
                                                           int32_t *__restrict__ brick_start, int chunk) {
    __shared__ int part[1024];
    __shared__ int partw[1024];
    constexpr int PER = (NBRK + 1 + 1023) / 1024;  // 5
    const int t = threadIdx.x;
    int32_t *work_start = brick_start + NBRK + 2;
    int loc[PER], locw[PER], s = 0, sw = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int i = t * PER + k;
        loc[k] = i <= NBRK ? brick_cnt[i] : 0;
        locw[k] = i < NBRK ? (loc[k] + chunk - 1) / chunk : 0;  // the out-of-box bucket does no work
        s += loc[k];
        sw += locw[k];
    }
    part[t] = s;
    partw[t] = sw;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = t >= o ? part[t - o] : 0;
        const int vw = t >= o ? partw[t - o] : 0;
        __syncthreads();
        part[t] += v;
        partw[t] += vw;
        __syncthreads();
    }
    int run = part[t] - s, runw = partw[t] - sw;
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int i = t * PER + k;
        if (i <= NBRK) {
            brick_start[i] = run;
            work_start[i] = runw;
        }
        run += loc[k];
        runw += locw[k];
    }
    if (t == 1023) brick_start[NBRK + 1] = part[1023], brick_start[BRK_CHUNK_WORD] = chunk;
}

__global__ __launch_bounds__(256) void bin_scatter_kernel(const float *__restrict__ x, int64_t M, int64_t chunk, float bound,
                                                          float two_bound, const int32_t *__restrict__ block_off,
                                                          const int32_t *__restrict__ brick_start, int32_t *__restrict__ perm) {
    __shared__ int cur[NBRK + 1];
    for (int i = threadIdx.x; i <= NBRK; i += 256) cur[i] = brick_start[i] + block_off[(int64_t)blockIdx.x * (NBRK + 1) + i];
    __syncthreads();
    const int64_t p0 = (int64_t)blockIdx.x * chunk, p1 = min(p0 + chunk, M);
    for (int64_t p = p0 + threadIdx.x; p < p1; p += 256) {
        const int slot = atomicAdd(&cur[brick_of(x, p, bound, two_bound)], 1);
        perm[slot] = (int32_t)p;
    }
}

// LDS float atomics (ds_add_f32) run ~40x slower than integer ones on gfx950 (177 vs 4.6-6.4 cycles per
// wave instruction, tools/micro/lds_atomics.hip), so vertex gradients are accumulated on-chip in 64-bit
// fixed point: q = (int64) (v * 2^40 / G),  G = power of two >= max|grad|.  A vertex receives at most 2048
// terms of magnitude <= 2^40 per work item (sum < 2^52 in an int64), every fp32 term is represented to 2^-40 G (i.e.
// exactly, for all practical purposes), and integer addition commutes: the on-chip stage is exact and
// order-independent -- more accurate than the float atomics it replaces, and ~25x faster.  (ds_add_f64 is also
// fast, 8.1 cycles, but its same-address rate is 40 vs 26 cycles and the kernel came out 25 % slower with it, even
// without the max|grad| pre-pass it makes unnecessary: measured, not kept.)
// (FX_BITS, FX_LIMIT and fx_scales: grid.h.  The magic add is this kernel's way of rounding onto that grid.)
#define FX_MAGIC 6755399441055744.0                 // 1.5 * 2^52
#define FX_MAGIC_BITS 0x4338000000000000ULL

// Workgroup = BRK_THREADS = 1024 lanes: 64 points x 16 levels in flight per iteration, 16 waves sharing one accumulator.
//
// Round-5 timing experiments on the d/dx form (2 tables at cfg3, same box; the wrong-result variants were never in this file):
//   as shipped in round 4 1.38 ms | VALU stream cut by 40 % (DPP sums, branch-free rows, contracted d/dx) 1.32 | LDS atomics
//   removed 1.21 | the eight table-row gathers of d/dx sent to ONE row 0.86 | both 0.76.
// Neither the instruction stream nor the LDS atomic pipe nor load latency (operands requested an iteration ahead: no gain) was
// the bound: a third of the kernel was the texture-address path working through 8 gathers x 64 distinct cache lines per wave
// and iteration -- the same 2.1 GB of L2 gathers per table the forward does.  But a brick's points only ever read the brick's own
// vertices, the very ones the accumulator has a slot for: the d/dx forms now STAGE the brick's table rows in LDS once per work
// item (4558 rows, against 1024 points x 16 levels x 8 corners = 131 k gathers), three 8-byte words per vertex {sum x, sum y, row},
// and the loop reads a corner's row beside the sums it adds the corner's gradient to.  ONE workgroup per CU (4 waves per SIMD,
// 128 registers), which pays for requesting the next point's operands an iteration ahead -- at 109 KB when the words were
// 24-byte slots, at 145 KB now that every level has its own LDS column per word (brick_layout; comment at `acc` in the kernel).
// (DESIGN.md section 3 "The hash grid" has the whole table; profiles/r05_ab_hashgrid.txt the final kernels' run of it.)
#define BRK_THREADS 1024
constexpr int BRK_PIPE = 2;             // 0 = every operand requested in the iteration that uses it, 2 = the index two iterations ahead, x / grad one
constexpr int BRK_STAGE = 1;            // 0 = the d/dx forms always gather their table rows from global memory (two workgroups per CU)
constexpr int BRK_STAGE_UNROLL = 8;     // staging gathers in flight per lane
constexpr int BRK_STAGE_MIN_POINTS = 1 << 20;      // initial value of mh_grid_stage_min_points
constexpr int BRK_STAGE_MIN = 96;       // a work item with fewer points gathers its rows directly (staging = 4558 gathers, ~36 points' worth, at half the occupancy)

// j / d for 0 <= j < 4608, 1 <= d <= 16 (a level's vertex block fits BRK_NODES_MAX: <= 16 vertices per axis): one multiply and a
// shift, m = ceil(2^16 / d) -- checked exhaustively over that range
__device__ __forceinline__ int brk_div(int j, int m) { return (int)(((uint32_t)j * (uint32_t)m) >> 16); }

// work item w -> (brick, first point, end) in item[0..2]; false for a surplus workgroup (w >= work_start[NBRK]).
// The brick b with work_start[b] <= w < work_start[b + 1] is unique (the table is monotone).  A binary search is twelve DEPENDENT
// loads before the workgroup can start; the 1024 lanes look at four bricks each instead, and the brick's point range comes with
// the same round trip.  Ends in a barrier: item[] is visible to every lane on return.
__device__ __forceinline__ bool brk_find_item(const int32_t *__restrict__ brick_start, int w, int *item) {
    const int32_t *work_start = brick_start + NBRK + 2;
    constexpr int PER = NBRK / BRK_THREADS;
    const int b0 = PER * (int)threadIdx.x;
    int ws[PER + 1], bs[PER + 1];
    const int chunk = brick_start[BRK_CHUNK_WORD];
#pragma unroll
    for (int k = 0; k <= PER; k++) ws[k] = work_start[b0 + k], bs[k] = brick_start[b0 + k];
    bool mine = false;
#pragma unroll
    for (int k = 0; k < PER; k++)
        if (ws[k] <= w && w < ws[k + 1]) {
            const int first = bs[k] + (w - ws[k]) * chunk;
            item[0] = b0 + k, item[1] = first, item[2] = min(first + chunk, bs[k + 1]), mine = true;
        }
    return __syncthreads_or(mine) != 0;
}

// this lane's level of the brick: geometry of the level, of the brick's vertex block inside it, and the row-index terms
struct BrickLevel {
    uint32_t res, T, my, mz, mask, sel;     // row = dense ? cx + cy my + cz mz : (cx ^ cy my ^ cz mz) & mask   (sel = dense mask)
    bool dense, pow2;
    int nn, base, lo[3];
    const float2 *tab;
};

__device__ __forceinline__ BrickLevel brk_level(const GridMeta &meta, const BrickMeta &bm, const float2 *__restrict__ emb, int l,
                                                int brick) {
    BrickLevel v;
    v.res = (uint32_t)meta.res[l];
    v.T = (uint32_t)(meta.offsets[l + 1] - meta.offsets[l]);
    v.dense = (uint64_t)v.res * v.res * v.res <= (uint64_t)v.T;
    v.pow2 = (v.T & (v.T - 1)) == 0;
    v.my = v.dense ? v.res : 2654435761u, v.mz = v.dense ? v.res * v.res : 805459861u;
    v.mask = v.pow2 ? v.T - 1 : 0xffffffffu, v.sel = v.dense ? 0xffffffffu : 0u;
    v.nn = bm.n[l], v.base = bm.lds_off[l];
    const int bxyz[3] = {brick % BRK, (brick / BRK) % BRK, brick / (BRK * BRK)};
#pragma unroll
    for (int d = 0; d < 3; d++) {
        // smallest cell index a point of this brick can have: same fmaf as grid_locate, monotone in u
        const float pos = fminf(fmaxf(fmaf((float)bxyz[d] / (float)BRK, (float)v.res, -0.5f), 0.0f), (float)(v.res - 1));
        v.lo[d] = (int)floorf(pos);
    }
    v.tab = emb + meta.offsets[l];
    return v;
}

// Stage the table rows of the lane's level of the brick in LDS: vertex j of the level's block goes to the 8-byte word
// at byte row0 + j * stride of lds.  The lane's level, vertices sub, sub + 64, ...: BRK_STAGE_UNROLL independent gathers in flight.
// A slot past the grid's last vertex (the brick at the upper border) is never read by a point; it gets the border row.
// (Branch-free row index as in grid_rows8: the 16 level-lanes of a wave mix dense and hashed levels.)
// ZERO (the backward): the vertex's two sums, at bytes z0 + j * stride and z1 + j * stride, are zeroed on the same walk.
template <bool ZERO>
__device__ __forceinline__ void brk_stage_rows(const BrickLevel &v, int sub, char *lds, int row0, int stride, int z0 = 0, int z1 = 0) {
    const int n3 = v.nn * v.nn * v.nn, m = (65536 + v.nn - 1) / v.nn;
    for (int j0 = sub; j0 < n3; j0 += 64 * BRK_STAGE_UNROLL) {
        float2 r[BRK_STAGE_UNROLL];
#pragma unroll
        for (int u = 0; u < BRK_STAGE_UNROLL; u++) {
            const int j = min(j0 + 64 * u, n3 - 1);
            const int t = brk_div(j, m), jz = brk_div(t, m);
            const int jx = j - t * v.nn, jy = t - jz * v.nn;
            const uint32_t cx = min((uint32_t)(v.lo[0] + jx), v.res - 1), ym = min((uint32_t)(v.lo[1] + jy), v.res - 1) * v.my,
                           zm = min((uint32_t)(v.lo[2] + jz), v.res - 1) * v.mz;
            uint32_t row = ((cx + ym + zm) & v.sel) | ((cx ^ ym ^ zm) & v.mask & ~v.sel);
            if (__builtin_expect(!v.dense && !v.pow2, 0)) row %= v.T;
            r[u] = v.tab[row];
        }
#pragma unroll
        for (int u = 0; u < BRK_STAGE_UNROLL; u++) {
            const int j = j0 + 64 * u;
            if (j < n3) {
                *reinterpret_cast<float2 *>(lds + row0 + j * stride) = r[u];
                if (ZERO) *reinterpret_cast<long long *>(lds + z0 + j * stride) = 0, *reinterpret_cast<long long *>(lds + z1 + j * stride) = 0;
            }
        }
    }
}

// the lane's level's sums zeroed without the rows (a work item too small to stage them): the same walk
__device__ __forceinline__ void brk_zero_sums(int n3, int sub, char *lds, int stride, int z0, int z1) {
    for (int j = sub; j < n3; j += 64)
        *reinterpret_cast<long long *>(lds + z0 + j * stride) = 0, *reinterpret_cast<long long *>(lds + z1 + j * stride) = 0;
}

// Brick-binned FORWARD.  The ungrouped forward is the texture-address path working through 8 gathers x 64 distinct cache lines
// per wave (0.46 ms per table at 2.1 M points: one line per clock and CU) -- and the training step bins its points into bricks
// for the backward anyway.  Binned BEFORE the forward, a work item stages its brick's 4558 rows in LDS (37 KB: two 1024-lane
// workgroups per CU) and its <= 1024 points read their corners there.  Per-point arithmetic is grid_fwd_kernel's: bit-identical
// features.  Points outside the box sit behind the last brick in `perm`; the surplus workgroups of the launch (there are at
// least ceil(#outside / 1024) of them) write their zero rows.
__global__ __launch_bounds__(BRK_THREADS, 8) void grid_fwd_brick_kernel(const float *__restrict__ x, const float2 *__restrict__ emb,
                                                                         GridMeta meta, BrickMeta bm,
                                                                         const int32_t *__restrict__ perm,
                                                                         const int32_t *__restrict__ brick_start,
                                                                         float2 *__restrict__ out, int L, int n_levels, float bound,
                                                                         float two_bound) {
    __shared__ long long val[BRK_NODES_MAX];    // float2 rows
    __shared__ int item[3];
    const int l = threadIdx.x & 15, sub = threadIdx.x >> 4;
    constexpr int PPI = BRK_THREADS / 16;
    if (!brk_find_item(brick_start, blockIdx.x, item)) {
        const int s = (int)blockIdx.x - brick_start[NBRK + 2 + NBRK];                  // surplus workgroup number
        const int first = brick_start[NBRK] + s * BRK_CHUNK_SMALL, stop = min(first + BRK_CHUNK_SMALL, brick_start[NBRK + 1]);
        for (int i = first + sub; i < stop; i += PPI) out[(int64_t)perm[i] * L + l] = make_float2(0.f, 0.f);
        return;
    }
    const int brick = item[0], start = item[1], end = item[2];
    const bool lev_on = l < n_levels;
    const BrickLevel lv = brk_level(meta, bm, emb, l, brick);
    if (lev_on) brk_stage_rows<false>(lv, sub, reinterpret_cast<char *>(val), 8 * lv.base, 8);
    __syncthreads();
    const int last = end - 1;
    // operands of the next point requested an iteration ahead, its index two ahead (as in the backward)
    int p_cur = perm[min(start + sub, last)], p_nxt = perm[min(start + sub + PPI, last)];
    float xv[3] = {x[(int64_t)p_cur * 3 + 0], x[(int64_t)p_cur * 3 + 1], x[(int64_t)p_cur * 3 + 2]};
    for (int i = start + sub; i < end; i += PPI) {
        const int p_nn = perm[min(i + 2 * PPI, last)];
        const float xn[3] = {x[(int64_t)p_nxt * 3 + 0], x[(int64_t)p_nxt * 3 + 1], x[(int64_t)p_nxt * 3 + 2]};
        float2 r = make_float2(0.f, 0.f);
        if (lev_on) {
            uint32_t g[3];
            float f[3];
            grid_locate(xv, bound, two_bound, lv.res, g, f);     // inside the box: the binning put the point into a brick
            const uint32_t g1[3] = {min(g[0] + 1, lv.res - 1), min(g[1] + 1, lv.res - 1), min(g[2] + 1, lv.res - 1)};
            const int lx[2] = {(int)g[0] - lv.lo[0], (int)g1[0] - lv.lo[0]}, ly[2] = {(int)g[1] - lv.lo[1], (int)g1[1] - lv.lo[1]},
                      lz[2] = {(int)g[2] - lv.lo[2], (int)g1[2] - lv.lo[2]};
            float2 v[8];
#pragma unroll
            for (int c = 0; c < 8; c++)
                v[c] = *reinterpret_cast<const float2 *>(
                    &val[lv.base + lx[c & 1] + __mul24(lv.nn, ly[(c >> 1) & 1] + __mul24(lv.nn, lz[(c >> 2) & 1]))]);
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const float w = ((c & 1) ? f[0] : 1.f - f[0]) * ((c & 2) ? f[1] : 1.f - f[1]) * ((c & 4) ? f[2] : 1.f - f[2]);
                r.x = fmaf(w, v[c].x, r.x);
                r.y = fmaf(w, v[c].y, r.y);
            }
        }
        out[(int64_t)p_cur * L + l] = r;
        p_cur = p_nxt, p_nxt = p_nn;
        xv[0] = xn[0], xv[1] = xn[1], xv[2] = xn[2];
    }
}

// NEED_DX 0: no d/dx; 1: grad_x = d/dx (pre-zeroed by the host side); 2: grad_x += d/dx.
// STAGED (d/dx forms): rows staged in LDS, one workgroup per CU.  The launcher takes it for calls of >= BRK_STAGE_MIN_POINTS
// points: the eight ~0.1 ms calls of a real-view training step (139 k - 830 k points, work items of a few hundred points whose
// zero / stage / flush phases nothing overlaps at one workgroup per CU) are faster in the direct form, 0.75 against 0.81 ms per
// step; cfg3's two calls of 2.1 M points 1.16 against 1.32 ms.  Inside the staged form a work item of fewer than BRK_STAGE_MIN
// points still gathers its rows directly (staging is 4558 gathers, 36 points' worth).  (Two launches over the same work-item
// table -- staged items in one, the others at two workgroups per CU in the second -- measured slower than either.)
template <int NEED_DX, bool STAGED>
__global__ __launch_bounds__(BRK_THREADS, STAGED ? 4 : 8) void grid_bwd_brick_kernel(
    const float2 *__restrict__ grad, const float *__restrict__ x, const float2 *__restrict__ emb, GridMeta meta, BrickMeta bm,
    const int32_t *__restrict__ perm, const int32_t *__restrict__ brick_start, long long *__restrict__ emb_acc, int acc_shift,
    float *__restrict__ grad_x, int L, int n_levels, float bound, float two_bound, const uint32_t *__restrict__ gmax_bits) {
    // per vertex: fixed-point sum of the x channel, of the y channel, and (d/dx forms) the vertex's table row -- 8-byte words.
    // Word k of vertex li of the lane's level is at byte cb_k + li * stride (BrickMeta, brick_layout).  An 8-byte LDS write or
    // atomic is served in four groups of 16 contiguous lanes, its bank pair is (byte / 8) mod 16 -- and a lane group here is the
    // 16 LEVELS of one point.  With the levels' regions laid end to end (24-byte slots) the 16 addresses of a group fall on bank
    // pairs at random and the pass is replayed: 127 M of the launch's 179 M SQ_LDS_IDX_ACTIVE cycles were SQ_LDS_BANK_CONFLICT,
    // a ds_add_u64 on random slots costs 13.3 cycles per wave and CU against 7.3 on consecutive words (tools/micro/lds_atomics.hip).
    // (Not same-vertex collisions of the points a wave carries: SQ_LDS_ADDR_CONFLICT is ~0, and walking the corners in a
    // different order per point measured the same time.)  The staged form therefore views the accumulator as rows of 16 words
    // and gives every level its OWN COLUMN for each of the three words: a group's 16 atomics are on 16 different bank pairs
    // whatever the vertices are (8.7 cycles in the micro-benchmark; the launch 18 M conflict cycles of 74 M, cfg3's two launches
    // 1.05 -> 0.89 ms; profiles/r20_grid_bwd_columns.txt).  The direct forms keep the end-to-end layout, 16-byte slots: two
    // words in columns need 1027 rows = 131 KB, which would cost them their second workgroup per CU.
    constexpr int ACC_WORDS = STAGED ? 16 * BRK_ACC_ROWS : 2 * BRK_NODES_MAX;
    __shared__ long long acc[ACC_WORDS];
    char *accb = reinterpret_cast<char *>(acc);
    // work item -> (brick, chunk of <= 1024 / 2048 points): hot bricks (all rays converge near the camera)
    // are split over several workgroups, each with its own LDS accumulation and flush
    __shared__ int item[3];
    if (!brk_find_item(brick_start, blockIdx.x, item)) return;
    const int brick = item[0], start = item[1], end = item[2];
    const bool staged = STAGED && end - start >= BRK_STAGE_MIN;     // uniform over the workgroup
    if (!STAGED)        // every word is a sum; the staged form zeroes its sums level by level, beside the rows (below)
        for (int i = threadIdx.x; i < BRK_NODES_MAX; i += BRK_THREADS) acc[2 * i] = 0, acc[2 * i + 1] = 0;
    float to_fx, from_fx;
    fx_scales(*gmax_bits, to_fx, from_fx);
    // the call's headroom (acc_shift) goes into the scale every term is quantized with: each term is rounded once, on the same grid
    // whichever work item of a split brick sums it, and every sum after that is exact
    to_fx = ldexpf(to_fx, -acc_shift);
    const float fx_lim = ldexpf(FX_LIMIT, -acc_shift);      // the clamp below saturates inside the same headroom
    const int l = threadIdx.x & 15, sub = threadIdx.x >> 4;
    // this lane's level
    const bool lev_on = l < n_levels;
    const BrickLevel lv = brk_level(meta, bm, emb, l, brick);
    const uint32_t res = lv.res, T = lv.T;
    const bool dense = lv.dense, pow2 = lv.pow2;
    const int nn = lv.nn, base = lv.base;
    const int lo[3] = {lv.lo[0], lv.lo[1], lv.lo[2]};
    const float2 *tab = lv.tab;
    // the direct forms' layout is fixed here, linear with two words per vertex (16-byte slots): its terms fold into the instructions
    const int stride = STAGED ? bm.stride : 16;
    const int cb0 = STAGED ? bm.cbase[0][l] : 16 * base, cb1 = STAGED ? bm.cbase[1][l] : cb0 + 8, cb2 = STAGED ? bm.cbase[2][l] : 0;
    const int d1 = cb1 - cb0, d2 = cb2 - cb0;
    if (STAGED && lev_on) {
        if (staged) brk_stage_rows<true>(lv, sub, accb, cb2, stride, cb0, cb1);
        else brk_zero_sums(nn * nn * nn, sub, accb, stride, cb0, cb1);
    }
    // per-level parameters of the flush (below), from the sixteen lanes that hold one level each: the flush walks the brick's 4558
    // vertex slots in ONE flat loop, every lane looking its slot's level up here
    static_assert(MH_MAX_LEVELS >= 16, "the brick kernels run on 16-level grids (L == 16 is checked by the launchers)");
    __shared__ int flush_par[16][16];
    if (threadIdx.x < 16) {
        int *fp = flush_par[l];
        fp[0] = nn, fp[1] = (65536 + nn - 1) / nn, fp[2] = base, fp[3] = lo[0], fp[4] = lo[1], fp[5] = lo[2];
        fp[6] = (int)(res - 1), fp[7] = (int)lv.my, fp[8] = (int)lv.mz, fp[9] = (int)lv.mask, fp[10] = (int)lv.sel, fp[11] = (int)T;
        fp[12] = (int)(!dense && !pow2), fp[13] = meta.offsets[l], fp[14] = cb0, fp[15] = cb1;
    }
    __syncthreads();
    constexpr int PPI = BRK_THREADS / 16;  // points per iteration
    const int end_r = start + ((end - start + PPI - 1) / PPI) * PPI;
    // (1.5 * 2^52 held in a scalar register pair: as a literal it occupies two vector registers of every lane)
    int magic_hi, magic_lo;
    asm("s_mov_b32 %0, 0x43380000" : "=s"(magic_hi));     // FX_MAGIC_BITS >> 32 (opaque to constant folding, which would put it
    asm("s_mov_b32 %0, 0" : "=s"(magic_lo));              //  back into vector registers)
    const double magic = __longlong_as_double(((long long)magic_hi << 32) | (unsigned)magic_lo);
    // Software pipeline: an iteration works on operands requested one iteration earlier (x, grad of the next point) and on an
    // index requested two iterations earlier; loads past the chunk's end re-read its last point (a valid address, no branch
    // around a load).  (Two points per lane and iteration, for more independent LDS work per wave, measured slower: 1.19
    // against 1.16 ms -- and needs the branch around a point's work gone, which costs the sparse work items of the training
    // steps their skipped waves: 0.75 -> 0.91 ms.)
    const int last = end - 1;
    // (the direct-gather d/dx form has no registers for it at two workgroups per CU: 10 spills, and measured no faster)
    constexpr int PIPE = (NEED_DX && !STAGED) ? 0 : BRK_PIPE;
    int p_cur = 0, p_nxt = 0;
    float xv[3] = {0.f, 0.f, 0.f};
    float2 gr = make_float2(0.f, 0.f);
    if (PIPE == 2) {
        p_cur = perm[min(start + sub, last)];
        p_nxt = perm[min(start + sub + PPI, last)];
#pragma unroll
        for (int d = 0; d < 3; d++) xv[d] = x[(int64_t)p_cur * 3 + d];
        gr = grad[(int64_t)p_cur * L + l];
    }
    const float inv_2b = 1.0f / two_bound;
    for (int i = start + sub; i < end_r; i += PPI) {
        const bool live = i < end;
        if (PIPE == 0) p_cur = perm[min(i, last)];
        const int64_t p = p_cur;
        int p_nn = 0;
        float xn[3] = {0.f, 0.f, 0.f};
        float2 grn = make_float2(0.f, 0.f);
        if (PIPE == 2) {
            p_nn = perm[min(i + 2 * PPI, last)];
#pragma unroll
            for (int d = 0; d < 3; d++) xn[d] = x[(int64_t)p_nxt * 3 + d];
            grn = grad[(int64_t)p_nxt * L + l];
        } else {
#pragma unroll
            for (int d = 0; d < 3; d++) xv[d] = x[p * 3 + d];
            gr = grad[p * L + l];
        }
        float gx_old[3] = {0.f, 0.f, 0.f};
        if (NEED_DX == 2 && l == 0) {       // the gradient this point already holds: requested now, added at the iteration's end
#pragma unroll
            for (int d = 0; d < 3; d++) gx_old[d] = grad_x[p * 3 + d];
        }
        float dx[3] = {0.f, 0.f, 0.f};
        if (live && lev_on) {
            uint32_t g[3];
            float f[3];
            grid_locate(xv, bound, two_bound, res, g, f);
            const uint32_t g1[3] = {min(g[0] + 1, res - 1), min(g[1] + 1, res - 1), min(g[2] + 1, res - 1)};
            const int lx0 = (int)g[0] - lo[0], ly0 = (int)g[1] - lo[1], lz0 = (int)g[2] - lo[2];
            const int lx1 = (int)g1[0] - lo[0], ly1 = (int)g1[1] - lo[1], lz1 = (int)g1[2] - lo[2];
            // fixed point of w * g: a float -> int64 conversion is ~11 VALU instructions and there are 16 per (point, level) -- a
            // quarter of the loop.  In double, w * (g 2^k) + 1.5 * 2^52 has the integer (|q| <= 2^40 < 2^51, round to nearest of
            // the EXACT 48-bit product) in its low bits: q = bits - bits(1.5 * 2^52), one v_fma_f64 and one 32-bit add.
            // (the magic add is exact only below 2^51: a NaN / Inf gradient or a stale maximum word must saturate to ONE bounded
            //  contribution, not write arbitrary bit patterns into the brick's accumulators -- one v_med3_f32 per value, outside the
            //  corner loop; v_med3 returns the smallest operand when one is a NaN)
            const double gxd = (double)__builtin_amdgcn_fmed3f(gr.x * to_fx, -fx_lim, fx_lim),
                         gyd = (double)__builtin_amdgcn_fmed3f(gr.y * to_fx, -fx_lim, fx_lim);
            // (Same-vertex collisions of the four points a wave carries are NOT what the atomics cost: with row k of the wave
            //  walking the corners in the order c ^ k -- four different vertices per instruction -- the kernel ran the same
            //  1.16 ms; without the atomics 0.77 ms.  It was the 16 levels of a lane group sharing bank pairs: the layout's
            //  columns, comment at `acc` above.)
            int slot[8];    // byte address of the corner's sum x; sum y and the row are d1 and d2 behind it
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const float w = ((c & 1) ? f[0] : 1.f - f[0]) * ((c & 2) ? f[1] : 1.f - f[1]) * ((c & 4) ? f[2] : 1.f - f[2]);
                // (24-bit multiplies: a brick has < 2^12 vertices per level, v_mul_lo_u32 is a quarter-rate instruction)
                const int li = ((c & 1) ? lx1 : lx0) + __mul24(nn, ((c & 2) ? ly1 : ly0) + __mul24(nn, (c & 4) ? lz1 : lz0));
                slot[c] = cb0 + __mul24(li, stride);
                const double wd = (double)w;
                const unsigned long long qx = (unsigned long long)__double_as_longlong(__builtin_fma(wd, gxd, magic)) - FX_MAGIC_BITS;
                const unsigned long long qy = (unsigned long long)__double_as_longlong(__builtin_fma(wd, gyd, magic)) - FX_MAGIC_BITS;
                atomicAdd(reinterpret_cast<unsigned long long *>(accb + slot[c]), qx);
                atomicAdd(reinterpret_cast<unsigned long long *>(accb + slot[c] + d1), qy);
            }
            if (NEED_DX) {
                float2 v[8];
                if (staged) {
#pragma unroll
                    for (int c = 0; c < 8; c++) v[c] = *reinterpret_cast<const float2 *>(accb + slot[c] + d2);
                } else {
                    // (requesting the rows before the sixteen LDS atomics, to cover their round trip, needs 16 more live registers
                    //  than the 64 that keep two workgroups on a CU: 18 spills -- the rows are asked for here)
                    uint32_t row[8];
                    grid_rows8(g, g1, res, T, dense, pow2, row);
#pragma unroll
                    for (int c = 0; c < 8; c++) v[c] = tab[row[c]];
                }
                grid_ddx(v, f, gr, (float)res, dx);
            }
        }
        if (NEED_DX) {
            const float sx = sum16(dx[0]), sy = sum16(dx[1]), sz = sum16(dx[2]);
            if (live && l == 0) {
                grad_x[p * 3 + 0] = gx_old[0] + sx * inv_2b;       // NEED_DX == 1: gx_old = 0 (grad_x was zero-filled: a point
                grad_x[p * 3 + 1] = gx_old[1] + sy * inv_2b;       // outside the box is never visited)
                grad_x[p * 3 + 2] = gx_old[2] + sz * inv_2b;
            }
        }
        if (PIPE == 2) {
            p_cur = p_nxt, p_nxt = p_nn;
            xv[0] = xn[0], xv[1] = xn[1], xv[2] = xn[2], gr = grn;
        }
    }
    __syncthreads();
    // flush touched vertices: one global atomic per (vertex, channel) instead of one per (point, corner, channel).  The flush stays in
    // fixed point: integer adds into the table-sized emb_acc commute, so the table gradient does not depend on the order in which the
    // work items sharing a row finish (float atomics here made two runs of one step differ); grid_acc_finalize_kernel converts once.
    // (the scale leaves acc_shift bits of headroom, so that a whole call's sum of a row stays inside the int64 range)
    // One flat loop over the brick's vertex slots (five rounds of the 1024 lanes) instead of one loop per level: eleven of the sixteen
    // levels have fewer than 256 slots, their rounds ran with three quarters of the lanes idle -- and the flush is instruction time, not
    // atomic throughput (round 6, same box, cfg3's two launches: shipped 1.08 ms, the same loop without its atomics 1.06, no flush 0.92;
    // profiles/r06_ab_grid_flush.txt).  A slot's level: the number of level starts at or below it (scalar compares); the level's
    // geometry: two 16-byte LDS reads of flush_par; j / n by multiply and shift (brk_div); the branch-free row index of grid_rows8.
    {
        int total = 0;                 // (no level switched on: nothing was accumulated, and there is no last level to index)
        if (n_levels > 0) {
            const int n_last = bm.n[n_levels - 1];
            total = bm.lds_off[n_levels - 1] + n_last * n_last * n_last;
        }
        for (int j = threadIdx.x; j < total; j += BRK_THREADS) {
            // (the staged form's slot address goes through its level's column; the direct forms look at the sums first and
            //  find the level only for a touched vertex)
            int lev = 0;
            if (STAGED) {
#pragma unroll
                for (int k = 1; k < 16; k++) lev += (k < n_levels && j >= bm.lds_off[k]) ? 1 : 0;
            }
            const int a0 = STAGED ? flush_par[lev][14] + (j - flush_par[lev][2]) * stride : 16 * j;
            const int a1 = STAGED ? flush_par[lev][15] + (j - flush_par[lev][2]) * stride : 16 * j + 8;
            const long long qx = *reinterpret_cast<const long long *>(accb + a0), qy = *reinterpret_cast<const long long *>(accb + a1);
            if (qx == 0 && qy == 0) continue;
            if (!STAGED) {
#pragma unroll
                for (int k = 1; k < 16; k++) lev += (k < n_levels && j >= bm.lds_off[k]) ? 1 : 0;
            }
            const int *fp = flush_par[lev];
            const int n = fp[0], m = fp[1], jl = j - fp[2];
            const int t = brk_div(jl, m), jz = brk_div(t, m);
            const int jx = jl - t * n, jy = t - jz * n;
            const uint32_t rmax = (uint32_t)fp[6];
            const uint32_t cx = min((uint32_t)(fp[3] + jx), rmax), ym = min((uint32_t)(fp[4] + jy), rmax) * (uint32_t)fp[7],
                           zm = min((uint32_t)(fp[5] + jz), rmax) * (uint32_t)fp[8];
            const uint32_t sel = (uint32_t)fp[10];
            uint32_t row = ((cx + ym + zm) & sel) | ((cx ^ ym ^ zm) & (uint32_t)fp[9] & ~sel);
            if (__builtin_expect(fp[12] != 0, 0)) row %= (uint32_t)fp[11];
            unsigned long long *ga = reinterpret_cast<unsigned long long *>(emb_acc + ((size_t)fp[13] + row) * 2);
            atomicAdd(ga + 0, (unsigned long long)qx);
            atomicAdd(ga + 1, (unsigned long long)qy);
        }
    }
}

extern "C" int mh_grid_encode_fwd(const float *x, const float *emb, const int32_t *offsets_host,
                                  const int32_t *res_host, float *out, int64_t M, int32_t L, int32_t n_levels,
                                  float bound, int32_t group, void *stream) {
    if (M == 0) return MH_OK;
    if (!x || !emb || !out || M < 0 || n_levels < 0 || n_levels > L || !(bound > 0.f) || group < 1) return MH_ERR_ARG;
    GridMeta meta;
    int st = grid_fill_meta(meta, offsets_host, res_host, L);
    if (st) return st;
    if (group == 6 && M % 6 == 0) {   // the finite-difference tap layout; any other hint runs ungrouped (same results)
        const int64_t n_groups = M / 6;
        const int64_t gblocks = (n_groups * L + 255) / 256;
        if (gblocks > 0x7fffffffLL) return MH_ERR_ARG;
        hipLaunchKernelGGL(grid_fwd_grouped_kernel<6>, dim3((unsigned)gblocks), dim3(256), 0, mh_stream(stream), x,
                           reinterpret_cast<const float2 *>(emb), meta, reinterpret_cast<float2 *>(out), n_groups, (int)L,
                           (int)n_levels, bound, 2.0f * bound);
        MH_CHECK_LAUNCH();
        return MH_OK;
    }
    const int64_t threads = M * L;
    const int64_t blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffLL) return MH_ERR_ARG;
    hipLaunchKernelGGL(grid_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, mh_stream(stream), x,
                       reinterpret_cast<const float2 *>(emb), meta, reinterpret_cast<float2 *>(out), M, (int)L, (int)n_levels,
                       bound, 2.0f * bound);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_grid_encode_bwd(const float *grad, const float *x, const float *emb, const int32_t *offsets_host,
                                  const int32_t *res_host, float *grad_emb, float *grad_x, int64_t M, int32_t L,
                                  int32_t n_levels, float bound, void *stream) {
    if (M == 0) return MH_OK;
    if (!grad || !x || !emb || !grad_emb || M < 0 || n_levels < 0 || n_levels > L || !(bound > 0.f)) return MH_ERR_ARG;
    if (grad_x && L != 16) return MH_ERR_ARG;  // d/dx reduction is specialised to 16-lane level groups
    GridMeta meta;
    int st = grid_fill_meta(meta, offsets_host, res_host, L);
    if (st) return st;
    const int64_t threads = M * L;
    const int64_t blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffLL) return MH_ERR_ARG;
    if (grad_x)
        hipLaunchKernelGGL(grid_bwd_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, mh_stream(stream),
                           reinterpret_cast<const float2 *>(grad), x, reinterpret_cast<const float2 *>(emb), meta,
                           grad_emb, grad_x, M, (int)L, (int)n_levels, bound, 2.0f * bound);
    else
        hipLaunchKernelGGL(grid_bwd_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, mh_stream(stream),
                           reinterpret_cast<const float2 *>(grad), x, reinterpret_cast<const float2 *>(emb), meta,
                           grad_emb, grad_x, M, (int)L, (int)n_levels, bound, 2.0f * bound);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

// ---- brick binning + binned backward --------------------------------------------------------
#define BIN_BLOCKS 256
extern "C" int64_t mh_grid_bin_workspace_ints(void) { return (int64_t)BIN_BLOCKS * (NBRK + 1) + (NBRK + 1); }
extern "C" int32_t mh_grid_bin_bricks(void) { return NBRK; }
extern "C" int32_t mh_grid_bin_index_ints(void) { return 2 * NBRK + 8; }  // brick_start | work_start | scratch

// calls of at least this many points take the staged forms (grid_fwd_brick_kernel, the d/dx forms of grid_bwd_brick_kernel) and
// the larger work items; a process-wide tuning knob.  It only chooses between forms that give the same feature values and d/dx bits
// (table gradients: equal to the fixed-point resolution); an atomic, so that a thread setting it while others launch is a data race in
// no sense of the word
static std::atomic<int64_t> g_stage_min_points{BRK_STAGE_MIN_POINTS};
extern "C" int64_t mh_grid_stage_min_points(int64_t set) {
    if (set >= 0) g_stage_min_points.store(set, std::memory_order_relaxed);
    return g_stage_min_points.load(std::memory_order_relaxed);
}

extern "C" int mh_grid_bin_points(const float *x, int64_t M, float bound, int32_t *workspace, int32_t *perm,
                                  int32_t *brick_start, void *stream) {
    if (M == 0) return MH_OK;
    if (!x || !workspace || !perm || !brick_start || M < 0 || M > 0x7fffffffLL || !(bound > 0.f)) return MH_ERR_ARG;
    // histogram blocks: one per 1024 points, 8 .. BIN_BLOCKS.  The column scan walks the blocks' histograms serially (one dependent
    // L2 round trip per 8 rows: 14 us at 256 blocks whatever M is), the histogram / scatter kernels want many blocks: measured per
    // call at 22 000 / 140 000 points, 256 blocks 30 / 30 us, one per 4096 points 20 / 37 us
    int64_t G = (M + 1023) / 1024;
    G = G < 8 ? 8 : (G > BIN_BLOCKS ? BIN_BLOCKS : G);
    const int64_t chunk = (M + G - 1) / G;
    int32_t *block_hist = workspace, *brick_cnt = workspace + (int64_t)BIN_BLOCKS * (NBRK + 1);
    hipLaunchKernelGGL(bin_hist_kernel, dim3((unsigned)G), dim3(256), 0, mh_stream(stream), x, M, chunk, bound, 2.0f * bound,
                       block_hist);
    hipLaunchKernelGGL(bin_colscan_kernel, dim3((NBRK + 1 + 255) / 256), dim3(256), 0, mh_stream(stream), block_hist,
                       (int)G, brick_cnt);
    hipLaunchKernelGGL(bin_rowscan_kernel, dim3(1), dim3(1024), 0, mh_stream(stream), brick_cnt, brick_start,
                       M >= g_stage_min_points.load(std::memory_order_relaxed) ? BRK_CHUNK_LARGE : BRK_CHUNK_SMALL);
    hipLaunchKernelGGL(bin_scatter_kernel, dim3((unsigned)G), dim3(256), 0, mh_stream(stream), x, M, chunk, bound,
                       2.0f * bound, block_hist, brick_start, perm);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

static int fill_brick_meta(BrickMeta &bm, const int32_t *res_host, int L) {
    bm = BrickMeta{};       // (cbase / stride: brick_layout, for the staged backward alone)
    int off = 0;
    for (int l = 0; l < L; l++) {
        const int n = (res_host[l] + BRK - 1) / BRK + 2;
        bm.n[l] = n;
        bm.lds_off[l] = off;
        off += n * n * n;
    }
    return off > BRK_NODES_MAX ? MH_ERR_ARG : MH_OK;
}

// The linear layout: the levels end to end, a vertex's three 8-byte words side by side (24-byte slots).
static int brick_layout_linear(BrickMeta &bm) {
    for (int k = 0; k < 3; k++)
        for (int l = 0; l < 16; l++) bm.cbase[k][l] = 8 * (3 * bm.lds_off[l] + k);
    bm.stride = 24;
    return (24 * (bm.lds_off[15] + bm.n[15] * bm.n[15] * bm.n[15]) + 127) / 128;
}

// The staged backward's accumulator layout for a 16-level geometry that passed fill_brick_meta; returns its rows of 128 bytes.
// COLUMNS: the accumulator is rows of 16 words; for each of a vertex's three words the 16 levels get 16 different columns, a
// column stacks its three segments (one of each word): word k of vertex li of level l at byte 128 (row0 + li) + 8 column.  The 16
// levels of a point -- one lane group of an 8-byte LDS access -- are then always on 16 different bank pairs.  The packing: the
// 48 segments, largest first, each onto the lowest column its word has not used; then two levels of a word change columns
// whenever that lowers the taller of the two (every exchange lowers the sorted heights lexicographically: it ends).  The shipped
// pyramid (27, 64 x 5, 125 x 2, 216 x 3, 343, 512, 729 x 2, 1000 vertices) reaches 1091 rows, the bound 1000 + 64 + 27.
// A geometry whose packing is taller than BRK_ACC_ROWS gets the linear layout of three words (110 KB at most): same kernel.
static int brick_layout(BrickMeta &bm) {
    int sz[16], col[3][16], h[16] = {}, order[48];
    bool used[3][16] = {};
    for (int l = 0; l < 16; l++) sz[l] = bm.n[l] * bm.n[l] * bm.n[l];
    for (int i = 0; i < 48; i++) order[i] = i;      // segment i = word i / 16 of level i % 16
    std::stable_sort(order, order + 48, [&](int a, int b) { return sz[a % 16] > sz[b % 16]; });
    for (int i = 0; i < 48; i++) {
        const int k = order[i] / 16, l = order[i] % 16;
        int best = -1;
        for (int c = 0; c < 16; c++)
            if (!used[k][c] && (best < 0 || h[c] < h[best])) best = c;
        used[k][best] = true, col[k][l] = best, h[best] += sz[l];
    }
    for (bool moved = true; moved;) {
        moved = false;
        for (int k = 0; k < 3; k++)
            for (int a = 0; a < 16; a++)
                for (int b = a + 1; b < 16; b++) {
                    const int ca = col[k][a], cb = col[k][b], d = sz[a] - sz[b];
                    if (std::max(h[ca] - d, h[cb] + d) < std::max(h[ca], h[cb]))
                        h[ca] -= d, h[cb] += d, col[k][a] = cb, col[k][b] = ca, moved = true;
                }
    }
    const int rows = *std::max_element(h, h + 16);
    if (rows > BRK_ACC_ROWS) return brick_layout_linear(bm);
    int top[16] = {};
    for (int k = 0; k < 3; k++)
        for (int l = 0; l < 16; l++) {
            const int c = col[k][l];
            bm.cbase[k][l] = 128 * top[c] + 8 * c;
            top[c] += sz[l];
        }
    bm.stride = 128;
    return rows;
}

extern "C" int mh_grid_bwd_layout(const int32_t *res_host, int32_t L, int32_t *cbase, int32_t *stride, int32_t *rows) {
    if (!res_host || !cbase || !stride || !rows || L != 16) return MH_ERR_ARG;
    for (int l = 0; l < L; l++)
        if (res_host[l] < 2) return MH_ERR_ARG;
    BrickMeta bm;
    if (int st = fill_brick_meta(bm, res_host, L)) return st;
    *rows = brick_layout(bm);
    *stride = bm.stride;
    for (int k = 0; k < 3; k++)
        for (int l = 0; l < 16; l++) cbase[16 * k + l] = bm.cbase[k][l];
    return MH_OK;
}

extern "C" int mh_grid_encode_fwd_binned(const float *x, const float *emb, const int32_t *offsets_host,
                                         const int32_t *res_host, const int32_t *perm, const int32_t *brick_start, float *out,
                                         int64_t M, int32_t L, int32_t n_levels, float bound, void *stream) {
    if (M == 0) return MH_OK;
    if (!x || !emb || !out || !perm || !brick_start || M < 0 || M > 0x7fffffffLL || n_levels < 0 || n_levels > L || L != 16 ||
        !(bound > 0.f))
        return MH_ERR_ARG;
    GridMeta meta;
    int st = grid_fill_meta(meta, offsets_host, res_host, L);
    if (st) return st;
    BrickMeta bm;
    if ((st = fill_brick_meta(bm, res_host, L))) return st;
    // upper bound on sum_b ceil(cnt_b / chunk) + ceil(#outside / BRK_CHUNK_SMALL) for either chunk size: the surplus
    // workgroups write the zero rows
    const unsigned work_items = (unsigned)(NBRK + M / BRK_CHUNK_SMALL + 1);
    hipLaunchKernelGGL(grid_fwd_brick_kernel, dim3(work_items), dim3(BRK_THREADS), 0, mh_stream(stream), x,
                       reinterpret_cast<const float2 *>(emb), meta, bm, perm, brick_start, reinterpret_cast<float2 *>(out), (int)L,
                       (int)n_levels, bound, 2.0f * bound);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_grid_encode_bwd_binned(const float *grad, const float *x, const float *emb, const int32_t *offsets_host,
                                         const int32_t *res_host, const int32_t *perm, const int32_t *brick_start,
                                         float *grad_emb, int64_t *emb_acc, float *grad_x, int32_t accumulate_dx, int64_t M,
                                         int32_t L, int32_t n_levels, float bound, const uint32_t *gmax_bits, void *stream) {
    if (M == 0) return MH_OK;
    if (!grad || !x || !emb || !grad_emb || !emb_acc || !perm || !brick_start || M < 0 || n_levels < 0 || n_levels > L || L != 16 ||
        !(bound > 0.f))
        return MH_ERR_ARG;
    GridMeta meta;
    int st = grid_fill_meta(meta, offsets_host, res_host, L);
    if (st) return st;
    BrickMeta bm;
    if ((st = fill_brick_meta(bm, res_host, L))) return st;
    const bool staged = BRK_STAGE && grad_x && M >= g_stage_min_points.load(std::memory_order_relaxed);
    if (staged) brick_layout(bm);       // (the direct forms' layout is fixed in the kernel: linear, two words)
    // upper bound on sum_b ceil(cnt_b / chunk) for either chunk size; surplus workgroups exit at once
    const unsigned work_items = (unsigned)(NBRK + M / BRK_CHUNK_SMALL + 1);
    // max|grad| (float bits): supplied by the producer of `grad` (mh_field_bwd_data computes it on the fly), else
    // reduced here into the scratch word behind the work-item table
    // a table row receives at most 8 terms per point (hash collisions included), each at most 2^(FX_BITS - acc_shift) in fixed
    // point (the scale and the NaN / Inf clamp of grid_bwd_brick_kernel): keep 8 M such terms inside +-2^62
    const int acc_shift = grid_acc_shift(M, 8);
    const int64_t n_acc = (int64_t)offsets_host[L] * 2;
    if (!mh_zero_async(emb_acc, sizeof(int64_t) * (size_t)n_acc, mh_stream(stream))) return MH_ERR_LAUNCH;
    const uint32_t *gmax = gmax_bits;
    if (!gmax) {
        uint32_t *own = reinterpret_cast<uint32_t *>(const_cast<int32_t *>(brick_start)) + (2 * NBRK + 4);
        if (!mh_zero_async(own, sizeof(uint32_t), mh_stream(stream))) return MH_ERR_LAUNCH;
        grid_absmax_launch(grad, M * (int64_t)L * 2, own, mh_stream(stream));
        gmax = own;
    }
#define BRK_LAUNCH(DXMODE, STG)                                                                                                \
    hipLaunchKernelGGL((grid_bwd_brick_kernel<DXMODE, STG>), dim3(work_items), dim3(BRK_THREADS), 0, mh_stream(stream),       \
                       reinterpret_cast<const float2 *>(grad), x, reinterpret_cast<const float2 *>(emb), meta, bm, perm,     \
                       brick_start, reinterpret_cast<long long *>(emb_acc), acc_shift, grad_x, (int)L, (int)n_levels, bound,          \
                       2.0f * bound, gmax)
    if (grad_x && accumulate_dx) {
        // grad_x already holds a gradient of the same points (the field nets' d/dx): each visited point adds to its own row
        if (staged) BRK_LAUNCH(2, true); else BRK_LAUNCH(2, false);
    } else if (grad_x) {
        // points outside the box are never visited by a brick: their d/dx is zero
        if (!mh_zero_async(grad_x, sizeof(float) * 3 * (size_t)M, mh_stream(stream))) return MH_ERR_LAUNCH;
        if (staged) BRK_LAUNCH(1, true); else BRK_LAUNCH(1, false);
    } else {
        BRK_LAUNCH(0, false);
    }
#undef BRK_LAUNCH
    MH_CHECK_LAUNCH();
    hipLaunchKernelGGL(grid_acc_finalize_kernel, dim3((unsigned)std::min<int64_t>((n_acc + 255) / 256, 4096)), dim3(256), 0,
                       mh_stream(stream), reinterpret_cast<const long long *>(emb_acc), grad_emb, n_acc, acc_shift, gmax, 0.0);
    MH_CHECK_LAUNCH();
    return MH_OK;
}
