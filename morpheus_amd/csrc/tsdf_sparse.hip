// TSDF fusion into a pooled block-sparse volume: the dense store of tsdf.hip behind an index volume, so that a logical box of more
// than 2^31 voxels costs 4 bytes per 8^3 block plus 10 KiB per block that a frame reached.  Conventions, limits and the layout
// are in include/morpheus_hip.h (TSDF fusion, the block-sparse store); the per-voxel arithmetic is tsdf_common.h's, shared with
// the dense kernels, and this file is built without FP contraction as well.  tests/tsdf_sparse_oracle.py restates the store.
//
//   sparse_touch_kernel      the dense touch with allocation: a lane per sampled pixel; a block without a slot is won by one
//                            compare-and-swap on its index entry (-1 -> -2), the winner takes the next slot from the counter
//   sparse_integrate_kernel  walks SLOTS: a wave per slot, SP_GROUP slots per workgroup; 8 steps of 64 lanes, each a contiguous
//                            256-byte line of each of the five planes; workgroups beyond the counter return
//   sparse_to_dense_kernel / sparse_from_dense_kernel   a workgroup per slot / per block of the dense box
//   sparse_mc_*_kernel       masked marching cubes, a workgroup per allocated block in ascending block id: the block's points
//                            and a one-point halo (10^3 values and observed flags, 9^3 cell marks) are staged in LDS through
//                            the index volume; count -> mc_scan_kernel -> vertices -> triangles as in mesh.hip
//   sparse_vertex_colors_kernel  a lane per vertex, colour reads through the index volume
// Every loop is bounded by the capacity, by a block's 512 points or by a pixel's clipped block range; a slot read from memory is
// used only when it lies in [0, capacity), a block id only when it lies in the box.
#include "mc_common.h"
#include "tsdf_common.h"

#define SP_GROUP 4                                      // slots per workgroup of sparse_integrate_kernel: a wave each
#define SP_VOX 512
#define SP_HALO 1000                                    // 10^3 points: the block and one point around it
#define SP_CELLS 729                                    // 9^3 cells with their corner 0 in [-1, 7]^3

struct SpGrid {
    int32_t nbx, nby, nbz, capacity;
};

__device__ __forceinline__ int sp_live(const int32_t *__restrict__ counters, int32_t capacity) {
    return max(0, min(counters[0], capacity));
}

// block id -> coordinates; false for an id outside the box
__device__ __forceinline__ bool sp_decode(const SpGrid &g, int32_t bid, int &bx, int &by, int &bz) {
    if (bid < 0) return false;
    const uint32_t r = (uint32_t)bid / (uint32_t)g.nbz;
    bz = (int)((uint32_t)bid - r * (uint32_t)g.nbz);
    bx = (int)(r / (uint32_t)g.nby);
    by = (int)(r - (uint32_t)bx * (uint32_t)g.nby);
    return bx < g.nbx;
}

// the slot of block (bx, by, bz), -1 when the block lies outside the box or has no storage
__device__ __forceinline__ int32_t sp_slot(const int32_t *__restrict__ slot, const SpGrid &g, int bx, int by, int bz) {
    if (bx < 0 || by < 0 || bz < 0 || bx >= g.nbx || by >= g.nby || bz >= g.nbz) return -1;
    const int32_t s = slot[((int64_t)bx * g.nby + by) * g.nbz + bz];
    return (s >= 0 && s < g.capacity) ? s : -1;
}

__global__ __launch_bounds__(TSDF_THREADS) void sparse_touch_kernel(const float *__restrict__ depth, const uint8_t *__restrict__ mask,
                                                                    TsdfFrame f, TsdfBox b, int32_t stride, int32_t ns_w,
                                                                    int64_t n_samples, int32_t capacity, int32_t *slot,
                                                                    int32_t *__restrict__ slot_block, int32_t *counters) {
    const int64_t s = (int64_t)blockIdx.x * TSDF_THREADS + threadIdx.x;
    if (s >= n_samples) return;
    int lo[3], hi[3];
    if (!tsdf_touch_range(depth, mask, f, b, stride, ns_w, s, lo, hi)) return;
    for (int x = lo[0]; x <= hi[0]; x++)
        for (int y = lo[1]; y <= hi[1]; y++)
            for (int z = lo[2]; z <= hi[2]; z++) {
                const int64_t bid = ((int64_t)x * b.nby + y) * b.nbz + z;
                int32_t *e = slot + bid;
                if (*e != -1) continue;                        // an entry only ever leaves -1, so a stale read costs one CAS
                if (atomicCAS(e, -1, -2) != -1) continue;      // another lane won the block
                const int32_t mine = atomicAdd(counters, 1);
                if (mine < capacity) {
                    slot_block[mine] = (int32_t)bid;
                    atomicExch(e, mine);
                } else {
                    counters[1] = 1;                           // the pool is full: the entry keeps -2 (no storage), the counter
                }                                              // goes on counting the blocks that wanted one
            }
}

__global__ __launch_bounds__(TSDF_THREADS) void sparse_integrate_kernel(const float *__restrict__ depth, const uint8_t *__restrict__ rgb,
                                                                        const uint8_t *__restrict__ mask, TsdfFrame f, TsdfBox b,
                                                                        int32_t capacity, const int32_t *__restrict__ slot_block,
                                                                        const int32_t *__restrict__ counters, float *__restrict__ tsdf,
                                                                        float *__restrict__ weight, float *__restrict__ color) {
    const int live = sp_live(counters, capacity);
    if ((int64_t)blockIdx.x * SP_GROUP >= live) return;        // uniform over the workgroup
    const int64_t sl = (int64_t)blockIdx.x * SP_GROUP + (threadIdx.x >> 6);
    if (sl >= live) return;
    const SpGrid g{b.nbx, b.nby, b.nbz, capacity};
    int bx, by, bz;
    if (!sp_decode(g, slot_block[sl], bx, by, bz)) return;
    const int lane = mh_lane();
    const int j = by * TSDF_BLOCK + (lane >> 3), k = bz * TSDF_BLOCK + (lane & 7);
    const int64_t plane = (int64_t)capacity * SP_VOX;
    const float py = b.oy + ((float)j + 0.5f) * b.voxel_length, pz = b.oz + ((float)k + 0.5f) * b.voxel_length;
#pragma unroll 4
    for (int xi = 0; xi < TSDF_BLOCK; xi++) {
        const int i = bx * TSDF_BLOCK + xi;
        const float px = b.ox + ((float)i + 0.5f) * b.voxel_length;
        const int64_t p = sl * SP_VOX + xi * 64 + lane;
        tsdf_update_voxel(depth, rgb, mask, f, b.sdf_trunc, px, py, pz, tsdf + p, weight + p, color + p, color + plane + p,
                          color + 2 * plane + p);
    }
}

__global__ __launch_bounds__(TSDF_THREADS) void sparse_to_dense_kernel(SpGrid g, const int32_t *__restrict__ slot_block,
                                                                       const int32_t *__restrict__ counters,
                                                                       const float *__restrict__ ptsdf, const float *__restrict__ pweight,
                                                                       const float *__restrict__ pcolor, float *__restrict__ tsdf,
                                                                       float *__restrict__ weight, float *__restrict__ color,
                                                                       uint8_t *__restrict__ active) {
    const int64_t sl = blockIdx.x;
    if (sl >= sp_live(counters, g.capacity)) return;
    const int32_t bid = slot_block[sl];
    int bx, by, bz;
    if (!sp_decode(g, bid, bx, by, bz)) return;
    const int64_t ny = (int64_t)g.nby * TSDF_BLOCK, nz = (int64_t)g.nbz * TSDF_BLOCK;
    const int64_t dplane = (int64_t)g.nbx * TSDF_BLOCK * ny * nz, pplane = (int64_t)g.capacity * SP_VOX;
    for (int l = threadIdx.x; l < SP_VOX; l += TSDF_THREADS) {
        const int i = bx * TSDF_BLOCK + (l >> 6), j = by * TSDF_BLOCK + ((l >> 3) & 7), k = bz * TSDF_BLOCK + (l & 7);
        const int64_t q = ((int64_t)i * ny + j) * nz + k, p = sl * SP_VOX + l;
        tsdf[q] = ptsdf[p];
        weight[q] = pweight[p];
#pragma unroll
        for (int ch = 0; ch < 3; ch++) color[ch * dplane + q] = pcolor[ch * pplane + p];
    }
    if (threadIdx.x == 0) active[bid] = 1;
}

__global__ __launch_bounds__(TSDF_THREADS) void sparse_from_dense_kernel(SpGrid g, const float *__restrict__ tsdf,
                                                                         const float *__restrict__ weight, const float *__restrict__ color,
                                                                         const uint8_t *__restrict__ keep, const int32_t *__restrict__ order,
                                                                         int32_t *__restrict__ slot, int32_t *__restrict__ slot_block,
                                                                         int32_t *counters, float *__restrict__ ptsdf,
                                                                         float *__restrict__ pweight, float *__restrict__ pcolor) {
    __shared__ int32_t mine;
    const int32_t bid = order ? order[blockIdx.x] : (int32_t)blockIdx.x;
    int bx, by, bz;
    if (!sp_decode(g, bid, bx, by, bz) || (keep && !keep[bid])) return;
    if (threadIdx.x == 0) {
        int32_t s = -1;
        if (atomicCAS(slot + bid, -1, -2) == -1) {             // a block listed twice in `order` is taken once
            s = atomicAdd(counters, 1);
            if (s < g.capacity) {
                slot_block[s] = bid;
                atomicExch(slot + bid, s);
            } else {
                counters[1] = 1;
                s = -1;
            }
        }
        mine = s;
    }
    __syncthreads();
    const int64_t sl = mine;
    if (sl < 0) return;
    const int64_t ny = (int64_t)g.nby * TSDF_BLOCK, nz = (int64_t)g.nbz * TSDF_BLOCK;
    const int64_t dplane = (int64_t)g.nbx * TSDF_BLOCK * ny * nz, pplane = (int64_t)g.capacity * SP_VOX;
    for (int l = threadIdx.x; l < SP_VOX; l += TSDF_THREADS) {
        const int i = bx * TSDF_BLOCK + (l >> 6), j = by * TSDF_BLOCK + ((l >> 3) & 7), k = bz * TSDF_BLOCK + (l & 7);
        const int64_t q = ((int64_t)i * ny + j) * nz + k, p = sl * SP_VOX + l;
        ptsdf[p] = tsdf[q];
        pweight[p] = weight[q];
#pragma unroll
        for (int ch = 0; ch < 3; ch++) pcolor[ch * pplane + p] = color[ch * dplane + q];
    }
}

// ---- marching cubes over the allocated blocks ------------------------------------------------------------------------------------

struct SpMcWorkspace {          // carved from the caller's buffer, see sp_mc_layout
    int64_t *blk_tot;           // [capacity][2] vertices, triangles of the r-th block in ascending block id
    int64_t *blk_off;           // [capacity + 1][2] exclusive scan of the above
    int32_t *vid;               // [capacity][512] by SLOT: first vertex id of a point (written where the point owns one)
    uint8_t *vmask;             // [capacity][512] by slot: crossed edges of a point, written with vid
};

static inline int64_t sp_mc_layout(int64_t capacity, void *base, SpMcWorkspace *ws) {
    const int64_t o_off = mc_align(capacity * 2 * 8);
    const int64_t o_vid = o_off + mc_align((capacity + 1) * 2 * 8);
    const int64_t o_mask = o_vid + mc_align(capacity * SP_VOX * 4);
    const int64_t total = o_mask + mc_align(capacity * SP_VOX);
    if (ws) {
        char *b = static_cast<char *>(base);
        ws->blk_tot = reinterpret_cast<int64_t *>(b);
        ws->blk_off = reinterpret_cast<int64_t *>(b + o_off);
        ws->vid = reinterpret_cast<int32_t *>(b + o_vid);
        ws->vmask = reinterpret_cast<uint8_t *>(b + o_mask);
    }
    return total;
}

struct SpHalo {
    float val[SP_HALO];         // point (i, j, k), each in [-1, 8], at ((i + 1) * 10 + (j + 1)) * 10 + (k + 1)
    uint8_t obs[SP_HALO];       // weight > 0; 0 outside the box and in a block without storage
    uint8_t cell[SP_CELLS];     // the cell with corner 0 at (i, j, k), each in [-1, 7], at ((i + 1) * 9 + (j + 1)) * 9 + (k + 1)
};

// the r-th allocated block in ascending id: its slot and coordinates; false when r is beyond the counter (or the list is not what
// the index volume holds: a caller error, answered by an empty block)
__device__ __forceinline__ bool sp_mc_block(const SpGrid &g, const int32_t *__restrict__ slot, const int32_t *__restrict__ sorted,
                                            const int32_t *__restrict__ counters, int64_t r, int &bx, int &by, int &bz, int32_t &sl) {
    if (r >= sp_live(counters, g.capacity)) return false;
    if (!sp_decode(g, sorted[r], bx, by, bz)) return false;
    sl = sp_slot(slot, g, bx, by, bz);
    return sl >= 0;
}

// stage the block's halo; ends with a barrier
__device__ __forceinline__ void sp_load_halo(const float *__restrict__ tsdf, const float *__restrict__ weight,
                                             const int32_t *__restrict__ slot, const SpGrid &g, int bx, int by, int bz, SpHalo &h) {
    for (int q = threadIdx.x; q < SP_HALO; q += MC_THREADS) {
        const int gi = bx * 8 + q / 100 - 1, gj = by * 8 + (q / 10) % 10 - 1, gk = bz * 8 + q % 10 - 1;
        const int32_t s = sp_slot(slot, g, gi >> 3, gj >> 3, gk >> 3);      // -1 >> 3 = -1: outside
        float v = 0.f, w = 0.f;
        if (s >= 0) {
            const int64_t p = (int64_t)s * SP_VOX + (((gi & 7) * 8 + (gj & 7)) * 8 + (gk & 7));
            v = tsdf[p];
            w = weight[p];
        }
        h.val[q] = v;
        h.obs[q] = w > 0.f ? 1 : 0;                            // a NaN weight is not observed
    }
    __syncthreads();
    for (int c = threadIdx.x; c < SP_CELLS; c += MC_THREADS) {
        const uint8_t *o = h.obs + ((c / 81) * 10 + (c / 9) % 9) * 10 + c % 9;
        h.cell[c] = o[0] & o[100] & o[110] & o[10] & o[1] & o[101] & o[111] & o[11];
    }
    __syncthreads();
}

// crossed-edge mask of the block's point l = (i * 8 + j) * 8 + k: bit a when the edge to p + e_a is crossed and one of the four
// cells around it exists
__device__ __forceinline__ uint32_t sp_edge_mask(const SpHalo &h, float iso, int l) {
    const int i = l >> 6, j = (l >> 3) & 7, k = l & 7;
    const float *v = h.val + ((i + 1) * 10 + (j + 1)) * 10 + (k + 1);
    const uint8_t *c = h.cell + ((i + 1) * 9 + (j + 1)) * 9 + (k + 1);
    const bool in0 = v[0] < iso;
    uint32_t m = 0;
    if ((v[100] < iso) != in0 && (c[0] | c[-9] | c[-1] | c[-10])) m |= 1u;
    if ((v[10] < iso) != in0 && (c[0] | c[-81] | c[-1] | c[-82])) m |= 2u;
    if ((v[1] < iso) != in0 && (c[0] | c[-81] | c[-9] | c[-90])) m |= 4u;
    return m;
}

// case index of the cell at the block's point l, -1 when the cell does not exist
__device__ __forceinline__ int sp_cube(const SpHalo &h, float iso, int l) {
    const int i = l >> 6, j = (l >> 3) & 7, k = l & 7;
    if (!h.cell[((i + 1) * 9 + (j + 1)) * 9 + (k + 1)]) return -1;
    const float *c = h.val + ((i + 1) * 10 + (j + 1)) * 10 + (k + 1);
    int cube = 0;
    cube |= (c[0] < iso) ? 1 : 0;
    cube |= (c[100] < iso) ? 2 : 0;
    cube |= (c[110] < iso) ? 4 : 0;
    cube |= (c[10] < iso) ? 8 : 0;
    cube |= (c[1] < iso) ? 16 : 0;
    cube |= (c[101] < iso) ? 32 : 0;
    cube |= (c[111] < iso) ? 64 : 0;
    cube |= (c[11] < iso) ? 128 : 0;
    return cube;
}

__global__ __launch_bounds__(MC_THREADS) void sparse_mc_count_kernel(const float *__restrict__ tsdf, const float *__restrict__ weight,
                                                                     const int32_t *__restrict__ slot, const int32_t *__restrict__ sorted,
                                                                     const int32_t *__restrict__ counters, SpGrid g, float iso,
                                                                     int64_t *__restrict__ blk_tot) {
    __shared__ SpHalo h;
    __shared__ uint8_t ntri[256];
    __shared__ int red[2][MC_WAVES];
    int bx, by, bz;
    int32_t sl;
    if (!sp_mc_block(g, slot, sorted, counters, blockIdx.x, bx, by, bz, sl)) {      // uniform over the workgroup
        if (threadIdx.x == 0) blk_tot[2 * (int64_t)blockIdx.x] = blk_tot[2 * (int64_t)blockIdx.x + 1] = 0;
        return;
    }
    ntri[threadIdx.x] = (uint8_t)(kMcTable[threadIdx.x] >> 60);
    sp_load_halo(tsdf, weight, slot, g, bx, by, bz, h);
    int nv = 0, nt = 0;
#pragma unroll
    for (int l = threadIdx.x; l < SP_VOX; l += MC_THREADS) {
        nv += __popc(sp_edge_mask(h, iso, l));
        const int cube = sp_cube(h, iso, l);
        if (cube >= 0) nt += ntri[cube];
    }
    nv = wave_sum(nv);
    nt = wave_sum(nt);
    if (mh_lane() == 0) {
        red[0][threadIdx.x >> 6] = nv;
        red[1][threadIdx.x >> 6] = nt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t v = 0, t = 0;
#pragma unroll
        for (int w = 0; w < MC_WAVES; w++) {
            v += red[0][w];
            t += red[1][w];
        }
        blk_tot[2 * (int64_t)blockIdx.x] = v;
        blk_tot[2 * (int64_t)blockIdx.x + 1] = t;
    }
}

__global__ __launch_bounds__(MC_THREADS) void sparse_mc_vertex_kernel(const float *__restrict__ tsdf, const float *__restrict__ weight,
                                                                      const int32_t *__restrict__ slot, const int32_t *__restrict__ sorted,
                                                                      const int32_t *__restrict__ counters, SpGrid g, float iso,
                                                                      const int64_t *__restrict__ blk_off, int32_t *__restrict__ vid,
                                                                      uint8_t *__restrict__ vmask, float *__restrict__ vertices) {
    __shared__ SpHalo h;
    __shared__ int red[MC_WAVES];
    const int64_t vbase = blk_off[2 * (int64_t)blockIdx.x], vend = blk_off[2 * (int64_t)blockIdx.x + 2];
    if (vend == vbase) return;                                 // no vertex in this block (uniform over the workgroup)
    int bx, by, bz;
    int32_t sl;
    if (!sp_mc_block(g, slot, sorted, counters, blockIdx.x, bx, by, bz, sl)) return;
    sp_load_halo(tsdf, weight, slot, g, bx, by, bz, h);
    int64_t run = vbase;
    for (int l = threadIdx.x; l < SP_VOX; l += MC_THREADS) {   // two steps, the same for every thread
        const uint32_t m = sp_edge_mask(h, iso, l);
        int total;
        const int pre = mc_block_scan(__popc(m), red, &total);
        const int64_t id = run + pre;
        if (m && id + __popc(m) <= vend) {
            const int i = l >> 6, j = (l >> 3) & 7, k = l & 7;
            vid[(int64_t)sl * SP_VOX + l] = (int32_t)id;
            vmask[(int64_t)sl * SP_VOX + l] = (uint8_t)m;
            const float *v = h.val + ((i + 1) * 10 + (j + 1)) * 10 + (k + 1);
            const float f0 = v[0];
            float *out = vertices + 3 * id;
            const float x = (float)(bx * 8 + i), y = (float)(by * 8 + j), z = (float)(bz * 8 + k);
            if (m & 1u) {
                out[0] = x + mc_t(iso, f0, v[100]);
                out[1] = y;
                out[2] = z;
                out += 3;
            }
            if (m & 2u) {
                out[0] = x;
                out[1] = y + mc_t(iso, f0, v[10]);
                out[2] = z;
                out += 3;
            }
            if (m & 4u) {
                out[0] = x;
                out[1] = y;
                out[2] = z + mc_t(iso, f0, v[1]);
            }
        }
        run += total;
    }
}

__global__ __launch_bounds__(MC_THREADS) void sparse_mc_tri_kernel(const float *__restrict__ tsdf, const float *__restrict__ weight,
                                                                   const int32_t *__restrict__ slot, const int32_t *__restrict__ sorted,
                                                                   const int32_t *__restrict__ counters, SpGrid g, float iso,
                                                                   const int64_t *__restrict__ blk_off, const int32_t *__restrict__ vid,
                                                                   const uint8_t *__restrict__ vmask, int32_t *__restrict__ triangles) {
    __shared__ SpHalo h;
    __shared__ uint64_t table[256];
    __shared__ int red[MC_WAVES];
    __shared__ int32_t nbr[8];                                // slots of the blocks at +{0, 1}^3: bit 0 x, bit 1 y, bit 2 z
    const int64_t tbase = blk_off[2 * (int64_t)blockIdx.x + 1], tend = blk_off[2 * (int64_t)blockIdx.x + 3];
    if (tend == tbase) return;                                 // no triangle in this block
    int bx, by, bz;
    int32_t sl;
    if (!sp_mc_block(g, slot, sorted, counters, blockIdx.x, bx, by, bz, sl)) return;
    table[threadIdx.x] = kMcTable[threadIdx.x];
    if (threadIdx.x < 8) nbr[threadIdx.x] = sp_slot(slot, g, bx + (threadIdx.x & 1), by + ((threadIdx.x >> 1) & 1), bz + (threadIdx.x >> 2));
    sp_load_halo(tsdf, weight, slot, g, bx, by, bz, h);
    int64_t run = tbase;
    for (int l = threadIdx.x; l < SP_VOX; l += MC_THREADS) {
        const int cube = sp_cube(h, iso, l);
        const uint64_t word = cube >= 0 ? table[cube] : 0;
        const int nt = (int)(word >> 60);
        int total;
        const int pre = mc_block_scan(nt, red, &total);
        const int64_t first = run + pre;
        if (nt && first + nt <= tend) {
            const int i = l >> 6, j = (l >> 3) & 7, k = l & 7;
            int32_t *out = triangles + 3 * first;
            for (int n = 0; n < 3 * nt; n++) {
                const int e = (int)(word >> (4 * n)) & 15;
                const int own = kMcEdgeOwner[e], axis = kMcEdgeAxis[e];
                const int qi = i + (own & 1), qj = j + ((own >> 1) & 1), qk = k + (own >> 2);      // each in [0, 8]
                const int32_t ns = nbr[(qi >> 3) | ((qj >> 3) << 1) | ((qk >> 3) << 2)];
                int32_t v = 0;
                if (ns >= 0) {                                 // a cell that exists has storage under all of its corners
                    const int64_t q = (int64_t)ns * SP_VOX + (((qi & 7) * 8 + (qj & 7)) * 8 + (qk & 7));
                    v = vid[q] + __popc((uint32_t)vmask[q] & ((1u << axis) - 1u));
                }
                // the table's winding points toward decreasing f: slots 1 and 2 of each triangle trade places
                const int sl3 = n % 3;
                out[n - sl3 + (sl3 == 0 ? 0 : 3 - sl3)] = v;
            }
        }
        run += total;
    }
}

__global__ __launch_bounds__(TSDF_THREADS) void sparse_vertex_colors_kernel(const float *__restrict__ vertices, int64_t V,
                                                                            const float *__restrict__ color,
                                                                            const int32_t *__restrict__ slot, SpGrid g,
                                                                            float *__restrict__ out) {
    const int64_t v = (int64_t)blockIdx.x * TSDF_THREADS + threadIdx.x;
    if (v >= V) return;
    const int n[3] = {g.nbx * 8, g.nby * 8, g.nbz * 8};
    int q0[3] = {0, 0, 0}, axis = -1;
    float t = 0.f;
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float x = vertices[3 * v + a], fl = floorf(x);
        if (!(fl >= 0.f && fl <= (float)(n[a] - 1))) {
            ok = false;
            continue;
        }
        q0[a] = (int)fl;
        const float fr = x - fl;
        if (fr > 0.f && axis < 0 && q0[a] + 1 < n[a]) {        // the edge's axis: the one coordinate off the grid
            t = fr;
            axis = a;
        }
    }
    int q1[3] = {q0[0], q0[1], q0[2]};
    if (axis >= 0) q1[axis] += 1;
    const int64_t plane = (int64_t)g.capacity * SP_VOX;
    int64_t p0 = -1, p1 = -1;
    if (ok) {
        const int32_t s0 = sp_slot(slot, g, q0[0] >> 3, q0[1] >> 3, q0[2] >> 3), s1 = sp_slot(slot, g, q1[0] >> 3, q1[1] >> 3, q1[2] >> 3);
        if (s0 >= 0) p0 = (int64_t)s0 * SP_VOX + (((q0[0] & 7) * 8 + (q0[1] & 7)) * 8 + (q0[2] & 7));
        if (s1 >= 0) p1 = (int64_t)s1 * SP_VOX + (((q1[0] & 7) * 8 + (q1[1] & 7)) * 8 + (q1[2] & 7));
    }
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        float c = 0.f;
        if (ok) {
            const float c0 = p0 >= 0 ? color[ch * plane + p0] : 0.f, c1 = p1 >= 0 ? color[ch * plane + p1] : 0.f;
            c = ((1.0f - t) * c0 + t * c1) / 255.0f;
        }
        out[3 * v + ch] = c;
    }
}

// ---- entry points -------------------------------------------------------------------------------------------------------------------

extern "C" int32_t mh_tsdf_sparse_group_slots(void) { return SP_GROUP; }
extern "C" int32_t mh_tsdf_sparse_max_side_blocks(void) { return TSDF_SPARSE_MAX_SIDE; }

extern "C" int mh_tsdf_sparse_touch(const float *depth, const uint8_t *mask, int32_t H, int32_t W, float fx, float fy, float cx,
                                    float cy, const float *c2w_host, float depth_scale, float depth_trunc, int32_t stride, float ox,
                                    float oy, float oz, float voxel_length, float sdf_trunc, int32_t nbx, int32_t nby, int32_t nbz,
                                    int32_t capacity, int32_t *slot, int32_t *slot_block, int32_t *counters, void *stream) {
    TsdfFrame f;
    TsdfBox b;
    if (!tsdf_frame(&f, depth, H, W, fx, fy, cx, cy, c2w_host, depth_scale, depth_trunc) || stride < 1 || capacity < 1 || !slot ||
        !slot_block || !counters || !tsdf_sparse_box(&b, ox, oy, oz, voxel_length, sdf_trunc, nbx, nby, nbz))
        return MH_ERR_ARG;
    const int32_t ns_w = (W + stride - 1) / stride, ns_h = (H + stride - 1) / stride;
    const int64_t n = (int64_t)ns_w * ns_h;
    hipLaunchKernelGGL(sparse_touch_kernel, dim3((unsigned)((n + TSDF_THREADS - 1) / TSDF_THREADS)), dim3(TSDF_THREADS), 0,
                       mh_stream(stream), depth, mask, f, b, stride, ns_w, n, capacity, slot, slot_block, counters);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_tsdf_sparse_integrate(const float *depth, const uint8_t *rgb, const uint8_t *mask, int32_t H, int32_t W, float fx,
                                        float fy, float cx, float cy, const float *w2c_host, float depth_scale, float depth_trunc,
                                        float ox, float oy, float oz, float voxel_length, float sdf_trunc, int32_t nbx, int32_t nby,
                                        int32_t nbz, int32_t capacity, const int32_t *slot_block, const int32_t *counters, float *tsdf,
                                        float *weight, float *color, void *stream) {
    TsdfFrame f;
    TsdfBox b;
    if (!tsdf_frame(&f, depth, H, W, fx, fy, cx, cy, w2c_host, depth_scale, depth_trunc) || !rgb || capacity < 1 || !slot_block ||
        !counters || !tsdf || !weight || !color || !tsdf_sparse_box(&b, ox, oy, oz, voxel_length, sdf_trunc, nbx, nby, nbz))
        return MH_ERR_ARG;
    const int64_t groups = ((int64_t)capacity + SP_GROUP - 1) / SP_GROUP;
    hipLaunchKernelGGL(sparse_integrate_kernel, dim3((unsigned)groups), dim3(TSDF_THREADS), 0, mh_stream(stream), depth, rgb, mask, f, b,
                       capacity, slot_block, counters, tsdf, weight, color);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_tsdf_sparse_to_dense(int32_t nbx, int32_t nby, int32_t nbz, int32_t capacity, const int32_t *slot_block,
                                       const int32_t *counters, const float *pool_tsdf, const float *pool_weight,
                                       const float *pool_color, float *tsdf, float *weight, float *color, uint8_t *active,
                                       void *stream) {
    if (capacity < 1 || !tsdf_sparse_grid(nbx, nby, nbz) || (int64_t)nbx * nby * nbz * SP_VOX >= ((int64_t)1 << 31) || !slot_block ||
        !counters || !pool_tsdf || !pool_weight || !pool_color || !tsdf || !weight || !color || !active)
        return MH_ERR_ARG;
    const SpGrid g{nbx, nby, nbz, capacity};
    hipLaunchKernelGGL(sparse_to_dense_kernel, dim3((unsigned)capacity), dim3(TSDF_THREADS), 0, mh_stream(stream), g, slot_block,
                       counters, pool_tsdf, pool_weight, pool_color, tsdf, weight, color, active);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_tsdf_sparse_from_dense(const float *tsdf, const float *weight, const float *color, const uint8_t *keep,
                                         const int32_t *order, int32_t nbx, int32_t nby, int32_t nbz, int32_t capacity,
                                         int32_t *slot, int32_t *slot_block, int32_t *counters, float *pool_tsdf, float *pool_weight,
                                         float *pool_color, void *stream) {
    if (capacity < 1 || !tsdf_sparse_grid(nbx, nby, nbz) || (int64_t)nbx * nby * nbz * SP_VOX >= ((int64_t)1 << 31) || !tsdf ||
        !weight || !color || !slot || !slot_block || !counters || !pool_tsdf || !pool_weight || !pool_color)
        return MH_ERR_ARG;
    const SpGrid g{nbx, nby, nbz, capacity};
    hipLaunchKernelGGL(sparse_from_dense_kernel, dim3((unsigned)(nbx * nby * nbz)), dim3(TSDF_THREADS), 0, mh_stream(stream), g, tsdf,
                       weight, color, keep, order, slot, slot_block, counters, pool_tsdf, pool_weight, pool_color);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int64_t mh_mc_sparse_workspace_bytes(int32_t capacity) {
    if (capacity < 1) return -1;
    return sp_mc_layout(capacity, nullptr, nullptr);
}

extern "C" int mh_mc_count_sparse(const float *pool_tsdf, const float *pool_weight, const int32_t *slot, const int32_t *sorted_blocks,
                                  const int32_t *counters, int32_t nbx, int32_t nby, int32_t nbz, int32_t capacity, float iso,
                                  void *workspace, int64_t *counts, void *stream) {
    if (capacity < 1 || !tsdf_sparse_grid(nbx, nby, nbz) || !pool_tsdf || !pool_weight || !slot || !sorted_blocks || !counters ||
        !workspace || !counts)
        return MH_ERR_ARG;
    const SpGrid g{nbx, nby, nbz, capacity};
    SpMcWorkspace ws;
    sp_mc_layout(capacity, workspace, &ws);
    hipStream_t s = mh_stream(stream);
    hipLaunchKernelGGL(sparse_mc_count_kernel, dim3((unsigned)capacity), dim3(MC_THREADS), 0, s, pool_tsdf, pool_weight, slot,
                       sorted_blocks, counters, g, iso, ws.blk_tot);
    MH_CHECK_LAUNCH();
    hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(MC_SCAN_THREADS), 0, s, ws.blk_tot, (int64_t)capacity, ws.blk_off, counts);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_mc_emit_sparse(const float *pool_tsdf, const float *pool_weight, const int32_t *slot, const int32_t *sorted_blocks,
                                 const int32_t *counters, int32_t nbx, int32_t nby, int32_t nbz, int32_t capacity, float iso,
                                 void *workspace, float *vertices, int32_t *triangles, void *stream) {
    if (capacity < 1 || !tsdf_sparse_grid(nbx, nby, nbz) || !pool_tsdf || !pool_weight || !slot || !sorted_blocks || !counters ||
        !workspace || !vertices || !triangles)
        return MH_ERR_ARG;
    const SpGrid g{nbx, nby, nbz, capacity};
    SpMcWorkspace ws;
    sp_mc_layout(capacity, workspace, &ws);
    hipStream_t s = mh_stream(stream);
    hipLaunchKernelGGL(sparse_mc_vertex_kernel, dim3((unsigned)capacity), dim3(MC_THREADS), 0, s, pool_tsdf, pool_weight, slot,
                       sorted_blocks, counters, g, iso, ws.blk_off, ws.vid, ws.vmask, vertices);
    MH_CHECK_LAUNCH();
    hipLaunchKernelGGL(sparse_mc_tri_kernel, dim3((unsigned)capacity), dim3(MC_THREADS), 0, s, pool_tsdf, pool_weight, slot,
                       sorted_blocks, counters, g, iso, ws.blk_off, ws.vid, ws.vmask, triangles);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_tsdf_sparse_vertex_colors(const float *vertices, int64_t V, const float *pool_color, const int32_t *slot, int32_t nbx,
                                            int32_t nby, int32_t nbz, int32_t capacity, float *out, void *stream) {
    if (V < 0 || V >= ((int64_t)1 << 31) || capacity < 1 || !tsdf_sparse_grid(nbx, nby, nbz)) return MH_ERR_ARG;
    if (V == 0) return MH_OK;
    if (!vertices || !pool_color || !slot || !out) return MH_ERR_ARG;
    const SpGrid g{nbx, nby, nbz, capacity};
    hipLaunchKernelGGL(sparse_vertex_colors_kernel, dim3((unsigned)((V + TSDF_THREADS - 1) / TSDF_THREADS)), dim3(TSDF_THREADS), 0,
                       mh_stream(stream), vertices, V, pool_color, slot, g, out);
    MH_CHECK_LAUNCH();
    return MH_OK;
}
