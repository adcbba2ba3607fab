// Marching cubes over a dense fp32 volume: the isosurface step of mesh export (export_mesh, morpheus.py:367-408, which ran
// mcubes.marching_cubes on the host).  Conventions, limits and the workspace are in include/morpheus_hip.h.
//
// Three launches count, two emit.  Every grid point p owns the edges that leave it in +x, +y, +z and the cell whose corner 0
// it is; a workgroup covers MC_TILE consecutive points (linear index (i*ny + j)*nz + k), MC_THREADS at a time.
//   mc_count_kernel   per tile: vertices owned (crossed edges) and triangles of the owned cells -> tile totals
//   mc_scan_kernel    one workgroup: exclusive int64 scan of the tile totals, V and T
//   mc_vertex_kernel  tiles with vertices: in-tile scan (wave ballot / popcount, LDS across waves) gives each point its first
//                     vertex id; writes the vertices, the id and the 3-bit crossed-edge mask of the point into the workspace
//   mc_tri_kernel     tiles with triangles: the same scan over the triangle counts; a cell's 12 edges map to the ids of their
//                     owners through the workspace
// Every write is also bounded by the tile's own range of the scan, so a volume that differs from the counted one (a caller
// error) cannot make the emit kernels write outside the caller's V / T rows.
//
// The masked pair (mh_mc_count_masked / mh_mc_emit_masked, for volumes with unobserved voxels: morpheus_amd/tsdf.py) is the
// same four kernels instantiated with MASKED = true, behind one more launch:
//   mc_cellmask_kernel  cell[p] = 1 when the cell at p exists and all eight of its corners have weight > 0
// A cell without its mark has no triangles; an edge is crossed only when one of the (up to four) cells around it is marked.
#include "mc_common.h"

#define MC_ITERS 8
#define MC_TILE (MC_THREADS * MC_ITERS)

struct McGrid {
    int32_t nx, ny, nz;
    int64_t n;                  // nx*ny*nz (< 2^31)
};

struct McWorkspace {            // carved from the caller's buffer, see mc_layout
    int64_t *tile_tot;          // [n_tiles][2] vertices, triangles of each tile
    int64_t *tile_off;          // [n_tiles + 1][2] exclusive scan of the above
    int32_t *vid;               // [n] first vertex id of a point (written where the point owns one)
    uint8_t *vmask;             // [n] crossed edges of a point (bit a = axis a), written with vid
    uint8_t *cell;              // [n] masked pair only: the cell at p exists and every corner of it is observed
};

static inline int64_t mc_layout(const McGrid &g, void *base, McWorkspace *ws, bool masked = false) {
    const int64_t tiles = (g.n + MC_TILE - 1) / MC_TILE;
    const int64_t o_off = mc_align(tiles * 2 * 8);
    const int64_t o_vid = o_off + mc_align((tiles + 1) * 2 * 8);
    const int64_t o_mask = o_vid + mc_align(g.n * 4);
    const int64_t o_cell = o_mask + mc_align(g.n);
    const int64_t total = o_cell + (masked ? mc_align(g.n) : 0);
    if (ws) {
        char *b = static_cast<char *>(base);
        ws->tile_tot = reinterpret_cast<int64_t *>(b);
        ws->tile_off = reinterpret_cast<int64_t *>(b + o_off);
        ws->vid = reinterpret_cast<int32_t *>(b + o_vid);
        ws->vmask = reinterpret_cast<uint8_t *>(b + o_mask);
        ws->cell = masked ? reinterpret_cast<uint8_t *>(b + o_cell) : nullptr;
    }
    return total;
}

static inline bool mc_valid(int32_t nx, int32_t ny, int32_t nz) {
    return nx >= 2 && ny >= 2 && nz >= 2 && (int64_t)nx * ny * nz < ((int64_t)1 << 31);
}

// point p -> (i, j, k); p < 2^31, so 32-bit division
__device__ __forceinline__ void mc_ijk(const McGrid &g, uint32_t p, int &i, int &j, int &k) {
    const uint32_t r = p / (uint32_t)g.nz;
    k = (int)(p - r * (uint32_t)g.nz);
    i = (int)(r / (uint32_t)g.ny);
    j = (int)(r - (uint32_t)i * (uint32_t)g.ny);
}

// masked pair: is one of the cells around the edge from p along `axis` marked?  Those cells have their corner 0 at p - u, p - v,
// p - u - v and p, u and v the other two axes; cell[] is 0 where no cell exists (the +x / +y / +z border), so only the lower
// border needs a test.
__device__ __forceinline__ bool mc_edge_cells(const uint8_t *__restrict__ cell, uint32_t p, bool has_u, int64_t su, bool has_v,
                                              int64_t sv) {
    uint32_t any = cell[p];
    if (has_u) any |= cell[p - su];
    if (has_v) any |= cell[p - sv];
    if (has_u && has_v) any |= cell[p - su - sv];
    return any != 0;
}

// crossed-edge mask of point p (bit a: the edge to p + e_a exists and its ends lie on different sides of iso; MASKED: and a
// marked cell contains it)
template <bool MASKED>
__device__ __forceinline__ uint32_t mc_edge_mask(const float *__restrict__ vol, const uint8_t *__restrict__ cell, const McGrid &g,
                                                 float iso, uint32_t p, int i, int j, int k) {
    const int64_t sy = g.nz, sx = (int64_t)g.ny * g.nz;
    const bool in0 = vol[p] < iso;
    uint32_t m = 0;
    if (i + 1 < g.nx && (vol[p + sx] < iso) != in0) m |= 1u;
    if (j + 1 < g.ny && (vol[p + sy] < iso) != in0) m |= 2u;
    if (k + 1 < g.nz && (vol[p + 1] < iso) != in0) m |= 4u;
    if constexpr (MASKED) {
        if ((m & 1u) && !mc_edge_cells(cell, p, j > 0, sy, k > 0, 1)) m &= ~1u;
        if ((m & 2u) && !mc_edge_cells(cell, p, i > 0, sx, k > 0, 1)) m &= ~2u;
        if ((m & 4u) && !mc_edge_cells(cell, p, i > 0, sx, j > 0, sy)) m &= ~4u;
    }
    return m;
}

// case index of the cell at p (bit c = corner c inside), or -1 when p is on the +x / +y / +z border (no cell; MASKED: or the
// cell is not marked)
template <bool MASKED>
__device__ __forceinline__ int mc_cube(const float *__restrict__ vol, const uint8_t *__restrict__ cell, const McGrid &g, float iso,
                                       uint32_t p, int i, int j, int k) {
    if (i + 1 >= g.nx || j + 1 >= g.ny || k + 1 >= g.nz) return -1;
    if constexpr (MASKED) {
        if (!cell[p]) return -1;
    }
    const int64_t sy = g.nz, sx = (int64_t)g.ny * g.nz;
    const float *c = vol + p;
    int cube = 0;
    cube |= (c[0] < iso) ? 1 : 0;
    cube |= (c[sx] < iso) ? 2 : 0;
    cube |= (c[sx + sy] < iso) ? 4 : 0;
    cube |= (c[sy] < iso) ? 8 : 0;
    cube |= (c[1] < iso) ? 16 : 0;
    cube |= (c[sx + 1] < iso) ? 32 : 0;
    cube |= (c[sx + sy + 1] < iso) ? 64 : 0;
    cube |= (c[sy + 1] < iso) ? 128 : 0;
    return cube;
}

// masked pair, first launch: a thread per grid point
__global__ __launch_bounds__(MC_THREADS) void mc_cellmask_kernel(const float *__restrict__ weight, McGrid g,
                                                                 uint8_t *__restrict__ cell) {
    const int64_t p = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (p >= g.n) return;
    int i, j, k;
    mc_ijk(g, (uint32_t)p, i, j, k);
    bool ok = i + 1 < g.nx && j + 1 < g.ny && k + 1 < g.nz;
    if (ok) {
        const int64_t sy = g.nz, sx = (int64_t)g.ny * g.nz;
        const float *c = weight + p;
        ok = c[0] > 0.f && c[sx] > 0.f && c[sx + sy] > 0.f && c[sy] > 0.f && c[1] > 0.f && c[sx + 1] > 0.f && c[sx + sy + 1] > 0.f &&
             c[sy + 1] > 0.f;
    }
    cell[p] = ok ? 1 : 0;
}

template <bool MASKED>
__global__ __launch_bounds__(MC_THREADS) void mc_count_kernel(const float *__restrict__ vol, const uint8_t *__restrict__ cell,
                                                              McGrid g, float iso, int64_t *__restrict__ tile_tot) {
    __shared__ uint8_t ntri[256];
    __shared__ int red[2][MC_WAVES];
    ntri[threadIdx.x] = (uint8_t)(kMcTable[threadIdx.x] >> 60);
    __syncthreads();
    int nv = 0, nt = 0;
    const int64_t base = (int64_t)blockIdx.x * MC_TILE;
#pragma unroll 2
    for (int it = 0; it < MC_ITERS; it++) {
        const int64_t p = base + it * MC_THREADS + threadIdx.x;
        if (p < g.n) {
            int i, j, k;
            mc_ijk(g, (uint32_t)p, i, j, k);
            nv += __popc(mc_edge_mask<MASKED>(vol, cell, g, iso, (uint32_t)p, i, j, k));
            const int cube = mc_cube<MASKED>(vol, cell, g, iso, (uint32_t)p, i, j, k);
            if (cube >= 0) nt += ntri[cube];
        }
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
        tile_tot[2 * blockIdx.x] = v;
        tile_tot[2 * blockIdx.x + 1] = t;
    }
}

template <bool MASKED>
__global__ __launch_bounds__(MC_THREADS) void mc_vertex_kernel(const float *__restrict__ vol, const uint8_t *__restrict__ cell,
                                                               McGrid g, float iso,
                                                               const int64_t *__restrict__ tile_off, int32_t *__restrict__ vid,
                                                               uint8_t *__restrict__ vmask, float *__restrict__ vertices) {
    __shared__ int red[MC_WAVES];
    const int64_t vbase = tile_off[2 * blockIdx.x], vend = tile_off[2 * blockIdx.x + 2];
    if (vend == vbase) return;                                 // no vertex in this tile (uniform over the workgroup)
    const int64_t sy = g.nz, sx = (int64_t)g.ny * g.nz;
    const int64_t base = (int64_t)blockIdx.x * MC_TILE;
    int64_t run = vbase;
    for (int it = 0; it < MC_ITERS; it++) {
        const int64_t p = base + it * MC_THREADS + threadIdx.x;
        int i = 0, j = 0, k = 0;
        uint32_t m = 0;
        if (p < g.n) {
            mc_ijk(g, (uint32_t)p, i, j, k);
            m = mc_edge_mask<MASKED>(vol, cell, g, iso, (uint32_t)p, i, j, k);
        }
        int total;
        const int pre = mc_block_scan(__popc(m), red, &total);
        const int64_t id = run + pre;
        if (m && id + __popc(m) <= vend) {
            vid[p] = (int32_t)id;
            vmask[p] = (uint8_t)m;
            const float f0 = vol[p];
            float *out = vertices + 3 * id;
            const float x = (float)i, y = (float)j, z = (float)k;
            if (m & 1u) {
                out[0] = x + mc_t(iso, f0, vol[p + sx]);
                out[1] = y;
                out[2] = z;
                out += 3;
            }
            if (m & 2u) {
                out[0] = x;
                out[1] = y + mc_t(iso, f0, vol[p + sy]);
                out[2] = z;
                out += 3;
            }
            if (m & 4u) {
                out[0] = x;
                out[1] = y;
                out[2] = z + mc_t(iso, f0, vol[p + 1]);
            }
        }
        run += total;
    }
}

template <bool MASKED>
__global__ __launch_bounds__(MC_THREADS) void mc_tri_kernel(const float *__restrict__ vol, const uint8_t *__restrict__ cell,
                                                            McGrid g, float iso, const int64_t *__restrict__ tile_off,
                                                            const int32_t *__restrict__ vid, const uint8_t *__restrict__ vmask,
                                                            int32_t *__restrict__ triangles) {
    __shared__ uint64_t table[256];
    __shared__ int red[MC_WAVES];
    const int64_t tbase = tile_off[2 * blockIdx.x + 1], tend = tile_off[2 * blockIdx.x + 3];
    if (tend == tbase) return;                                 // no triangle in this tile
    table[threadIdx.x] = kMcTable[threadIdx.x];
    __syncthreads();
    const int64_t sy = g.nz, sx = (int64_t)g.ny * g.nz;
    const int64_t base = (int64_t)blockIdx.x * MC_TILE;
    int64_t run = tbase;
    for (int it = 0; it < MC_ITERS; it++) {
        const int64_t p = base + it * MC_THREADS + threadIdx.x;
        uint64_t word = 0;
        if (p < g.n) {
            int i, j, k;
            mc_ijk(g, (uint32_t)p, i, j, k);
            const int cube = mc_cube<MASKED>(vol, cell, g, iso, (uint32_t)p, i, j, k);
            if (cube >= 0) word = table[cube];
        }
        const int nt = (int)(word >> 60);
        int total;
        const int pre = mc_block_scan(nt, red, &total);
        const int64_t first = run + pre;
        if (nt && first + nt <= tend) {
            int32_t *out = triangles + 3 * first;
            for (int n = 0; n < 3 * nt; n++) {
                const int e = (int)(word >> (4 * n)) & 15;
                const int own = kMcEdgeOwner[e], axis = kMcEdgeAxis[e];
                const int64_t q = p + ((own & 1) ? sx : 0) + ((own & 2) ? sy : 0) + ((own & 4) ? 1 : 0);
                const int32_t v = vid[q] + __popc((uint32_t)vmask[q] & ((1u << axis) - 1u));
                // the table's winding points toward decreasing f: slots 1 and 2 of each triangle trade places
                const int slot = n % 3;
                out[n - slot + (slot == 0 ? 0 : 3 - slot)] = v;
            }
        }
        run += total;
    }
}

extern "C" int64_t mh_mc_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
    if (!mc_valid(nx, ny, nz)) return -1;
    const McGrid g{nx, ny, nz, (int64_t)nx * ny * nz};
    return mc_layout(g, nullptr, nullptr);
}

extern "C" int64_t mh_mc_masked_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
    if (!mc_valid(nx, ny, nz)) return -1;
    const McGrid g{nx, ny, nz, (int64_t)nx * ny * nz};
    return mc_layout(g, nullptr, nullptr, true);
}

template <bool MASKED>
static int mc_count(const float *vol, const float *weight, int32_t nx, int32_t ny, int32_t nz, float iso, void *workspace,
                    int64_t *counts, void *stream) {
    if (!vol || (MASKED && !weight) || !workspace || !counts || !mc_valid(nx, ny, nz)) return MH_ERR_ARG;
    const McGrid g{nx, ny, nz, (int64_t)nx * ny * nz};
    McWorkspace ws;
    mc_layout(g, workspace, &ws, MASKED);
    const int64_t tiles = (g.n + MC_TILE - 1) / MC_TILE;
    hipStream_t s = mh_stream(stream);
    if (MASKED) {
        hipLaunchKernelGGL(mc_cellmask_kernel, dim3((unsigned)((g.n + MC_THREADS - 1) / MC_THREADS)), dim3(MC_THREADS), 0, s, weight,
                           g, ws.cell);
        MH_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(mc_count_kernel<MASKED>, dim3((unsigned)tiles), dim3(MC_THREADS), 0, s, vol, ws.cell, g, iso, ws.tile_tot);
    MH_CHECK_LAUNCH();
    hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(MC_SCAN_THREADS), 0, s, ws.tile_tot, tiles, ws.tile_off, counts);
    MH_CHECK_LAUNCH();
    // the caller sizes the outputs from V and T, so it waits for them anyway: read them here to report an overflow
    int64_t host[2] = {0, 0};
    if (hipMemcpyAsync(host, counts, sizeof(host), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return MH_ERR_LAUNCH;
    if (host[0] >= ((int64_t)1 << 31) || host[1] >= ((int64_t)1 << 31)) return MH_ERR_OVERFLOW;
    return MH_OK;
}

template <bool MASKED>
static int mc_emit(const float *vol, int32_t nx, int32_t ny, int32_t nz, float iso, void *workspace, float *vertices,
                   int32_t *triangles, void *stream) {
    if (!vol || !workspace || !vertices || !triangles || !mc_valid(nx, ny, nz)) return MH_ERR_ARG;
    const McGrid g{nx, ny, nz, (int64_t)nx * ny * nz};
    McWorkspace ws;
    mc_layout(g, workspace, &ws, MASKED);
    const int64_t tiles = (g.n + MC_TILE - 1) / MC_TILE;
    hipStream_t s = mh_stream(stream);
    hipLaunchKernelGGL(mc_vertex_kernel<MASKED>, dim3((unsigned)tiles), dim3(MC_THREADS), 0, s, vol, ws.cell, g, iso, ws.tile_off,
                       ws.vid, ws.vmask, vertices);
    MH_CHECK_LAUNCH();
    hipLaunchKernelGGL(mc_tri_kernel<MASKED>, dim3((unsigned)tiles), dim3(MC_THREADS), 0, s, vol, ws.cell, g, iso, ws.tile_off,
                       ws.vid, ws.vmask, triangles);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_mc_count(const float *vol, int32_t nx, int32_t ny, int32_t nz, float iso, void *workspace, int64_t *counts,
                           void *stream) {
    return mc_count<false>(vol, nullptr, nx, ny, nz, iso, workspace, counts, stream);
}

extern "C" int mh_mc_emit(const float *vol, int32_t nx, int32_t ny, int32_t nz, float iso, void *workspace, float *vertices,
                          int32_t *triangles, void *stream) {
    return mc_emit<false>(vol, nx, ny, nz, iso, workspace, vertices, triangles, stream);
}

extern "C" int mh_mc_count_masked(const float *vol, const float *weight, int32_t nx, int32_t ny, int32_t nz, float iso,
                                  void *workspace, int64_t *counts, void *stream) {
    return mc_count<true>(vol, weight, nx, ny, nz, iso, workspace, counts, stream);
}

extern "C" int mh_mc_emit_masked(const float *vol, int32_t nx, int32_t ny, int32_t nz, float iso, void *workspace, float *vertices,
                                 int32_t *triangles, void *stream) {
    return mc_emit<true>(vol, nx, ny, nz, iso, workspace, vertices, triangles, stream);
}
