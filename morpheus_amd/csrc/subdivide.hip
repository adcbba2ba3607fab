// Midpoint subdivision to a maximum edge length: the device side of trimesh.remesh.subdivide_to_size, which cull_one_mesh of
// the reference (tools/culling.py:86-131) runs before it culls.  The four children of a midpoint split have the parent's edges
// halved, so the recursion ends, per input triangle, at a uniform tessellation of depth d on a barycentric lattice of n = 2^d
// intervals: count -> the caller's prefix sums -> emit, no sort, no edge hash, no iteration.  Definition, operator order and limits
// are in include/morpheus_hip.h (mh_subdiv_count, mh_subdiv_emit); tests/subdivide_oracle.py restates them in numpy.
//
//   sd_count_kernel     one thread per input triangle: depth, new-vertex count, sub-triangle count
//   sd_emit_vertices    one thread per OUTPUT vertex (the V copied ones, then the new ones)
//   sd_emit_triangles   one thread per OUTPUT triangle
// An emit thread finds its input triangle by binary search over the exclusive prefix sums and its lattice position by an
// 11-step search over the row starts (integers only: no float sqrt is taken anywhere).  Work is never handed out per input
// triangle: one of depth 10 owns 4^10 outputs, its neighbour one.  Both emit kernels are write streams of 12-byte records; the
// records of a workgroup go through LDS so that neighbouring lanes store neighbouring words.
// Every loop is bounded: by max_iter + 1 <= 11, by 32 rounds over T, by 11 rounds over a lattice's rows.
#include "common.h"

#pragma clang fp contract(off)

#define SD_THREADS 256
#define SD_MAX_ITER 10

static inline bool sd_count_valid(int64_t n) { return n >= 0 && n < ((int64_t)1 << 31); }

static inline unsigned sd_blocks(int64_t n) { return (unsigned)((n + SD_THREADS - 1) / SD_THREADS); }

// the smallest d in [0, max_iter + 1] for which l2 * 4^-d > m2 is false (a NaN l2: 0; an infinite one: max_iter + 1)
__device__ __forceinline__ int sd_edge_depth(const float *__restrict__ p, const float *__restrict__ q, double m2, int max_iter) {
    const double dx = (double)q[0] - (double)p[0], dy = (double)q[1] - (double)p[1], dz = (double)q[2] - (double)p[2];
    const double l2 = (dx * dx + dy * dy) + dz * dz;
    int d = 0;
    double s = 1.0;                                // 4^-d, exact
    while (d <= max_iter && l2 * s > m2) {
        d++;
        s *= 0.25;
    }
    return d;
}

__global__ __launch_bounds__(SD_THREADS) void sd_count_kernel(const float *__restrict__ vertices, int64_t V,
                                                              const int32_t *__restrict__ triangles, int64_t T, double m2,
                                                              int max_iter, int32_t *__restrict__ depth,
                                                              int64_t *__restrict__ n_vert, int64_t *__restrict__ n_tri) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    int32_t idx[3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        idx[k] = triangles[3 * t + k];
        ok = ok && idx[k] >= 0 && idx[k] < V;
    }
    int d = 0;
    if (ok) {
        const float *a = vertices + 3 * (int64_t)idx[0], *b = vertices + 3 * (int64_t)idx[1], *c = vertices + 3 * (int64_t)idx[2];
        d = max(max(sd_edge_depth(a, b, m2, max_iter), sd_edge_depth(b, c, m2, max_iter)), sd_edge_depth(c, a, m2, max_iter));
    }
    const bool split = d >= 1 && d <= max_iter;    // d = max_iter + 1, "too long", counts as a copy: the caller refuses it
    const int64_t n = (int64_t)1 << d;
    depth[t] = d;
    n_vert[t] = split ? (n + 1) * (n + 2) / 2 - 3 : 0;
    n_tri[t] = split ? n * n : 1;
}

// the last t in [0, T) with start[t] <= g: the owner of output g (start = exclusive prefix sums, start[T] > g).  <= 32 rounds.
__device__ __forceinline__ int64_t sd_owner(const int64_t *__restrict__ start, int64_t T, int64_t g) {
    int64_t lo = 0, hi = T - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (start[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// full lattice index of the first point of row j: q(0, j) = j(n + 1) - j(j - 1)/2
__device__ __forceinline__ int32_t sd_row_q(int32_t j, int32_t n) { return j * (n + 1) - j * (j - 1) / 2; }

// q in [0, L) -> (i, j): the last row j in [0, n] that starts at or before q.  <= 11 rounds for n <= 1024.
__device__ __forceinline__ void sd_decode_q(int32_t q, int32_t n, int32_t &i, int32_t &j) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (sd_row_q(mid, n) <= q) lo = mid;
        else hi = mid - 1;
    }
    j = lo;
    i = q - sd_row_q(lo, n);
}

// local triangle l in [0, n^2) -> (j, s): the last row j in [0, n - 1] whose first triangle j(2n - j) is at or before l
__device__ __forceinline__ void sd_decode_tri(int32_t l, int32_t n, int32_t &j, int32_t &s) {
    int32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (mid * (2 * n - mid) <= l) lo = mid;
        else hi = mid - 1;
    }
    j = lo;
    s = l - lo * (2 * n - lo);
}

// a workgroup's 3-word records, staged in LDS by their owners (stride 3 words: conflict-free), leave as three rows of
// consecutive words; base = the workgroup's first record, limit = the number of records of the whole output
template <typename W>
__device__ __forceinline__ void sd_store_records(W *stage, W *__restrict__ out, int64_t base, int64_t limit) {
    __syncthreads();
    const int64_t first = 3 * base, words = 3 * limit;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const int32_t w = r * SD_THREADS + (int32_t)threadIdx.x;
        if (first + w < words) out[first + w] = stage[w];
    }
}

__global__ __launch_bounds__(SD_THREADS) void sd_emit_vertices(const float *__restrict__ vertices, const float *__restrict__ colors,
                                                               int64_t V, const int32_t *__restrict__ triangles, int64_t T,
                                                               const int32_t *__restrict__ depth,
                                                               const int64_t *__restrict__ vert_start, int64_t total,
                                                               float *__restrict__ out_vertices, float *__restrict__ out_colors) {
    __shared__ float stage[2][3 * SD_THREADS];
    const int64_t base = (int64_t)blockIdx.x * SD_THREADS;
    const int64_t g = base + threadIdx.x;          // output vertex; total = V + new vertices
    const bool with_colors = colors != nullptr;    // the same in every lane
    float p[3] = {NAN, NAN, NAN}, pc[3] = {NAN, NAN, NAN};
    if (g < V) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            p[a] = vertices[3 * g + a];
            if (with_colors) pc[a] = colors[3 * g + a];
        }
    } else if (g < total) {
        const int64_t t = sd_owner(vert_start, T, g - V);
        const int32_t d = depth[t];
        int32_t idx[3];
        bool ok = d >= 1 && d <= SD_MAX_ITER;      // holds for every owner of a new vertex when depth and vert_start belong together
#pragma unroll
        for (int k = 0; k < 3; k++) {
            idx[k] = triangles[3 * t + k];
            ok = ok && idx[k] >= 0 && idx[k] < V;
        }
        if (ok) {
            const int32_t n = 1 << d;
            const int32_t r = (int32_t)(g - V - vert_start[t]);
            int32_t i, j;
            sd_decode_q(r < n - 1 ? r + 1 : r + 2, n, i, j);       // the corners q = 0 and q = n are not emitted
            // / n as a multiplication by 2^-d: the same real number rounded once, so the same bits as the division
            const double wk = (double)(n - i - j), wi = (double)i, wj = (double)j, inv_n = 1.0 / (double)n;
            const int64_t ia = 3 * (int64_t)idx[0], ib = 3 * (int64_t)idx[1], ic = 3 * (int64_t)idx[2];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                p[a] = (float)(((wk * (double)vertices[ia + a] + wi * (double)vertices[ib + a]) + wj * (double)vertices[ic + a]) * inv_n);
                if (with_colors)
                    pc[a] = (float)(((wk * (double)colors[ia + a] + wi * (double)colors[ib + a]) + wj * (double)colors[ic + a]) * inv_n);
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        stage[0][3 * threadIdx.x + a] = p[a];
        stage[1][3 * threadIdx.x + a] = pc[a];
    }
    sd_store_records(stage[0], out_vertices, base, total);
    if (with_colors) sd_store_records(stage[1], out_colors, base, total);
}

// output vertex of lattice point (i, j) of a split triangle: a corner is the input vertex, anything else a new one
__device__ __forceinline__ int32_t sd_vertex_id(int32_t i, int32_t j, int32_t n, const int32_t *idx, int64_t first_new) {
    const int32_t q = sd_row_q(j, n) + i, L = (n + 1) * (n + 2) / 2;
    if (q == 0) return idx[0];
    if (q == n) return idx[1];
    if (q == L - 1) return idx[2];
    return (int32_t)(first_new + (q < n ? q - 1 : q - 2));
}

__global__ __launch_bounds__(SD_THREADS) void sd_emit_triangles(const int32_t *__restrict__ triangles, int64_t V, int64_t T,
                                                                const int32_t *__restrict__ depth,
                                                                const int64_t *__restrict__ vert_start,
                                                                const int64_t *__restrict__ tri_start, int64_t total,
                                                                int32_t *__restrict__ out_triangles,
                                                                int32_t *__restrict__ out_index) {
    __shared__ int32_t stage[3 * SD_THREADS];
    const int64_t base = (int64_t)blockIdx.x * SD_THREADS;
    const int64_t g = base + threadIdx.x;          // output triangle
    int32_t out[3] = {0, 0, 0};
    if (g < total) {
        const int64_t t = sd_owner(tri_start, T, g);
        const int32_t d = depth[t];
        int32_t idx[3];
#pragma unroll
        for (int k = 0; k < 3; k++) idx[k] = out[k] = triangles[3 * t + k];        // d = 0 (and "too long"): a copy
        if (d >= 1 && d <= SD_MAX_ITER) {
            const int32_t n = 1 << d;
            int32_t j, s;
            sd_decode_tri((int32_t)(g - tri_start[t]), n, j, s);
            const int32_t i = s >> 1;
            const int64_t first_new = V + vert_start[t];
            if (s & 1) {
                out[0] = sd_vertex_id(i + 1, j, n, idx, first_new);
                out[1] = sd_vertex_id(i + 1, j + 1, n, idx, first_new);
                out[2] = sd_vertex_id(i, j + 1, n, idx, first_new);
            } else {
                out[0] = sd_vertex_id(i, j, n, idx, first_new);
                out[1] = sd_vertex_id(i + 1, j, n, idx, first_new);
                out[2] = sd_vertex_id(i, j + 1, n, idx, first_new);
            }
        }
        if (out_index != nullptr) out_index[g] = (int32_t)t;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) stage[3 * threadIdx.x + k] = out[k];
    sd_store_records(stage, out_triangles, base, total);
}

static inline bool sd_threshold_valid(float max_edge, int32_t max_iter) {
    return max_edge > 0.0f && max_edge < INFINITY && max_iter >= 0 && max_iter <= SD_MAX_ITER;
}

extern "C" int mh_subdiv_count(const float *vertices, int64_t V, const int32_t *triangles, int64_t T, float max_edge,
                               int32_t max_iter, int32_t *depth, int64_t *n_vert, int64_t *n_tri, void *stream) {
    if (!sd_count_valid(V) || !sd_count_valid(T) || !sd_threshold_valid(max_edge, max_iter)) return MH_ERR_ARG;
    if (T == 0) return MH_OK;
    if (!triangles || !depth || !n_vert || !n_tri || (V > 0 && !vertices)) return MH_ERR_ARG;
    const double m = (double)max_edge;
    hipLaunchKernelGGL(sd_count_kernel, dim3(sd_blocks(T)), dim3(SD_THREADS), 0, mh_stream(stream), vertices, V, triangles, T,
                       m * m, (int)max_iter, depth, n_vert, n_tri);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_subdiv_emit(const float *vertices, const float *colors, int64_t V, const int32_t *triangles, int64_t T,
                              const int32_t *depth, const int64_t *vert_start, const int64_t *tri_start, int64_t n_new_vertices,
                              int64_t n_triangles, float *out_vertices, float *out_colors, int32_t *out_triangles,
                              int32_t *out_index, void *stream) {
    if (!sd_count_valid(V) || !sd_count_valid(T) || n_new_vertices < 0 || n_triangles < T) return MH_ERR_ARG;
    if (V + n_new_vertices >= ((int64_t)1 << 31) || n_triangles >= ((int64_t)1 << 31)) return MH_ERR_OVERFLOW;
    if (T == 0) return MH_OK;
    if (!triangles || !depth || !vert_start || !tri_start || !out_vertices || !out_triangles || (V > 0 && !vertices) ||
        (colors != nullptr) != (out_colors != nullptr))
        return MH_ERR_ARG;
    hipStream_t s = mh_stream(stream);
    const int64_t total_v = V + n_new_vertices;
    if (total_v > 0) {
        hipLaunchKernelGGL(sd_emit_vertices, dim3(sd_blocks(total_v)), dim3(SD_THREADS), 0, s, vertices, colors, V, triangles, T,
                           depth, vert_start, total_v, out_vertices, out_colors);
        MH_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(sd_emit_triangles, dim3(sd_blocks(n_triangles)), dim3(SD_THREADS), 0, s, triangles, V, T, depth, vert_start,
                       tri_start, n_triangles, out_triangles, out_index);
    MH_CHECK_LAUNCH();
    return MH_OK;
}
