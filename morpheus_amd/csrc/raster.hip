// Triangle rasteriser for exported meshes: the depth maps and images of render_all_meshes (morpheus.py:418-470, an Open3D
// window per frame there).  Conventions, operator order and limits are in include/morpheus_hip.h (mh_raster_*,
// mh_mesh_vertex_normals); tests/raster_oracle.py restates them in numpy and pins depth, triangle ids and the fixed-point
// normal sums bit for bit.
//
// Launches of mh_raster_depth:
//   rs_init_kernel    keys = empty, queue length = 0, clipped = 0
//   rs_small_kernel   one lane per triangle: vertex stage, set-up; a triangle whose clamped bounding box holds at most
//                     `small_area` pixel centres is walked by its lane, the others are appended to the queue
//   rs_large_kernel   one wavefront per (queue entry, slice): the 64 lanes walk the box 64 centres at a time; RS_SLICES
//                     wavefronts share one box.  The queue length is read from device memory, the host never waits.
// Every loop is bounded by the clamped box (<= W*H centres) or by the queue length (<= T).  The depth test is one 64-bit
// atomicMin per covered centre on (depth bits << 32 | triangle), so the key buffer does not depend on the order of anything.
// mh_raster_resolve: one lane per pixel.  mh_mesh_vertex_normals: max |cross component| (atomicMax on float bits), 64-bit
// integer atomic sums on the grid that maximum fixes, one conversion per vertex.
#include "common.h"
#include "wave.h"

#pragma clang fp contract(off)

#define RS_THREADS 256
#define RS_SLICES 16
#define RS_MAX_SIDE 16384
#define RS_SMALL_AREA 256                         // default of the small / large split (profiles/r08_mesh_render.txt)
#define RS_EMPTY 0xffffffffffffffffull
#define RS_SNAP_LIMIT 8388608.0f                  // 2^23

struct RsCam {
    float w[12];                                  // world -> camera, row-major [3][4]
    float fx, fy, cx, cy, near;
    int32_t H, W;
};

struct RsWorkspace {
    unsigned long long *keys;                     // [H*W]
    uint32_t *qlen;                               // queue length (one word of a 256-byte slot)
    int32_t *queue;                               // [T]
};

struct RsSetup {
    int32_t X[3], Y[3];                           // snapped screen coordinates, ordered so that the doubled area is > 0
    int32_t i0, i1, j0, j1;                       // pixel centres inside the bounding box, clamped to the image
    float n[3], na;                               // plane of the triangle in camera space: n . P = na
};

static inline int64_t rs_align(int64_t b) { return (b + 255) & ~(int64_t)255; }

static inline bool rs_valid(int32_t H, int32_t W, int64_t T) {
    return H >= 1 && W >= 1 && H <= RS_MAX_SIDE && W <= RS_MAX_SIDE && T >= 0 && T < ((int64_t)1 << 31);
}

static inline int64_t rs_layout(int32_t H, int32_t W, int64_t T, void *base, RsWorkspace *ws) {
    const int64_t o_q = rs_align((int64_t)H * W * 8);
    const int64_t o_queue = o_q + 256;
    const int64_t total = o_queue + rs_align(T * 4);
    if (ws) {
        char *b = static_cast<char *>(base);
        ws->keys = reinterpret_cast<unsigned long long *>(b);
        ws->qlen = reinterpret_cast<uint32_t *>(b + o_q);
        ws->queue = reinterpret_cast<int32_t *>(b + o_queue);
    }
    return total;
}

static inline RsCam rs_cam(const float *w2c_host, float fx, float fy, float cx, float cy, float near, int32_t H, int32_t W) {
    RsCam c;
    for (int k = 0; k < 12; k++) c.w[k] = w2c_host[k];
    c.fx = fx, c.fy = fy, c.cx = cx, c.cy = cy, c.near = near, c.H = H, c.W = W;
    return c;
}

__device__ __forceinline__ void rs_to_cam(const RsCam &cam, const float *__restrict__ p, float *o) {
#pragma unroll
    for (int r = 0; r < 3; r++)
        o[r] = ((cam.w[4 * r] * p[0] + cam.w[4 * r + 1] * p[1]) + cam.w[4 * r + 2] * p[2]) + cam.w[4 * r + 3];
}

__device__ __forceinline__ void rs_cross(const float *a, const float *b, const float *c, float *n) {
    const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const float e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
}

__device__ __forceinline__ float rs_dot(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// the three vertices of triangle t in camera space; false when an index is outside [0, V)
__device__ __forceinline__ bool rs_load(const RsCam &cam, const float *__restrict__ vertices, int64_t V,
                                        const int32_t *__restrict__ triangles, int64_t t, int32_t *idx, float (*p)[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        idx[k] = triangles[3 * t + k];
        if (idx[k] < 0 || idx[k] >= V) return false;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) rs_to_cam(cam, vertices + 3 * (int64_t)idx[k], p[k]);
    return true;
}

// 0: draw, 1: dropped and counted (behind `near`, or a snapped coordinate outside +-2^23 / not finite), 2: dropped
__device__ __forceinline__ int rs_setup(const RsCam &cam, const float *__restrict__ vertices, int64_t V,
                                        const int32_t *__restrict__ triangles, int64_t t, RsSetup &s) {
    int32_t idx[3];
    float p[3][3];
    if (!rs_load(cam, vertices, V, triangles, t, idx, p)) return 2;
#pragma unroll
    for (int k = 0; k < 3; k++)
        if (!(p[k][2] >= cam.near)) return 1;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float sx = (cam.fx * p[k][0]) / p[k][2] + cam.cx;
        const float sy = (cam.fy * p[k][1]) / p[k][2] + cam.cy;
        const float X = rintf(sx * 256.0f), Y = rintf(sy * 256.0f);
        if (!(fabsf(X) < RS_SNAP_LIMIT) || !(fabsf(Y) < RS_SNAP_LIMIT)) return 1;
        s.X[k] = (int32_t)X;
        s.Y[k] = (int32_t)Y;
    }
    const int64_t area2 = (int64_t)(s.X[1] - s.X[0]) * (s.Y[2] - s.Y[0]) - (int64_t)(s.Y[1] - s.Y[0]) * (s.X[2] - s.X[0]);
    if (area2 == 0) return 2;
    if (area2 < 0) {
        int32_t q = s.X[1];
        s.X[1] = s.X[2], s.X[2] = q;
        q = s.Y[1];
        s.Y[1] = s.Y[2], s.Y[2] = q;
    }
    const int32_t xmin = min(s.X[0], min(s.X[1], s.X[2])), xmax = max(s.X[0], max(s.X[1], s.X[2]));
    const int32_t ymin = min(s.Y[0], min(s.Y[1], s.Y[2])), ymax = max(s.Y[0], max(s.Y[1], s.Y[2]));
    // centres 256 i + 128 inside [min, max]; >> is the arithmetic shift (floor)
    s.i0 = max((xmin + 127) >> 8, 0);
    s.i1 = min((xmax - 128) >> 8, cam.W - 1);
    s.j0 = max((ymin + 127) >> 8, 0);
    s.j1 = min((ymax - 128) >> 8, cam.H - 1);
    if (s.i0 > s.i1 || s.j0 > s.j1) return 2;
    rs_cross(p[0], p[1], p[2], s.n);
    s.na = rs_dot(s.n, p[0]);
    return 0;
}

// is the centre of pixel (i, j) covered?  E > 0 on all three edges, or E == 0 on an edge that owns its points: the directed
// edge (dx, dy) of the positively ordered triangle owns them when dy > 0, or dy == 0 and dx > 0 -- its reverse never does
__device__ __forceinline__ bool rs_covers(const RsSetup &s, int32_t i, int32_t j) {
    const int64_t px = 256 * (int64_t)i + 128, py = 256 * (int64_t)j + 128;
    bool in = true;
#pragma unroll
    for (int e = 0; e < 3; e++) {
        const int f = (e + 1) % 3;
        const int64_t dx = s.X[f] - s.X[e], dy = s.Y[f] - s.Y[e];
        const int64_t E = dx * (py - s.Y[e]) - dy * (px - s.X[e]);
        in = in && (E > 0 || (E == 0 && (dy > 0 || (dy == 0 && dx > 0))));
    }
    return in;
}

__device__ __forceinline__ void rs_pixel_dir(const RsCam &cam, int32_t i, int32_t j, float *d) {
    d[0] = (((float)i + 0.5f) - cam.cx) / cam.fx;
    d[1] = (((float)j + 0.5f) - cam.cy) / cam.fy;
    d[2] = 1.0f;
}

__device__ __forceinline__ void rs_fragment(const RsCam &cam, const RsSetup &s, unsigned long long *__restrict__ keys,
                                            int32_t i, int32_t j, int64_t t) {
    if (!rs_covers(s, i, j)) return;
    float d[3];
    rs_pixel_dir(cam, i, j, d);
    const float nd = (s.n[0] * d[0] + s.n[1] * d[1]) + s.n[2];
    const float z = s.na / nd;
    if (!(z >= cam.near && z < INFINITY)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)(uint32_t)t;
    atomicMin(keys + ((int64_t)j * cam.W + i), key);           // i, j are inside the image: the box is clamped to it
}

__global__ __launch_bounds__(RS_THREADS) void rs_init_kernel(unsigned long long *__restrict__ keys, int64_t n,
                                                             uint32_t *__restrict__ qlen, int64_t *__restrict__ clipped) {
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t k = first; k < n; k += (int64_t)gridDim.x * blockDim.x) keys[k] = RS_EMPTY;
    if (first == 0) {
        *qlen = 0u;
        *clipped = 0;
    }
}

__global__ __launch_bounds__(RS_THREADS) void rs_small_kernel(RsCam cam, const float *__restrict__ vertices, int64_t V,
                                                              const int32_t *__restrict__ triangles, int64_t T,
                                                              int32_t small_area, RsWorkspace ws,
                                                              int64_t *__restrict__ clipped) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    RsSetup s;
    const int st = t < T ? rs_setup(cam, vertices, V, triangles, t, s) : 2;
    const unsigned long long counted = __ballot(st == 1);
    if (counted && mh_lane() == 0) atomicAdd(reinterpret_cast<unsigned long long *>(clipped), (unsigned long long)__popcll(counted));
    if (st != 0) return;
    const int64_t area = (int64_t)(s.i1 - s.i0 + 1) * (s.j1 - s.j0 + 1);
    // queue append, one atomic per wavefront: the lowest appending lane reserves the wave's slots.  The lanes that returned
    // above take no part in the ballot (it counts active lanes only), so no lane waits for an absent one.
    const bool large = area > small_area;
    const unsigned long long appending = __ballot(large);
    if (large) {
        const int lane = mh_lane();
        const int leader = __ffsll(appending) - 1;
        uint32_t base = 0u;
        if (lane == leader) base = atomicAdd(ws.qlen, (uint32_t)__popcll(appending));
        base = (uint32_t)__shfl((int)base, leader);
        const uint32_t slot = base + (uint32_t)wave_rank(appending, lane);
        if (slot < T) ws.queue[slot] = (int32_t)t;             // each triangle is appended at most once: slot < T always
        return;
    }
    for (int32_t j = s.j0; j <= s.j1; j++)
        for (int32_t i = s.i0; i <= s.i1; i++) rs_fragment(cam, s, ws.keys, i, j, t);
}

__global__ __launch_bounds__(RS_THREADS) void rs_large_kernel(RsCam cam, const float *__restrict__ vertices, int64_t V,
                                                              const int32_t *__restrict__ triangles, int64_t T,
                                                              RsWorkspace ws) {
    const int64_t n_q = min((int64_t)*ws.qlen, T);
    const int64_t waves = (int64_t)gridDim.x * (RS_THREADS / MH_WAVE);
    const int lane = mh_lane();
    for (int64_t q = (int64_t)blockIdx.x * (RS_THREADS / MH_WAVE) + (threadIdx.x >> 6); q < n_q; q += waves) {
        const int64_t t = ws.queue[q];
        if (t < 0 || t >= T) continue;
        RsSetup s;
        if (rs_setup(cam, vertices, V, triangles, t, s) != 0) continue;       // the same for the 64 lanes
        const int32_t bw = s.i1 - s.i0 + 1;
        const int32_t area = bw * (s.j1 - s.j0 + 1);                          // <= 2^28
        const int32_t n_it = (area + MH_WAVE - 1) / MH_WAVE;
        const int32_t per = (n_it + RS_SLICES - 1) / RS_SLICES;
        const int32_t it0 = (int32_t)blockIdx.y * per, it1 = min(n_it, it0 + per);
        for (int32_t it = it0; it < it1; it++) {
            const int32_t k = it * MH_WAVE + lane;
            if (k < area) {
                const int32_t y = k / bw;
                rs_fragment(cam, s, ws.keys, s.i0 + (k - y * bw), s.j0 + y, t);
            }
        }
    }
}

// |v| as sqrt((x x + y y) + z z); v / |v|, or (0, 0, 1) when that is not > 0
__device__ __forceinline__ void rs_normalize(const float *v, float *o) {
    const float len = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    if (len > 0.0f && len < INFINITY) {
        o[0] = v[0] / len, o[1] = v[1] / len, o[2] = v[2] / len;
    } else {
        o[0] = 0.0f, o[1] = 0.0f, o[2] = 1.0f;
    }
}

__global__ __launch_bounds__(RS_THREADS) void rs_resolve_kernel(RsCam cam, const float *__restrict__ vertices, int64_t V,
                                                                const int32_t *__restrict__ triangles, int64_t T,
                                                                const float *__restrict__ colors,
                                                                const float *__restrict__ normals, int32_t mode, float ambient,
                                                                float bg0, float bg1, float bg2,
                                                                const unsigned long long *__restrict__ keys,
                                                                float *__restrict__ depth, int32_t *__restrict__ tri_id,
                                                                float *__restrict__ image) {
    const int64_t pix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= (int64_t)cam.H * cam.W) return;
    const unsigned long long key = keys[pix];
    const int64_t t = (int64_t)(key & 0xffffffffull);
    int32_t idx[3];
    float p[3][3];
    if (key == RS_EMPTY || t >= T || !rs_load(cam, vertices, V, triangles, t, idx, p)) {
        depth[pix] = 0.0f;
        tri_id[pix] = -1;
        image[3 * pix] = bg0, image[3 * pix + 1] = bg1, image[3 * pix + 2] = bg2;
        return;
    }
    const float z = __uint_as_float((uint32_t)(key >> 32));
    depth[pix] = z;
    tri_id[pix] = (int32_t)t;
    const int32_t j = (int32_t)(pix / cam.W), i = (int32_t)(pix - (int64_t)j * cam.W);
    float d[3], n[3];
    rs_pixel_dir(cam, i, j, d);
    rs_cross(p[0], p[1], p[2], n);
    const float P[3] = {z * d[0], z * d[1], z};
    // barycentrics from the 3-D sub-areas against n
    float r[3][3], c[3], wgt[3];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int a = 0; a < 3; a++) r[k][a] = p[k][a] - P[a];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float *u = r[(k + 1) % 3], *v = r[(k + 2) % 3];
        c[0] = u[1] * v[2] - u[2] * v[1];
        c[1] = u[2] * v[0] - u[0] * v[2];
        c[2] = u[0] * v[1] - u[1] * v[0];
        wgt[k] = rs_dot(n, c);
    }
    const float sum = (wgt[0] + wgt[1]) + wgt[2];
    float l0 = wgt[0] / sum, l1 = wgt[1] / sum, l2 = wgt[2] / sum;
    // a sliver whose sub-areas underflow or cancel (sum == 0, or a weight that is not finite): the centroid's attributes
    if (!(fabsf(l0) < INFINITY && fabsf(l1) < INFINITY && fabsf(l2) < INFINITY)) l0 = l1 = l2 = 1.0f / 3.0f;
    float base[3] = {0.7f, 0.7f, 0.7f};
    if (colors) {
#pragma unroll
        for (int a = 0; a < 3; a++)
            base[a] = (l0 * colors[3 * (int64_t)idx[0] + a] + l1 * colors[3 * (int64_t)idx[1] + a]) +
                      l2 * colors[3 * (int64_t)idx[2] + a];
    }
    float out[3] = {base[0], base[1], base[2]};
    if (mode != 0) {
        float nw[3], nc[3], nn[3];
#pragma unroll
        for (int a = 0; a < 3; a++)
            nw[a] = (l0 * normals[3 * (int64_t)idx[0] + a] + l1 * normals[3 * (int64_t)idx[1] + a]) +
                    l2 * normals[3 * (int64_t)idx[2] + a];
#pragma unroll
        for (int a = 0; a < 3; a++) nc[a] = (cam.w[4 * a] * nw[0] + cam.w[4 * a + 1] * nw[1]) + cam.w[4 * a + 2] * nw[2];
        rs_normalize(nc, nn);
        if (mode == 1) {
#pragma unroll
            for (int a = 0; a < 3; a++) out[a] = (nn[a] + 1.0f) / 2.0f;
        } else {
            const float mv[3] = {-P[0], -P[1], -P[2]};
            float vv[3];
            rs_normalize(mv, vv);
            const float shade = ambient + (1.0f - ambient) * fabsf(rs_dot(nn, vv));
#pragma unroll
            for (int a = 0; a < 3; a++) out[a] = base[a] * shade;
        }
    }
    image[3 * pix] = out[0], image[3 * pix + 1] = out[1], image[3 * pix + 2] = out[2];
}

// ---- vertex normals ------------------------------------------------------------------------------------------------------

// un-normalised cross product of triangle t in world space; false: index outside [0, V) or a component not finite
__device__ __forceinline__ bool vn_cross(const float *__restrict__ vertices, int64_t V, const int32_t *__restrict__ triangles,
                                         int64_t t, int32_t *idx, float *n) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        idx[k] = triangles[3 * t + k];
        if (idx[k] < 0 || idx[k] >= V) return false;
    }
    rs_cross(vertices + 3 * (int64_t)idx[0], vertices + 3 * (int64_t)idx[1], vertices + 3 * (int64_t)idx[2], n);
    return fabsf(n[0]) < INFINITY && fabsf(n[1]) < INFINITY && fabsf(n[2]) < INFINITY;
}

__global__ __launch_bounds__(RS_THREADS) void vn_max_kernel(const float *__restrict__ vertices, int64_t V,
                                                            const int32_t *__restrict__ triangles, int64_t T,
                                                            uint32_t *__restrict__ gmax_bits) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t idx[3];
    float n[3];
    uint32_t m = 0u;
    if (t < T && vn_cross(vertices, V, triangles, t, idx, n))
        m = __float_as_uint(fmaxf(fabsf(n[0]), fmaxf(fabsf(n[1]), fabsf(n[2]))));      // bits of a float >= 0 order like it
    m = wave_max(m);
    if (mh_lane() == 0 && m) atomicMax(gmax_bits, m);
}

__global__ __launch_bounds__(RS_THREADS) void vn_add_kernel(const float *__restrict__ vertices, int64_t V,
                                                            const int32_t *__restrict__ triangles, int64_t T,
                                                            const uint32_t *__restrict__ gmax_bits,
                                                            unsigned long long *__restrict__ acc) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t idx[3];
    float n[3];
    if (t >= T || !vn_cross(vertices, V, triangles, t, idx, n)) return;
    const int E = (int)(*gmax_bits >> 23);                     // biased exponent of the maximum: G = 2^(E - 126)
    const double scale = ldexp(1.0, 166 - E);                  // 2^40 / G
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const long long k = llrint((double)n[a] * scale);      // |k| <= 2^40
#pragma unroll
        for (int v = 0; v < 3; v++) atomicAdd(acc + 3 * (int64_t)idx[v] + a, (unsigned long long)k);
    }
}

__global__ __launch_bounds__(RS_THREADS) void vn_finish_kernel(const int64_t *__restrict__ acc, int64_t V,
                                                               float *__restrict__ normals) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const float s[3] = {(float)acc[3 * v], (float)acc[3 * v + 1], (float)acc[3 * v + 2]};
    float o[3];
    rs_normalize(s, o);
    normals[3 * v] = o[0], normals[3 * v + 1] = o[1], normals[3 * v + 2] = o[2];
}

static inline bool rs_count_valid(int64_t V, int64_t T) {
    return V >= 0 && T >= 0 && V < ((int64_t)1 << 31) && T < ((int64_t)1 << 31);
}

extern "C" int mh_mesh_vertex_normals(const float *vertices, int64_t V, const int32_t *triangles, int64_t T, int64_t *acc,
                                      float *normals, void *stream) {
    if (!rs_count_valid(V, T) || !acc || (V > 0 && (!vertices || !normals)) || (T > 0 && !triangles)) return MH_ERR_ARG;
    hipStream_t s = mh_stream(stream);
    if (!mh_zero_async(acc, (size_t)(3 * V + 1) * 8, s)) return MH_ERR_LAUNCH;
    if (V == 0) return MH_OK;
    uint32_t *gmax = reinterpret_cast<uint32_t *>(acc + 3 * V);
    if (T > 0) {
        const unsigned blocks = (unsigned)((T + RS_THREADS - 1) / RS_THREADS);
        hipLaunchKernelGGL(vn_max_kernel, dim3(blocks), dim3(RS_THREADS), 0, s, vertices, V, triangles, T, gmax);
        MH_CHECK_LAUNCH();
        hipLaunchKernelGGL(vn_add_kernel, dim3(blocks), dim3(RS_THREADS), 0, s, vertices, V, triangles, T, gmax,
                           reinterpret_cast<unsigned long long *>(acc));
        MH_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(vn_finish_kernel, dim3((unsigned)((V + RS_THREADS - 1) / RS_THREADS)), dim3(RS_THREADS), 0, s, acc, V,
                       normals);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int64_t mh_raster_workspace_bytes(int32_t H, int32_t W, int64_t T) {
    if (!rs_valid(H, W, T)) return -1;
    return rs_layout(H, W, T, nullptr, nullptr);
}

static inline bool rs_cam_valid(const float *w2c_host, float fx, float fy) {
    return w2c_host && fx > 0.0f && fy > 0.0f && fx < INFINITY && fy < INFINITY;
}

extern "C" int mh_raster_depth(const float *vertices, int64_t V, const int32_t *triangles, int64_t T, const float *w2c_host,
                               float fx, float fy, float cx, float cy, int32_t H, int32_t W, float near, int32_t small_area,
                               void *workspace, int64_t *clipped, void *stream) {
    if (!rs_valid(H, W, T) || !rs_count_valid(V, T) || !rs_cam_valid(w2c_host, fx, fy) || !(near > 0.0f && near < INFINITY) ||
        !workspace || !clipped || (T > 0 && (!triangles || (V > 0 && !vertices))))
        return MH_ERR_ARG;
    const RsCam cam = rs_cam(w2c_host, fx, fy, cx, cy, near, H, W);
    RsWorkspace ws;
    rs_layout(H, W, T, workspace, &ws);
    hipStream_t s = mh_stream(stream);
    const int64_t n = (int64_t)H * W;
    const int64_t init_blocks = (n + RS_THREADS - 1) / RS_THREADS < 4096 ? (n + RS_THREADS - 1) / RS_THREADS : 4096;
    hipLaunchKernelGGL(rs_init_kernel, dim3((unsigned)init_blocks), dim3(RS_THREADS), 0,
                       s, ws.keys, n, ws.qlen, clipped);
    MH_CHECK_LAUNCH();
    if (T == 0 || V == 0) return MH_OK;
    if (small_area <= 0) small_area = RS_SMALL_AREA;
    hipLaunchKernelGGL(rs_small_kernel, dim3((unsigned)((T + RS_THREADS - 1) / RS_THREADS)), dim3(RS_THREADS), 0, s, cam, vertices,
                       V, triangles, T, small_area, ws, clipped);
    MH_CHECK_LAUNCH();
    const int64_t cap = 2 * (int64_t)mh_cu_count();
    const int64_t wave_blocks = (T + 3) / 4 < cap ? (T + 3) / 4 : cap;
    hipLaunchKernelGGL(rs_large_kernel, dim3((unsigned)wave_blocks, RS_SLICES), dim3(RS_THREADS), 0, s, cam, vertices, V,
                       triangles, T, ws);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_raster_resolve(const float *vertices, int64_t V, const int32_t *triangles, int64_t T, const float *colors,
                                 const float *normals, const float *w2c_host, float fx, float fy, float cx, float cy, int32_t H,
                                 int32_t W, int32_t mode, float ambient, float bg_r, float bg_g, float bg_b,
                                 const void *workspace, float *depth, int32_t *tri_id, float *image, void *stream) {
    if (!rs_valid(H, W, T) || !rs_count_valid(V, T) || !rs_cam_valid(w2c_host, fx, fy) || !workspace || !depth || !tri_id ||
        !image || mode < 0 || mode > 2 || (T > 0 && V > 0 && (!triangles || !vertices || (mode != 0 && !normals))))
        return MH_ERR_ARG;
    const RsCam cam = rs_cam(w2c_host, fx, fy, cx, cy, 0.0f, H, W);
    RsWorkspace ws;
    rs_layout(H, W, T, const_cast<void *>(workspace), &ws);
    if (V == 0) T = 0;                                         // nothing was drawn: every key is empty
    const int64_t n = (int64_t)H * W;
    hipLaunchKernelGGL(rs_resolve_kernel, dim3((unsigned)((n + RS_THREADS - 1) / RS_THREADS)), dim3(RS_THREADS), 0,
                       mh_stream(stream), cam, vertices, V, triangles, T, colors, normals, mode, ambient, bg_r, bg_g, bg_b,
                       ws.keys, depth, tri_id, image);
    MH_CHECK_LAUNCH();
    return MH_OK;
}
