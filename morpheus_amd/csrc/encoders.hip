// The reference's two other native encoders: the frequency encoding and the real spherical harmonics.
//
// Replaces external/encoders/freqencoder/src/freqencoder.cu:28-94 and external/encoders/shencoder/src/shencoder.cu:28-end
// (definitions and layouts: include/morpheus_hip.h).  Both are pure streaming: 4 .. 32 bytes of input a point against 4 .. 1056
// bytes of output, so what matters is that a wave's stores are whole contiguous lines.
//   frequency forward   one lane per (point, dimension): ONE sincosf per band gives the sine and the cosine column (an
//                       element-parallel form evaluates it once per output element, twice the work, and was bound by it:
//                       0.171 ms against 0.077 at 2^21 x 39); a workgroup's ~84 rows are laid down in LDS and leave
//                       as one contiguous run of 16-byte stores
//   frequency backward  the gradient rows come in the same way in reverse, one lane per (point, dimension) walks its bands in
//                       LDS; grad_x is written contiguously
//   SH forward          one lane per point (the 64 polynomials share their terms, sh_table.inc), one wave per workgroup: the
//                       wave's 64 x degree^2 tile is laid down in LDS column by column (stride 65: the lanes of a column write 64
//                       different banks, the lanes of the copy-out read (column + point) mod 32) and leaves as 16-byte stores
//   SH backward         the gradient tile comes in the same way in reverse, each lane walks the derivative polynomials against
//                       its column of it; the three sums leave through LDS as one contiguous run of 768 bytes
// The 16-byte accesses need 16-byte aligned buffers; a call with a buffer that is not takes the same kernels with dword accesses.
// Built with -ffp-contract=off: tests/encoders_oracle.py walks the statements of sh_table.inc in numpy and must get the same bits.
#include "common.h"

#define ENC_BLOCK 256
#define SH_STRIDE 65      // floats between two columns of the LDS tile

static inline bool enc_aligned16(const void *a, const void *b) { return ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0; }

// ---------------------------------------------------------------------------------------------- frequency
// A workgroup's tile: P = (256 / D) & ~3 points (84 at D = 3), one thread per (point, dimension), the P x C rows in LDS
// (P C = 256 (1 + 2 degree) floats at most: 33 KB at degree 16).  P is a multiple of 4, so a tile starts 16-byte aligned.
extern __shared__ __attribute__((aligned(16))) float enc_tile[];

// rows [0, n) of floats between global memory and the LDS tile, 16 bytes a lane where the buffer allows
template <bool TO_LDS>
__device__ __forceinline__ void freq_tile_copy(float *__restrict__ g, float *__restrict__ tile, int n, int vec) {
    const int t = threadIdx.x;
    if (vec) {
        for (int i0 = t * 4; i0 + 4 <= n; i0 += ENC_BLOCK * 4) {
            if (TO_LDS) *reinterpret_cast<f32x4 *>(tile + i0) = *reinterpret_cast<const f32x4 *>(g + i0);
            else *reinterpret_cast<f32x4 *>(g + i0) = *reinterpret_cast<const f32x4 *>(tile + i0);
        }
        for (int i = (n & ~3) + t; i < n; i += ENC_BLOCK) {
            if (TO_LDS) tile[i] = g[i]; else g[i] = tile[i];
        }
    } else {
        for (int i = t; i < n; i += ENC_BLOCK) {
            if (TO_LDS) tile[i] = g[i]; else g[i] = tile[i];
        }
    }
}

// forward: thread (p, d) lays x, then per band the sine and the cosine of ONE sincosf, into its row of the tile; the tile leaves
// as one contiguous run
__global__ __launch_bounds__(ENC_BLOCK) void freq_fwd_kernel(const float *__restrict__ x, float *__restrict__ out, int64_t B,
                                                              int64_t n_tiles, int P, int D, int degree, int n_keep, int vec) {
    const int C = D + 2 * D * degree, t = threadIdx.x;
    const int p = t / D, d = t - p * D;
    for (int64_t tile_id = blockIdx.x; tile_id < n_tiles; tile_id += gridDim.x) {
        const int64_t base = tile_id * P;
        const int rows = (B - base) < P ? (int)(B - base) : P;
        if (p < rows) {
            const float xv = x[base * D + t];
            float *row = enc_tile + p * C + d;
            row[0] = xv;
            row += D;
            for (int f = 0; f < degree; f++) {
                float s = 0.0f, co = 0.0f;
                if (f < n_keep) sincosf(ldexpf(xv, f), &s, &co);
                row[0] = s, row[D] = co;
                row += 2 * D;
            }
        }
        __syncthreads();
        freq_tile_copy<false>(out + base * C, enc_tile, rows * C, vec);
        __syncthreads();
    }
}

// backward: the gradient tile comes in as one contiguous run; thread (p, d) then forms
// grad_x[b,d] = grad[b,d] + sum over f < n_keep, ascending, of ldexp(g_sin cos - g_cos sin, f): two rounded products, their rounded
// difference, an exact scaling, one rounded addition per band
__global__ __launch_bounds__(ENC_BLOCK) void freq_bwd_kernel(const float *__restrict__ x, const float *__restrict__ grad,
                                                              float *__restrict__ grad_x, int64_t B, int64_t n_tiles, int P, int D,
                                                              int degree, int n_keep, int vec) {
    const int C = D + 2 * D * degree, t = threadIdx.x;
    const int p = t / D, d = t - p * D;
    for (int64_t tile_id = blockIdx.x; tile_id < n_tiles; tile_id += gridDim.x) {
        const int64_t base = tile_id * P;
        const int rows = (B - base) < P ? (int)(B - base) : P;
        freq_tile_copy<true>(const_cast<float *>(grad) + base * C, enc_tile, rows * C, vec);
        __syncthreads();
        if (p < rows) {
            const float xv = x[base * D + t];
            const float *g = enc_tile + p * C + d;
            float acc = g[0];
            g += D;
            for (int f = 0; f < n_keep; f++) {
                float s, co;
                sincosf(ldexpf(xv, f), &s, &co);
                const float a = g[0] * co, b = g[D] * s;
                const float diff = a - b;
                acc = acc + ldexpf(diff, f);
                g += 2 * D;
            }
            grad_x[base * D + t] = acc;
        }
        __syncthreads();
    }
}

static inline bool freq_args_ok(int64_t B, int32_t D, int32_t degree, int32_t n_keep) {
    return B >= 0 && D >= 1 && D <= 8 && degree >= 0 && degree <= 16 && n_keep >= 0 && n_keep <= degree;
}

static int freq_launch(const float *x, const float *grad, float *dst, int64_t B, int32_t D, int32_t degree, int32_t n_keep,
                       hipStream_t stream) {
    const int C = D + 2 * D * degree, P = (ENC_BLOCK / D) & ~3;
    if (B > INT64_MAX / (4 * C)) return MH_ERR_ARG;          // B C floats must be addressable
    const int64_t n_tiles = (B + P - 1) / P;
    const unsigned blocks = (unsigned)(n_tiles < (1 << 22) ? n_tiles : (1 << 22));      // the kernels stride over the tiles that are left
    const size_t lds = (size_t)P * C * sizeof(float);
    if (grad)
        hipLaunchKernelGGL(freq_bwd_kernel, dim3(blocks), dim3(ENC_BLOCK), lds, stream, x, grad, dst, B, n_tiles, P, (int)D, (int)degree,
                           (int)n_keep, enc_aligned16(grad, nullptr) ? 1 : 0);
    else
        hipLaunchKernelGGL(freq_fwd_kernel, dim3(blocks), dim3(ENC_BLOCK), lds, stream, x, dst, B, n_tiles, P, (int)D, (int)degree,
                           (int)n_keep, enc_aligned16(dst, nullptr) ? 1 : 0);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_freq_encode_fwd(const float *x, int64_t B, int32_t D, int32_t degree, int32_t n_keep, float *out, void *stream) {
    if (!freq_args_ok(B, D, degree, n_keep)) return MH_ERR_ARG;
    if (B == 0) return MH_OK;
    if (!x || !out) return MH_ERR_ARG;
    return freq_launch(x, nullptr, out, B, D, degree, n_keep, mh_stream(stream));
}

extern "C" int mh_freq_encode_bwd(const float *x, const float *grad, int64_t B, int32_t D, int32_t degree, int32_t n_keep,
                                  float *grad_x, void *stream) {
    if (!freq_args_ok(B, D, degree, n_keep)) return MH_ERR_ARG;
    if (B == 0) return MH_OK;
    if (!x || !grad || !grad_x) return MH_ERR_ARG;
    return freq_launch(x, grad, grad_x, B, D, degree, n_keep, mh_stream(stream));
}

// ---------------------------------------------------------------------------------------------- spherical harmonics
// The wave's tile of n = rows * C2 floats at `g` (contiguous, point-major) <-> the LDS image tile[column * 65 + point].
template <int C2, bool TO_LDS>
__device__ __forceinline__ void sh_tile_copy(float *__restrict__ g, float *__restrict__ tile, int n, int vec) {
    constexpr int ITER = (MH_WAVE * C2 + 255) / 256;      // 16-byte groups a lane moves: all loads are issued before the first use
    const int lane = threadIdx.x;
    float v[ITER][4];
    if (TO_LDS) {
#pragma unroll
        for (int it = 0; it < ITER; it++) {
            const int i0 = lane * 4 + it * 256;
            if (i0 + 4 <= n && vec) {
                const f32x4 a = *reinterpret_cast<const f32x4 *>(g + i0);
#pragma unroll
                for (int k = 0; k < 4; k++) v[it][k] = a[k];
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) v[it][k] = (i0 + k < n) ? g[i0 + k] : 0.0f;
            }
        }
    }
#pragma unroll
    for (int it = 0; it < ITER; it++) {
        const int i0 = lane * 4 + it * 256;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (i0 + k < n) {
                const int p = (i0 + k) / C2, c = (i0 + k) - p * C2;
                if (TO_LDS) tile[c * SH_STRIDE + p] = v[it][k]; else v[it][k] = tile[c * SH_STRIDE + p];
            }
        }
        if (!TO_LDS) {
            if (i0 + 4 <= n && vec) {
                f32x4 a;
#pragma unroll
                for (int k = 0; k < 4; k++) a[k] = v[it][k];
                *reinterpret_cast<f32x4 *>(g + i0) = a;
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (i0 + k < n) g[i0 + k] = v[it][k];
            }
        }
    }
}

template <int DEG>
__global__ __launch_bounds__(MH_WAVE) void sh_fwd_kernel(const float *__restrict__ xin, float *__restrict__ out, int64_t B, int vec) {
    constexpr int C2 = DEG * DEG;
    __shared__ float tile[C2 * SH_STRIDE];
    const int lane = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * MH_WAVE;
    const int rows = (B - base) < MH_WAVE ? (int)(B - base) : MH_WAVE;
    float x = 0.f, y = 0.f, z = 0.f;
    if (lane < rows) x = xin[(base + lane) * 3], y = xin[(base + lane) * 3 + 1], z = xin[(base + lane) * 3 + 2];
#define SH_Y(c, v) if constexpr ((c) < C2) tile[(c) * SH_STRIDE + lane] = (v)
#define SH_DX(c, v)
#define SH_DY(c, v)
#define SH_DZ(c, v)
#define SH_TABLE_FORWARD
#include "sh_table.inc"
#undef SH_TABLE_FORWARD
#undef SH_Y
#undef SH_DX
#undef SH_DY
#undef SH_DZ
    __syncthreads();
    sh_tile_copy<C2, false>(out + base * C2, tile, rows * C2, vec);
}

// grad_x[a] = sum over the columns c < degree^2, ascending, of grad[c] (dY_c / dx_a): each product rounded, then added to the
// running sum, which starts at +0; a derivative that is identically zero contributes no term
template <int DEG>
__global__ __launch_bounds__(MH_WAVE) void sh_bwd_kernel(const float *__restrict__ xin, const float *__restrict__ grad,
                                                         float *__restrict__ grad_x, int64_t B, int vec) {
    constexpr int C2 = DEG * DEG;
    __shared__ float tile[C2 * SH_STRIDE];
    __shared__ float gout[MH_WAVE * 3];
    const int lane = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * MH_WAVE;
    const int rows = (B - base) < MH_WAVE ? (int)(B - base) : MH_WAVE;
    sh_tile_copy<C2, true>(const_cast<float *>(grad) + base * C2, tile, rows * C2, vec);
    float x = 0.f, y = 0.f, z = 0.f;
    if (lane < rows) x = xin[(base + lane) * 3], y = xin[(base + lane) * 3 + 1], z = xin[(base + lane) * 3 + 2];
    __syncthreads();
    float gx = 0.f, gy = 0.f, gz = 0.f;
    if (lane < rows) {      // (the columns of the lanes beyond the tile's rows were never written)
#define SH_Y(c, v)
#define SH_DX(c, v) if constexpr ((c) < C2) gx = gx + tile[(c) * SH_STRIDE + lane] * (v)
#define SH_DY(c, v) if constexpr ((c) < C2) gy = gy + tile[(c) * SH_STRIDE + lane] * (v)
#define SH_DZ(c, v) if constexpr ((c) < C2) gz = gz + tile[(c) * SH_STRIDE + lane] * (v)
#define SH_TABLE_BACKWARD
#include "sh_table.inc"
#undef SH_TABLE_BACKWARD
#undef SH_Y
#undef SH_DX
#undef SH_DY
#undef SH_DZ
    }
    gout[lane * 3] = gx, gout[lane * 3 + 1] = gy, gout[lane * 3 + 2] = gz;
    __syncthreads();
    float *dst = grad_x + base * 3;
    const int n = rows * 3;
    if (vec) {
        const int i0 = lane * 4;
        if (i0 + 4 <= n) {
            f32x4 a;
#pragma unroll
            for (int k = 0; k < 4; k++) a[k] = gout[i0 + k];
            *reinterpret_cast<f32x4 *>(dst + i0) = a;
        } else {
            for (int i = i0; i < n; i++) dst[i] = gout[i];
        }
    } else {
        for (int i = lane; i < n; i += MH_WAVE) dst[i] = gout[i];
    }
}

template <int DEG>
static int sh_launch(const float *x, const float *grad, float *dst, int64_t B, hipStream_t stream) {
    const unsigned blocks = (unsigned)((B + MH_WAVE - 1) / MH_WAVE);
    if (grad)
        hipLaunchKernelGGL(sh_bwd_kernel<DEG>, dim3(blocks), dim3(MH_WAVE), 0, stream, x, grad, dst, B, enc_aligned16(grad, dst) ? 1 : 0);
    else
        hipLaunchKernelGGL(sh_fwd_kernel<DEG>, dim3(blocks), dim3(MH_WAVE), 0, stream, x, dst, B, enc_aligned16(dst, nullptr) ? 1 : 0);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

static int sh_dispatch(const float *x, const float *grad, float *dst, int64_t B, int32_t degree, hipStream_t stream) {
    switch (degree) {
        case 1: return sh_launch<1>(x, grad, dst, B, stream);
        case 2: return sh_launch<2>(x, grad, dst, B, stream);
        case 3: return sh_launch<3>(x, grad, dst, B, stream);
        case 4: return sh_launch<4>(x, grad, dst, B, stream);
        case 5: return sh_launch<5>(x, grad, dst, B, stream);
        case 6: return sh_launch<6>(x, grad, dst, B, stream);
        case 7: return sh_launch<7>(x, grad, dst, B, stream);
        case 8: return sh_launch<8>(x, grad, dst, B, stream);
    }
    return MH_ERR_ARG;
}

// one wave per workgroup and 64 points each: B is bounded by the grid's 2^31 - 1 workgroups
static inline bool sh_args_ok(int64_t B, int32_t degree) { return B >= 0 && B <= (int64_t)MH_WAVE * 0x7fffffff && degree >= 1 && degree <= 8; }

extern "C" int mh_sh_encode_fwd(const float *x, int64_t B, int32_t degree, float *out, void *stream) {
    if (!sh_args_ok(B, degree)) return MH_ERR_ARG;
    if (B == 0) return MH_OK;
    if (!x || !out) return MH_ERR_ARG;
    return sh_dispatch(x, nullptr, out, B, degree, mh_stream(stream));
}

extern "C" int mh_sh_encode_bwd(const float *x, const float *grad, int64_t B, int32_t degree, float *grad_x, void *stream) {
    if (!sh_args_ok(B, degree)) return MH_ERR_ARG;
    if (B == 0) return MH_OK;
    if (!x || !grad || !grad_x) return MH_ERR_ARG;
    return sh_dispatch(x, grad, grad_x, B, degree, mh_stream(stream));
}
