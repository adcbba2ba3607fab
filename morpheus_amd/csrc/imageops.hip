// Image resampling around the guidance and the test video (morpheus_amd/imageops.py is the Python face).
//
//   mh_resize_bilinear_fwd / _bwd   PyTorch's upsample_bilinear2d, align_corners=False, no scale factor, with the layout change of
//                                   get_pred_from_outputs and an affine map (`* 2 - 1`) folded in; the backward is a gather
//   mh_resize_area_masked           the white composite of get_embeddings (morpheus.py:254-259) and a shrinking area resize
//   mh_frame_to_u8 / mh_depth_to_u8 render_test_video's quantisation (morpheus.py:1317-1322), the depth's range found on the device
//
// The bilinear rule, one axis (each statement one rounded fp32 operation; tests/imageops_oracle.py restates it):
//   scale = (float)in / (float)out
//   src   = scale * ((float)dst + 0.5f) - 0.5f, 0 where that is negative
//   i0    = (int)src,  i1 = i0 + (i0 < in - 1),  l1 = src - (float)i0,  l0 = 1.0f - l1
//   y     = mul * (l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11)) + add
// out == in gives scale = 1, src = dst, l1 = 0: the input itself (and mul = 1, add = 0 keep its bits).
//
// The backward is the adjoint written as a gather: input pixel (iy, ix) sums l(oy) * l(ox) * gy[oy, ox] over the output pixels whose
// OWN i0 / i1 name it, rows ascending and columns ascending inside a row -- one thread per input pixel, no atomics, the same bits
// on every run.  The candidate rows come from the inverse map in INTEGERS (src in [iy - 1, iy + 1] <=> (2 iy - 1) out <=
// in (2 oy + 1) <= (2 iy + 3) out), widened by one on each side for the rounding of the forward's fp32 src; whether a candidate
// counts is decided by the forward's arithmetic alone (axis_weight), so a pixel is never counted twice or missed at a boundary.
//
// Area resize: output pixel o covers source [o in / out, (o + 1) in / out); in units of 1 / out source pixel i is [i out, (i + 1) out)
// and the box [o in, (o + 1) in), so the overlap is an integer and the weight (float)overlap / (float)in: exact fractions that sum
// to 1.  Only shrinking (out <= in) axes are served.
#include "common.h"

// No FMA contraction: the statements above are separate IEEE round-to-nearest operations (tests/imageops_oracle.py).
#pragma clang fp contract(off)

#include "wave.h"

#define IM_MAX_C 4

struct AxisTap {
    int i0, i1;
    float l0, l1;
};

__device__ __forceinline__ AxisTap axis_tap(int dst, int in, float scale) {
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    AxisTap t;
    t.i0 = min((int)src, in - 1);               // (int)src <= in - 1 already for dst < out; the hold keeps every read in bounds
    t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
    t.l1 = src - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}

__device__ __forceinline__ int64_t in_index(bool nhwc, int b, int c, int y, int x, int C, int H, int W) {
    return nhwc ? (((int64_t)b * H + y) * W + x) * C + c : (((int64_t)b * C + c) * H + y) * W + x;
}

template <int C>
__global__ __launch_bounds__(256) void resize_bilinear_fwd_kernel(const float *__restrict__ x, int B, int Hi, int Wi, int Ho, int Wo,
                                                                  int nhwc, float mul, float add, float *__restrict__ y) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)B * Ho * Wo) return;
    const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho), b = (int)(p / ((int64_t)Wo * Ho));
    const AxisTap h = axis_tap(oy, Hi, (float)Hi / (float)Ho), w = axis_tap(ox, Wi, (float)Wi / (float)Wo);
#pragma unroll
    for (int c = 0; c < C; c++) {
        const float v00 = x[in_index(nhwc, b, c, h.i0, w.i0, C, Hi, Wi)], v01 = x[in_index(nhwc, b, c, h.i0, w.i1, C, Hi, Wi)];
        const float v10 = x[in_index(nhwc, b, c, h.i1, w.i0, C, Hi, Wi)], v11 = x[in_index(nhwc, b, c, h.i1, w.i1, C, Hi, Wi)];
        const float v = h.l0 * (w.l0 * v00 + w.l1 * v01) + h.l1 * (w.l0 * v10 + w.l1 * v11);
        y[(((int64_t)b * C + c) * Ho + oy) * Wo + ox] = mul * v + add;
    }
}

// the candidate output range [lo, hi] of input index i (the header's inequality, widened by one, held to [0, out - 1])
__device__ __forceinline__ void candidates(int i, int in, int out, int *lo, int *hi) {
    const int64_t a = (int64_t)(2 * i - 1) * out - in, b = (int64_t)(2 * i + 3) * out - in, d = 2 * (int64_t)in;
    const int64_t fl = a >= 0 ? a / d : -((-a + d - 1) / d);            // floor(a / d)
    const int64_t l = fl - 1, h = (b >= 0 ? b / d : -((-b + d - 1) / d)) + 1;
    *lo = (int)(l < 0 ? 0 : l);
    *hi = (int)(h > out - 1 ? out - 1 : h);
}

// the weight with which output index `dst` reads input index i -- the forward's own taps; *hit says whether it reads it at all
__device__ __forceinline__ float axis_weight(int dst, int i, int in, float scale, bool *hit) {
    const AxisTap t = axis_tap(dst, in, scale);
    float w = 0.f;
    *hit = t.i0 == i || t.i1 == i;
    if (t.i0 == i) w = t.l0;
    if (t.i1 == i) w = t.i0 == i ? w + t.l1 : t.l1;                    // the last source index is both taps of its readers
    return w;
}

template <int C>
__global__ __launch_bounds__(256) void resize_bilinear_bwd_kernel(const float *__restrict__ gy, int B, int Hi, int Wi, int Ho, int Wo,
                                                                  int nhwc, float mul, float *__restrict__ gx) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)B * Hi * Wi) return;
    const int ix = (int)(p % Wi), iy = (int)((p / Wi) % Hi), b = (int)(p / ((int64_t)Wi * Hi));
    const float sh = (float)Hi / (float)Ho, sw = (float)Wi / (float)Wo;
    int y0, y1, x0, x1;
    candidates(iy, Hi, Ho, &y0, &y1);
    candidates(ix, Wi, Wo, &x0, &x1);
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = 0.f;
    for (int oy = y0; oy <= y1; oy++) {
        bool hy;
        const float wy = axis_weight(oy, iy, Hi, sh, &hy);
        if (!hy) continue;
        for (int ox = x0; ox <= x1; ox++) {
            bool hx;
            const float wx = axis_weight(ox, ix, Wi, sw, &hx);
            if (!hx) continue;
            const float wgt = wy * wx;
#pragma unroll
            for (int c = 0; c < C; c++) acc[c] = acc[c] + wgt * gy[(((int64_t)b * C + c) * Ho + oy) * Wo + ox];
        }
    }
#pragma unroll
    for (int c = 0; c < C; c++) gx[in_index(nhwc, b, c, iy, ix, C, Hi, Wi)] = mul * acc[c];
}

// ---- area resize of the frame composited on white ---------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ float pixel_value(T v);
template <>
__device__ __forceinline__ float pixel_value<float>(float v) { return v; }
template <>
__device__ __forceinline__ float pixel_value<uint8_t>(uint8_t v) { return (float)v / 255.0f; }

template <class T>
__global__ __launch_bounds__(256) void resize_area_masked_kernel(const T *__restrict__ img, const float *__restrict__ mask, int Hi,
                                                                 int Wi, int Ho, int Wo, float *__restrict__ out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= Ho * Wo) return;
    const int ox = p % Wo, oy = p / Wo;
    // source rows [ya, yb) and columns [xa, xb) that overlap the box; Ho <= Hi and Wo <= Wi
    const int64_t top = (int64_t)oy * Hi, bot = top + Hi, left = (int64_t)ox * Wi, right = left + Wi;
    const int ya = (int)(top / Ho), yb = (int)((bot + Ho - 1) / Ho), xa = (int)(left / Wo), xb = (int)((right + Wo - 1) / Wo);
    float acc[3] = {0.f, 0.f, 0.f};
    for (int iy = ya; iy < yb && iy < Hi; iy++) {
        const int64_t oh = min(bot, (int64_t)(iy + 1) * Ho) - max(top, (int64_t)iy * Ho);
        const float wy = (float)oh / (float)Hi;
        float row[3] = {0.f, 0.f, 0.f};
        for (int ix = xa; ix < xb && ix < Wi; ix++) {
            const int64_t ow = min(right, (int64_t)(ix + 1) * Wo) - max(left, (int64_t)ix * Wo);
            const float wx = (float)ow / (float)Wi;
            const int64_t q = (int64_t)iy * Wi + ix;
            const float m = mask ? (mask[q] > 0.5f ? 1.0f : 0.0f) : 1.0f;
#pragma unroll
            for (int c = 0; c < 3; c++) row[c] = row[c] + wx * (pixel_value<T>(img[q * 3 + c]) * m + (1.0f - m));
        }
#pragma unroll
        for (int c = 0; c < 3; c++) acc[c] = acc[c] + wy * row[c];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) out[((int64_t)c * Ho + oy) * Wo + ox] = acc[c];
}

// ---- uint8 frames ------------------------------------------------------------------------------------------------------------
// (x * 255).astype(uint8) for values in [0, 1]; outside that range numpy's cast is not defined and the value is held to 0 / 255
__device__ __forceinline__ uint8_t to_u8(float v) {
    return (uint8_t)(int)fminf(fmaxf(v, 0.0f), 255.0f);             // fmaxf drops a NaN: 0
}

__global__ __launch_bounds__(256) void frame_to_u8_kernel(const float *__restrict__ x, int64_t n, uint8_t *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = to_u8(x[i] * 255.0f);
}

// the order-preserving integer image of a float (wave.h reduces it as a signed integer) and its inverse
__device__ __forceinline__ int32_t ordered(float f) {
    const int32_t b = __float_as_int(f);
    return b >= 0 ? b : b ^ 0x7fffffff;
}
__device__ __forceinline__ float unordered(int32_t o) { return __int_as_float(o >= 0 ? o : o ^ 0x7fffffff); }

#define IM_RANGE_BLOCKS 256

// min / max of a block's threads' values -> thread 0 of the block holds them
__device__ __forceinline__ void block_range(int32_t &lo, int32_t &hi) {
    __shared__ int32_t s_lo[4], s_hi[4];
    lo = wave_min(lo);
    hi = wave_max(hi);
    if ((threadIdx.x & 63) == 0) {
        s_lo[threadIdx.x >> 6] = lo;
        s_hi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    for (int w = 0; w < 4; w++) {
        lo = min(lo, s_lo[w]);
        hi = max(hi, s_hi[w]);
    }
    __syncthreads();
}

// launch 1: every block's range of its grid-stride share -> range[2 * block], range[2 * block + 1]
__global__ __launch_bounds__(256) void depth_range_kernel(const float *__restrict__ d, int64_t n, int32_t *__restrict__ range) {
    int32_t lo = 0x7fffffff, hi = (int32_t)0x80000000;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t o = ordered(d[i]);
        lo = min(lo, o);
        hi = max(hi, o);
    }
    block_range(lo, hi);
    if (threadIdx.x == 0) {
        range[2 * blockIdx.x] = lo;
        range[2 * blockIdx.x + 1] = hi;
    }
}

// launch 2: every block folds the `blocks` <= 256 ranges again (min and max are exact: every block finds the same two values),
// then quantises its share: (d - min) / (max - min + 1e-6) * 255, truncated
__global__ __launch_bounds__(256) void depth_to_u8_kernel(const float *__restrict__ d, int64_t n, const int32_t *__restrict__ range,
                                                          int blocks, uint8_t *__restrict__ out) {
    __shared__ float s_mm[2];
    int32_t lo = 0x7fffffff, hi = (int32_t)0x80000000;
    if ((int)threadIdx.x < blocks) {
        lo = range[2 * threadIdx.x];
        hi = range[2 * threadIdx.x + 1];
    }
    block_range(lo, hi);
    if (threadIdx.x == 0) {
        s_mm[0] = unordered(lo);
        s_mm[1] = unordered(hi);
    }
    __syncthreads();
    const float mn = s_mm[0], den = (s_mm[1] - mn) + 1e-6f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = to_u8((d[i] - mn) / den * 255.0f);
}

// ---- entry points ------------------------------------------------------------------------------------------------------------
static inline bool resize_args_ok(const void *a, const void *b, int32_t B, int32_t C, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo) {
    return a && b && B >= 0 && C >= 1 && C <= IM_MAX_C && Hi >= 1 && Wi >= 1 && Ho >= 1 && Wo >= 1 &&
           (int64_t)B * C * Hi * Wi <= 0x7fffffffLL && (int64_t)B * C * Ho * Wo <= 0x7fffffffLL;
}

extern "C" int mh_resize_bilinear_fwd(const float *x, int32_t B, int32_t C, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                                      int32_t nhwc, float mul, float add, float *y, void *stream) {
    if (!resize_args_ok(x, y, B, C, Hi, Wi, Ho, Wo)) return MH_ERR_ARG;
    if (B == 0) return MH_OK;
    const dim3 grid((unsigned)(((int64_t)B * Ho * Wo + 255) / 256)), block(256);
    hipStream_t s = mh_stream(stream);
    switch (C) {
    case 1: hipLaunchKernelGGL(resize_bilinear_fwd_kernel<1>, grid, block, 0, s, x, (int)B, (int)Hi, (int)Wi, (int)Ho, (int)Wo, (int)nhwc, mul, add, y); break;
    case 2: hipLaunchKernelGGL(resize_bilinear_fwd_kernel<2>, grid, block, 0, s, x, (int)B, (int)Hi, (int)Wi, (int)Ho, (int)Wo, (int)nhwc, mul, add, y); break;
    case 3: hipLaunchKernelGGL(resize_bilinear_fwd_kernel<3>, grid, block, 0, s, x, (int)B, (int)Hi, (int)Wi, (int)Ho, (int)Wo, (int)nhwc, mul, add, y); break;
    default: hipLaunchKernelGGL(resize_bilinear_fwd_kernel<4>, grid, block, 0, s, x, (int)B, (int)Hi, (int)Wi, (int)Ho, (int)Wo, (int)nhwc, mul, add, y); break;
    }
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_resize_bilinear_bwd(const float *gy, int32_t B, int32_t C, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                                      int32_t nhwc, float mul, float *gx, void *stream) {
    if (!resize_args_ok(gy, gx, B, C, Hi, Wi, Ho, Wo)) return MH_ERR_ARG;
    if (B == 0) return MH_OK;
    const dim3 grid((unsigned)(((int64_t)B * Hi * Wi + 255) / 256)), block(256);
    hipStream_t s = mh_stream(stream);
    switch (C) {
    case 1: hipLaunchKernelGGL(resize_bilinear_bwd_kernel<1>, grid, block, 0, s, gy, (int)B, (int)Hi, (int)Wi, (int)Ho, (int)Wo, (int)nhwc, mul, gx); break;
    case 2: hipLaunchKernelGGL(resize_bilinear_bwd_kernel<2>, grid, block, 0, s, gy, (int)B, (int)Hi, (int)Wi, (int)Ho, (int)Wo, (int)nhwc, mul, gx); break;
    case 3: hipLaunchKernelGGL(resize_bilinear_bwd_kernel<3>, grid, block, 0, s, gy, (int)B, (int)Hi, (int)Wi, (int)Ho, (int)Wo, (int)nhwc, mul, gx); break;
    default: hipLaunchKernelGGL(resize_bilinear_bwd_kernel<4>, grid, block, 0, s, gy, (int)B, (int)Hi, (int)Wi, (int)Ho, (int)Wo, (int)nhwc, mul, gx); break;
    }
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_resize_area_masked(const void *image, int32_t image_u8, const float *mask, int32_t Hi, int32_t Wi, int32_t Ho,
                                     int32_t Wo, float *out, void *stream) {
    if (!image || !out || Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1 || (int64_t)Hi * Wi > 0x1fffffffLL) return MH_ERR_ARG;
    if (Ho > Hi || Wo > Wi) return MH_ERR_ARG;                        // an enlarging axis is not served
    const dim3 grid((unsigned)((Ho * Wo + 255) / 256)), block(256);
    if (image_u8)
        hipLaunchKernelGGL(resize_area_masked_kernel<uint8_t>, grid, block, 0, mh_stream(stream), (const uint8_t *)image, mask,
                           (int)Hi, (int)Wi, (int)Ho, (int)Wo, out);
    else
        hipLaunchKernelGGL(resize_area_masked_kernel<float>, grid, block, 0, mh_stream(stream), (const float *)image, mask, (int)Hi,
                           (int)Wi, (int)Ho, (int)Wo, out);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

static inline unsigned stride_blocks(int64_t n) {
    const int64_t b = (n + 255) / 256;
    return (unsigned)(b > IM_RANGE_BLOCKS ? IM_RANGE_BLOCKS : b);
}

extern "C" int mh_frame_to_u8(const float *x, int64_t n, uint8_t *out, void *stream) {
    if (n == 0) return MH_OK;
    if (!x || !out || n < 0) return MH_ERR_ARG;
    hipLaunchKernelGGL(frame_to_u8_kernel, dim3(stride_blocks(n)), dim3(256), 0, mh_stream(stream), x, n, out);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int32_t mh_depth_range_words(void) { return 2 * IM_RANGE_BLOCKS; }

extern "C" int mh_depth_to_u8(const float *depth, int64_t n, int32_t *range, uint8_t *out, void *stream) {
    if (n == 0) return MH_OK;
    if (!depth || !out || !range || n < 0) return MH_ERR_ARG;
    const unsigned blocks = stride_blocks(n);
    hipLaunchKernelGGL(depth_range_kernel, dim3(blocks), dim3(256), 0, mh_stream(stream), depth, n, range);
    MH_CHECK_LAUNCH();
    hipLaunchKernelGGL(depth_to_u8_kernel, dim3(blocks), dim3(256), 0, mh_stream(stream), depth, n, (const int32_t *)range,
                       (int)blocks, out);
    MH_CHECK_LAUNCH();
    return MH_OK;
}
