// Preprocessing of a raw RGB-D sequence: rotate every frame about its projected world centre, cut a window, mark the padding.
//
// Stands where the reference's preprocess/preprocess.py:DataProcessor.rotate_and_crop_frames and the four imwrite lines of
// DataProcessor.preprocess stand (morpheus_amd/preprocess.py is the Python face; it forms the cameras, the window origins, the
// inverse affine maps and the depth tables on the host).  One launch does all frames of a sequence and writes them in
// DeviceDataset's storage layout: rgb uint8 [F,h,w,3], depth uint16 [F,h,w], mask uint8 [F,h,w], plus padding uint8 [F,h,w].
//
// The window.  Output pixel (y, x) of frame f looks at canvas pixel (Y, X) = (top_f + y, left_f + x), formed in 64 bits.  Outside
// [0,H) x [0,W) rgb, depth and mask are 0 and padding is 255; inside padding is 0.  That is the rule for EVERY position of the
// window.  The reference's crop_image_2d / crop_image_3d raise a numpy shape error for a window that crosses two different sides
// of the frame, one that lies wholly outside it and one larger than the frame; for every window they can run they compute this
// rule, and this build defines the other three kinds by it.
//
// Depth.  The reference rewrites the depth: raw / depth_scale rounded to fp32, times the frame's scale in fp32, and on writing
// `(d * 1000).astype(uint16)` -- where the product is fp32 for a window that passes its inside test (the crop is a slice of the
// fp32 array) and float64 for every other window (the crop is np.zeros((h, w))).  Both are functions of the raw 16 bits alone, so
// the host tabulates them with the reference's own expressions and the kernel looks up table_inside[raw] when the frame's window
// satisfies top >= 0 && left >= 0 && top + h < H && left + w < W (strict: a window that touches the bottom or right edge is not
// inside) and table_padded[raw] otherwise.
//
// Unrotated frames (rotated[f] == 0; rot_degree = 0 in every shipped config): rgb and mask bytes are copied (x / 255.0 * 255.
// truncated gives x back for all 256 bytes).
//
// Rotated frames.  The reference warps with cv2.warpAffine (INTER_LINEAR for rgb, INTER_NEAREST for depth and mask, constant
// border 0).  cv2 is not available where this project is built or run and its fixed-point coordinate arithmetic is not restated:
// the definition below is this build's own, AGREEMENT WITH cv2 UNVERIFIED.  With inv = (a0 .. a5) the inverse affine map of the
// frame (float64, formed on the host; no sine or cosine runs here), canvas pixel (X, Y) samples the source at
//     u = (a0 X + a1 Y) + a2        v = (a3 X + a4 Y) + a5                                 in float64, no contraction
//   nearest (depth, mask): column floor(u + 0.5), row floor(v + 0.5); outside the image: 0 (raw depth 0 -> table[0])
//   bilinear (rgb): fu = floor(u), fv = floor(v), ax = u - fu, ay = v - fv; the taps p00 = (fv, fu), p01 = (fv, fu + 1),
//     p10 = (fv + 1, fu), p11 = (fv + 1, fu + 1) are byte / 255.0 in float64, 0 outside the image;
//     val = ((p00 ((1 - ax)(1 - ay)) + p01 (ax (1 - ay))) + p10 ((1 - ax) ay)) + p11 (ax ay);   byte = (uint8)(val * 255.0), a truncation.
// tests/preprocess_oracle.py states the same order in numpy float64; the kernel equals it bit for bit.
//
// Shape.  A memory-bound gather: about 6 bytes read and 7 written per pixel.  A lane owns PREP_PX = 4 consecutive pixels of the
// FLAT output [F h w], so that every lane stores whole dwords whatever h and w are: 3 dwords of rgb, 2 of depth, 1 of mask and 1
// of padding, each wave instruction writing 256 contiguous bytes per plane.
//   * The common lane -- unrotated frame, its four pixels in one output row and all four on the canvas -- reads its 12 rgb bytes,
//     4 depth values and 4 mask bytes with three wide loads at the window's own alignment (left is arbitrary, so source dwords do
//     not line up with output dwords; gfx950 takes unaligned global loads and the compiler emits dwordx3 / dwordx2 / dword for
//     them) and copies the rgb and mask dwords through.
//   * Every other lane (a group that straddles a row or a frame, touches the canvas's edge, or belongs to a rotated frame) goes
//     pixel by pixel; the frame's parameters are re-read when the frame changes.
//   * byte / 255.0 of the bilinear taps is a 256-entry float64 table in LDS, filled with that very division by the blocks whose
//     pixel range meets a rotated frame (a block-uniform test): twelve float64 divisions per pixel become twelve LDS reads.
#include "common.h"

// the float64 chains are pinned bit for bit (tests/preprocess_oracle.py): no FMA contraction
#pragma clang fp contract(off)

#define PREP_PX 4
#define PREP_BLOCK 256

struct PrepFrame {
    int64_t top, left;
    const uint16_t *table;
    bool rotated;
};

__device__ __forceinline__ PrepFrame prep_frame(uint32_t f, const int32_t *__restrict__ origin, const uint8_t *__restrict__ rotated,
                                                const uint16_t *__restrict__ table_inside,
                                                const uint16_t *__restrict__ table_padded, int H, int W, int h, int w) {
    PrepFrame fr;
    fr.top = (int64_t)origin[(int64_t)f * 2 + 0];
    fr.left = (int64_t)origin[(int64_t)f * 2 + 1];
    const bool inside = fr.top >= 0 && fr.left >= 0 && fr.top + h < (int64_t)H && fr.left + w < (int64_t)W;
    fr.table = inside ? table_inside : table_padded;
    fr.rotated = rotated[f] != 0;
    return fr;
}

// canvas pixel (X, Y), on the canvas, of the ROTATED frame at `base` (pixels) -> rgb bytes c[0..2], raw depth, mask byte
__device__ __forceinline__ void prep_rotated_pixel(const uint8_t *__restrict__ rgb, const uint16_t *__restrict__ depth,
                                                   const uint8_t *__restrict__ mask, int64_t base, int H, int W,
                                                   const double *__restrict__ a, const double *unit, int64_t X, int64_t Y,
                                                   uint32_t *c, uint32_t &raw, uint32_t &m) {
    const double Xd = (double)X, Yd = (double)Y;
    const double u = (a[0] * Xd + a[1] * Yd) + a[2];
    const double v = (a[3] * Xd + a[4] * Yd) + a[5];
    // nearest: depth and mask (a NaN fails every comparison: outside)
    const double un = floor(u + 0.5), vn = floor(v + 0.5);
    if (un >= 0.0 && un < (double)W && vn >= 0.0 && vn < (double)H) {
        const int64_t src = base + (int64_t)vn * W + (int64_t)un;
        raw = depth[src];
        m = mask[src];
    }
    // bilinear: rgb.  All four taps are outside unless -1 < u < W and -1 < v < H
    if (u > -1.0 && u < (double)W && v > -1.0 && v < (double)H) {
        const double fu = floor(u), fv = floor(v);
        const double ax = u - fu, ay = v - fv;
        const int iu = (int)fu, iv = (int)fv;      // in [-1, W - 1] and [-1, H - 1]
        const bool x0 = iu >= 0, x1 = iu + 1 < W, y0 = iv >= 0, y1 = iv + 1 < H;
        const double w00 = (1.0 - ax) * (1.0 - ay), w01 = ax * (1.0 - ay), w10 = (1.0 - ax) * ay, w11 = ax * ay;
        const int64_t s00 = base + (int64_t)iv * W + iu;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const double p00 = (y0 && x0) ? unit[rgb[s00 * 3 + ch]] : 0.0;
            const double p01 = (y0 && x1) ? unit[rgb[(s00 + 1) * 3 + ch]] : 0.0;
            const double p10 = (y1 && x0) ? unit[rgb[(s00 + W) * 3 + ch]] : 0.0;
            const double p11 = (y1 && x1) ? unit[rgb[(s00 + W + 1) * 3 + ch]] : 0.0;
            const double val = ((p00 * w00 + p01 * w01) + p10 * w10) + p11 * w11;
            c[ch] = (uint32_t)(int)(val * 255.0) & 255u;
        }
    }
}

__global__ __launch_bounds__(PREP_BLOCK) void prep_frames_kernel(
    const uint8_t *__restrict__ rgb, const uint16_t *__restrict__ depth, const uint8_t *__restrict__ mask, int H, int W,
    const int32_t *__restrict__ origin, const double *__restrict__ inv, const uint8_t *__restrict__ rotated,
    const uint16_t *__restrict__ table_inside, const uint16_t *__restrict__ table_padded, int h, int w, uint32_t total,
    uint8_t *__restrict__ rgb_out, uint16_t *__restrict__ depth_out, uint8_t *__restrict__ mask_out,
    uint8_t *__restrict__ padding_out) {
    __shared__ double unit[256];      // byte / 255.0
    const uint32_t hw = (uint32_t)h * (uint32_t)w;
    {   // the frames this block's pixels belong to: does any of them rotate?  (the same answer in every thread of the block)
        const uint32_t first = blockIdx.x * (uint32_t)(PREP_BLOCK * PREP_PX);      // < total: the grid is sized from it
        const uint32_t last = total - first > (uint32_t)(PREP_BLOCK * PREP_PX) ? first + (uint32_t)(PREP_BLOCK * PREP_PX) - 1u : total - 1u;
        bool any = false;
        for (uint32_t f = first / hw; f <= last / hw; f++) any = any || rotated[f] != 0;
        if (any) {
            unit[threadIdx.x] = (double)threadIdx.x / 255.0;
            __syncthreads();
        }
    }
    const uint32_t g = blockIdx.x * (uint32_t)PREP_BLOCK + threadIdx.x;
    if ((uint64_t)g * PREP_PX >= (uint64_t)total) return;
    const uint32_t p0 = g * PREP_PX;
    uint32_t f = p0 / hw;
    const uint32_t rem = p0 - f * hw;
    uint32_t y = rem / (uint32_t)w;
    uint32_t x = rem - y * (uint32_t)w;
    const int n = total - p0 < (uint32_t)PREP_PX ? (int)(total - p0) : PREP_PX;
    const int64_t HW = (int64_t)H * W;

    PrepFrame fr = prep_frame(f, origin, rotated, table_inside, table_padded, H, W, h, w);
    {   // the common lane: four pixels of one output row, all on the canvas of an unrotated frame
        const int64_t Y = fr.top + (int64_t)y, X = fr.left + (int64_t)x;
        if (n == PREP_PX && !fr.rotated && x + (uint32_t)(PREP_PX - 1) < (uint32_t)w && Y >= 0 && Y < (int64_t)H && X >= 0 &&
            X + (PREP_PX - 1) < (int64_t)W) {
            const int64_t src = (int64_t)f * HW + Y * W + X;      // src .. src + 3 are pixels of row Y
            uint32_t c3[3], m4;
            uint16_t d4[PREP_PX];
            __builtin_memcpy(c3, rgb + src * 3, 12);
            __builtin_memcpy(d4, depth + src, 8);
            __builtin_memcpy(&m4, mask + src, 4);
            uint32_t *ro = reinterpret_cast<uint32_t *>(rgb_out) + (int64_t)g * 3;
            ro[0] = c3[0];
            ro[1] = c3[1];
            ro[2] = c3[2];
            uint2 dd;
            dd.x = (uint32_t)fr.table[d4[0]] | ((uint32_t)fr.table[d4[1]] << 16);
            dd.y = (uint32_t)fr.table[d4[2]] | ((uint32_t)fr.table[d4[3]] << 16);
            reinterpret_cast<uint2 *>(depth_out)[g] = dd;
            reinterpret_cast<uint32_t *>(mask_out)[g] = m4;
            reinterpret_cast<uint32_t *>(padding_out)[g] = 0u;
            return;
        }
    }

    // every other lane: pixel by pixel, packed as it goes (pixel k's rgb at bit 24 k of 96, depth at 16 k of 64, mask and
    // padding at 8 k of 32).  The loop stays rolled: one copy of the rotated chain, not four, keeps the register count down.
    unsigned __int128 c96 = 0;
    uint64_t d64 = 0;
    uint32_t m32 = 0u, pad32 = 0u;
#pragma unroll 1
    for (int k = 0; k < n; k++) {
        const int64_t Y = fr.top + (int64_t)y, X = fr.left + (int64_t)x;
        uint32_t c[3] = {0u, 0u, 0u}, d = 0u, m = 0u;
        if (Y < 0 || Y >= (int64_t)H || X < 0 || X >= (int64_t)W) {
            pad32 |= 255u << (8 * k);
        } else if (!fr.rotated) {
            const int64_t src = (int64_t)f * HW + Y * W + X;
            c[0] = rgb[src * 3];
            c[1] = rgb[src * 3 + 1];
            c[2] = rgb[src * 3 + 2];
            d = fr.table[depth[src]];
            m = mask[src];
        } else {
            uint32_t raw = 0u;
            prep_rotated_pixel(rgb, depth, mask, (int64_t)f * HW, H, W, inv + (int64_t)f * 6, unit, X, Y, c, raw, m);
            d = fr.table[raw];
        }
        c96 |= (unsigned __int128)(c[0] | (c[1] << 8) | (c[2] << 16)) << (24 * k);
        d64 |= (uint64_t)d << (16 * k);
        m32 |= m << (8 * k);
        // the next pixel of the flat output
        if (++x == (uint32_t)w) {
            x = 0u;
            if (++y == (uint32_t)h) {
                y = 0u;
                ++f;
                if (k + 1 < n) fr = prep_frame(f, origin, rotated, table_inside, table_padded, H, W, h, w);
            }
        }
    }

    if (n == PREP_PX) {      // whole dwords; the entry point checked the bases' alignment
        uint32_t *ro = reinterpret_cast<uint32_t *>(rgb_out) + (int64_t)g * 3;
        ro[0] = (uint32_t)c96;
        ro[1] = (uint32_t)(c96 >> 32);
        ro[2] = (uint32_t)(c96 >> 64);
        uint2 dd;
        dd.x = (uint32_t)d64;
        dd.y = (uint32_t)(d64 >> 32);
        reinterpret_cast<uint2 *>(depth_out)[g] = dd;
        reinterpret_cast<uint32_t *>(mask_out)[g] = m32;
        reinterpret_cast<uint32_t *>(padding_out)[g] = pad32;
    } else {                 // the last lane when F h w is no multiple of PREP_PX: element stores, nothing past the end
        for (int k = 0; k < n; k++) {
            const int64_t p = (int64_t)p0 + k;
            const uint32_t c24 = (uint32_t)(c96 >> (24 * k));
            rgb_out[p * 3] = (uint8_t)c24;
            rgb_out[p * 3 + 1] = (uint8_t)(c24 >> 8);
            rgb_out[p * 3 + 2] = (uint8_t)(c24 >> 16);
            depth_out[p] = (uint16_t)(d64 >> (16 * k));
            mask_out[p] = (uint8_t)(m32 >> (8 * k));
            padding_out[p] = (uint8_t)(pad32 >> (8 * k));
        }
    }
}

extern "C" int mh_prep_frames(const uint8_t *rgb, const uint16_t *depth, const uint8_t *mask, int32_t F, int32_t H, int32_t W,
                              const int32_t *origin, const double *inv_affine, const uint8_t *rotated,
                              const uint16_t *table_inside, const uint16_t *table_padded, int32_t h, int32_t w, uint8_t *rgb_out,
                              uint16_t *depth_out, uint8_t *mask_out, uint8_t *padding_out, void *stream) {
    if (F == 0) return MH_OK;
    if (!rgb || !depth || !mask || !origin || !inv_affine || !rotated || !table_inside || !table_padded || !rgb_out ||
        !depth_out || !mask_out || !padding_out || F < 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0)
        return MH_ERR_ARG;
    if ((int64_t)H * W > 0x7fffffffLL || (int64_t)h * w > 0x7fffffffLL || (int64_t)F * h * w > 0x7fffffffLL) return MH_ERR_ARG;
    if (((uintptr_t)rgb_out & 3) || ((uintptr_t)depth_out & 7) || ((uintptr_t)mask_out & 3) || ((uintptr_t)padding_out & 3) ||
        ((uintptr_t)inv_affine & 7) || ((uintptr_t)origin & 3) || ((uintptr_t)depth & 1) || ((uintptr_t)table_inside & 1) ||
        ((uintptr_t)table_padded & 1))
        return MH_ERR_ARG;
    const int64_t total = (int64_t)F * h * w;
    const int64_t per_block = (int64_t)PREP_BLOCK * PREP_PX;
    hipLaunchKernelGGL(prep_frames_kernel, dim3((unsigned)((total + per_block - 1) / per_block)), dim3(PREP_BLOCK), 0,
                       mh_stream(stream), rgb, depth, mask, (int)H, (int)W, origin, inv_affine, rotated, table_inside,
                       table_padded, (int)h, (int)w, (uint32_t)total, rgb_out, depth_out, mask_out, padding_out);
    MH_CHECK_LAUNCH();
    return MH_OK;
}
