// Baseline sequential-DCT JPEG (ITU-T T.81, 8-bit samples, Huffman coding) for a batch of F frames of equal size, on the device.
// morpheus_amd/video.py is the Python face (it writes the markers around the entropy-coded segment produced here, and the
// Motion-JPEG AVI container); tests/video_oracle.py restates this file's definition sequentially, and the two agree byte for byte.
//
// DEFINITION.  Everything below is integer arithmetic; `>>` is the arithmetic shift (floor), `/` divides non-negative integers.
//   input     uint8 [F,H,W,3] (RGB) or [F,H,W] (one component), 1 <= H, W <= 65535.
//   colour    component = (cr R + cg G + cb B + offset) >> 16 with the rows of JPEG_YCC (JFIF's matrix times 2^16, rounded so
//             that the rows add up to 65536, 0, 0; offset = 2^15 for Y, 128 * 2^16 + 2^15 - 1 for Cb and Cr).  Results lie in
//             [0, 255] for every input (Cb, Cr: at most (32768 * 255 + 128 * 65536 + 32767) >> 16 = 255).
//   padding   the image is extended to a multiple of the MCU (8 x 8; 16 x 16 in 4:2:0) by edge replication: pixel (y, x) of the
//             padded image is pixel (min(y, H - 1), min(x, W - 1)).
//   4:2:0     a chroma sample is (c00 + c01 + c10 + c11 + 2) >> 2 of the four chroma values of its 2 x 2 padded pixels.
//   shift     s = sample - 128, in [-128, 127].
//   DCT       separable, with the integer table C[u][x] = round(2^14 c(u) / 2 cos((2 x + 1) u pi / 16)) of jpeg_tables.inc
//             (evaluated in float64 by tools/gen_jpeg_tables.py):
//               row pass      t[y][u] = (sum_x C[u][x] s[y][x] + 2^8) >> 9             5 fraction bits are kept
//               column pass   F[v][u] = sum_y C[v][y] t[y][u]                           no shift: 2^19 times the DCT
//             The sums are evaluated as sums and differences of the mirrored inputs (C[u][7 - x] = (-1)^u C[u][x] holds exactly
//             in the table), which is the same integer.
//   quantise  D = Q[v][u] * 2^19;  q = sign(F) * ((|F| + D / 2) / D): round half away from zero on the magnitude.  Q: the Annex K
//             table scaled by the IJG rule (mh_jpeg_quant_table).
//   ranges    |sum_x C s| <= 8 * 8035 * 128 < 2^23;  |t| <= 2^14;  |F| <= 8 * 8035 * 2^14 < 2^30.1;  |F| + D / 2 < 2^30.1 + 2^26:
//             nothing leaves int32.
//   error     against the float64 DCT c of the same block: a table entry is off by at most 1/2 of 2^-14, so the row sum is off by
//             8 * 128 / 2 * 2^-14 = 2^-5 and its rounding by 2^-6 (e1 = 0.047); in the column pass the table error costs at most
//             8 * 2^-15 * 363 = 0.089 and the rows' error sum_y |c(v) / 2 cos| e1 <= 2.83 * 0.047 = 0.133:  |F 2^-19 - c| <= 0.25,
//             hence |q Q - c| <= Q / 2 + 0.25 (tests/test_video_host.py).
//   scan      one interleaved scan; MCUs row by row, inside an MCU Y00 Y01 Y10 Y11 Cb Cr (4:2:0), Y Cb Cr (4:4:4) or the single
//             block.  DC: the difference against the previous block of the same component in that order (0 at a frame's first),
//             held to +-2047; AC: run / size symbols in zigzag order, values held to +-1023 (neither bound is reached: |c| < 1025
//             + 0.25), ZRL for every 16 zeros in front of a non-zero coefficient, EOB unless coefficient 63 is non-zero.  The four
//             Huffman tables are Annex K.3 - K.6.  A value of category n is written as n bits, v for v >= 0, v + 2^n - 1 below.
//             Bits are written most significant first; the last byte is filled with 1-bits; in the output every byte 0xFF is
//             followed by 0x00.
//
// LAUNCHES of mh_jpeg_encode, all on the caller's stream, nothing read by the host in between:
//   0  zero the word buffer and the overflow flag
//   1  transform   one lane per block in scan order: pixels -> quantised coefficients, int16 [F][blocks][64] in zigzag order
//   2  count       one lane per block: its exact bit count (the same walk as the packer's, with a counting sink), scanned
//                  inside the workgroup of 256 blocks (block_excl_scan, wave.h); one partial per workgroup
//   3  partials    one workgroup per frame scans the partials and leaves the frame's total
//   4  pack        one lane per block writes its codes at its bit offset into the zeroed big-endian word buffer.  The first and
//                  the last word a block touches may be shared with its neighbours and are combined with a vector atomic OR of
//                  disjoint bits; the words between belong to the block alone and are stored.  No result depends on the order of
//                  arrival.  The frame's last block also writes the 1-padding.
//   5  0xFF count  one lane per 16 bytes of the packed segment, scanned as in 2
//   6  partials    as 3
//   7  stuff       one lane per 16 bytes writes them and the 0x00 behind every 0xFF at its final place; nbytes[f] is written
//
// MEMORY SAFETY.  A block is at most 20 + 63 * 26 = 1658 bits (a 9-bit DC code + 11 bits; 63 times a 16-bit code + 10 bits), so a
// frame's packed segment is at most mh_jpeg_scan_capacity / 2 bytes and stuffing at most doubles it.  Independently of that proof,
// every word index in 4 and every byte index in 7 is compared with the capacity the caller passed; what lies beyond is dropped
// and *overflow is set.  Pixel loads are held inside the frame batch (load_run), table indices inside their tables (the +-2047
// and +-1023 bounds above), block indices inside [0, blocks).
//
// One lane holds a whole block in registers (every index into the 8 x 8 arrays is a constant after unrolling), so there is no
// per-lane tile in LDS and no bank conflict to pad away; LDS holds only the four wave totals of a workgroup scan.  A lane reads its
// 8 (or, for sub-sampled chroma, 16) pixels of a row as one run of dwords -- 4-byte aligned whatever W is, which is all that
// global dwordx4 / dwordx3 loads need -- and shifts the run into place; single-byte loads serve only the replicated edge.
#include "common.h"
#include "wave.h"

#include "jpeg_tables.inc"

#define JPEG_MAX_BLOCKS (0x7fffffffLL / JPEG_MAX_BLOCK_BITS)        // a frame's bit count fits int32
#define JPEG_GRAY 0
#define JPEG_444 1
#define JPEG_420 2

struct JpegGeom {
    int H, W, C, mode;       // C: bytes per pixel (1 or 3); mode: JPEG_GRAY / JPEG_444 / JPEG_420
    int mcux, mcuy, nb;      // MCUs per row and column, blocks per frame
};
struct JpegQuant {
    uint16_t q[2][64];       // natural order; [0] luminance, [1] chrominance
};

static inline int64_t jpeg_blocks(int64_t H, int64_t W, int C, int sub, JpegGeom *g) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || (C != 1 && C != 3) || (C == 3 && sub != 420 && sub != 444)) return -1;
    const int mode = C == 1 ? JPEG_GRAY : (sub == 420 ? JPEG_420 : JPEG_444);
    const int m = mode == JPEG_420 ? 16 : 8;
    const int64_t mcux = (W + m - 1) / m, mcuy = (H + m - 1) / m;
    const int64_t nb = mcux * mcuy * (mode == JPEG_GRAY ? 1 : (mode == JPEG_444 ? 3 : 6));
    if (nb > JPEG_MAX_BLOCKS) return -1;
    if (g) *g = JpegGeom{(int)H, (int)W, C, mode, (int)mcux, (int)mcuy, (int)nb};
    return nb;
}

// block b of the scan order -> its component and its place in that component's block grid
__device__ __forceinline__ void jpeg_place(const JpegGeom &g, int b, int *comp, int *by, int *bx) {
    if (g.mode == JPEG_GRAY) {
        *comp = 0, *by = b / g.mcux, *bx = b % g.mcux;
    } else if (g.mode == JPEG_444) {
        const int m = b / 3;
        *comp = b % 3, *by = m / g.mcux, *bx = m % g.mcux;
    } else {
        const int m = b / 6, j = b % 6, my = m / g.mcux, mx = m % g.mcux;
        if (j < 4) *comp = 0, *by = 2 * my + (j >> 1), *bx = 2 * mx + (j & 1);
        else *comp = j - 3, *by = my, *bx = mx;
    }
}
// the previous block of the same component in scan order; negative at a frame's first
__device__ __forceinline__ int jpeg_prev(const JpegGeom &g, int b) {
    if (g.mode == JPEG_GRAY) return b - 1;
    if (g.mode == JPEG_444) return b - 3;
    const int j = b % 6;
    return j >= 4 ? b - 6 : (j == 0 ? b - 3 : b - 1);
}

// ND dwords of the byte run that starts at byte `o` of the batch, through 4-byte aligned loads of ND + 1 dwords: false, and
// nothing read, unless all of them lie inside the batch's whole dwords
template <int ND>
__device__ __forceinline__ bool load_run(const uint32_t *__restrict__ base, int64_t whole_words, int64_t o, uint32_t (&w)[ND]) {
    const int64_t d0 = o >> 2;
    if (d0 + ND + 1 > whole_words) return false;
    uint32_t t[ND + 1];
#pragma unroll
    for (int i = 0; i <= ND; ++i) t[i] = base[d0 + i];
    const int sh = (int)(o & 3) * 8;
#pragma unroll
    for (int i = 0; i < ND; ++i) w[i] = (uint32_t)(((((uint64_t)t[i + 1]) << 32) | t[i]) >> sh);
    return true;
}
__device__ __forceinline__ int run_byte(const uint32_t *w, int j) { return (w[j >> 2] >> (8 * (j & 3))) & 0xff; }

// N values of one component (k: the row of JPEG_YCC, per lane) of the pixels (y, x0 .. x0 + N - 1) of frame f's padded image
template <int N>
__device__ __forceinline__ void fetch_row(const uint8_t *__restrict__ px, int64_t total_bytes, const JpegGeom &g, int f, int y,
                                          int x0, int kr, int kg, int kb, int koff, int (&val)[N]) {
    y = min(y, g.H - 1);
    const int64_t row = ((int64_t)f * g.H + y) * g.W;
    const uint32_t *base = reinterpret_cast<const uint32_t *>(px);
    if (g.C == 1) {
        uint32_t w[N / 4];
        if (x0 + N <= g.W && load_run<N / 4>(base, total_bytes >> 2, row + x0, w)) {
#pragma unroll
            for (int i = 0; i < N; ++i) val[i] = run_byte(w, i);
        } else {
#pragma unroll
            for (int i = 0; i < N; ++i) val[i] = px[row + min(x0 + i, g.W - 1)];
        }
    } else {
        uint32_t w[3 * N / 4];
        if (x0 + N <= g.W && load_run<3 * N / 4>(base, total_bytes >> 2, (row + x0) * 3, w)) {
#pragma unroll
            for (int i = 0; i < N; ++i)
                val[i] = (kr * run_byte(w, 3 * i) + kg * run_byte(w, 3 * i + 1) + kb * run_byte(w, 3 * i + 2) + koff) >> 16;
        } else {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const uint8_t *p = px + (row + min(x0 + i, g.W - 1)) * 3;
                val[i] = (kr * p[0] + kg * p[1] + kb * p[2] + koff) >> 16;
            }
        }
    }
}

// o[u] = sum_x C[u][x] s[x], through the mirrored sums and differences
__device__ __forceinline__ void dct8(const int (&s)[8], int (&o)[8]) {
    int a[4], d[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = s[i] + s[7 - i], d[i] = s[i] - s[7 - i];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        int acc = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc += JPEG_COS[u][i] * ((u & 1) ? d[i] : a[i]);
        o[u] = acc;
    }
}

__global__ __launch_bounds__(256) void jpeg_transform_kernel(const uint8_t *__restrict__ px, int64_t total_bytes, JpegGeom g,
                                                             JpegQuant quant, uint32_t *__restrict__ coef) {
    const int b = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (b >= g.nb) return;
    int comp, by, bx;
    jpeg_place(g, b, &comp, &by, &bx);
    // the colour row as per-lane values: lanes of different components run the same instructions
    int kr = 0, kg = 0, kb = 0, koff = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (comp == k) kr = JPEG_YCC[k][0], kg = JPEG_YCC[k][1], kb = JPEG_YCC[k][2], koff = JPEG_YCC[k][3];
    const bool wide = g.mode == JPEG_420 && comp > 0;        // a chroma block of 4:2:0 covers 16 x 16 pixels
    int t[8][8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        int s[8];
        if (wide) {
            int c0[16], c1[16];
            fetch_row<16>(px, total_bytes, g, f, 2 * (by * 8 + r), bx * 16, kr, kg, kb, koff, c0);
            fetch_row<16>(px, total_bytes, g, f, 2 * (by * 8 + r) + 1, bx * 16, kr, kg, kb, koff, c1);
#pragma unroll
            for (int i = 0; i < 8; ++i) s[i] = (c0[2 * i] + c0[2 * i + 1] + c1[2 * i] + c1[2 * i + 1] + 2) >> 2;
        } else {
            fetch_row<8>(px, total_bytes, g, f, by * 8 + r, bx * 8, kr, kg, kb, koff, s);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] -= 128;
        int o[8];
        dct8(s, o);
#pragma unroll
        for (int u = 0; u < 8; ++u) t[r][u] = (o[u] + (1 << (JPEG_ROW_SHIFT - 1))) >> JPEG_ROW_SHIFT;
    }
    const int tab = comp > 0;
    uint32_t out[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) out[i] = 0u;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        int col[8], F[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) col[y] = t[y][u];
        dct8(col, F);
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const uint32_t Q = tab ? quant.q[1][v * 8 + u] : quant.q[0][v * 8 + u];
            const uint32_t D = Q << JPEG_OUT_BITS;
            const uint32_t mag = ((uint32_t)abs(F[v]) + (D >> 1)) / D;
            const int q = F[v] < 0 ? -(int)mag : (int)mag;
            const int k = JPEG_UNZIGZAG[v * 8 + u];
            out[k >> 1] |= ((uint32_t)q & 0xffffu) << (16 * (k & 1));
        }
    }
    uint4 *dst = reinterpret_cast<uint4 *>(coef + ((int64_t)f * g.nb + b) * 32);
#pragma unroll
    for (int i = 0; i < 8; ++i) dst[i] = make_uint4(out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]);
}

// ---- the entropy coder: one walk over a block's symbols, with a sink that counts or a sink that writes ---------------------
struct CountSink {
    int bits = 0;
    __device__ __forceinline__ void put(uint32_t, int len) { bits += len; }
};
// Bit p of a frame's segment is bit 31 - (p & 31) of word p >> 5.  acc holds the nacc < 32 bits not yet written, in its low end.
struct PackSink {
    uint32_t *words;
    int wcap, widx, nacc;
    bool shared;             // the next word written may hold bits of the block in front
    uint64_t acc;
    int32_t *overflow;
    __device__ __forceinline__ void word(uint32_t w, bool atomic) {
        if (widx < wcap) {
            if (atomic) atomicOr(&words[widx], w);
            else words[widx] = w;
        } else {
            *overflow = 1;
        }
        ++widx;
    }
    __device__ __forceinline__ void put(uint32_t v, int len) {       // len <= 27
        acc = (acc << len) | v;
        nacc += len;
        if (nacc >= 32) {
            nacc -= 32;
            word((uint32_t)(acc >> nacc), shared);
            shared = false;
            acc &= (1ull << nacc) - 1ull;
        }
    }
    __device__ __forceinline__ void finish() {                       // the last, partial word is shared with the block behind
        if (nacc > 0) word((uint32_t)(acc << (32 - nacc)), true);
    }
};

__device__ __forceinline__ int coef_at(const uint32_t (&c)[32], int k) { return (int)(int16_t)(c[k >> 1] >> (16 * (k & 1))); }

__device__ __forceinline__ void value_code(int v, int *cat, uint32_t *bits) {
    const int n = 32 - __clz(abs(v));                                // 0 for v == 0
    *cat = n;
    *bits = (uint32_t)(v < 0 ? v + (1 << n) - 1 : v);
}

template <class Sink>
__device__ __forceinline__ void jpeg_walk(const uint32_t (&c)[32], int pred, int tab, Sink &s) {
    int cat;
    uint32_t bits;
    value_code(max(-2047, min(2047, coef_at(c, 0) - pred)), &cat, &bits);
    const uint32_t dc = JPEG_DC_CODE[tab][cat];
    s.put(((dc & 0xffffu) << cat) | bits, (int)(dc >> 16) + cat);
    const uint32_t zrl = JPEG_AC_CODE[tab][0xf0], eob = JPEG_AC_CODE[tab][0x00];
    int run = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const int v = max(-1023, min(1023, coef_at(c, k)));
        if (v == 0) {
            ++run;
            continue;
        }
        for (; run > 15; run -= 16) s.put(zrl & 0xffffu, (int)(zrl >> 16));
        value_code(v, &cat, &bits);
        const uint32_t ac = JPEG_AC_CODE[tab][(run << 4) | cat];
        s.put(((ac & 0xffffu) << cat) | bits, (int)(ac >> 16) + cat);
        run = 0;
    }
    if (run) s.put(eob & 0xffffu, (int)(eob >> 16));
}

// the block's coefficients, its predictor and its table; false past the frame's end
__device__ __forceinline__ bool jpeg_block(const uint32_t *__restrict__ coef, const JpegGeom &g, int f, int b, uint32_t (&c)[32],
                                           int *pred, int *tab) {
    if (b >= g.nb) return false;
    const uint32_t *frame = coef + (int64_t)f * g.nb * 32;
    const uint4 *src = reinterpret_cast<const uint4 *>(frame + (int64_t)b * 32);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 q = src[i];
        c[4 * i] = q.x, c[4 * i + 1] = q.y, c[4 * i + 2] = q.z, c[4 * i + 3] = q.w;
    }
    const int p = jpeg_prev(g, b);
    *pred = p < 0 ? 0 : (int)(int16_t)frame[(int64_t)p * 32];
    int comp, by, bx;
    jpeg_place(g, b, &comp, &by, &bx);
    *tab = comp > 0;
    return true;
}

__global__ __launch_bounds__(256) void jpeg_count_kernel(const uint32_t *__restrict__ coef, JpegGeom g, int32_t *__restrict__ bitoff,
                                                         int32_t *__restrict__ part) {
    __shared__ int lds[4];
    const int b = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    uint32_t c[32];
    int pred, tab;
    CountSink s;
    const bool live = jpeg_block(coef, g, f, b, c, &pred, &tab);
    if (live) jpeg_walk(c, pred, tab, s);
    int total;
    const int excl = block_excl_scan<4>(s.bits, lds, &total);
    if (live) bitoff[(int64_t)f * g.nb + b] = excl;
    if (threadIdx.x == 0) part[(int64_t)f * gridDim.x + blockIdx.x] = total;
}

// part[f][0 .. n): replaced by its exclusive scan; total[f] = its sum.  One workgroup per frame.
__global__ __launch_bounds__(256) void jpeg_partials_kernel(int32_t *__restrict__ part, int n, int32_t *__restrict__ total) {
    __shared__ int lds[4];
    int32_t *p = part + (int64_t)blockIdx.x * n;
    int carry = 0;
    for (int base = 0; base < n; base += 256) {
        const int i = base + threadIdx.x;
        const int v = i < n ? p[i] : 0;
        int sum;
        const int excl = block_excl_scan<4>(v, lds, &sum);
        if (i < n) p[i] = carry + excl;
        carry += sum;
    }
    if (threadIdx.x == 0) total[blockIdx.x] = carry;
}

__global__ __launch_bounds__(256) void jpeg_pack_kernel(const uint32_t *__restrict__ coef, JpegGeom g, const int32_t *__restrict__ bitoff,
                                                        const int32_t *__restrict__ part, uint32_t *__restrict__ words, int wcap,
                                                        int32_t *__restrict__ overflow) {
    const int b = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    uint32_t c[32];
    int pred, tab;
    if (!jpeg_block(coef, g, f, b, c, &pred, &tab)) return;
    const uint32_t off = (uint32_t)(bitoff[(int64_t)f * g.nb + b] + part[(int64_t)f * gridDim.x + blockIdx.x]);
    PackSink s;
    s.words = words + (int64_t)f * wcap, s.wcap = wcap, s.overflow = overflow;
    s.widx = (int)(off >> 5), s.nacc = (int)(off & 31u), s.acc = 0ull, s.shared = true;
    jpeg_walk(c, pred, tab, s);
    if (b == g.nb - 1) {                                             // the frame's last byte is filled with 1-bits
        const int pad = (32 - s.nacc) & 7;
        if (pad) s.put((1u << pad) - 1u, pad);
    }
    s.finish();
}

// ---- byte stuffing: one lane per 16 bytes (four words) of a frame's packed segment ------------------------------------------
__device__ __forceinline__ int jpeg_packed_bytes(int total_bits, int wcap) { return min((int)(((int64_t)total_bits + 7) >> 3), wcap * 4); }
__device__ __forceinline__ int word_byte(const uint4 &q, int j) {
    const uint32_t w = (j >> 2) == 0 ? q.x : ((j >> 2) == 1 ? q.y : ((j >> 2) == 2 ? q.z : q.w));
    return (w >> (24 - 8 * (j & 3))) & 0xff;
}
// the lane's 16 bytes and how many of them are 0xFF; *n = how many of them belong to the segment
__device__ __forceinline__ int jpeg_quad(const uint32_t *__restrict__ words, int wcap, int f, int quad, int nbytes, uint4 *q, int *n) {
    *n = max(0, min(16, nbytes - 16 * quad));
    *q = make_uint4(0u, 0u, 0u, 0u);
    if (*n > 0 && 4 * quad + 4 <= wcap) *q = *reinterpret_cast<const uint4 *>(words + (int64_t)f * wcap + 4 * (int64_t)quad);
    int ff = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) ff += (j < *n && word_byte(*q, j) == 0xff) ? 1 : 0;
    return ff;
}

__global__ __launch_bounds__(256) void jpeg_ff_count_kernel(const uint32_t *__restrict__ words, int wcap, const int32_t *__restrict__ total_bits,
                                                            int32_t *__restrict__ part) {
    __shared__ int lds[4];
    const int quad = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    uint4 q;
    int n, total;
    const int ff = jpeg_quad(words, wcap, f, quad, jpeg_packed_bytes(total_bits[f], wcap), &q, &n);
    block_excl_scan<4>(ff, lds, &total);
    if (threadIdx.x == 0) part[(int64_t)f * gridDim.x + blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void jpeg_stuff_kernel(const uint32_t *__restrict__ words, int wcap, const int32_t *__restrict__ total_bits,
                                                         const int32_t *__restrict__ part, const int32_t *__restrict__ ff_total,
                                                         uint8_t *__restrict__ out, int64_t cap, int32_t *__restrict__ nbytes,
                                                         int32_t *__restrict__ overflow) {
    __shared__ int lds[4];
    const int quad = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    const int packed = jpeg_packed_bytes(total_bits[f], wcap);
    uint4 q;
    int n, total;
    const int ff = jpeg_quad(words, wcap, f, quad, packed, &q, &n);
    const int excl = block_excl_scan<4>(ff, lds, &total);
    if (quad == 0) {
        const int64_t all = (int64_t)packed + ff_total[f];
        nbytes[f] = (int32_t)min(all, cap);
        if (all > cap) *overflow = 1;
    }
    int64_t at = 16 * (int64_t)quad + part[(int64_t)f * gridDim.x + blockIdx.x] + excl;
    uint8_t *dst = out + (int64_t)f * cap;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (j >= n) break;
        const int v = word_byte(q, j);
        if (at < cap) dst[at] = (uint8_t)v;
        ++at;
        if (v == 0xff) {
            if (at < cap) dst[at] = 0;
            ++at;
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
static inline int64_t align16(int64_t n) { return (n + 15) & ~(int64_t)15; }

struct JpegLayout {
    int64_t coef, bitoff, part_bits, total_bits, words, part_ff, total_ff, bytes;
    int groups_blocks, groups_quads, wcap;
};
// cap: bytes per frame of the output, a positive multiple of 32; the word buffer holds cap / 2 bytes per frame
static bool jpeg_layout(int64_t F, int64_t nb, int64_t cap, JpegLayout *L) {
    if (F < 1 || F > 65535 || nb < 1 || nb > JPEG_MAX_BLOCKS || cap < 32 || (cap & 31) || cap > 0x7fffffe0LL) return false;
    L->wcap = (int)(cap / 8);
    L->groups_blocks = (int)((nb + 255) / 256);
    L->groups_quads = (L->wcap / 4 + 255) / 256;
    int64_t at = 0;
    L->coef = at, at += F * nb * 128;
    L->bitoff = at, at += align16(F * nb * 4);
    L->part_bits = at, at += align16(F * L->groups_blocks * 4);
    L->total_bits = at, at += align16(F * 4);
    L->words = at, at += F * (int64_t)L->wcap * 4;
    L->part_ff = at, at += align16(F * L->groups_quads * 4);
    L->total_ff = at, at += align16(F * 4);
    L->bytes = at;
    return true;
}

extern "C" int64_t mh_jpeg_blocks(int32_t H, int32_t W, int32_t channels, int32_t subsampling) {
    return jpeg_blocks(H, W, channels, subsampling, nullptr);
}

extern "C" int64_t mh_jpeg_scan_capacity(int64_t blocks) {
    if (blocks < 1 || blocks > JPEG_MAX_BLOCKS) return -1;
    return 2 * align16((blocks * JPEG_MAX_BLOCK_BITS + 7) / 8);
}

extern "C" int64_t mh_jpeg_workspace_bytes(int32_t F, int64_t blocks, int64_t cap) {
    JpegLayout L;
    return jpeg_layout(F, blocks, cap, &L) ? L.bytes : -1;
}

extern "C" int mh_jpeg_quant_table(int32_t quality, int32_t chroma, int32_t *table) {
    if (quality < 1 || quality > 100 || (chroma != 0 && chroma != 1) || !table) return MH_ERR_ARG;
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        const int q = (JPEG_QBASE[chroma][i] * s + 50) / 100;
        table[i] = q < 1 ? 1 : (q > 255 ? 255 : q);
    }
    return MH_OK;
}

extern "C" int mh_jpeg_encode(const uint8_t *frames, int32_t F, int32_t H, int32_t W, int32_t channels, int32_t subsampling,
                              int32_t quality, void *workspace, uint8_t *out, int64_t cap, int32_t *nbytes, int32_t *overflow,
                              void *stream) {
    JpegGeom g;
    JpegLayout L;
    JpegQuant quant;
    int32_t table[64];
    if (!frames || !workspace || !out || !nbytes || !overflow) return MH_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(frames) & 3) || (reinterpret_cast<uintptr_t>(workspace) & 15) ||
        (reinterpret_cast<uintptr_t>(overflow) & 3))
        return MH_ERR_ARG;
    const int64_t nb = jpeg_blocks(H, W, channels, subsampling, &g);
    if (nb < 0 || !jpeg_layout(F, nb, cap, &L)) return MH_ERR_ARG;
    for (int t = 0; t < 2; ++t) {
        if (mh_jpeg_quant_table(quality, t, table) != MH_OK) return MH_ERR_ARG;
        for (int i = 0; i < 64; ++i) quant.q[t][i] = (uint16_t)table[i];
    }
    hipStream_t s = mh_stream(stream);
    char *ws = static_cast<char *>(workspace);
    uint32_t *coef = reinterpret_cast<uint32_t *>(ws + L.coef);
    int32_t *bitoff = reinterpret_cast<int32_t *>(ws + L.bitoff), *part_bits = reinterpret_cast<int32_t *>(ws + L.part_bits);
    int32_t *total_bits = reinterpret_cast<int32_t *>(ws + L.total_bits), *part_ff = reinterpret_cast<int32_t *>(ws + L.part_ff);
    int32_t *total_ff = reinterpret_cast<int32_t *>(ws + L.total_ff);
    uint32_t *words = reinterpret_cast<uint32_t *>(ws + L.words);
    const int64_t total_bytes = (int64_t)F * H * W * channels;
    if (!mh_zero_async(words, (size_t)F * L.wcap * 4, s) || !mh_zero_async(overflow, 4, s)) return MH_ERR_LAUNCH;
    const dim3 by_block((unsigned)L.groups_blocks, (unsigned)F), by_quad((unsigned)L.groups_quads, (unsigned)F), wg(256);
    hipLaunchKernelGGL(jpeg_transform_kernel, by_block, wg, 0, s, frames, total_bytes, g, quant, coef);
    MH_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_count_kernel, by_block, wg, 0, s, coef, g, bitoff, part_bits);
    MH_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_partials_kernel, dim3((unsigned)F), wg, 0, s, part_bits, L.groups_blocks, total_bits);
    MH_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_pack_kernel, by_block, wg, 0, s, coef, g, bitoff, part_bits, words, L.wcap, overflow);
    MH_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_ff_count_kernel, by_quad, wg, 0, s, words, L.wcap, total_bits, part_ff);
    MH_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_partials_kernel, dim3((unsigned)F), wg, 0, s, part_ff, L.groups_quads, total_ff);
    MH_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_stuff_kernel, by_quad, wg, 0, s, words, L.wcap, total_bits, part_ff, total_ff, out, cap, nbytes, overflow);
    MH_CHECK_LAUNCH();
    return MH_OK;
}
