"""The constant tables of baseline JPEG (ITU-T T.81 Annex K) and what follows from them, in pure Python with no import of its own:
video.py writes its DQT / DHT segments from them, tools/gen_jpeg_tables.py writes csrc/jpeg_tables.inc from them and
tests/video_oracle.py reads them.  tests/test_video_host.py holds every table here against the files PIL writes.
"""
import math

# K.1 / K.2: luminance and chrominance quantisation tables in natural (row-major) order
QBASE = (
    (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
     103, 99),
    (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99)
    + (99,) * 32,
)

# K.3 - K.6: BITS (codes of length 1 .. 16) and HUFFVAL of the DC and AC tables, [0] luminance, [1] chrominance
DC_BITS = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0))
DC_VALS = (tuple(range(12)), tuple(range(12)))
AC_BITS = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D), (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77))


def _rows(first, last, lo):
    """the symbols 0x<r><s> for r = first .. last and s = lo .. 0xA, row after row: the runs both AC lists end in"""
    return tuple((r << 4) | s for r in range(first, last + 1) for s in range(lo, 11))


AC_VALS = (
    (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18,
     0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A)
    + _rows(4, 8, 3) + _rows(9, 13, 2) + _rows(14, 15, 1),
    (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25,
     0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A)
    + _rows(4, 7, 3) + _rows(8, 15, 2),
)

ZRL, EOB = 0xF0, 0x00
MAX_BLOCK_BITS = 20 + 63 * 26        # DC: 9-bit code + 11 bits; every AC coefficient a 16-bit code + 10 bits


def zigzag():
    """-> Z[64]: Z[k] = the natural (row-major) index of the k-th coefficient in zigzag order (T.81 figure 5)"""
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8) if (i // 8 + i % 8) % 2 else (i % 8)))
    return tuple(order)


ZIGZAG = zigzag()


def quant_table(quality: int, chroma: int):
    """The IJG rule: s = 5000 // q below 50, else 200 - 2 q; Q = clamp((base * s + 50) // 100, 1, 255), natural order"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality: 1 .. 100 expected, got {quality!r}")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(min(max((b * s + 50) // 100, 1), 255) for b in QBASE[chroma])


def huffman_codes(bits, vals):
    """Annex C: -> {symbol: (code, length)}, codes handed out in order of length, counting up"""
    if sum(bits) != len(vals):
        raise ValueError("BITS does not add up to the number of symbols")
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


# the integer DCT's cosine table: COS[u][x] = round(2^COS_BITS * c(u) / 2 * cos((2 x + 1) u pi / 16)), c(0) = 1 / sqrt 2, c(u) = 1
# x = 0 .. 3 is rounded from float64; x = 4 .. 7 follows from the cosine's symmetry, COS[u][7 - x] = (-1)^u COS[u][x]
COS_BITS = 14
ROW_SHIFT = 9                        # the row pass keeps COS_BITS - ROW_SHIFT = 5 fraction bits
OUT_BITS = 2 * COS_BITS - ROW_SHIFT  # the column pass's results carry 19 fraction bits; the quantiser divides them away


def cos_table():
    half = [[int(math.floor((1 << COS_BITS) * (math.sqrt(0.5) if u == 0 else 1.0) / 2 * math.cos((2 * x + 1) * u * math.pi / 16)
                            + 0.5)) for x in range(4)] for u in range(8)]
    return tuple(tuple(row + [(-1) ** u * row[3 - x] for x in range(4)]) for u, row in enumerate(half))


COS = cos_table()

# JFIF's RGB -> YCbCr in 16-bit fixed point: component = (cr R + cg G + cb B + offset) >> 16.  The rows add up to 65536, 0 and 0,
# so grey stays grey; the chroma offset is 128 and a rounding term one below a half, which keeps 255 from becoming 256.
YCC = ((19595, 38470, 7471, 32768),
       (-11059, -21709, 32768, (128 << 16) + 32767),
       (32768, -27439, -5329, (128 << 16) + 32767))
