"""A CPU restatement of the device JPEG encoder (faster_rcnn_amd/csrc/jpeg.hip, include/ext/frcnn_hip_jpeg.h) and the definition of its
stream: ``encode(frame, quality)`` is the file the kernels must produce, byte for byte.  Integer arithmetic only, so the file is a
function of (frame, quality) alone.

The stream.  JFIF baseline sequential DCT (SOF0), 8 bits, Y Cb Cr at 1x1 each (4:4:4): an MCU is one 8x8 block of Y, of Cb, of Cr.
Segments: SOI, APP0 "JFIF" 1.01 (no units, 1:1), DQT luma, DQT chroma, SOF0, DHT DC-luma, AC-luma, DC-chroma, AC-chroma, DRI, SOS, the
entropy-coded data, EOI: HEADER_BYTES in front of the data whatever the frame.
  tables    ITU-T T.81 Annex K.1 / K.2 scaled by the IJG rule (s = 5000 // q below 50, else 200 - 2q; entry = clamp((base * s + 50)
            // 100, 1, 255)), written in zigzag order; the Huffman tables of Annex K.3 (K.3 - K.6), as they stand.
  colour    16 fractional bits: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + CHROMA_ROUND) >> 16,
            Cr = (32768 R - 27439 G - 5329 B + CHROMA_ROUND) >> 16, CHROMA_ROUND = (128 << 16) + 32767; each lands in 0..255 without a
            clamp; 128 is subtracted for the DCT.  A frame whose sides are no multiple of 8 has its last column / row repeated.
  DCT       COS[u][x] = round(2^13 * c(u) / 2 * cos((2x + 1) u pi / 16)), c(0) = 1 / sqrt 2, else 1.  Rows first: t[y][u] = (sum_x
            COS[u][x] * s[y][x] + 512) >> 10 (an arithmetic shift; |sum| <= 2^22, t keeps 3 fractional bits), then columns: F[v][u] =
            sum_y COS[v][y] * t[y][u] (|F| < 2^28), which is 2^16 times the DCT coefficient.
  quantise  one division: |F| + (Q << 15) over Q << 16, floored, with the sign of F (half away from zero).  |DC| <= 1024, |AC| < 1024.
  entropy   per block the DC difference to the previous block of the same component in the same restart interval (0 at its start):
            the code of its category, then the category's low bits (of diff, or of diff - 1 when negative); then per non-zero AC
            coefficient in zigzag order one ZRL (0xF0) per 16 zeros in front of it, the code of (zeros % 16) << 4 | category, and the
            value bits; EOB (0x00) unless coefficient 63 is non-zero.
  intervals RESTART_MCUS MCUs in raster order (the last may be shorter), padded to a byte with 1-bits, 0x00 behind every 0xFF byte
            (one completed by the padding too), then RSTm, m = 0..7 cyclically, except behind the last interval.
``bound(h, w)`` restates frcnn_jpeg_bound."""
import math

import numpy as np

RESTART_MCUS = 16
BLOCK_BYTES = 208                    # (20 + 63 * 26 bits) rounded up to bytes: the longest block
CHROMA_ROUND = (128 << 16) + 32767

K1_LUMA = [16, 11, 10, 16, 24, 40, 51, 61,
           12, 12, 14, 19, 26, 58, 60, 55,
           14, 13, 16, 24, 40, 57, 69, 56,
           14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77,
           24, 35, 55, 64, 81, 104, 113, 92,
           49, 64, 78, 87, 103, 121, 120, 101,
           72, 92, 95, 98, 112, 100, 103, 99]
K2_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99,
             18, 21, 26, 66, 99, 99, 99, 99,
             24, 26, 56, 99, 99, 99, 99, 99,
             47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32

# Annex K.3: (BITS: codes per length 1..16, HUFFVAL: the symbols in code order)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
# the tails of both AC tables run through the remaining (run, size) pairs in rising order
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
            0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18,
            0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
            0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75,
            0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
            0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
            0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5,
            0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
              0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34,
              0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44,
              0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
              0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92,
              0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
              0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6,
              0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
              0xF9, 0xFA])
HUFFMAN = (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)       # in the order of their DHT segments; (class, id) = (0, 0) (1, 0) (0, 1) (1, 1)


def zigzag():
    """zigzag position -> natural index 8 * v + u: the anti-diagonals of the block, alternately up and down."""
    order = []
    for d in range(15):
        cells = [(d - u, u) for u in range(8) if 0 <= d - u < 8]          # (v, u), u rising: up along the diagonal
        order += cells[::-1] if d % 2 else cells
    return [8 * v + u for v, u in order]


ZIGZAG = zigzag()
COS = np.array([[int(round(8192 * (math.sqrt(0.5) if u == 0 else 1.0) / 2 * math.cos((2 * x + 1) * u * math.pi / 16))) for x in range(8)]
                for u in range(8)], dtype=np.int64)


def quant_tables(quality):
    """-> [luma, chroma], 64 entries each in ZIGZAG order (as the DQT segments and the kernels hold them)."""
    assert 1 <= quality <= 100
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [[min(255, max(1, (base[n] * s + 50) // 100)) for n in ZIGZAG] for base in (K1_LUMA, K2_CHROMA)]


def huffman_codes(bits, vals):
    """Annex C: symbol -> (code, length), codes of one length consecutive, in HUFFVAL order."""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


def segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def header(h, w, qt):
    out = b"\xFF\xD8" + segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    out += segment(0xDB, bytes([0] + qt[0])) + segment(0xDB, bytes([1] + qt[1]))
    out += segment(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for (bits, vals), tc_th in zip(HUFFMAN, (0x00, 0x10, 0x01, 0x11)):
        out += segment(0xC4, bytes([tc_th] + bits + vals))
    out += segment(0xDD, RESTART_MCUS.to_bytes(2, "big"))
    out += segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


HEADER_BYTES = len(header(1, 1, quant_tables(50)))


def bound(h, w):
    """frcnn_jpeg_bound: header + EOI + per interval (3 blocks of BLOCK_BYTES per MCU, each byte stuffed; a padding byte and its stuffing;
    RSTm); 0 for a refused size."""
    if not (1 <= h <= 65535 and 1 <= w <= 65535):
        return 0
    mcus = -(-h // 8) * -(-w // 8)
    b = HEADER_BYTES + 2 + 2 * BLOCK_BYTES * 3 * mcus + 4 * -(-mcus // RESTART_MCUS)
    return b if b <= 2 ** 31 - 1 else 0


def coefficients(frame, qt, bgr=False):
    """-> int array [MCU rows][MCU columns][3][64]: the quantised coefficients of every block in zigzag order."""
    h, w = frame.shape[:2]
    rgb = (frame[:, :, ::-1] if bgr else frame).astype(np.int64)
    rgb = np.pad(rgb, ((0, -h % 8), (0, -w % 8), (0, 0)), mode="edge")
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    ycc = np.stack([(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
                    (-11059 * r - 21709 * g + 32768 * b + CHROMA_ROUND) >> 16,
                    (32768 * r - 27439 * g - 5329 * b + CHROMA_ROUND) >> 16], 0)
    assert ycc.min() >= 0 and ycc.max() <= 255
    H, W = ycc.shape[1:]
    s = (ycc - 128).reshape(3, H // 8, 8, W // 8, 8).transpose(1, 3, 0, 2, 4)             # [my][mx][c][y][x]
    rows = s @ COS.T                                                                    # [..][y][u]
    assert np.abs(rows).max() <= 1 << 22
    t = (rows + 512) >> 10
    F = COS @ t                                                                         # [..][v][u]
    assert np.abs(F).max() < 1 << 28
    F = F.reshape(F.shape[:3] + (64,))[..., ZIGZAG]
    Q = np.array([qt[0], qt[1], qt[1]], dtype=np.int64)[None, None]
    return np.sign(F) * ((np.abs(F) + (Q << 15)) // (Q << 16))


class Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, count):
        assert 0 <= value < 1 << count
        self.acc, self.n = (self.acc << count) | value, self.n + count

    def finish(self):
        """Padded with 1-bits to a byte, then 0x00 behind every 0xFF."""
        pad = -self.n % 8
        self.put((1 << pad) - 1, pad)
        return self.acc.to_bytes(self.n // 8, "big").replace(b"\xFF", b"\xFF\x00")


def value_bits(v):
    """(category, its low bits) of a DC difference or an AC coefficient."""
    size = abs(int(v)).bit_length()
    return size, (int(v) if v >= 0 else int(v) - 1) & ((1 << size) - 1)


def encode(frame, quality, bgr=False, info=None):
    """The .jpg file of ``frame`` ((h, w, 3) uint8, R,G,B or with ``bgr`` B,G,R) as bytes.  ``info`` (a dict) receives "intervals": the
    file offset at which each restart interval starts; "nonzero": per block in coding order the zigzag positions of its non-zero
    coefficients; "max_category": the largest DC and AC categories coded."""
    h, w = frame.shape[:2]
    qt = quant_tables(quality)
    coef = coefficients(frame, qt, bgr)
    dc_codes = [huffman_codes(*DC_LUMA), huffman_codes(*DC_CHROMA), huffman_codes(*DC_CHROMA)]
    ac_codes = [huffman_codes(*AC_LUMA), huffman_codes(*AC_CHROMA), huffman_codes(*AC_CHROMA)]
    mcus = [(my, mx) for my in range(coef.shape[0]) for mx in range(coef.shape[1])]
    out = bytearray(header(h, w, qt))
    starts, nonzero, max_dc, max_ac = [], [], 0, 0
    n_int = -(-len(mcus) // RESTART_MCUS)
    for i in range(n_int):
        starts.append(len(out))
        bits, pred = Bits(), [0, 0, 0]
        for my, mx in mcus[i * RESTART_MCUS:(i + 1) * RESTART_MCUS]:
            for c in range(3):
                blk = coef[my, mx, c]
                size, low = value_bits(blk[0] - pred[c])
                pred[c] = blk[0]
                bits.put(*dc_codes[c][size])
                bits.put(low, size)
                max_dc = max(max_dc, size)
                nz = [z for z in range(1, 64) if blk[z]]
                nonzero.append(([0] if blk[0] else []) + nz)
                last = 0
                for z in nz:
                    run = z - last - 1
                    for _ in range(run >> 4):
                        bits.put(*ac_codes[c][0xF0])
                    size, low = value_bits(blk[z])
                    bits.put(*ac_codes[c][(run & 15) << 4 | size])
                    bits.put(low, size)
                    max_ac = max(max_ac, size)
                    last = z
                if last != 63:
                    bits.put(*ac_codes[c][0x00])
        out += bits.finish()
        if i + 1 < n_int:
            out += bytes([0xFF, 0xD0 + (i & 7)])
    out += b"\xFF\xD9"
    if info is not None:
        info.update(intervals=starts, nonzero=nonzero, max_category=(max_dc, max_ac))
    return bytes(out)
