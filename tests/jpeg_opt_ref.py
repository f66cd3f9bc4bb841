"""A CPU restatement of the device JPEG encoder's second entry point (faster_rcnn_amd/csrc/jpeg_opt.hip,
include/ext/frcnn_hip_jpeg_opt.h) and the definition of its stream: ``encode(frame, quality, subsampling, huffman)`` is the file the
kernels must produce, byte for byte.  Everything that tests/jpeg_ref.py states (tables, colour transform, DCT, quantisation, the
entropy code, intervals, stuffing) holds here unchanged and is reused by import; this file adds two independent knobs.

  subsampling  444: tests/jpeg_ref.py's stream.  420: SOF0 with Y at 2x2 and Cb, Cr at 1x1.  An MCU is 16x16 pixels, in block order
               Y00 Y01 Y10 Y11 Cb Cr.  The frame's last column / row is repeated to multiples of 16.  Cb and Cr are computed per pixel
               (16 fractional bits, as at 4:4:4) and each 2x2 group is averaged as (a + b + c + d + bias) >> 2, bias 1 at even and 2 at
               odd output columns (libjpeg's h2v2_downsample).  The restart interval is 8 MCUs = 48 blocks (16 MCUs = 48 blocks at 444).
  huffman      "standard": Annex K.3.  "optimized": four tables per frame (DC / AC for luma and for chroma) from the frame's own symbol
               counts -- DC categories with the predictor reset at every interval, AC (run, size) with ZRL and EOB -- by libjpeg's
               jpeg_gen_optimal_table (``optimal_table``); the four DHT segments carry them, so the header is at most HEADER_BYTES long.

(444, "standard") is tests/jpeg_ref.py's file.  ``bound(h, w, subsampling)`` restates frcnn_jpeg_opt_bound: a block is at most 23 + 63 *
26 bits with an optimised DC code of 12 bits (12 categories and the pseudo-symbol: 13 leaves), 20 + 63 * 26 with Annex K's: 208 bytes
either way, so the bound does not depend on ``huffman``."""
import numpy as np

from tests import jpeg_ref as R

SUBSAMPLINGS = (444, 420)
HUFFMANS = ("standard", "optimized")
RESTART = {444: 16, 420: 8}          # MCUs per restart interval: 48 blocks either way
MAX_DEPTH = 257                      # a Huffman tree over 257 leaves is at most this deep: ``optimal_table`` indexes safely up to it
TABLE_IDS = (0x00, 0x10, 0x01, 0x11)     # DHT order: DC luma, AC luma, DC chroma, AC chroma = histogram / table index 0..3


def check_mode(subsampling, huffman):
    if subsampling not in SUBSAMPLINGS or huffman not in HUFFMANS:
        raise ValueError("subsampling=%r huffman=%r" % (subsampling, huffman))


def mcu_grid(h, w, subsampling):
    side = 16 if subsampling == 420 else 8
    return -(-h // side), -(-w // side)


def bound(h, w, subsampling=444):
    """frcnn_jpeg_opt_bound: header + EOI + per interval (its blocks of BLOCK_BYTES, each byte stuffed; a padding byte and its
    stuffing; RSTm); 0 for a refused size."""
    if subsampling not in SUBSAMPLINGS or not (1 <= h <= 65535 and 1 <= w <= 65535):
        return 0
    my, mx = mcu_grid(h, w, subsampling)
    mcus = my * mx
    b = R.HEADER_BYTES + 2 + 2 * R.BLOCK_BYTES * (6 if subsampling == 420 else 3) * mcus + 4 * -(-mcus // RESTART[subsampling])
    return b if b <= 2 ** 31 - 1 else 0


def optimal_table(hist):
    """libjpeg's jpeg_gen_optimal_table over 256 symbol counts -> (BITS[16], HUFFVAL).  A 257th pseudo-symbol of count 1 keeps the
    all-ones code free; of the two smallest counts the LARGEST index wins a tie; lengths past 16 are pulled in from the longest down;
    the pseudo-symbol is removed from the longest remaining length; HUFFVAL lists the symbols by (tree depth, symbol).  libjpeg stops at
    depth 32 with an error; here the same loop starts at MAX_DEPTH, so any histogram is handled.  No symbol at all: an empty table."""
    freq = [int(v) for v in hist] + [1]
    assert len(freq) == 257 and min(freq) >= 0
    codesize, group = [0] * 257, list(range(257))          # group: the tree a symbol hangs in, named by the index its count lives at
    while True:
        live = [i for i in range(257) if freq[i]]
        if len(live) < 2:
            break
        c1 = min(live, key=lambda i: (freq[i], -i))
        c2 = min((i for i in live if i != c1), key=lambda i: (freq[i], -i))
        freq[c1] += freq[c2]
        freq[c2] = 0
        for i in range(257):                               # (libjpeg walks the ``others`` chains of c1 and c2: the same symbols)
            if group[i] in (c1, c2) and (i == 256 or hist[i]):
                codesize[i] += 1
                group[i] = c1
    bits = [0] * (MAX_DEPTH + 1)
    for i in range(257):
        if codesize[i]:
            bits[codesize[i]] += 1
    for i in range(MAX_DEPTH, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while j > 0 and bits[j] == 0:
                j -= 1
            if j == 0:
                break
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while i > 0 and bits[i] == 0:
        i -= 1
    if i > 0:
        bits[i] -= 1
    vals = sorted((s for s in range(256) if codesize[s]), key=lambda s: (codesize[s], s))
    assert sum(bits[1:17]) == len(vals)
    return bits[1:17], vals


def planes(frame, subsampling, bgr=False):
    """-> [Y, Cb, Cr] int64 planes (0..255), the frame padded by edge replication to whole MCUs; chroma at half size for 420."""
    h, w = frame.shape[:2]
    side = 16 if subsampling == 420 else 8
    rgb = (frame[:, :, ::-1] if bgr else frame).astype(np.int64)
    rgb = np.pad(rgb, ((0, -h % side), (0, -w % side), (0, 0)), mode="edge")
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + R.CHROMA_ROUND) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + R.CHROMA_ROUND) >> 16
    if subsampling == 420:
        bias = 1 + (np.arange(cb.shape[1] // 2) & 1)[None, :]
        cb, cr = [(p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2 for p in (cb, cr)]
    return [y, cb, cr]


def plane_blocks(plane, q):
    """A plane (sides multiples of 8) -> [block rows][block columns][64] quantised coefficients in zigzag order (tests/jpeg_ref.py's
    DCT and quantisation)."""
    H, W = plane.shape
    s = (plane - 128).reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)
    t = ((s @ R.COS.T) + 512) >> 10
    F = R.COS @ t
    F = F.reshape(F.shape[:2] + (64,))[..., R.ZIGZAG]
    Q = np.array(q, dtype=np.int64)[None, None]
    return np.sign(F) * ((np.abs(F) + (Q << 15)) // (Q << 16))


def mcu_blocks(frame, quality, subsampling, bgr=False):
    """-> [MCU in raster order][(component, its 64 coefficients)] in coding order."""
    qt = R.quant_tables(quality)
    y, cb, cr = [plane_blocks(p, qt[1 if c else 0]) for c, p in enumerate(planes(frame, subsampling, bgr))]
    my, mx = mcu_grid(frame.shape[0], frame.shape[1], subsampling)
    out = []
    for j in range(my):
        for i in range(mx):
            if subsampling == 420:
                blocks = [(0, y[2 * j + v, 2 * i + u]) for v in (0, 1) for u in (0, 1)]
            else:
                blocks = [(0, y[j, i])]
            out.append(blocks + [(1, cb[j, i]), (2, cr[j, i])])
    return out


def interval_symbols(mcus):
    """The symbols of one restart interval: [(table 0..3, symbol, value bits, their number)], predictors 0 at its start."""
    out, pred = [], [0, 0, 0]
    for blocks in mcus:
        for c, blk in blocks:
            size, low = R.value_bits(blk[0] - pred[c])
            pred[c] = blk[0]
            out.append((2 if c else 0, size, low, size))
            last = 0
            for z in range(1, 64):
                if blk[z]:
                    run = z - last - 1
                    out += [(3 if c else 1, 0xF0, 0, 0)] * (run >> 4)
                    size, low = R.value_bits(blk[z])
                    out.append((3 if c else 1, (run & 15) << 4 | size, low, size))
                    last = z
            if last != 63:
                out.append((3 if c else 1, 0x00, 0, 0))
    return out


def histograms(intervals):
    hist = np.zeros((4, 256), np.int64)
    for syms in intervals:
        for t, s, _, _ in syms:
            hist[t, s] += 1
    return hist


def header(h, w, qt, subsampling, tables):
    out = b"\xFF\xD8" + R.segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    out += R.segment(0xDB, bytes([0] + qt[0])) + R.segment(0xDB, bytes([1] + qt[1]))
    out += R.segment(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") +
                     bytes([3, 1, 0x22 if subsampling == 420 else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for (bits, vals), tc_th in zip(tables, TABLE_IDS):
        out += R.segment(0xC4, bytes([tc_th] + list(bits) + list(vals)))
    out += R.segment(0xDD, RESTART[subsampling].to_bytes(2, "big"))
    out += R.segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def encode(frame, quality, subsampling=444, huffman="standard", bgr=False, info=None):
    """The .jpg file of ``frame`` ((h, w, 3) uint8) as bytes.  ``info`` (a dict) receives "tables": the four (BITS, HUFFVAL) in DHT
    order, "hist": the [4][256] symbol counts, "intervals": the file offset at which each restart interval starts."""
    check_mode(subsampling, huffman)
    h, w = frame.shape[:2]
    mcus = mcu_blocks(frame, quality, subsampling, bgr)
    n = RESTART[subsampling]
    intervals = [interval_symbols(mcus[i:i + n]) for i in range(0, len(mcus), n)]
    hist = histograms(intervals)
    tables = [optimal_table(hist[t]) for t in range(4)] if huffman == "optimized" else list(R.HUFFMAN)
    codes = [R.huffman_codes(*t) for t in tables]
    out = bytearray(header(h, w, R.quant_tables(quality), subsampling, tables))
    assert len(out) <= R.HEADER_BYTES
    starts = []
    for i, syms in enumerate(intervals):
        starts.append(len(out))
        bits = R.Bits()
        for t, s, low, size in syms:
            bits.put(*codes[t][s])
            bits.put(low, size)
        out += bits.finish()
        if i + 1 < len(intervals):
            out += bytes([0xFF, 0xD0 + (i & 7)])
    out += b"\xFF\xD9"
    if info is not None:
        info.update(tables=tables, hist=hist, intervals=starts)
    return bytes(out)
