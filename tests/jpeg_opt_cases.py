"""The frames the device JPEG encoder's 4:2:0 / optimised-Huffman modes are tested on (tests/test_jpeg_opt_cpu.py runs the CPU
restatement tests/jpeg_opt_ref.py over them, tests/test_jpeg_opt_gpu.py holds the kernels to it): the smallest at which each mechanism
can go wrong."""
import functools
import io
import os

import numpy as np

from tests.jpeg_cases import extremes, noise, photo_crop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [(s, f) for s in (444, 420) for f in ("standard", "optimized")]

CASES = {
    "1x1": noise(1, 1, 11),
    "1x17": noise(1, 17, 12),
    "17x1": noise(17, 1, 13),
    "noise_16x16": noise(16, 16, 14),
    "noise_13x21": noise(13, 21, 15),                   # replication to 16 both ways, odd chroma sides
    "noise_33x47": noise(33, 47, 16),
    "flat_32x48": np.full((32, 48, 3), (90, 140, 200), np.uint8),          # one-symbol tables
    "grey_24x40": np.repeat(noise(24, 40, 17)[:, :, :1], 3, axis=2),      # chroma tables: category 0 and EOB only
    "extremes_16x16": extremes(),
    "photo_96x128": photo_crop(),
    "noise_48x352": noise(48, 352, 18),                 # 66 MCUs at 4:2:0 = 9 intervals: RST7 then RST0, the last interval 2 MCUs
}
# every case at quality 90; three of them at the ends of the scale too -- each in all four mode pairs
QUALITIES = [(name, 90) for name in sorted(CASES)] + [(name, q) for name in ("photo_96x128", "extremes_16x16", "noise_48x352") for q in (100, 10)]
RUNS = [(name, q, s, f) for name, q in QUALITIES for s, f in MODES]


@functools.lru_cache(maxsize=None)
def reference(name, quality, subsampling, huffman):
    """-> (the restatement's file of a run, its info): computed once per process, shared by the tests and left unchanged."""
    from tests import jpeg_opt_ref as O
    info = {}
    return O.encode(CASES[name], quality, subsampling, huffman, info=info), info


def golden_image():
    from PIL import Image
    return np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "VOC_test", "JPEGImages", "000005.jpg")).convert("RGB"))


@functools.lru_cache(maxsize=None)
def pillow_tables():
    """[(label, [4][256] symbol counts, the file's own four (BITS, HUFFVAL))] over ``pillow_optimized_files``: computed once."""
    return [(label,) + file_histograms(data) for label, data in pillow_optimized_files()]


def pillow_optimized_files():
    """[(label, bytes)]: Pillow's own ``optimize=True`` files of the golden image, its crop and 64x136 noise at qualities 10 / 90 / 100,
    subsampling 0 and 2, with and without restart_marker_blocks=8."""
    from PIL import Image
    out = []
    for label, frame in (("golden", golden_image()), ("crop", photo_crop()), ("noise", noise(64, 136, 6))):
        for q in (10, 90, 100):
            for sub in (0, 2):
                for rst in (0, 8):
                    buf = io.BytesIO()
                    kw = dict(restart_marker_blocks=rst) if rst else {}
                    Image.fromarray(frame).save(buf, format="JPEG", quality=q, subsampling=sub, optimize=True, **kw)
                    out.append(("%s q%d s%d r%d" % (label, q, sub, rst), buf.getvalue()))
    return out


def file_histograms(data):
    """-> ([4][256] symbol counts of a baseline file in DHT order (DC luma, AC luma, DC chroma, AC chroma), its four (BITS, HUFFVAL)):
    the symbols that tests/jpeg_dec_ref.Entropy.serial() decodes, recounted from its coefficients (DC differences, zigzag runs with
    ZRL and EOB)."""
    from tests import jpeg_dec_ref as D
    p = D.plan(data)
    e = D.Entropy(data, p)
    coef, _, total, status = e.serial()
    assert status == 0 and total == p.expected_blocks
    hist = np.zeros((4, 256), np.int64)
    zz = coef.astype(np.int64)[:, D.ZIGZAG]
    luma = p.hs * p.vs
    for k in range(total):
        chroma = 1 if (k % p.bpm) >= luma else 0
        blk = zz[k]
        hist[2 * chroma, abs(int(blk[0])).bit_length()] += 1
        last = 0
        for z in np.nonzero(blk[1:])[0] + 1:
            run = int(z) - last - 1
            hist[2 * chroma + 1, 0xF0] += run >> 4
            hist[2 * chroma + 1, (run & 15) << 4 | abs(int(blk[z])).bit_length()] += 1
            last = int(z)
        if last != 63:
            hist[2 * chroma + 1, 0x00] += 1
    tables = []
    for tc, th in ((0, 0), (1, 0), (0, 1), (1, 1)):
        off, n = p.dht_off[tc][th], p.dht_n[tc][th]
        tables.append((list(data[off:off + 16]), list(data[off + 16:off + 16 + n])))
    return hist, tables


def fibonacci_histogram():
    """30 symbols with the Fibonacci counts 2, 3, 5, 8, ..., the largest at the smallest symbol: with the pseudo-symbol's 1 in front every
    merge takes the running sum and the next count, so the unconstrained Huffman tree is a chain 30 deep and the length-limiting loop
    must act; HUFFVAL (by tree depth, then symbol) runs through the symbols in rising order."""
    hist = np.zeros(256, np.int64)
    a, b = 2, 3
    for s in reversed(range(30)):
        hist[3 * s + 1] = a
        a, b = b, a + b
    return hist
