"""The frames the device JPEG encoder is tested on (tests/test_jpeg_cpu.py runs the CPU restatement over them, tests/test_jpeg_gpu.py
holds the kernels to the restatement on them): the smallest at which each mechanism can go wrong."""
import math
import os

import numpy as np

from tests import jpeg_ref as R
from tests.png_huff_cases import banded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPARSE_AT = (17, 33, 49, 63)            # zigzag positions of sparse_hf's lone coefficients: 1, 2, 3 ZRLs in front; 63: no EOB


def noise(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def sparse_hf(quality=90):
    """A grey 8x32 frame, one block per entry of SPARSE_AT: 128 plus the one DCT basis function of that zigzag position, at six
    quantisation steps of ``quality``.  Grey pixels have Cb = Cr = 128 exactly, so the chroma blocks are all zero."""
    qt = R.quant_tables(quality)[0]
    frame = np.zeros((8, 32, 3), np.uint8)
    for k, z in enumerate(SPARSE_AT):
        v, u = divmod(R.ZIGZAG[z], 8)
        amp = 6 * qt[z] / 4.0
        for y in range(8):
            for x in range(8):
                frame[y, 8 * k + x] = int(round(128 + amp * math.cos((2 * x + 1) * u * math.pi / 16) * math.cos((2 * y + 1) * v * math.pi / 16)))
    return frame


def extremes():
    """16x16: a checkerboard of 0 / 255 pixels (the largest coefficient 63), a black block, a white block behind it (the largest DC
    difference) and a 0 | 255 step (the largest low-frequency AC coefficient)."""
    y, x = np.mgrid[0:8, 0:8]
    a = np.zeros((16, 16), np.uint8)
    a[:8, :8] = 255 * ((x + y) & 1)
    a[8:, :8] = 255
    a[8:, 8:] = 255 * (x >= 4)
    return np.repeat(a[:, :, None], 3, axis=2)


def photo_crop():
    from PIL import Image
    rgb = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "VOC_test", "JPEGImages", "000005.jpg")).convert("RGB"))
    return np.ascontiguousarray(rgb[100:196, 200:328])


CASES = {
    "1x1": noise(1, 1, 1),
    "1x9": noise(1, 9, 2),
    "9x1": noise(9, 1, 3),
    "8x8": noise(8, 8, 4),
    "noise_13x21": noise(13, 21, 5),                    # edge replication both ways
    "flat_24x40": np.full((24, 40, 3), (90, 140, 200), np.uint8),
    "noise_64x136": noise(64, 136, 6),                  # 136 MCUs = 9 intervals: RST7 then RST0, the last interval 8 MCUs
    "banded_40x131": banded(40, 131),
    "sparse_hf": sparse_hf(),
    "extremes_16x16": extremes(),
    "photo_96x128": photo_crop(),
}
# every case at quality 90; three of them at the ends of the scale too
RUNS = [(name, 90) for name in sorted(CASES)] + [(name, q) for name in ("noise_64x136", "extremes_16x16", "photo_96x128") for q in (100, 10)]
