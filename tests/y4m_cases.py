"""Case builders for the YUV4MPEG2 tests: synthetic frames from a seeded RNG at the sizes where edge replication, odd planes, ragged
vector tails and a second tile can each go wrong, and the 2^8 x 2^8 Cb x Cr sweep at a few Y values, which hits every clamp."""
import zlib

import numpy as np

from tests import y4m_ref as R

# 1x1 .. 3x3: planes of one or two samples, every edge rule at once; 5x7: odd planes; 16x16: whole words only; 17x33: ragged tails behind
# whole words; 48x64: several rows of groups; 130x258: more than one tile of 256 groups in every mode, a ragged last group
SIZES = ((1, 1), (1, 2), (2, 1), (3, 3), (5, 7), (16, 16), (17, 33), (48, 64), (130, 258))
SWEEP_Y = (0, 16, 126, 235, 255)


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def frame(h, w, chroma, seed=0):
    """One frame's planes as bytes: smooth gradients plus noise, with runs of 0 and 255 so that the clamps and the edges meet."""
    rng = _rng("y4m", h, w, chroma, seed)
    n = R.frame_bytes(h, w, chroma)
    buf = rng.randint(0, 256, n).astype(np.uint8)
    ramp = (np.arange(n) * 7 // max(1, w)) % 256
    mix = rng.randint(0, 4, n)
    buf = np.where(mix == 0, ramp, buf).astype(np.uint8)
    buf[rng.randint(0, n, max(1, n // 16))] = 0
    buf[rng.randint(0, n, max(1, n // 16))] = 255
    return buf.tobytes()


def rgb_frame(h, w, seed=0):
    rng = _rng("rgb", h, w, seed)
    f = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    f[rng.randint(0, h, 3), :, :] = 255
    f[:, rng.randint(0, w, 3), :] = 0
    return f


def sweep_444(y):
    """A 256 x 256 C444 frame: Y = ``y`` everywhere, Cb = column, Cr = row."""
    cr, cb = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    return np.concatenate([np.full(65536, y), cb.ravel(), cr.ravel()]).astype(np.uint8).tobytes()


def stream(frames, h, w, chroma="420jpeg", range_="limited", tags="F25:1 Ip A1:1", frame_tags=""):
    """The bytes of a y4m stream that holds ``frames``."""
    head = "YUV4MPEG2 W%d H%d %s C%s%s\n" % (w, h, tags, chroma, " XCOLORRANGE=FULL" if range_ == "full" else "")
    return head.encode() + b"".join(b"FRAME" + frame_tags.encode() + b"\n" + f for f in frames)
