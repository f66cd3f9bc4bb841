"""Plain numpy references of VALID NHWC pooling for the forward pooling kernels of csrc/pool.hip (frcnn_pool2d_fwd,
frcnn_pool2d_fwd_planes), the fp16-plane arithmetic their comment states, the status rule of csrc/conv_f32_common.h, and the shapes and
inputs tests/test_pool_ref_cpu.py and tests/test_pool_kernels_gpu.py share.

The windows come from numpy's sliding_window_view, not from the kernels' index arithmetic.  U = 2^-24, one f32 rounding."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

U = 2.0 ** -24

# (n, h, w, c, k, stride)
ONE_WINDOW = [(1, 2, 2, 4, 2, 2), (1, 3, 3, 4, 3, 2), (1, 7, 7, 4, 7, 7)]            # Ho = Wo = 1, C/4 = 1
ODD_PIECES = [(2, 5, 7, 12, 2, 2), (1, 9, 11, 68, 3, 2)]                            # C/4 = 3, 17; two images
DROPPED = [(1, 5, 7, 8, 2, 2), (1, 6, 8, 8, 3, 2), (1, 15, 20, 4, 7, 7), (3, 7, 7, 16, 7, 7)]     # rows / columns no window covers
OVERLAP_HOLES = [(1, 6, 9, 8, 3, 1), (1, 8, 11, 8, 2, 3)]                           # stride < k, stride > k
SUITE = [(2, 17, 23, 64, 3, 2), (2, 17, 23, 64, 2, 2), (2, 17, 23, 64, 7, 7)]       # test_conv_gpu.test_pool_and_softmax's
SMALL = ONE_WINDOW + ODD_PIECES + DROPPED + OVERLAP_HOLES + SUITE
GRID_CAP = 8192 * 256                                                                # output pieces (float4) one trip of the capped grid writes
GRID_STRIDE = [(1, 1025, 512, 16, 1, 1), (1, 1026, 1024, 32, 2, 2)]                  # 2 099 200 and 2 101 248 pieces: a second trip
CASES = SMALL + GRID_STRIDE
PLANE_CASES = [c for c in CASES if c[3] % 4 == 0]
STATUS_SMALL = (1, 8, 8, 8, 2, 2)                                                    # 32 pieces: one workgroup, half a wave
STATUS_WAVE = (1, 8, 8, 16, 2, 2)                                                    # 64 pieces: one whole wave, so lanes 32..63 report too
STATUS_CASES = [STATUS_SMALL, STATUS_WAVE, GRID_STRIDE[1]]


def out_hw(h, w, k, s):
    return (h - k) // s + 1, (w - k) // s + 1


def pieces(case):
    n, h, w, c, k, s = case
    ho, wo = out_hw(h, w, k, s)
    return n * ho * wo * (c // 4)


def position_coded(case, seed=None):
    """f32 (n,h,w,c): normal noise plus a term that differs along every axis, so a swapped or dropped index changes the result.
    No zeros of either sign (checked)."""
    n, h, w, c = case[:4]
    rng = np.random.default_rng(sum(v * 31 ** i for i, v in enumerate(case)) if seed is None else seed)
    x = rng.standard_normal((n, h, w, c), dtype=np.float32)
    x += (np.float32(0.37) * np.arange(n, dtype=np.float32)[:, None, None, None] + np.float32(0.011) * np.arange(h, dtype=np.float32)[None, :, None, None]
          - np.float32(0.007) * np.arange(w, dtype=np.float32)[None, None, :, None] + np.float32(0.05) * np.arange(c, dtype=np.float32)[None, None, None, :])
    assert (x != 0).all()
    return x


def windows(x, k, s):
    """(n, Ho, Wo, c, k, k): every VALID k x k window of the NHWC tensor x at the given stride (a view)."""
    return sliding_window_view(x, (k, k), axis=(1, 2))[:, ::s, ::s]


def pool_max(x, k, s):
    """The exact maximum of each window (the input's dtype)."""
    return np.ascontiguousarray(windows(x, k, s).max(axis=(4, 5)))


def pool_avg64(x, k, s):
    """-> (float64 mean, sum|x| / k^2) per output."""
    w = windows(np.asarray(x, np.float64), k, s)
    return w.sum(axis=(4, 5)) / (k * k), np.abs(w).sum(axis=(4, 5)) / (k * k)


def pool_avg32_seq(x, k, s):
    """The f32 model pool.hip documents: the k*k taps added in raster order in f32 from +0.0, then ONE IEEE division by f32(k*k)."""
    w = windows(np.asarray(x, np.float32), k, s)
    acc = np.zeros(w.shape[:4], np.float32)
    for r in range(k):
        for q in range(k):
            acc = acc + w[..., r, q]
    return acc / np.float32(k * k)


def avg_bound(mag, k):
    """|f32 sequential mean - f64 mean|: k^2 - 1 additions and one division, each within U of a partial result no larger than
    sum|x| (resp. sum|x| / k^2): at most k^2 U sum|x| / k^2."""
    return k * k * U * mag


def plane_exponent(amax):
    """e with amax * 2^e in [2^14, 2^15)."""
    return 15 - int(np.frexp(np.float32(amax))[1])


def scaled(v, e):
    return (np.asarray(v, np.float32) * np.float32(2.0 ** e)).astype(np.float32)


def planes_model(v, e):
    """pool.hip's comment: xs = f32(v 2^e), hi = f16(xs) to nearest even, lo = f16((xs - f32(hi)) 2048).
    -> (hi, lo, the reconstruction (hi + lo / 2048) / 2^e in float64)."""
    xs = scaled(v, e)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = xs.astype(np.float16)
        lo = ((xs - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi, lo, plane_values(hi, lo, e)


def plane_values(hi, lo, e):
    with np.errstate(invalid="ignore"):
        return (np.asarray(hi, np.float64) + np.asarray(lo, np.float64) / 2048.0) / 2.0 ** e


def plane_bound(v):
    """The bar tests/test_conv_h3_gpu.py holds planes to: 2^-22 |v| + 2^-38 max|v|."""
    v = np.abs(np.asarray(v, np.float64))
    return 2.0 ** -22 * v + 2.0 ** -38 * v.max()


def below_f16_normal(v, e):
    """Elements whose scaled magnitude is under 2^-14, fp16's smallest normal: left out of the hi plane's bit comparison."""
    return np.abs(scaled(v, e)) < np.float32(2.0 ** -14)


H3_UNDER, H3_SATURATED, H3_NONFINITE = 1, 2, 4


def status_bits(hi):
    """csrc/conv_f32_common.h h3_status_bits on the largest |hi| bit pattern."""
    m = int((np.ascontiguousarray(hi, np.float16).view(np.uint16) & 0x7FFF).max())
    return 7 if m > 0x7BFF else 3 if m == 0x7BFF else 1 if m >= 0x7800 else 0


def status_input(case, seed=5):
    """-> (x, peak): a position-coded tensor for the status tests and a power of two `peak` >= 8 max|x|.  With windows of +-peak written
    into x, e = plane_exponent(peak) puts the peak at exactly 2^14; at e + 1 it sits at 2^15 (hi pattern 0x7800, the lowest that reports)
    and at e + 3 at 2^17 (clamped to 65504), while every other value stays at or under 2^14 -- the piece holding the peak is the only one
    that can raise the status word."""
    x = position_coded(case, seed)
    peak = float(2.0 ** int(np.frexp(np.float32(8.0 * np.abs(x).max()))[1]))
    assert 8.0 * float(np.abs(x).max()) <= peak
    return x, peak
