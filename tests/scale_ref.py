"""The scale rule (DESIGN §8 "Scale rule", include/ext/frcnn_hip_scale.h) restated in numpy int64: what csrc/scale.hip must give, byte for
byte.  Written from the rule's text, not from the kernel: the full weight matrices, one matrix product per axis, one division."""
import numpy as np

MAX_RATIO = 16


def weights(n_out, n_in):
    """The (n_out, n_in) int64 matrix of overlaps of output pixel X and source pixel x on a line of n_in * n_out units:
    max(0, min((X + 1) n_in, (x + 1) n_out) - max(X n_in, x n_out))."""
    X = np.arange(n_out, dtype=np.int64)[:, None]
    x = np.arange(n_in, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((X + 1) * n_in, (x + 1) * n_out) - np.maximum(X * n_in, x * n_out))


def check_size(h, w, H, W):
    if not (1 <= H <= h and 1 <= W <= w and h <= MAX_RATIO * H and w <= MAX_RATIO * W):
        raise ValueError("scale rule: %dx%d -> %dx%d" % (h, w, H, W))


def downscale(frame, H, W):
    """``frame`` uint8 (h, w, 3) -> uint8 (H, W, 3): out = (sum_y sum_x ry cx S + (h w) // 2) // (h w)."""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.ndim == 3
    h, w = frame.shape[:2]
    check_size(h, w, H, W)
    ry, cx = weights(H, h), weights(W, w)
    num = np.einsum("Yy,Xx,yxc->YXc", ry, cx, frame.astype(np.int64), optimize=True)
    out = (num + (h * w) // 2) // (h * w)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def target(option, h, w):
    """The output size (H, W) of an option ("size", W, H) or ("scale", N) for a source of (h, w)."""
    if option[0] == "scale":
        N = option[1]
        return (h + N - 1) // N, (w + N - 1) // N
    return option[2], option[1]
