"""The shape rule (DESIGN §8 "Shape rule", include/ext/frcnn_hip_redact_shape.h) restated in numpy / Python ints on top of
tests/redact_ref.py, which gives R: the comparand of tests/test_redact_shape_*.py.  It follows the rule as written -- per eligible row
the smallest e in 0..F at which the pixel lies inside the shape grown by e, the weight of that e, the maximum over the rows, the blend --
not the kernel (csrc/redact_shape.hip).  The ellipse test is evaluated as the rule states it, in Python ints where the products pass
2^62: they compare exactly at any size.

Detections are given as the kernel sees them (tests/redact_ref.py's docstring)."""
import numpy as np

from tests import redact_ref as R

SHAPES = ("box", "ellipse")
FEATHER_MAX = 32
MAX_SIDE = 131072                                         # a grown box with a larger side is a box row


def distance(h, w, box, margin=0, shape="box", feather=0):
    """(h, w) ints: e of every pixel for the row ``box`` = (x1, y1, x2, y2), ``feather`` + 1 where it lies beyond the feather."""
    F = int(feather)
    x1, y1, x2, y2 = [int(v) for v in box]
    X0, X1, Y0, Y1 = min(x1, x2) - margin, max(x1, x2) + margin, min(y1, y2) - margin, max(y1, y2) + margin      # NOT clipped
    A, B = X1 - X0 + 1, Y1 - Y0 + 1
    e = np.full((h, w), F + 1, dtype=np.int64)
    xa, xb, ya, yb = max(X0 - F, 0), min(X1 + F, w - 1), max(Y0 - F, 0), min(Y1 + F, h - 1)
    if xa > xb or ya > yb:
        return e                                          # no pixel of the frame within F of the grown box
    xs, ys = np.arange(xa, xb + 1), np.arange(ya, yb + 1)
    if shape == "box" or A > MAX_SIDE or B > MAX_SIDE:
        ex = np.array([max(X0 - int(x), int(x) - X1, 0) for x in xs], dtype=np.int64)
        ey = np.array([max(Y0 - int(y), int(y) - Y1, 0) for y in ys], dtype=np.int64)
        e[ya:yb + 1, xa:xb + 1] = np.minimum(np.maximum(ey[:, None], ex[None, :]), F + 1)
        return e
    assert shape == "ellipse", shape
    exact = (A + 2 * F) ** 2 * (B + 2 * F) ** 2 >= 1 << 61                  # Python ints (object arrays) where int64 would wrap
    u = np.array([2 * int(x) - (X0 + X1) for x in xs], dtype=object if exact else np.int64)[None, :]
    v = np.array([2 * int(y) - (Y0 + Y1) for y in ys], dtype=object if exact else np.int64)[:, None]
    part = e[ya:yb + 1, xa:xb + 1]
    for k in range(F, -1, -1):                            # downwards: what stays is the SMALLEST e at which the pixel is inside
        Ae2, Be2 = (A + 2 * k) ** 2, (B + 2 * k) ** 2
        inside = (u * u * Be2 + v * v * Ae2 <= Ae2 * Be2).astype(bool)
        part[inside] = k
    return e


def weight_of(e, feather):
    """W_r of the distances ``e``: 256 at 0, (256 (F + 1 - e)) // (F + 1) up to F, 0 beyond."""
    F = int(feather)
    e = np.asarray(e, dtype=np.int64)
    return np.where(e == 0, 256, np.where(e <= F, (256 * (F + 1 - e)) // (F + 1), 0))


def weights(h, w, bbox, cls, n_dets, table, margin=0, shape="box", feather=0):
    """The (h, w) weight W of every pixel: the maximum of W_r over the eligible rows (the Redaction rule's: live, of a redacted class)."""
    assert shape in SHAPES and 0 <= int(feather) <= FEATHER_MAX, (shape, feather)
    W = np.zeros((h, w), dtype=np.int64)
    bbox = np.asarray(bbox).reshape(-1, 4)
    for r in range(int(n_dets)):
        c = int(cls[r])
        if not 0 <= c < len(table) or not table[c]:
            continue
        W = np.maximum(W, weight_of(distance(h, w, bbox[r], margin, shape, feather), feather))
    return W


def redact(frame, bbox, cls, n_dets, table, mode="pixelate", size=None, margin=0, shape="box", feather=0):
    """A copy of ``frame`` (h, w, 3) uint8 with out = (W R + (256 - W) S + 128) >> 8 per byte, R from the source alone; W = 0 leaves S."""
    frame = np.asarray(frame, dtype=np.uint8)
    W = weights(frame.shape[0], frame.shape[1], bbox, cls, n_dets, table, margin, shape, feather)[:, :, None]
    S, Rep = frame.astype(np.int64), R.replacement(frame, mode, size).astype(np.int64)
    return np.where(W > 0, (W * Rep + (256 - W) * S + 128) >> 8, S).astype(np.uint8)


def redact_dets(frame, dets, class_mapping, classes, mode="pixelate", size=None, margin=0, shape="box", feather=0):
    """``redact`` over host dets (dicts with "bbox" and "cls_name"); ``classes``: names, or "all" = every class but "bg"."""
    C = max(class_mapping.values()) + 1
    table = np.zeros(C, dtype=np.uint8)
    for name, idx in class_mapping.items():
        table[idx] = (name != "bg") if classes == "all" else (name in classes)
    bbox = np.array([[int(v) for v in d["bbox"]] for d in dets], dtype=np.int64).reshape(-1, 4)
    cls = np.array([class_mapping[d["cls_name"]] for d in dets], dtype=np.int64)
    return redact(frame, bbox, cls, len(dets), table, mode, size, margin, shape, feather)
