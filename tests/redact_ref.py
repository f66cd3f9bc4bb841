"""Numpy restatement of the redaction rule (DESIGN §8 "Redaction rule"), the comparand of tests/test_redact_*.py.  It follows the
rule as written -- the mask as the union of clipped boxes, the replacement computed for the WHOLE source frame and then selected by the
mask -- not the kernels (csrc/redact.hip).  Integers throughout: a frame has one right answer.

Detections are given as the kernel sees them: ``bbox`` (rows, 4) x1, y1, x2, y2, ``cls`` (rows,) class indices, ``n_dets`` live rows,
``table`` (num_classes,) non-zero where a class is redacted."""
import numpy as np

MODES = ("fill", "pixelate", "blur")
SIZES = {"fill": (0, 0, 0), "pixelate": (2, 64, 16), "blur": (1, 32, 12)}      # mode -> (smallest, largest, default) size


def mask(h, w, bbox, cls, n_dets, table, margin=0):
    """The (h, w) bool mask: pixel (x, y) lies in the clipped box of a live row of a redacted class."""
    m = np.zeros((h, w), dtype=bool)
    bbox = np.asarray(bbox).reshape(-1, 4)
    for r in range(int(n_dets)):
        c = int(cls[r])
        if not 0 <= c < len(table) or not table[c]:
            continue
        x1, y1, x2, y2 = [int(v) for v in bbox[r]]
        xa, xb = max(min(x1, x2) - margin, 0), min(max(x1, x2) + margin, w - 1)
        ya, yb = max(min(y1, y2) - margin, 0), min(max(y1, y2) + margin, h - 1)
        if xa > xb or ya > yb:
            continue
        m[ya:yb + 1, xa:xb + 1] = True                    # inclusive at both ends
    return m


def pixelated(frame, P):
    """R of mode pixelate: every pixel takes (sum of its cell + n // 2) // n; the grid is anchored at the origin, the last cells short."""
    h, w = frame.shape[:2]
    out = np.empty_like(frame)
    for y0 in range(0, h, P):
        for x0 in range(0, w, P):
            cell = frame[y0:y0 + P, x0:x0 + P].astype(np.int64)
            n = cell.shape[0] * cell.shape[1]
            out[y0:y0 + P, x0:x0 + P] = (cell.sum(axis=(0, 1)) + n // 2) // n
    return out


def _box_1d(a, r, axis):
    """(sum over d = -r..r of a at the index clamped to the axis + k // 2) // k, k = 2r + 1, rounded to uint8 as written."""
    n, k = a.shape[axis], 2 * r + 1
    acc = np.zeros(a.shape, dtype=np.int64)
    for d in range(-r, r + 1):
        acc += np.take(a, np.clip(np.arange(n) + d, 0, n - 1), axis=axis)
    return ((acc + k // 2) // k).astype(np.uint8)


def blurred(frame, r):
    """R of mode blur: H along x, then R along y, each stage rounded to uint8."""
    return _box_1d(_box_1d(np.asarray(frame, dtype=np.uint8), r, 1), r, 0)


def replacement(frame, mode, size=None):
    lo, hi, default = SIZES[mode]
    size = default if size is None else size
    assert lo <= size <= hi, (mode, size)
    if mode == "fill":
        return np.zeros_like(frame)
    return pixelated(frame, size) if mode == "pixelate" else blurred(frame, size)


def redact(frame, bbox, cls, n_dets, table, mode="pixelate", size=None, margin=0):
    """A copy of ``frame`` (h, w, 3) uint8 with the masked pixels replaced: out = masked ? R : S, R from the source alone."""
    frame = np.asarray(frame, dtype=np.uint8)
    m = mask(frame.shape[0], frame.shape[1], bbox, cls, n_dets, table, margin)
    out = frame.copy()
    out[m] = replacement(frame, mode, size)[m]
    return out


def redact_dets(frame, dets, class_mapping, classes, mode="pixelate", size=None, margin=0):
    """``redact`` over host dets (dicts with "bbox" and "cls_name"); ``classes``: names, or "all" = every class but "bg"."""
    C = max(class_mapping.values()) + 1
    table = np.zeros(C, dtype=np.uint8)
    for name, idx in class_mapping.items():
        table[idx] = (name != "bg") if classes == "all" else (name in classes)
    bbox = np.array([[int(v) for v in d["bbox"]] for d in dets], dtype=np.int64).reshape(-1, 4)
    cls = np.array([class_mapping[d["cls_name"]] for d in dets], dtype=np.int64)
    return redact(frame, bbox, cls, len(dets), table, mode, size, margin)
