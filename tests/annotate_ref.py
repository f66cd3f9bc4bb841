"""Numpy restatement of the annotation drawing rule, the comparand of tests/test_annotate_*.py.  It follows the
rule as written -- the box as two inequalities per edge, labels formatted by Python's own ``format`` -- not the kernel."""
import numpy as np

SKIP = ("DontCare", "Misc")                       # the reference's annotate_video.py:33-34
GREEN = np.array([0, 255, 0], dtype=np.uint8)


def is_drawn(det, width, height):
    if det["cls_name"] in SKIP:
        return False
    x1, y1, x2, y2 = [int(v) for v in det["bbox"]]
    return not (x1 < 0 or x2 > width or y1 < 0 or y2 > height)


def label_text(det):
    return "{} {:6.2f}".format(det["cls_name"], det["prob"])


def paint_mask(height, width, dets, glyphs):
    """The (height, width) bool mask of the pixels the rule paints for these dets."""
    mask = np.zeros((height, width), dtype=bool)
    for det in dets:
        if not is_drawn(det, width, height):
            continue
        x1, y1, x2, y2 = [int(v) for v in det["bbox"]]
        xa, xb, ya, yb = min(x1, x2), max(x1, x2), min(y1, y2), max(y1, y2)
        # the box, h = 1: evaluated over its bounding window (clipped), outside of which neither inequality holds
        r0, r1 = max(0, ya - 1), min(height - 1, yb + 1)
        c0, c1 = max(0, xa - 1), min(width - 1, xb + 1)
        if r0 <= r1 and c0 <= c1:
            y = np.arange(r0, r1 + 1)[:, None]
            x = np.arange(c0, c1 + 1)[None, :]
            horiz = (xa - 1 <= x) & (x <= xb + 1) & ((np.abs(y - ya) <= 1) | (np.abs(y - yb) <= 1))
            vert = (ya - 1 <= y) & (y <= yb + 1) & ((np.abs(x - xa) <= 1) | (np.abs(x - xb) <= 1))
            mask[r0:r1 + 1, c0:c1 + 1] |= horiz | vert
        # the label at (x1, y2 + 16), 5x7 glyphs at scale 2, advance 12
        ox, oy = x1, y2 + 16
        for k, code in enumerate(label_text(det).encode("ascii", "replace")):
            if not 0x20 <= code <= 0x7E:
                code = ord("?")
            rows = glyphs[code - 0x20]
            for r in range(7):
                for c in range(5):
                    if (int(rows[r]) >> (4 - c)) & 1:
                        bx, by = ox + 12 * k + 2 * c, oy - 13 + 2 * r
                        xs0, xs1 = max(0, bx), min(width, bx + 2)
                        ys0, ys1 = max(0, by), min(height, by + 2)
                        if xs0 < xs1 and ys0 < ys1:
                            mask[ys0:ys1, xs0:xs1] = True
    return mask


def annotate(frame, dets, glyphs=None):
    """A copy of ``frame`` (h, w, 3) uint8 with the rule's pixels set to (0,255,0)."""
    if glyphs is None:
        from faster_rcnn_amd.annotate_font import GLYPHS as glyphs
    out = np.array(frame, dtype=np.uint8, copy=True)
    out[paint_mask(out.shape[0], out.shape[1], dets, glyphs)] = GREEN
    return out
