"""The region rule (DESIGN §8 "Region rule", include/ext/frcnn_hip_redact_region.h) restated in numpy integers on top of
tests/zone_ref.py, which gives INSIDE, tests/redact_ref.py, which gives R, and tests/redact_shape_ref.py, which gives the weight of a
distance: the comparand of tests/test_redact_region_*.py.  It follows the rule as written -- the hard set over the domain padded by F,
d1 along the rows, e across them, the weight, the blend -- not the kernels (csrc/redact_region.hip).

    regions   polygons of (x, y), 0..8 of them, the Zone rule's grammar
    mask      None or (h, w) uint8: >= 128 is hard
"""
import numpy as np

from tests import redact_ref as R
from tests import redact_shape_ref as S
from tests import zone_ref as Z

MAX_REGIONS = 8
FEATHER_MAX = 32
DEFAULT_MODE = "fill"


def hard_set(h, w, regions, mask, feather):
    """(h + 2F, w + 2F) bool: HARD of the point (x, y) at [y + F][x + F].  INSIDE compares differences of coordinates only, so the
    polygon moved by (F, F) over a domain that starts at 0 is the polygon itself over the domain that starts at -F."""
    F = int(feather)
    assert 0 <= F <= FEATHER_MAX and len(regions) <= MAX_REGIONS and (len(regions) or mask is not None)
    hard = np.zeros((h + 2 * F, w + 2 * F), dtype=bool)
    for poly in regions:
        hard |= Z.inside_mask([(int(x) + F, int(y) + F) for x, y in poly], h + 2 * F, w + 2 * F)
    if mask is not None:
        mask = np.asarray(mask)
        assert mask.shape == (h, w) and mask.dtype == np.uint8
        hard[F:F + h, F:F + w] |= mask >= 128
    return hard


def distance(h, w, regions, mask, feather):
    """(h, w) ints: e of every pixel, F + 1 beyond the feather: d1 along the padded rows, then the min over |y - y'| <= F."""
    F = int(feather)
    hard = hard_set(h, w, regions, mask, F)
    d1 = np.full((h + 2 * F, w), F + 1, dtype=np.int64)                     # d1(x, y') at [y' + F][x]
    for dx in range(F, -1, -1):                                             # downwards: what stays is the smallest |x - x'|
        near = hard[:, F - dx:F - dx + w] | hard[:, F + dx:F + dx + w]
        d1[near] = dx
    e = np.full((h, w), F + 1, dtype=np.int64)
    for dy in range(-F, F + 1):
        e = np.minimum(e, np.maximum(d1[F + dy:F + dy + h], abs(dy)))
    return e


def weights(h, w, regions, mask=None, feather=0):
    """The (h, w) weight W of every pixel: the Shape rule's weight of e."""
    return S.weight_of(distance(h, w, regions, mask, feather), feather)


def stats(W):
    """(covered, full) of a weight plane."""
    W = np.asarray(W)
    return int((W > 0).sum()), int((W == 256).sum())


def apply(current, source, regions, mask=None, mode=DEFAULT_MODE, size=None, feather=0):
    """A copy of ``current`` (h, w, 3) uint8 -- the frame as the steps in front left it -- with out = (W R + (256 - W) C + 128) >> 8 per
    byte, R from ``source``, the untouched frame, alone; W = 0 leaves C."""
    current, source = np.asarray(current, dtype=np.uint8), np.asarray(source, dtype=np.uint8)
    assert current.shape == source.shape
    W = weights(source.shape[0], source.shape[1], regions, mask, feather)[:, :, None]
    C, Rep = current.astype(np.int64), R.replacement(source, mode, size).astype(np.int64)
    return np.where(W > 0, (W * Rep + (256 - W) * C + 128) >> 8, C).astype(np.uint8)


def redact(frame, regions, mask=None, mode=DEFAULT_MODE, size=None, feather=0):
    """``apply`` on an untouched frame."""
    return apply(frame, frame, regions, mask, mode, size, feather)


def box_polygon(x0, y0, x1, y1):
    """The polygon whose hard set is the box (x0, y0, x1, y1), inclusive on all four sides: a polygon owns its left and top boundary."""
    return [(x0, y0), (x1 + 1, y0), (x1 + 1, y1 + 1), (x0, y1 + 1)]


def summary_line(w, h, regions, mask, W):
    """The line printed per frame size at the end of a list."""
    what = (["%d region%s" % (len(regions), "" if len(regions) == 1 else "s")] if regions else []) + (["mask"] if mask is not None else [])
    return "redact regions %dx%d: %s, %.1f %% of the frame hidden" % (w, h, " + ".join(what), 100.0 * stats(W)[0] / (w * h))
