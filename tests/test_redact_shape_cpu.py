"""The shape rule on the host: what follows from tests/redact_shape_ref.py's restatement, one hand-worked frame, annotate_video's
arguments and their refusals, the pass keys, and the header against the binding.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import redact_ref as R
from tests import redact_shape_ref as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = np.array([1, 0, 1], dtype=np.uint8)                                # class 1 is not redacted


def noise(h, w, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def some_rows(h, w, seed):
    """Boxes inside, across and outside the frame, inverted corners, a class that is not redacted and one out of range."""
    rs = np.random.RandomState(seed)
    x, y = rs.randint(-6, w + 6, 12), rs.randint(-6, h + 6, 12)
    bbox = np.stack([x, y, x + rs.randint(-4, 14, 12), y + rs.randint(-4, 9, 12)], axis=1)
    cls = np.array([0, 2, 1, 0, 2, 7, 0, 2, -1, 0, 2, 0])
    return bbox, cls


# ------------------------------------------------------------------------------------------------------------ the identities
@pytest.mark.parametrize("mode,size", [("fill", 0), ("pixelate", 5), ("blur", 3)])
@pytest.mark.parametrize("margin", [0, 3])
def test_box_without_feather_is_the_redaction_rule(mode, size, margin):
    h, w = 23, 31
    frame = noise(h, w, 1)
    bbox, cls = some_rows(h, w, 2)
    want = R.redact(frame, bbox, cls, len(cls), TABLE, mode, size, margin)
    assert np.array_equal(RS.redact(frame, bbox, cls, len(cls), TABLE, mode, size, margin, "box", 0), want)
    assert (want != frame).any()
    W = RS.weights(h, w, bbox, cls, len(cls), TABLE, margin, "box", 0)
    assert np.array_equal(W == 256, R.mask(h, w, bbox, cls, len(cls), TABLE, margin)) and set(np.unique(W)) <= {0, 256}


@pytest.mark.parametrize("F", [0, 1, 5, 32])
def test_the_ellipse_hides_a_subset_of_the_box(F):
    h, w = 23, 31
    bbox, cls = some_rows(h, w, 3)
    for margin in (0, 3):
        Wb = RS.weights(h, w, bbox, cls, len(cls), TABLE, margin, "box", F)
        We = RS.weights(h, w, bbox, cls, len(cls), TABLE, margin, "ellipse", F)
        assert (We <= Wb).all() and (We > 0).any() and (We < Wb).any()
        # the same row by row, on the distances themselves
        for box in bbox:
            assert (RS.distance(h, w, box, margin, "ellipse", F) >= RS.distance(h, w, box, margin, "box", F)).all()


@pytest.mark.parametrize("shape", RS.SHAPES)
def test_the_weight_never_falls_when_the_feather_grows(shape):
    h, w = 23, 31
    bbox, cls = some_rows(h, w, 4)
    last = None
    for F in range(0, 33):
        W = RS.weights(h, w, bbox, cls, len(cls), TABLE, 1, shape, F)
        if last is not None:
            assert (W >= last).all(), F
            assert np.array_equal(W == 256, last == 256)                   # the feather goes OUTWARDS: the hard shape is what it was
        last = W
    assert (last > 0).sum() > (RS.weights(h, w, bbox, cls, len(cls), TABLE, 1, shape, 0) > 0).sum()


def test_a_shape_across_the_border_is_the_shape_of_the_whole_box():
    """The grown box is not clipped: the ellipse of a box half outside the frame is cut by the border, not squeezed into the frame."""
    h, w = 12, 12
    inside = RS.weights(h + 10, w + 10, [[5 + 1, 5 + 3, 5 + 9, 5 + 8]], [0], 1, TABLE, 0, "ellipse", 3)
    shifted = RS.weights(h + 10, w + 10, [[-4 + 5, 5 + 3, 4 + 5, 5 + 8]], [0], 1, TABLE, 0, "ellipse", 3)
    across = RS.weights(h, w, [[-4, 3, 4, 8]], [0], 1, TABLE, 0, "ellipse", 3)
    assert np.array_equal(inside[:, 5:], shifted[:, :-5])                  # (the rule moves with the box)
    assert np.array_equal(across, shifted[5:5 + h, 5:5 + w]) and (across[:, 0] == 256).any()
    # a box wholly outside the frame: only its ring reaches in
    ring = RS.weights(h, w, [[-9, 2, -2, 9]], [0], 1, TABLE, 0, "box", 4)
    assert ring.max() == (256 * 3) // 5 and (ring[:, 3:] == 0).all() and (ring[2:10, 0] == (256 * 3) // 5).all()


def test_a_side_above_the_limit_is_a_box_row_and_large_ellipses_compare_exactly():
    h, w = 9, 11
    big = [[-70000, -3, 70000, 4]]                                          # A = 140 001 > 131 072
    assert np.array_equal(RS.weights(h, w, big, [0], 1, TABLE, 0, "ellipse", 2), RS.weights(h, w, big, [0], 1, TABLE, 0, "box", 2))
    # A = B = 98 001: a circle of radius 49 000.5 about (34 654, 34 653), whose edge crosses the frame on its diagonal (49 001.5 /
    # sqrt(2) = 34 649.3 from the frame's middle): (A + 2e)^2 (B + 2e)^2 is about 2^66
    box = [-14346, -14347, -14346 + 98000, -14347 + 98000]
    e = RS.distance(h, w, box, 0, "ellipse", 2)
    assert len(np.unique(e)) == 4                                           # inside, e = 1, e = 2 and beyond, all inside one small frame
    X0, Y0, A = box[0], box[1], 98001
    for y in range(h):
        for x in range(w):
            u, v = 2 * x - (2 * X0 + A - 1), 2 * y - (2 * Y0 + A - 1)
            want = next((k for k in range(3) if (u * u + v * v) * (A + 2 * k) ** 2 <= (A + 2 * k) ** 4), 3)      # a circle: A = B
            assert e[y, x] == want, (x, y)


def test_the_max_rule_and_the_blend():
    h, w = 7, 20
    frame = noise(h, w, 5)
    bbox, cls = [[2, 2, 6, 4], [9, 1, 9, 5]], [0, 2]
    W = RS.weights(h, w, bbox, cls, 2, TABLE, 0, "box", 3)
    both = np.maximum(RS.weights(h, w, bbox[:1], cls[:1], 1, TABLE, 0, "box", 3), RS.weights(h, w, bbox[1:], cls[1:], 1, TABLE, 0, "box", 3))
    assert np.array_equal(W, both) and W[3, 8] == 192 and W[3, 7] == 192   # x = 8: 1 from the second box beats 2 from the first
    out = RS.redact(frame, bbox, cls, 2, TABLE, "blur", 2, 0, "box", 3)
    Rep = R.blurred(frame, 2).astype(np.int64)
    assert np.array_equal(out[W == 256], Rep[W == 256].astype(np.uint8)) and np.array_equal(out[W == 0], frame[W == 0])
    assert out[3, 8, 1] == (192 * Rep[3, 8, 1] + 64 * int(frame[3, 8, 1]) + 128) >> 8


# ------------------------------------------------------------------------------------------------------------ by hand
def test_literal_9x9_ellipse_feather_2_fill():
    """A 5 x 3 box at x 2..6, y 3..5: u = 2x - 8, v = 2y - 8.
    e = 0 (A, B = 5, 3):  9 u^2 + 25 v^2 <= 225:    v = 0: |u| <= 5 -> x 2..6;  |v| = 2: u^2 <= 13 -> x 3..5
    e = 1 (7, 5):        25 u^2 + 49 v^2 <= 1225:   v = 0: |u| <= 7 -> x 1..7;  |v| = 2: u^2 <= 41 -> x 1..7;  |v| = 4: u^2 <= 17 -> x 2..6
    e = 2 (9, 7):        49 u^2 + 81 v^2 <= 3969:   v = 0, |v| = 2: u^2 <= 81, 74 -> x 0..8;  |v| = 4: u^2 <= 54 -> x 1..7;
                                                    |v| = 6: u^2 <= 21 -> x 2..6;  |v| = 8: 81 * 64 > 3969 -> none
    W: 256 at e = 0, (256 * 2) // 3 = 170 at e = 1, 256 // 3 = 85 at e = 2."""
    want = np.array([[0, 0, 0, 0, 0, 0, 0, 0, 0],
                     [0, 0, 85, 85, 85, 85, 85, 0, 0],
                     [0, 85, 170, 170, 170, 170, 170, 85, 0],
                     [85, 170, 170, 256, 256, 256, 170, 170, 85],
                     [85, 170, 256, 256, 256, 256, 256, 170, 85],
                     [85, 170, 170, 256, 256, 256, 170, 170, 85],
                     [0, 85, 170, 170, 170, 170, 170, 85, 0],
                     [0, 0, 85, 85, 85, 85, 85, 0, 0],
                     [0, 0, 0, 0, 0, 0, 0, 0, 0]])
    W = RS.weights(9, 9, [[2, 3, 6, 5]], [0], 1, TABLE, 0, "ellipse", 2)
    assert np.array_equal(W, want)
    assert np.array_equal(RS.weights(9, 9, [[6, 5, 2, 3]], [0], 1, TABLE, 0, "ellipse", 2), want)          # inverted corners
    assert np.array_equal(RS.weights(9, 9, [[3, 4, 5, 4]], [0], 1, TABLE, 1, "ellipse", 2), want)          # the same box, by the margin
    frame = np.full((9, 9, 3), 200, dtype=np.uint8)
    out = RS.redact(frame, [[2, 3, 6, 5]], [0], 1, TABLE, "fill", 0, 0, "ellipse", 2)
    # fill: R = 0, out = ((256 - W) * 200 + 128) >> 8: 200, (171 * 200 + 128) >> 8 = 134, (86 * 200 + 128) >> 8 = 67, 0
    shade = {0: 200, 85: 134, 170: 67, 256: 0}
    assert all(np.array_equal(out[:, :, c], np.vectorize(shade.get)(want)) for c in range(3))


# ------------------------------------------------------------------------------------------------------------ the command line
def _args(*argv):
    from faster_rcnn_amd import annotate_video
    return annotate_video.build_parser().parse_args(["rpn.npz", "det.npz", "frames"] + list(argv))


def test_redact_shape_from_args():
    from faster_rcnn_amd.annotate_video import redact_from_args, redact_shape_from_args
    from faster_rcnn_amd.data.voc_data_helpers import VOC_CLASS_MAPPING
    a = _args()
    assert (a.redact_shape, a.redact_feather) == (None, None) and redact_shape_from_args(a) is None
    assert redact_shape_from_args(_args("--redact", "all")) is None
    assert redact_shape_from_args(_args("--redact", "all", "--redact_shape", "ellipse")) == ("ellipse", 0)
    assert redact_shape_from_args(_args("--redact", "person", "--redact_feather", "8")) == ("box", 8)
    assert redact_shape_from_args(_args("--redact", "all", "--redact_shape", "ellipse", "--redact_feather", "32")) == ("ellipse", 32)
    # the default stated in full is the default: the plain redaction, its pass and its key
    assert redact_shape_from_args(_args("--redact", "all", "--redact_shape", "box", "--redact_feather", "0")) is None
    assert redact_from_args(_args("--redact", "all", "--redact_shape", "ellipse"), VOC_CLASS_MAPPING) == ("all", "pixelate", 16, 0)
    for extra in (("--redact_shape", "ellipse"), ("--redact_shape", "box"), ("--redact_feather", "4"), ("--redact_feather", "0")):
        with pytest.raises(ValueError) as e:
            redact_shape_from_args(_args(*extra))
        assert extra[0] in str(e.value) and "--redact CLASSES" in str(e.value)
    for feather in ("-1", "33", "1000"):
        with pytest.raises(ValueError) as e:
            redact_shape_from_args(_args("--redact", "all", "--redact_feather", feather))
        assert "0..32" in str(e.value)
    with pytest.raises(SystemExit):
        _args("--redact", "all", "--redact_shape", "circle")              # (argparse's choices)


def test_redact_shape_option():
    from faster_rcnn_amd import _lib, ops
    assert ops.REDACT_SHAPES == RS.SHAPES == ("box", "ellipse") and ops.REDACT_FEATHER == (0, RS.FEATHER_MAX) == (0, 32)
    assert ops.redact_shape_option() == ("box", 0) and ops.redact_shape_option("ellipse", None) == ("ellipse", 0)
    assert ops.redact_shape_option(None, np.int64(7)) == ("box", 7) and ops.redact_shape_option("ellipse", 32) == ("ellipse", 32)
    for shape, feather, word in (("circle", 0, "shape"), (1, 0, "shape"), ("box", -1, "feather"), ("box", 33, "feather"), ("ellipse", 2.0, "feather"),
                                 ("ellipse", True, "feather"), ("box", "4", "feather")):
        with pytest.raises(ValueError) as e:
            ops.redact_shape_option(shape, feather)
        assert word in str(e.value)
    assert _lib.REDACT_SHAPES == {"box": 0, "ellipse": 1}


def test_the_keyword_is_refused_by_name_without_a_device():
    from faster_rcnn_amd import annotate_video
    frame = noise(8, 8)
    for bad, word in ((("ellipse", 4), "redact="),):
        with pytest.raises(ValueError) as e:
            annotate_video.draw_eager(frame, [], {"bg": 0, "car": 1}, redact=None, redact_shape=bad)
        assert word in str(e.value)
    for bad in (("circle", 0), ("box", 33), ("ellipse",), "ellipse"):
        with pytest.raises(ValueError):
            annotate_video.draw_eager(frame, [], {"bg": 0, "car": 1}, redact=("all", "fill", 0, 0), redact_shape=bad)


# ------------------------------------------------------------------------------------------------------------ the pass key
class _Engine:
    """What PassSpec.checked asks of an engine for these options, from the real one's methods."""
    batch, device_preprocess = 4, True

    def class_names(self):
        return ["bg", "car", "person"]

    def __getattr__(self, name):
        import inspect
        from faster_rcnn_amd import entry
        return inspect.getattr_static(entry.DetectionEntry, name).__get__(self, type(self))       # (static methods stay static)


def test_pass_keys():
    from faster_rcnn_amd import entry
    from faster_rcnn_amd._lib import FrcnnError
    eng = _Engine()
    redact = ("all", "blur", 3, 2)
    plain = entry.PassSpec.checked(eng, 4, annotate=True, redact=redact)
    today = (4, "annotate", "redact", "all", "blur", 3, 2)
    assert plain.redact_shape is None and plain.key_tail(4) == today
    for same in (None, ("box", 0), ("box", None), (None, None), (None, 0)):
        spec = entry.PassSpec.checked(eng, 4, annotate=True, redact=redact, redact_shape=same)
        assert spec == plain and spec.key_tail(4) == today, same
    shaped = entry.PassSpec.checked(eng, 4, annotate=True, redact=redact, redact_shape=("ellipse", 4))
    assert shaped.redact_shape == ("ellipse", 4) and shaped.key_tail(4) == today + ("shape", "ellipse", 4)
    assert entry.PassSpec.checked(eng, 4, annotate=True, redact=redact, redact_shape=("box", 1)).key_tail(4) == today + ("shape", "box", 1)
    # the tag stands directly behind the redaction's, in front of every later option's
    full = entry.PassSpec.checked(eng, 1, annotate=True, redact=redact, redact_shape=("ellipse", 4), draw=False, track=(30, 8, 0))
    assert full.key_tail(1) == ("annotate", "redact", "all", "blur", 3, 2, "shape", "ellipse", 4, "nodraw", "track", 30, 8, 0)
    # a spec without the option: every key is today's
    assert entry.PassSpec(annotate=True).key_tail(1) == ("annotate",) and entry.PassSpec().redact_shape is None
    for kw, word in ((dict(annotate=True, redact_shape=("ellipse", 4)), "redact="), (dict(annotate=True, redact=redact, redact_shape=("circle", 0)), "shape"),
                     (dict(annotate=True, redact=redact, redact_shape=("box", 33)), "feather"),
                     (dict(annotate=True, redact=redact, redact_shape=("ellipse", -1)), "feather"),
                     (dict(annotate=True, redact=redact, redact_shape="ellipse"), "(shape, feather)"),
                     (dict(annotate=True, redact=redact, redact_shape=("ellipse", 1, 2)), "(shape, feather)")):
        with pytest.raises(FrcnnError) as e:
            entry.PassSpec.checked(eng, 4, **kw)
        assert word in str(e.value), kw


# ------------------------------------------------------------------------------------------------------------ header and binding
def test_header_binding_and_library_agree():
    from faster_rcnn_amd import _lib
    from faster_rcnn_amd.build import build_library
    ext = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_redact_shape.h")).read()
    version = int(re.search(r"#define FRCNN_REDACT_SHAPE_VERSION (\d+)", ext).group(1))
    assert version == _lib.REDACT_SHAPE_VERSION == 1 and re.search(r"^ \*   1 = ", ext, flags=re.M)
    define = lambda k: int(re.search(r"#define FRCNN_REDACT_%s (\d+)" % k, ext).group(1))
    assert {"box": define("SHAPE_BOX"), "ellipse": define("SHAPE_ELLIPSE")} == _lib.REDACT_SHAPES
    assert (0, define("FEATHER_MAX")) == _lib.REDACT_FEATHER == (0, RS.FEATHER_MAX) and define("SHAPE_MAX_SIDE") == RS.MAX_SIDE == 131072
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    names = sorted(set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", code)))
    assert names == sorted(_lib.REDACT_SHAPE_SIGNATURES) == ["frcnn_redact_shape_version", "frcnn_redact_shaped_u8"]
    build_library(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        m = re.search(r"\bint %s\s*\(([^)]*)\)" % name, code)
        assert m, name
        decls = [d for d in m.group(1).split(",") if d.strip() != "void"]
        restype, argtypes = _lib.REDACT_SHAPE_SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(decls), name
        for decl, ct in zip(decls, argtypes):
            assert ("*" in decl) == (ct is ctypes.c_void_p), (name, decl)
            assert ("size_t" in decl) == (ct is ctypes.c_size_t), (name, decl)
        assert hasattr(lib, name), name
    # the core header and the other extensions do not know the new symbols, and no revision but the new one moved
    core = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    ext_dir = os.path.join(ROOT, "include", "ext")
    others = "".join(open(os.path.join(ext_dir, f)).read() for f in sorted(os.listdir(ext_dir)) if f != "frcnn_hip_redact_shape.h")
    assert not any(n in core or n in others for n in names)
    loaded = _lib.load()
    assert loaded.frcnn_redact_shape_version() == version and loaded.frcnn_redact_version() == _lib.REDACT_VERSION == 1
    assert loaded.frcnn_version() == _lib.ABI_VERSION == int(re.search(r"#define FRCNN_ABI_VERSION (\d+)", core).group(1))
    assert "frcnn_hip_redact_shape.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # the argument checks run on the host, in front of any device call: refused without a GPU too
    assert loaded.frcnn_redact_shaped_u8(None, 8, 8, None, None, None, 1, None, 1, 0, 0, 0, 0, 0, None, 0, None) == -1
    assert b"redact_shaped_u8: null pointer" in loaded.frcnn_last_error()
