"""The region rule on the host: what follows from tests/redact_region_ref.py's restatement -- the two identities against the Redaction
rule and the Shape rule among them --, one hand-worked plane, the option, annotate_video's arguments and their refusals, the pass keys,
the blackened plate picture, and the header against the binding.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import redact_ref as R
from tests import redact_region_ref as RR
from tests import redact_shape_ref as RS
from tests import zone_ref as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = np.array([1], dtype=np.uint8)
TRIANGLE = [(3, 2), (27, 9), (8, 20)]
BOXES = [(4, 3, 12, 9), (-5, -4, 6, 5), (20, 15, 40, 30), (-3, 6, 33, 8), (5, -2, 7, 25), (-9, -9, 50, 50), (10, 10, 10, 10)]


def noise(h, w, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------ the identities
@pytest.mark.parametrize("mode,size", [("fill", 0), ("pixelate", 5), ("blur", 3)])
def test_a_box_polygon_without_feather_is_the_redaction_rule(mode, size):
    h, w = 23, 31
    frame = noise(h, w, 1)
    for box in BOXES:                                                       # inside, across every border, larger than the frame, one pixel
        want = R.redact(frame, [box], [0], 1, TABLE, mode, size, 0)
        assert np.array_equal(RR.redact(frame, [RR.box_polygon(*box)], None, mode, size, 0), want), box
        assert (want != frame).any()


@pytest.mark.parametrize("F", [1, 8, 32])
@pytest.mark.parametrize("mode,size", [("fill", 0), ("pixelate", 5), ("blur", 3)])
def test_a_box_polygon_with_feather_is_the_shape_rule(mode, size, F):
    h, w = 23, 31
    frame = noise(h, w, 2)
    for box in BOXES:
        want = RS.redact(frame, [box], [0], 1, TABLE, mode, size, 0, "box", F)
        assert np.array_equal(RR.weights(h, w, [RR.box_polygon(*box)], None, F), RS.weights(h, w, [box], [0], 1, TABLE, 0, "box", F)), box
        assert np.array_equal(RR.redact(frame, [RR.box_polygon(*box)], None, mode, size, F), want), box
    # a box wholly outside the frame: only its ring reaches in, as the unclipped box's does
    ring = RR.weights(12, 12, [RR.box_polygon(-9, 2, -2, 9)], None, 4)
    assert ring.max() == (256 * 3) // 5 and (ring[:, 3:] == 0).all() and (ring[2:10, 0] == (256 * 3) // 5).all()


def test_the_weight_never_falls_when_the_feather_grows():
    h, w = 23, 31
    mask = np.zeros((h, w), dtype=np.uint8)
    mask[18:21, 25:] = 200
    mask[0, 0] = 127                                                        # under the threshold: not hard
    last = None
    for F in range(0, 33):
        W = RR.weights(h, w, [TRIANGLE, Z.BOW], mask, F)
        if last is not None:
            assert (W >= last).all(), F
            assert np.array_equal(W == 256, last == 256)                   # the feather goes OUTWARDS: the hard set is what it was
        last = W
    assert (last > 0).sum() > (RR.weights(h, w, [TRIANGLE, Z.BOW], mask, 0) > 0).sum()
    assert RR.weights(h, w, [TRIANGLE], mask, 0)[0, 0] == 0 and RR.weights(h, w, [], mask, 0)[19, 30] == 256


def test_a_plane_with_no_hard_point_writes_no_byte():
    h, w = 9, 14
    frame, touched = noise(h, w, 3), noise(h, w, 4)
    far = [(200, 200), (230, 200), (215, 230)]
    for F in (0, 32):
        assert not RR.weights(h, w, [far], np.zeros((h, w), dtype=np.uint8), F).any()
        assert np.array_equal(RR.apply(touched, frame, [far], None, "blur", 2, F), touched)


def test_shared_edges_are_hidden_exactly_once_and_the_blend_reads_the_source():
    h, w = 32, 40
    a, b = Z.inside_mask(Z.A, h, w), Z.inside_mask(Z.B, h, w)
    assert not (a & b).any() and (a | b)[10:20, 10:30].all() and (a | b).sum() == 200          # no gap, no overlap
    assert np.array_equal(RR.weights(h, w, [Z.A, Z.B], None, 0) == 256, a | b)
    source, current = noise(h, w, 5), noise(h, w, 6)
    W = RR.weights(h, w, [Z.A], None, 3)
    out = RR.apply(current, source, [Z.A], None, "blur", 2, 3)
    Rep = R.blurred(source, 2).astype(np.int64)
    assert np.array_equal(out[W == 256], Rep[W == 256].astype(np.uint8)) and np.array_equal(out[W == 0], current[W == 0])
    assert W[15, 8] == 128 and out[15, 8, 1] == (128 * Rep[15, 8, 1] + 128 * int(current[15, 8, 1]) + 128) >> 8


def test_literal_7x9_triangle_and_mask_feather_1():
    """The triangle (1, 1), (5, 1), (1, 5): a row y in 1..4 is inside for 1 <= x < 6 - y (the slanted edge is a right edge: not owned),
    row 5 is the bottom vertex: not owned.  The mask adds (7, 5).  F = 1: every pixel with a hard neighbour (Chebyshev) gets 128."""
    hard = np.zeros((7, 9), dtype=bool)
    for y in range(1, 5):
        hard[y, 1:6 - y] = True
    mask = np.zeros((7, 9), dtype=np.uint8)
    mask[5, 7] = 128
    assert np.array_equal(RR.hard_set(7, 9, [[(1, 1), (5, 1), (1, 5)]], None, 0), hard)
    hard[5, 7] = True
    want = np.zeros((7, 9), dtype=np.int64)
    for y in range(7):
        for x in range(9):
            near = hard[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].any()
            want[y, x] = 256 if hard[y, x] else 128 if near else 0
    W = RR.weights(7, 9, [[(1, 1), (5, 1), (1, 5)]], mask, 1)
    assert np.array_equal(W, want) and RR.stats(W) == (int((want > 0).sum()), 11)
    frame = np.full((7, 9, 3), 200, dtype=np.uint8)
    out = RR.redact(frame, [[(1, 1), (5, 1), (1, 5)]], mask, "fill", 0, 1)
    shade = {0: 200, 128: 100, 256: 0}                                      # (128 * 200 + 128) >> 8 = 100
    assert all(np.array_equal(out[:, :, c], np.vectorize(shade.get)(want)) for c in range(3))


# ------------------------------------------------------------------------------------------------------------ the option
def test_redact_region_option():
    from faster_rcnn_amd import _lib, ops
    assert ops.REDACT_REGION_MAX == RR.MAX_REGIONS == 8 and ops.REDACT_REGION_FEATHER == (0, RR.FEATHER_MAX) == (0, 32)
    tri = tuple(TRIANGLE)
    assert ops.redact_region_option([TRIANGLE]) == ((tri,), None, "fill", 0, 0)
    assert ops.redact_region_option(TRIANGLE, None, "blur", None, 8) == ((tri,), None, "blur", 12, 8)      # one polygon alone
    assert ops.redact_region_option([(3, 2, 27, 9, 8, 20)], None, "pixelate", 4, np.int64(2)) == ((tri,), None, "pixelate", 4, 2)
    mask = np.zeros((5, 7), dtype=np.uint8)
    mask[2, 3] = 255
    regions, m, mode, size, feather = ops.redact_region_option(None, mask, None, None, None)
    assert regions == () and isinstance(m, ops.RegionMask) and m.shape == (5, 7) and (mode, size, feather) == ("fill", 0, 0)
    assert np.array_equal(m.array, mask) and not m.array.flags.writeable
    mask[0, 0] = 255                                                        # (the option holds a copy)
    assert m.array[0, 0] == 0 and m == ops.RegionMask(m.array) and m != ops.RegionMask(mask) and hash(m) == hash(ops.RegionMask(m.array))
    assert ops.redact_region_option([], np.ones((2, 2), dtype=bool))[1].array.tolist() == [[255, 255], [255, 255]]
    assert ops.redact_region_key(ops.redact_region_option(TRIANGLE, m)) == ((tri,), m.digest, "fill", 0, 0)
    assert ops.redact_region_key(ops.redact_region_option(TRIANGLE))[1] is None
    eight = [[(10 * k, 0), (10 * k + 5, 0), (10 * k, 5)] for k in range(8)]
    assert len(ops.redact_region_option(eight)[0]) == 8
    for kw, word in ((dict(), "neither"), (dict(regions=[]), "neither"), (dict(regions=eight + [TRIANGLE]), "1..8"),
                     (dict(regions=[[(0, 0), (1, 1)]]), "vertices"), (dict(regions=[[(0, 0), (0, 0), (1, 1)]]), "consecutive"),
                     (dict(regions=[[(0, 0), (70000, 0), (1, 1)]]), "-32768..65535"), (dict(regions=[(0, 0, 1, 1, 2)]), "odd"),
                     (dict(regions=7), "polygons"), (dict(regions=TRIANGLE, mode="smear"), "mode"), (dict(regions=TRIANGLE, mode=2), "mode"),
                     (dict(regions=TRIANGLE, size=3), "size"), (dict(regions=TRIANGLE, mode="blur", size=33), "size"),
                     (dict(regions=TRIANGLE, mode="pixelate", size=1), "size"), (dict(regions=TRIANGLE, feather=33), "feather"),
                     (dict(regions=TRIANGLE, feather=-1), "feather"), (dict(regions=TRIANGLE, feather=2.0), "feather"),
                     (dict(regions=TRIANGLE, feather=True), "feather"), (dict(mask=np.zeros((2, 2, 3), dtype=np.uint8)), "mask"),
                     (dict(mask=np.zeros((2, 2), dtype=np.float32)), "mask"), (dict(mask=np.zeros((0, 4), dtype=np.uint8)), "mask")):
        with pytest.raises(ValueError) as e:
            ops.redact_region_option(**kw)
        assert word in str(e.value) and "region" in str(e.value), (kw, str(e.value))
    assert "zone" not in str(pytest.raises(ValueError, ops.redact_region_option, [[(0, 0), (1, 1)]]).value)
    assert _lib.REDACT_REGION_MAX == 8 and _lib.REDACT_REGION_HEAD_WORDS == 8


# ------------------------------------------------------------------------------------------------------------ the command line
def _args(*argv):
    from faster_rcnn_amd import annotate_video
    return annotate_video.build_parser().parse_args(["rpn.npz", "det.npz", "frames"] + list(argv))


def test_redact_region_from_args(tmp_path):
    from PIL import Image
    from faster_rcnn_amd.annotate_video import redact_from_args, redact_region_from_args, redact_shape_from_args
    from faster_rcnn_amd.data.voc_data_helpers import VOC_CLASS_MAPPING
    a = _args()
    assert (a.redact_region, a.redact_mask, a.region_mode, a.region_size, a.region_feather) == (None,) * 5 and redact_region_from_args(a) is None
    tri = tuple(TRIANGLE)
    assert redact_region_from_args(_args("--redact_region", "3,2,27,9,8,20")) == ((tri,), None, "fill", 0, 0)
    got = redact_region_from_args(_args("--redact_region", "3,2,27,9,8,20", "--redact_region=-5, 0, 9, 0, 9, 9", "--region_mode", "blur",
                                        "--region_feather", "8"))
    assert got == ((tri, ((-5, 0), (9, 0), (9, 9))), None, "blur", 12, 8)
    assert redact_region_from_args(_args("--redact_region", "3,2,27,9,8,20", "--region_mode", "pixelate", "--region_size", "4"))[2:4] == ("pixelate", 4)
    # the regions need neither --redact nor --track, and leave their options alone
    assert redact_from_args(_args("--redact_region", "3,2,27,9,8,20"), VOC_CLASS_MAPPING) is None
    assert redact_shape_from_args(_args("--redact_region", "3,2,27,9,8,20")) is None
    # a mask: any file PIL opens, read as grey; >= 128 hides
    grey = np.zeros((6, 9), dtype=np.uint8)
    grey[1:3, 2:5] = 255
    Image.fromarray(grey).save(tmp_path / "mask.png")
    rgb = np.zeros((6, 9, 3), dtype=np.uint8)
    rgb[4, 4] = 255
    Image.fromarray(rgb).save(tmp_path / "mask_rgb.png")
    regions, m, mode, size, feather = redact_region_from_args(_args("--redact_mask", str(tmp_path / "mask.png")))
    assert regions == () and np.array_equal(m.array, grey) and (mode, size, feather) == ("fill", 0, 0)
    both = redact_region_from_args(_args("--redact_mask", str(tmp_path / "mask_rgb.png"), "--redact_region", "3,2,27,9,8,20"))
    assert both[0] == (tri,) and both[1].shape == (6, 9) and both[1].array[4, 4] == 255 and both[1].array.sum() == 255
    # the three settings are refused by name without an area
    for extra in (("--region_mode", "blur"), ("--region_size", "4"), ("--region_feather", "0")):
        with pytest.raises(ValueError) as e:
            redact_region_from_args(_args(*extra))
        assert extra[0] in str(e.value) and "--redact_region" in str(e.value) and "--redact_mask" in str(e.value)
    for bad, word in (("3,2,27,9", "six"), ("3,2,27,9,8", "even"), ("3,2,27,9,8,x", "integers"), ("3,2,27,9,8,2.5", "integers"),
                      ("0,0,0,0,5,5", "consecutive"), ("0,0,70000,0,5,5", "-32768..65535")):
        with pytest.raises(ValueError) as e:
            redact_region_from_args(_args("--redact_region", bad))
        assert word in str(e.value) and "--redact_region" in str(e.value), bad
    with pytest.raises(ValueError) as e:
        redact_region_from_args(_args(*sum((["--redact_region", "%d,0,%d,0,%d,5" % (10 * k, 10 * k + 5, 10 * k)] for k in range(9)), [])))
    assert "1..8" in str(e.value)
    for extra, word in ((("--region_feather", "33"), "0..32"), (("--region_feather", "-1"), "0..32"), (("--region_size", "3"), "size"),
                        (("--region_mode", "blur", "--region_size", "40"), "size")):
        with pytest.raises(ValueError) as e:
            redact_region_from_args(_args("--redact_region", "3,2,27,9,8,20", *extra))
        assert word in str(e.value)
    with pytest.raises(ValueError) as e:
        redact_region_from_args(_args("--redact_mask", str(tmp_path / "missing.png")))
    assert "--redact_mask" in str(e.value)
    with pytest.raises(SystemExit):
        _args("--redact_region", "3,2,27,9,8,20", "--region_mode", "smear")   # (argparse's choices)


def test_the_keyword_is_refused_by_name_without_a_device():
    from faster_rcnn_amd import annotate_video
    frame = noise(8, 8)
    for bad, word in (((None, None, None, None, None), "neither"), (([TRIANGLE], None, "fill", 0, 33), "feather"), (([TRIANGLE], None), "(regions, mask"),
                      ("triangle", "(regions, mask"), (([TRIANGLE], None, "smear", None, 0), "mode"),
                      ((None, np.zeros((8, 9), dtype=np.uint8), None, None, None), "9x8")):
        with pytest.raises(ValueError) as e:
            annotate_video.draw_eager(frame, [], {"bg": 0, "car": 1}, redact_region=bad)
        assert word in str(e.value), bad


def test_the_line_and_the_blackened_plate():
    from faster_rcnn_amd import annotate_video
    h, w = 23, 31
    mask = np.zeros((h, w), dtype=np.uint8)
    mask[20:, :4] = 255
    W = RR.weights(h, w, [TRIANGLE, Z.BOW], mask, 2)
    covered, full = RR.stats(W)
    option = ((tuple(TRIANGLE), tuple(Z.BOW)), object(), "blur", 12, 2)
    line = annotate_video.region_line(w, h, option, {"covered": covered, "full": full})
    assert line == RR.summary_line(w, h, [TRIANGLE, Z.BOW], mask, W) == "redact regions 31x23: 2 regions + mask, %.1f %% of the frame hidden" % (100.0 * covered / (h * w))
    assert annotate_video.region_line(w, h, ((tuple(TRIANGLE),), None, "fill", 0, 0), {"covered": 0}) == "redact regions 31x23: 1 region, 0.0 % of the frame hidden"
    assert annotate_video.region_line(w, h, ((), object(), "fill", 0, 0), {"covered": h * w}) == "redact regions 31x23: mask, 100.0 % of the frame hidden"
    # --plate_out: every pixel with W > 0 is black in the picture, the feathered ring included; the rest is the plate's
    plate = noise(h, w, 7) | 1                                              # (no byte of it is 0)
    out = annotate_video.blacken_plate(plate, W)
    assert (out[W > 0] == 0).all() and np.array_equal(out[W == 0], plate[W == 0]) and (W > 0).sum() > (W == 256).sum() > 0
    assert (plate != 0).all()                                               # (the caller's array is left alone)


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
    from faster_rcnn_amd import entry, ops
    from faster_rcnn_amd._lib import FrcnnError
    eng = _Engine()
    tri = tuple(TRIANGLE)
    plain = entry.PassSpec.checked(eng, 4, annotate=True)
    assert plain.redact_region is None and plain.key_tail(4) == (4, "annotate") and entry.PassSpec().redact_region is None
    spec = entry.PassSpec.checked(eng, 4, annotate=True, redact_region=([TRIANGLE], None, None, None, None))
    assert spec.redact_region == ((tri,), None, "fill", 0, 0) and spec.key_tail(4) == (4, "annotate", "region", (tri,), None, "fill", 0, 0)
    mask = np.zeros((5, 7), dtype=np.uint8)
    masked = entry.PassSpec.checked(eng, 1, annotate=True, redact_region=(None, mask, "blur", None, 8))
    assert masked.key_tail(1) == ("annotate", "region", (), ops.RegionMask(mask).digest, "blur", 12, 8)
    assert hash(masked) == hash(entry.PassSpec.checked(eng, 1, annotate=True, redact_region=(None, mask.copy(), "blur", 12, 8)))
    # the tag comes last, behind every other option's, and the keys without the option are what they were
    redact = ("all", "blur", 3, 2)
    kw = dict(annotate=True, redact=redact, redact_shape=("ellipse", 4), draw=False, track=(30, 8, 0), out_size=("scale", 2), track_strong=0.5)
    before = entry.PassSpec.checked(eng, 1, **kw).key_tail(1)
    assert before[-2:] == ("weak", 0.5)
    assert entry.PassSpec.checked(eng, 1, redact_region=(TRIANGLE, None, "pixelate", 4, 1), **kw).key_tail(1) == before + ("region", (tri,), None, "pixelate", 4, 1)
    # the mask is held to the pass's source size
    masked.region_fits((5, 7))
    spec.region_fits((1, 1))
    plain.region_fits((1, 1))
    with pytest.raises(FrcnnError) as e:
        masked.region_fits((7, 5))
    assert "7x5" in str(e.value) and "5x7" in str(e.value) and "redact_region" in str(e.value)
    for kw, word in ((dict(redact_region=([TRIANGLE], None, None, None, None)), "annotate=True"),
                     (dict(annotate=True, redact_region=(None, None, None, None, None)), "neither"),
                     (dict(annotate=True, redact_region=([TRIANGLE], None, "fill", 0, 33)), "feather"),
                     (dict(annotate=True, redact_region=([TRIANGLE], None, "blur", 0, 0)), "size"),
                     (dict(annotate=True, redact_region=([TRIANGLE], None, "smear", None, 0)), "mode"),
                     (dict(annotate=True, redact_region=([[(0, 0), (1, 1)]], None, None, None, None)), "vertices"),
                     (dict(annotate=True, redact_region=[TRIANGLE]), "(regions, mask, mode, size, feather)"),
                     (dict(annotate=True, redact_region="all"), "(regions, mask, mode, size, feather)")):
        with pytest.raises(FrcnnError) as e:
            entry.PassSpec.checked(eng, 4, **kw)
        assert word in str(e.value) and "redact" in str(e.value), kw


# ------------------------------------------------------------------------------------------------------------ header and binding
def test_header_binding_and_library_agree():
    from faster_rcnn_amd import _lib
    from faster_rcnn_amd.build import build_library
    ext = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_redact_region.h")).read()
    version = int(re.search(r"#define FRCNN_REDACT_REGION_VERSION (\d+)", ext).group(1))
    assert version == _lib.REDACT_REGION_VERSION == 1 and re.search(r"^ \*   1 = ", ext, flags=re.M)
    define = lambda k: int(re.search(r"#define FRCNN_REDACT_REGION_%s (\d+)" % k, ext).group(1))
    assert define("MAX") == _lib.REDACT_REGION_MAX == RR.MAX_REGIONS == Z.MAX_ZONES == 8
    assert (0, define("FEATHER_MAX")) == _lib.REDACT_REGION_FEATHER == (0, RR.FEATHER_MAX) == _lib.REDACT_FEATHER
    assert define("HEAD_WORDS") == _lib.REDACT_REGION_HEAD_WORDS == 8
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    names = sorted(set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", code)))
    assert names == sorted(_lib.REDACT_REGION_SIGNATURES) == ["frcnn_redact_region_apply_u8", "frcnn_redact_region_build", "frcnn_redact_region_plane_bytes",
                                                              "frcnn_redact_region_prepare", "frcnn_redact_region_version"]
    build_library(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        m = re.search(r"\b(int|size_t) %s\s*\(([^)]*)\)" % name, code)
        assert m, name
        decls = [d for d in m.group(2).split(",") if d.strip() != "void"]
        restype, argtypes = _lib.REDACT_REGION_SIGNATURES[name]
        assert restype is (ctypes.c_int if m.group(1) == "int" else ctypes.c_size_t) and len(argtypes) == len(decls), name
        for decl, ct in zip(decls, argtypes):
            assert ("*" in decl) == (ct is ctypes.c_void_p), (name, decl)
            assert ("size_t" in decl) == (ct is ctypes.c_size_t), (name, decl)
        assert hasattr(lib, name), name
    # the core header and the other extensions do not know the new symbols, and no revision but the new one moved
    core = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    ext_dir = os.path.join(ROOT, "include", "ext")
    others = "".join(open(os.path.join(ext_dir, f)).read() for f in sorted(os.listdir(ext_dir)) if f != "frcnn_hip_redact_region.h")
    assert not any(n in core or n in others for n in names)
    loaded = _lib.load()
    assert loaded.frcnn_redact_region_version() == version
    assert loaded.frcnn_redact_version() == _lib.REDACT_VERSION == 1 and loaded.frcnn_redact_shape_version() == _lib.REDACT_SHAPE_VERSION == 1
    assert loaded.frcnn_zone_version() == _lib.ZONE_VERSION == 1
    assert loaded.frcnn_version() == _lib.ABI_VERSION == int(re.search(r"#define FRCNN_ABI_VERSION (\d+)", core).group(1))
    assert "frcnn_hip_redact_region.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_host_side_checks_refuse_without_a_gpu():
    """Every FRCNN_E_ARG is found on the host, in front of any device call.  The pointers are never followed: 64 stands for a device
    address."""
    from faster_rcnn_amd import _lib
    lib = _lib.load()
    plane_bytes = lib.frcnn_redact_region_plane_bytes
    assert plane_bytes(0, 8) == plane_bytes(8, 0) == plane_bytes(32769, 8) == plane_bytes(8, 32769) == 0
    # [32 | 2 h w | flags | hard (h + 64)(w + 64) | d1 (h + 64) w], each piece padded to 16
    pad = lambda v: (v + 15) // 16 * 16
    for h, w in ((1, 1), (37, 91), (375, 1242)):
        tiles = -(-3 * w // 256) * -(-h // 16)
        want = pad(pad(pad(pad(32 + 2 * h * w) + tiles) + (h + 64) * (w + 64)) + (h + 64) * w)
        assert plane_bytes(h, w) == want, (h, w)
    P = ctypes.c_void_p(64)
    verts = np.array([3, 2, 27, 9, 8, 20], dtype=np.int32)
    nv = np.array([3], dtype=np.int32)
    vp, np_ = verts.ctypes.data_as(ctypes.c_void_p), nv.ctypes.data_as(ctypes.c_void_p)

    def refused(code, word):
        assert code == -1 and word.encode() in lib.frcnn_last_error(), (code, lib.frcnn_last_error())

    build = lib.frcnn_redact_region_build
    refused(build(None, 8, 8, vp, np_, 1, None, 0, None), "redact_region_build: null pointer")
    refused(build(P, 0, 8, vp, np_, 1, None, 0, None), "out of range")
    refused(build(P, 8, 32769, vp, np_, 1, None, 0, None), "out of range")
    refused(build(P, 8, 8, vp, np_, 1, None, -1, None), "feather=-1")
    refused(build(P, 8, 8, vp, np_, 1, None, 33, None), "feather=33")
    refused(build(P, 8, 8, vp, np_, -1, None, 0, None), "n_regions=-1")
    refused(build(P, 8, 8, vp, np_, 9, None, 0, None), "n_regions=9")
    refused(build(P, 8, 8, None, None, 0, None, 0, None), "neither a polygon nor a mask")
    refused(build(P, 8, 8, None, np_, 1, None, 0, None), "null pointer")
    refused(build(P, 8, 8, vp, None, 1, P, 0, None), "null pointer")
    for count in (2, 17):
        bad_nv = np.array([count], dtype=np.int32)
        refused(build(P, 8, 8, vp, bad_nv.ctypes.data_as(ctypes.c_void_p), 1, None, 0, None), "region 0 has %d vertices" % count)
    for bad, word in (([3, 2, 3, 2, 8, 20], "both at (3, 2)"), ([3, 2, 27, 9, 3, 2], "both at (3, 2)"), ([3, 2, 65536, 9, 8, 20], "coordinate 65536"),
                      ([3, -32769, 27, 9, 8, 20], "coordinate -32769")):
        bad_v = np.array(bad, dtype=np.int32)
        refused(build(P, 8, 8, bad_v.ctypes.data_as(ctypes.c_void_p), np_, 1, None, 0, None), word)
    for name in ("frcnn_redact_region_prepare", "frcnn_redact_region_apply_u8"):
        fn, who = getattr(lib, name), name[len("frcnn_"):]
        refused(fn(None, 8, 8, P, 0, 0, None, 0, None), who + ": null pointer")
        refused(fn(P, 8, 8, None, 0, 0, None, 0, None), who + ": null pointer")
        refused(fn(P, 0, 8, P, 0, 0, None, 0, None), "out of range")
        refused(fn(P, 8, 32769, P, 0, 0, None, 0, None), "out of range")
        refused(fn(P, 8, 8, P, 3, 0, None, 0, None), "mode=3")
        refused(fn(P, 8, 8, P, -1, 0, None, 0, None), "mode=-1")
        refused(fn(P, 8, 8, P, 0, 1, None, 0, None), "size=1")
        refused(fn(P, 8, 8, P, 1, 65, P, 1 << 20, None), "size=65")
        refused(fn(P, 8, 8, P, 2, 0, P, 1 << 20, None), "size=0")
        refused(fn(P, 8, 8, P, 2, 3, None, 1 << 20, None), "null workspace")
        refused(fn(P, 8, 8, P, 2, 3, P, 8 * 8 * 3 - 1, None), "workspace of 191 bytes, 192 needed")
        refused(fn(P, 8, 8, P, 1, 4, P, 11, None), "workspace of 11 bytes, 12 needed")
