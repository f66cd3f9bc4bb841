"""The scale rule on the host: what follows from tests/scale_ref.py's restatement, ops.scale_option, annotate_video's arguments, the pass
key and its refusals, and the header against the binding.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import scale_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def noise(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("n_in,n_out", [(1, 1), (5, 5), (8, 4), (9, 4), (16, 1), (65, 5), (300, 19), (20, 19), (1242, 621), (375, 188)])
def test_weights_sum_to_the_source_side_and_lie_together(n_in, n_out):
    wt = R.weights(n_out, n_in)
    assert wt.shape == (n_out, n_in) and (wt >= 0).all()
    assert (wt.sum(axis=1) == n_in).all()                                   # an output pixel is n_in units long
    assert (wt.sum(axis=0) == n_out).all()                                  # a source pixel is n_out units long: nothing is lost
    for row in wt:
        nz = np.flatnonzero(row)
        assert nz.size <= -(-n_in // n_out) + 1 and (np.diff(nz) == 1).all()


def test_the_same_size_is_the_identity():
    frame = noise(7, 5, 1)
    assert np.array_equal(R.downscale(frame, 7, 5), frame)


@pytest.mark.parametrize("N", [2, 3, 16])
def test_a_whole_ratio_is_the_box_mean_rounded_half_up(N):
    H, W = 3, 2
    frame = noise(N * H, N * W, N)
    box = frame.reshape(H, N, W, N, 3).astype(np.int64).sum(axis=(1, 3))
    assert np.array_equal(R.downscale(frame, H, W), ((2 * box + N * N) // (2 * N * N)).astype(np.uint8))
    # half up, by hand: the mean of (0, 0, 0, 2) is 0.5 -> 1, of (0, 0, 0, 1) is 0.25 -> 0
    quad = lambda v: np.array([[[0] * 3, [0] * 3], [[0] * 3, [v] * 3]], dtype=np.uint8)
    assert R.downscale(quad(2), 1, 1).tolist() == [[[1, 1, 1]]] and R.downscale(quad(1), 1, 1).tolist() == [[[0, 0, 0]]]


@pytest.mark.parametrize("value", [0, 1, 127, 255])
def test_a_constant_frame_stays_constant(value):
    for (h, w), (H, W) in (((9, 7), (4, 3)), ((33, 65), (3, 5)), ((40, 20), (39, 19)), ((16, 16), (1, 1))):
        assert (R.downscale(np.full((h, w, 3), value, dtype=np.uint8), H, W) == value).all()


def test_the_double_sum_is_separable_without_intermediate_rounding():
    (h, w), (H, W) = (9, 7), (4, 3)
    frame = noise(h, w, 5)
    ry, cx = R.weights(H, h), R.weights(W, w)
    rows = np.einsum("Xx,yxc->yXc", cx, frame.astype(np.int64))            # the horizontal partial sums, below 255 w
    assert rows.max() <= 255 * w
    two_stage = (np.einsum("Yy,yXc->YXc", ry, rows) + (h * w) // 2) // (h * w)
    assert np.array_equal(two_stage.astype(np.uint8), R.downscale(frame, H, W))
    direct = np.zeros((H, W, 3), dtype=np.int64)
    for Y in range(H):
        for X in range(W):
            for y in range(h):
                for x in range(w):
                    direct[Y, X] += ry[Y, y] * cx[X, x] * frame[y, x].astype(np.int64)
    assert np.array_equal(((direct + (h * w) // 2) // (h * w)).astype(np.uint8), R.downscale(frame, H, W))
    # the largest numerator stays below 2^38 at the largest sides
    assert 255 * 32768 * 32768 < 2 ** 38


def test_the_restatement_refuses_what_the_rule_refuses():
    for h, w, H, W in ((4, 4, 5, 4), (4, 4, 4, 5), (17, 4, 1, 4), (4, 17, 4, 1), (4, 4, 0, 4)):
        with pytest.raises(ValueError):
            R.check_size(h, w, H, W)
    R.check_size(16, 16, 1, 1)


# ------------------------------------------------------------------------------------------------------------ ops.scale_option
def test_scale_option_results_and_refusals():
    from faster_rcnn_amd import ops
    assert ops.scale_option(("scale", 2), (375, 1242)) == (188, 621)
    assert ops.scale_option(("scale", 16), (375, 1242)) == (24, 78)
    assert ops.scale_option(("scale", 3), (1, 1)) == (1, 1)
    assert ops.scale_option(("size", 1920, 1080), (2160, 3840)) == (1080, 1920)      # width first, as a command line states it
    assert ops.scale_option(("size", 5, 7), (7, 5)) == (7, 5)
    assert ops.scale_option(("size", np.int64(2), np.int32(1)), (16, 32)) == (1, 2)
    assert ops.scale_form(["scale", 4]) == ("scale", 4) and ops.scale_form(("size", 3, 2)) == ("size", 3, 2)
    for option, hw in ((("scale", 2), (375, 1242)), (("size", 111, 67), (200, 330))):
        assert ops.scale_option(option, hw) == R.target(option, *hw)
    for option, hw, why in ((("size", 6, 7), (7, 5), "larger than the 5x7 frame"), (("size", 5, 8), (7, 5), "larger than the 5x7 frame"),
                            (("size", 1, 7), (7, 17), "less than 1/16"), (("size", 5, 1), (17, 5), "less than 1/16"),
                            (("size", 0, 3), (7, 5), "at least 1"), (("size", 3, 0), (7, 5), "at least 1"), (("size", -1, 3), (7, 5), "at least 1"),
                            (("scale", 1), (7, 5), "a divisor in 2..16"), (("scale", 17), (70, 50), "a divisor in 2..16"),
                            (("scale", 2.0), (7, 5), "out_size="), (("scale", True), (7, 5), "out_size="), (("size", 3), (7, 5), "out_size="),
                            (("half",), (7, 5), "out_size="), (None, (7, 5), "out_size="), (7, (7, 5), "out_size=")):
        with pytest.raises(ValueError, match=why):
            ops.scale_option(option, hw)


# ------------------------------------------------------------------------------------------------------------ the command line
def test_the_command_line():
    from faster_rcnn_amd import annotate_video as av
    parse = lambda *extra: av.build_parser().parse_args(["a.h5", "b.h5", "frames", *extra])
    assert av.out_size_from_args(parse()) is None
    assert av.out_size_from_args(parse("--out_size", "1280x720")) == ("size", 1280, 720)
    assert av.out_size_from_args(parse("--out_size", " 64 X 48 ")) == ("size", 64, 48)
    assert av.out_size_from_args(parse("--out_scale", "2")) == ("scale", 2) and av.out_size_from_args(parse("--out_scale", "16")) == ("scale", 16)
    with pytest.raises(ValueError, match=r"--out_size=64x48 and --out_scale=2 both state the output size"):
        av.out_size_from_args(parse("--out_size", "64x48", "--out_scale", "2"))
    for bad in ("1", "17", "0", "-2"):
        with pytest.raises(ValueError, match=r"a divisor in 2..16"):
            av.out_size_from_args(parse("--out_scale", bad))
    for bad in ("64", "64x", "x48", "64x48x3", "6.4x48", "64x-48"):
        with pytest.raises(ValueError, match=r"--out_size=.*WxH"):
            av.out_size_from_args(parse("--out_size", bad))
    with pytest.raises(ValueError, match=r"at least 1"):
        av.out_size_from_args(parse("--out_size", "0x48"))
    # --out_size larger than a frame: refused with the frame's name; --out_scale applies per frame size
    assert av.scaled_size(("size", 64, 48), "a.png", 128, 96) == (64, 48)
    assert av.scaled_size(("scale", 2), "a.png", 1242, 375) == (621, 188) and av.scaled_size(("scale", 2), "b.png", 500, 375) == (250, 188)
    with pytest.raises(ValueError, match=r"b\.png \(60x96\): out_size 64x48 is larger than the 60x96 frame"):
        av.scaled_size(("size", 64, 48), "b.png", 60, 96)
    with pytest.raises(ValueError, match=r"c\.png \(2000x96\): out_size 64x48 is less than 1/16"):
        av.scaled_size(("size", 64, 48), "c.png", 2000, 96)


def test_annotate_refuses_a_frame_smaller_than_out_size_by_name(tmp_path):
    """The check both paths make on every frame, on the y4m sink's side too: no model is needed to reach it."""
    import io

    from faster_rcnn_amd import annotate_video as av
    from faster_rcnn_amd import y4m

    class Frame:
        width, height = 60, 96

    writer = y4m.Y4mWriter(io.BytesIO(), 64, 48, "444", "full", {})
    sink = av._y4m_sink(writer, None, ("size", 64, 48))
    try:
        with pytest.raises(ValueError, match=r"f1 \(60x96\): out_size 64x48 is larger"):
            sink.check("f1", Frame)
        Frame.width, Frame.height = 128, 96
        sink.check("f2", Frame)                                             # scaled to the writer's size: taken
        other = av._y4m_sink(y4m.Y4mWriter(io.BytesIO(), 128, 96, "444", "full", {}), None, ("scale", 2))
        with pytest.raises(ValueError, match=r"f3 is 128x96 \(scaled: 64x48\), the output stream's frames are 128x96"):
            other.check("f3", Frame)
        other.close()
    finally:
        sink.close()


# ------------------------------------------------------------------------------------------------------------ the pass key
def test_the_cache_key_and_the_refusals_in_front_of_any_capture():
    from faster_rcnn_amd import entry
    from faster_rcnn_amd._lib import FrcnnError
    base = dict(annotate=True, track=(30, 8, 0), track_motion=8, heat=("all", 160, 0), remove=("all", 8, 10, 8), track_reid=(25, 250))
    spec = entry.PassSpec(**base)
    assert spec.key_tail(4) == (4, "annotate", "track", 30, 8, 0, "motion", 8, "heat", "all", 160, 0, "remove", "all", 8, 10, 8,
                                "track_reid", 25, 250)                       # the parent's form
    assert entry.PassSpec(out_size=("scale", 2), **base).key_tail(4) == spec.key_tail(4) + ("scale", "scale", 2)      # the tag comes last
    assert entry.PassSpec(annotate=True, encode="png", out_size=("size", 64, 48)).key_tail(1) == ("annotate", "png", "scale", "size", 64, 48)
    assert entry.PassSpec().out_size is None and entry.PassSpec(annotate=True).key_tail(1) == ("annotate",)

    class Engine:                                                           # what ``PassSpec.checked`` asks of an engine
        device_preprocess = True
        batch = 4

    eng = Engine()
    assert entry.PassSpec.checked(eng, None, annotate=True, out_size=["scale", 2]).out_size == ("scale", 2)
    assert entry.PassSpec.checked(eng, None, annotate=True).key_tail(4) == (4, "annotate")
    with pytest.raises(FrcnnError, match=r"submit_batch: out_size= scales the frame an ANNOTATING pass returns: pass annotate=True"):
        entry.PassSpec.checked(eng, None, out_size=("scale", 2))
    for bad, why in ((("scale", 1), "2..16"), (("scale", 17), "2..16"), (("size", 0, 4), "at least 1"), ("2", "out_size="), (("size", 4), "out_size=")):
        with pytest.raises(FrcnnError, match=r"submit_batch: .*%s" % why):
            entry.PassSpec.checked(eng, None, annotate=True, out_size=bad)
    # the pass's frame size, and the size its encoder is handed
    small = entry.PassSpec.checked(eng, None, annotate=True, encode="png", out_size=("size", 64, 48))
    assert small.out_hw((96, 128)) == (48, 64) and entry.PassSpec(annotate=True).out_hw((96, 128)) == (96, 128)
    for hw, why in (((40, 128), "larger than the 128x40 frame"), ((96, 2000), "less than 1/16")):
        with pytest.raises(FrcnnError, match=r"submit_batch: out_size 64x48 .*%s" % why):
            small.out_hw(hw)


def test_a_size_the_encoder_refuses_carries_the_encoders_reason(monkeypatch):
    from faster_rcnn_amd import entry, ops
    from faster_rcnn_amd._lib import FrcnnError

    def refuse(h, w, *a):
        raise FrcnnError("png_bound: frame %dx%d unsupported" % (h, w))
    monkeypatch.setattr(ops, "png_bound", refuse)
    spec = entry.PassSpec(annotate=True, encode="png", out_size=("scale", 2))
    with pytest.raises(FrcnnError, match=r"submit_batch: out_size 64x48 with encode=\"png\": png_bound: frame 48x64 unsupported"):
        spec.out_hw((96, 128))
    assert entry.PassSpec(annotate=True, out_size=("scale", 2)).out_hw((96, 128)) == (48, 64)      # no encoder, nobody to ask


# ------------------------------------------------------------------------------------------------------------ header and binding
def test_header_binding_and_library_agree():
    from faster_rcnn_amd import _lib
    from faster_rcnn_amd.build import build_library
    ext = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_scale.h")).read()
    version = int(re.search(r"#define FRCNN_SCALE_VERSION (\d+)", ext).group(1))
    assert version == _lib.SCALE_VERSION == 1 and re.search(r"^ \*   1 = ", ext, flags=re.M)
    assert int(re.search(r"#define FRCNN_SCALE_MAX_RATIO (\d+)", ext).group(1)) == _lib.SCALE_MAX_RATIO == R.MAX_RATIO == 16
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    names = sorted(set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", code)))
    assert names == sorted(_lib.SCALE_SIGNATURES) == ["frcnn_downscale_u8", "frcnn_scale_version"]
    build_library(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        m = re.search(r"\bint %s\s*\(([^)]*)\)" % name, code)
        assert m, name
        decls = [d for d in m.group(1).split(",") if d.strip() != "void"]
        restype, argtypes = _lib.SCALE_SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(decls), name
        for decl, ct in zip(decls, argtypes):
            assert ("*" in decl) == (ct is ctypes.c_void_p), (name, decl)
            assert ("long long" in decl) == (ct is ctypes.c_longlong), (name, decl)
        assert hasattr(lib, name), name
    # the core header and the other extensions do not know the new symbols, and no revision but the new one moved
    core = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    ext_dir = os.path.join(ROOT, "include", "ext")
    others = "".join(open(os.path.join(ext_dir, f)).read() for f in sorted(os.listdir(ext_dir)) if f != "frcnn_hip_scale.h")
    assert not any(n in core or n in others for n in names)
    loaded = _lib.load()
    assert loaded.frcnn_scale_version() == version
    assert loaded.frcnn_version() == _lib.ABI_VERSION == int(re.search(r"#define FRCNN_ABI_VERSION (\d+)", core).group(1))
    assert "frcnn_hip_scale.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # the argument checks run on the host, in front of any device call: refused without a GPU too
    assert loaded.frcnn_downscale_u8(None, 0, 1, None, 8, 8, None, 0, 4, 4, None) == -1
    assert b"downscale_u8: null pointer" in loaded.frcnn_last_error()
