"""The plate rule on the host: hand-worked cases of tests/plate_ref.py, ops.plate_option, annotate_video's arguments, the pass key, and
the header against the binding.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import plate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = R.packed(2, [])


def one(value):
    return np.full((1, 1, 3), value, dtype=np.uint8)


def px(state):
    """(P0, V, C0, N) of the one pixel of a 1 x 1 state."""
    P, V, C, N = R.unpack(state, 1, 1)
    return int(P[0, 0, 0]), int(V[0, 0]), int(C[0, 0, 0]), int(N[0, 0])


# ------------------------------------------------------------------------------------------------------------ the reference, by hand
def test_a_run_settles_at_exactly_S_frames():
    s = R.empty(1, 1)
    for f in range(3):
        R.update(s, one(40 + f), NONE, 2, 4, 10, 0)                         # 40, 41, 42: all within 10 of the anchor 40
        assert px(s) == (0, 0, 40, f + 1) and s[1] == 0
    R.update(s, one(43), NONE, 2, 4, 10, 0)
    assert px(s) == (43, 1, 40, 4) and list(s[:4]) == [4, 1, 0, 0]         # the 4th frame: P = x of THAT frame, the anchor stays
    R.update(s, one(44), NONE, 2, 4, 10, 0)
    assert px(s) == (44, 1, 40, 5)                                          # and P follows while the run lasts


def test_all_three_channels_count_and_the_byte_order_is_the_frames():
    s = R.empty(1, 1)
    R.update(s, np.array([[[1, 2, 3]]], dtype=np.uint8), NONE, 2, 1, 0, 0)
    assert s[4] == 1 | 2 << 8 | 3 << 16 | 1 << 24 and s[5] == s[4]          # S = 1: known at once; word 1: C and N = 1
    R.update(s, np.array([[[1, 2, 9]]], dtype=np.uint8), NONE, 2, 2, 5, 0)  # the third channel alone is 6 away
    assert R.unpack(s, 1, 1)[3][0, 0] == 1 and s[5] == 1 | 2 << 8 | 9 << 16 | 1 << 24 and s[4] == 1 | 2 << 8 | 3 << 16 | 1 << 24


def test_a_block_resets_N_but_keeps_P():
    s = R.empty(1, 1)
    for _ in range(2):
        R.update(s, one(70), NONE, 2, 2, 0, 0)
    assert px(s) == (70, 1, 70, 2)
    R.update(s, one(200), R.packed(2, [(0, 0, 0, 0, 99)]), 2, 2, 0, 0)      # any class blocks, one the table does not know too
    assert px(s) == (70, 1, 70, 0) and list(s[:2]) == [3, 1]
    R.update(s, one(70), NONE, 2, 2, 0, 0)
    assert px(s) == (70, 1, 70, 1)                                          # N was 0: the run starts over, even on the old value
    R.update(s, one(9), R.packed(2, [(5, 5, 3, 3, 1)]), 2, 2, 0, 4)          # the margin brings the box over the pixel: 3 - 4 <= 0
    assert px(s) == (70, 1, 70, 0)
    R.update(s, one(9), R.packed(2, [(5, 5, 6, 6, 1)]), 2, 2, 0, 4)          # 5 - 4 = 1 > 0: not over it
    assert px(s) == (70, 1, 9, 1)


def test_drift_beyond_T_from_the_anchor_restarts_the_run():
    s = R.empty(1, 1)
    for f, v in enumerate([100, 104, 108, 110]):                            # steps of 4 with T = 10: within T of the ANCHOR 100
        R.update(s, one(v), NONE, 2, 200, 10, 0)
        assert px(s)[2:] == (100, f + 1)
    R.update(s, one(111), NONE, 2, 200, 10, 0)                              # 1 from the frame before, 11 from the anchor
    assert px(s)[2:] == (111, 1)
    R.update(s, one(101), NONE, 2, 200, 10, 0)                              # downwards counts alike
    assert px(s)[2:] == (111, 2)
    R.update(s, one(100), NONE, 2, 200, 10, 0)
    assert px(s)[2:] == (100, 1)


def test_N_stops_at_255():
    s = R.empty(1, 1)
    for f in range(300):
        R.update(s, one(5), NONE, 2, 255, 0, 0)
        assert px(s) == ((5, 1, 5, 255) if f >= 254 else (0, 0, 5, f + 1))
    assert s[0] == 300


def test_a_cut_empties_the_state_and_an_unreal_frame_writes_nothing():
    s = R.empty(2, 2)
    frame = np.arange(12, dtype=np.uint8).reshape(2, 2, 3)
    for _ in range(3):
        R.update(s, frame, NONE, 2, 3, 0, 0)
    assert s[1] == 4 and R.known(s, 2, 2) == 4
    before = s.copy()
    for kw in (dict(frame_index=1, n_frames=1), dict(n_frames=0), dict(n_frames=-1), dict(gate=0), dict(frame_index=2, n_frames=2, gate=1)):
        R.update(s, 255 - frame, NONE, 2, 3, 0, 0, cut=1, **kw)
        assert np.array_equal(s, before), kw
    R.update(s, frame, NONE, 2, 3, 0, 0, cut=0, gate=5)
    assert s[0] == 4 and s[1] == 4
    R.update(s, frame, R.packed(2, [(0, 0, 0, 0, 1)]), 2, 1, 0, 0, cut=7)   # the old plate is gone in the same call; S = 1: the new one
    P, V, C, N = R.unpack(s, 2, 2)                                          # is known but under the box, where nothing is left
    assert s[0] == 5 and s[1] == 3 and V.tolist() == [[0, 1], [1, 1]] and N.tolist() == [[0, 1], [1, 1]] and s[4] == 0 and s[5] == 0
    assert np.array_equal(P[0, 1], frame[0, 1])


def test_boxes_clip_as_the_redaction_and_fill_is_a_subset_of_block():
    h, w = 6, 9
    table = np.array([0, 1, 0], dtype=np.uint8)
    det = R.tracked(6, [(7, 4, 2, 1, 1),          # reversed: columns 2..7, rows 1..4
                        (-9, -9, -3, -3, 1),      # outside, and the margin 2 does not bring it in: empty
                        (-9, 0, -2, 0, 1),        # the margin brings column 0 of row 0..2 in
                        (8, 5, 30, 30, 2),        # crosses the border; class 2: blocks, does not fill
                        (0, 5, 0, 5, 7),          # a class outside the table: blocks, does not fill
                        (4, 4, 4, 4, -1)], n_live=2)
    assert R.boxes(det, 6, h, w, 0) == [(2, 7, 1, 4), (8, 8, 5, 5), (0, 0, 5, 5), (4, 4, 4, 4)]
    assert R.boxes(det, 6, h, w, 2, table) == [(0, 8, 0, 5), (0, 0, 0, 2)]
    block, fill = R.mask(det, 6, h, w, 0), R.mask(det, 6, h, w, 0, table)
    assert fill.sum() == 24 and block.sum() == 26 and not (fill & ~block).any()
    det[0] = 99                                                             # counts are clamped to the rows
    assert len(R.boxes(det, 6, h, w, 0)) == 4
    det[0] = -1
    assert R.boxes(det, 6, h, w, 0) == []


def test_the_fill_and_keep_unknown():
    s = R.empty(1, 3)
    frame = np.array([[[10, 11, 12], [20, 21, 22], [30, 31, 32]]], dtype=np.uint8)
    R.update(s, frame, R.packed(1, [(1, 0, 1, 0, 1)]), 1, 1, 0, 0)          # pixel 1 is never learned
    table = np.array([0, 1], dtype=np.uint8)
    det = R.packed(1, [(0, 0, 1, 0, 1)])
    for keep, middle in ((False, [0, 0, 0]), (True, [7, 7, 7])):
        out, from_plate, unknown = R.fill(np.full((1, 3, 3), 7, np.uint8), s, det, 1, table, 0, keep)
        assert out.tolist() == [[[10, 11, 12], middle, [7, 7, 7]]]
        assert from_plate.tolist() == [[True, False, False]] and unknown.tolist() == [[False, True, False]]
    out, _, _ = R.fill(np.full((1, 3, 3), 7, np.uint8), s, R.packed(1, [(0, 0, 2, 0, 0)]), 1, table, 0)
    assert (out == 7).all()                                                 # class 0 is not in the table: nothing is written


# ------------------------------------------------------------------------------------------------------------ options and arguments
def test_plate_option():
    from faster_rcnn_amd import ops
    assert ops.plate_option("all") == ("all", 8, 10, 8) and ops.plate_option(["all"]) == ("all", 8, 10, 8)
    assert ops.plate_option("car", 1, 0, 0) == (("car",), 1, 0, 0) and ops.plate_option(("a", "b"), 255, 255, 64) == (("a", "b"), 255, 255, 64)
    assert (ops.PLATE_SETTLE, ops.PLATE_TOL, ops.PLATE_MARGIN) == ((1, 255, 8), (0, 255, 10), (0, 64, 8))
    for kw, why in ((dict(settle=0), "remove settle=0: an integer in 1..255"), (dict(settle=256), "remove settle=256"),
                    (dict(tol=-1), "remove tol=-1: an integer in 0..255"), (dict(tol=256), "remove tol=256"),
                    (dict(margin=-1), "remove margin=-1: an integer in 0..64"), (dict(margin=65), "remove margin=65"),
                    (dict(settle=2.0), "remove settle=2.0"), (dict(tol=True), "remove tol=True")):
        with pytest.raises(ValueError, match=why):
            ops.plate_option("all", **kw)
    for bad in ((), [""], 5, [3]):
        with pytest.raises(ValueError, match="remove classes="):
            ops.plate_option(bad)


MAPPING = {"bg": 0, "car": 1, "person": 2}


def parse(*argv):
    from faster_rcnn_amd import annotate_video
    return annotate_video.remove_from_args(annotate_video.build_parser().parse_args(["a.h5", "b.h5", "frames"] + list(argv)), MAPPING)


def test_the_command_line():
    from faster_rcnn_amd import annotate_video
    args = annotate_video.build_parser().parse_args(["a.h5", "b.h5", "frames"])
    assert (args.remove, args.remove_settle, args.remove_tol, args.remove_margin, args.plate_out) == (None,) * 5
    assert parse() == (None, None) and parse("--track", "--redact", "all") == (None, None)
    assert parse("--remove", "all") == (("all", 8, 10, 8), None)
    assert parse("--remove", "person, car", "--remove_settle", "255", "--remove_tol", "0", "--remove_margin", "64") \
        == ((("person", "car"), 255, 0, 64), None)
    assert parse("--remove", "car", "--plate_out", "out/plate.PNG") == ((("car",), 8, 10, 8), "out/plate.PNG")
    assert parse("--remove", "all", "--no_draw", "--redact", "all", "--track", "--track_lookback") == (("all", 8, 10, 8), None)
    for flag, value in (("--remove_settle", "9"), ("--remove_tol", "2"), ("--remove_margin", "0"), ("--plate_out", "x.png")):
        with pytest.raises(ValueError, match=r"%s=%s is a setting of the removal: it needs --remove CLASSES" % (flag, value)):
            parse(flag, value)
    with pytest.raises(ValueError, match=r"--remove takes comma-separated class names, or all"):
        parse("--remove", " , ")
    with pytest.raises(ValueError, match=r"margin: remove: unknown class name 'tram'; the classes are: car, person") as e:
        parse("--remove", "car,tram")
    assert "redact" not in str(e.value)                                     # (the refusal names the option it refuses)
    with pytest.raises(ValueError, match=r"remove: unknown class name 'bg'"):
        parse("--remove", "bg")
    from faster_rcnn_amd import annotate_video as av
    for argv in (["--plate_out", "x.png"], ["--remove_tol", "3"], ["--remove", "tram"], ["--remove", "all", "--remove_settle", "0"],
                 ["--remove", "all", "--plate_out", "x.jpg"]):
        with pytest.raises(ValueError, match="remov|plate_out"):             # ... through main, before any model file is opened
            av.main(["no.npz", "no.npz", "nowhere"] + argv)
    for flag, name, values in (("--remove_settle", "settle", ("0", "256")), ("--remove_tol", "tol", ("-1", "256")),
                               ("--remove_margin", "margin", ("-1", "65"))):
        for v in values:
            with pytest.raises(ValueError, match=r"--remove / --remove_settle / --remove_tol / --remove_margin: remove %s=%s" % (name, v)):
                parse("--remove", "all", "%s=%s" % (flag, v))
    with pytest.raises(ValueError, match=r"plate_out='plate.jpg': .* a path that ends in .png"):
        parse("--remove", "all", "--plate_out", "plate.jpg")


def test_the_api_refusals_the_summaries_and_the_files(tmp_path, capsys):
    from PIL import Image as PilImage
    from faster_rcnn_amd import annotate_video as av
    assert av._remove(None) is None and av._remove(("all", None, None, None)) == ("all", 8, 10, 8)
    assert av._remove((["car"], 9, 3, 1)) == (("car",), 9, 3, 1)
    with pytest.raises(ValueError, match=r"remove='all': \(classes, settle, tol, margin\)"):
        av._remove("all")
    with pytest.raises(ValueError, match="remove settle=300"):
        av._remove(("all", 300, 0, 0))
    assert av._plate_out(None, None) is None
    with pytest.raises(ValueError, match=r"plate_out='a.png' is where the background plate is written: it needs remove="):
        av._plate_out("a.png", None)
    # two sizes, one of them in both channel orders, one that saw no frame
    a = R.empty(1, 2)
    R.update(a, np.array([[[1, 2, 3], [4, 5, 6]]], dtype=np.uint8), R.packed(1, [(1, 0, 1, 0, 0)]), 1, 1, 0, 0)
    b = R.empty(2, 1)
    for _ in range(2):
        R.update(b, np.array([[[9, 8, 7]], [[6, 5, 4]]], dtype=np.uint8), R.packed(1, []), 1, 1, 0, 0)
    b_other = R.empty(2, 1)
    R.update(b_other, np.zeros((2, 1, 3), np.uint8), R.packed(1, []), 1, 1, 0, 0)
    tail = np.zeros(3, dtype=np.int32)                                      # (a buffer is longer than its state: the scratch words)
    met = av.plate_summaries({(1, 2, True): np.concatenate([a, tail]), (2, 1, False): b, (2, 1, True): b_other, (5, 5, False): R.empty(5, 5)})
    assert sorted(met) == [(1, 2, True), (2, 1, False), (2, 1, True)]       # nothing learned is dropped: both plates of the size met twice
    assert met[(1, 2, True)][:2] == (1, 1) and met[(2, 1, False)][:2] == (2, 2) and met[(2, 1, True)][:2] == (1, 2)
    assert met[(1, 2, True)][2].tolist() == [[[1, 2, 3], [0, 0, 0]]] and met[(2, 1, False)][2].tolist() == [[[7, 8, 9]], [[4, 5, 6]]]      # B, G, R turned
    av.print_plates(met)
    assert capsys.readouterr().out == ("plate 2x1: 1 frames, 50.0 % known\nplate 1x2 (bgr frames): 2 frames, 100.0 % known\n"
                                       "plate 1x2 (rgb frames): 1 frames, 100.0 % known\n")
    path = str(tmp_path / "plate.png")
    assert av.write_plates(path, {(1, 2, True): met[(1, 2, True)]}) == [path]
    with PilImage.open(path) as im:
        assert im.mode == "RGB" and np.asarray(im).tolist() == [[[1, 2, 3], [0, 0, 0]]]
    one_order = {k: v for k, v in met.items() if k != (2, 1, True)}
    assert av.write_plates(path, one_order) == [str(tmp_path / "plate_2x1.png"), str(tmp_path / "plate_1x2.png")]
    assert av.write_plates(path, met) == [str(tmp_path / "plate_2x1.png"), str(tmp_path / "plate_1x2_bgr.png"), str(tmp_path / "plate_1x2_rgb.png")]
    with PilImage.open(str(tmp_path / "plate_1x2_bgr.png")) as im:
        assert np.asarray(im).tolist() == [[[7, 8, 9]], [[4, 5, 6]]]
    with PilImage.open(str(tmp_path / "plate_1x2_rgb.png")) as im:
        assert not np.asarray(im).any()


def test_the_cache_key_and_the_refusals_in_front_of_any_capture():
    from faster_rcnn_amd import entry
    from faster_rcnn_amd._lib import FrcnnError
    base = dict(annotate=True, track=(30, 8, 0), track_motion=8, heat=("all", 160, 0))
    spec, with_remove = entry.PassSpec(**base), entry.PassSpec(remove=("all", 8, 10, 8), **base)
    assert with_remove.key_tail(4) == spec.key_tail(4) + ("remove", "all", 8, 10, 8) and "remove" not in spec.key_tail(4)
    assert spec.key_tail(4) == (4, "annotate", "track", 30, 8, 0, "motion", 8, "heat", "all", 160, 0)          # the parent's form
    assert entry.PassSpec(annotate=True, remove=(("car",), 9, 2, 0)).key_tail(1) == ("annotate", "remove", ("car",), 9, 2, 0)
    assert entry.PassSpec().remove is None

    class Engine:                                                           # what ``PassSpec.checked`` asks of an engine
        device_preprocess = True
        batch = 4
        class_names = staticmethod(lambda: ["bg", "car", "person"])
        remove_option = entry.DetectionEntry.remove_option

    eng = Engine()
    assert entry.PassSpec.checked(eng, None, annotate=True, remove=("all", None, None, None)).remove == ("all", 8, 10, 8)
    assert entry.PassSpec.checked(eng, None, annotate=True, remove=(["person"], 200, 4, 0), draw=False).remove == (("person",), 200, 4, 0)
    assert entry.PassSpec.checked(eng, None, annotate=True).key_tail(4) == (4, "annotate")
    with pytest.raises(FrcnnError, match=r"remove= paints the objects out of the frame an ANNOTATING pass returns: pass annotate=True"):
        entry.PassSpec.checked(eng, None, remove=("all", None, None, None))
    for bad, why in ((("all", 0, 0, 0), "remove settle=0"), (("all", 8, 256, 0), "remove tol=256"), (("all", 8, 0, 65), "remove margin=65"),
                     (("tram", 8, 0, 0), "remove: unknown class name 'tram'"), ("all", r"\(classes, settle, tol, margin\)"),
                     (((), 1, 1, 1), "remove classes=")):
        with pytest.raises(FrcnnError, match=r"submit_batch: remove=.*%s" % why):
            entry.PassSpec.checked(eng, None, annotate=True, remove=bad)
    eng.device_preprocess = False
    with pytest.raises(FrcnnError, match=r"remove= needs the device-side preprocess: a foreign preprocess_func"):
        entry.PassSpec.checked(eng, None, annotate=True, remove=("all", None, None, None))


# ------------------------------------------------------------------------------------------------------------ header and binding
def test_header_binding_and_library_agree():
    from faster_rcnn_amd import _lib
    from faster_rcnn_amd.build import build_library
    ext = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_plate.h")).read()
    version = int(re.search(r"#define FRCNN_PLATE_VERSION (\d+)", ext).group(1))
    assert version == _lib.PLATE_VERSION == 1 and re.search(r"^ \*   1 = ", ext, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    names = sorted(set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", code)))
    assert names == sorted(_lib.PLATE_SIGNATURES) == ["frcnn_plate_fill_u8", "frcnn_plate_state_bytes", "frcnn_plate_update",
                                                       "frcnn_plate_version"]
    build_library(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        m = re.search(r"\b(int|size_t) %s\s*\(([^)]*)\)" % name, code)
        assert m, name
        decls = [d for d in m.group(2).split(",") if d.strip() != "void"]
        restype, argtypes = _lib.PLATE_SIGNATURES[name]
        assert restype is {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[m.group(1)] and len(argtypes) == len(decls), name
        for decl, ct in zip(decls, argtypes):
            assert ("*" in decl) == (ct is ctypes.c_void_p), (name, decl)
        assert hasattr(lib, name), name
    define = lambda k: int(re.search(r"#define FRCNN_PLATE_%s (\d+)" % k, ext).group(1))
    assert (1, define("MAX_SETTLE"), define("DEFAULT_SETTLE")) == _lib.PLATE_SETTLE == (1, 255, 8)
    assert (0, 255, define("DEFAULT_TOL")) == _lib.PLATE_TOL and (0, define("MAX_MARGIN"), define("DEFAULT_MARGIN")) == _lib.PLATE_MARGIN
    assert define("MAX_FRAMES") == _lib.PLATE_MAX_FRAMES and (define("TILE_W"), define("TILE_H")) == _lib.PLATE_TILE
    assert "PROVISIONAL" in ext
    # the core header and the other extensions do not know the new symbols, and no revision but the new one moved
    core = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    ext_dir = os.path.join(ROOT, "include", "ext")
    others = "".join(open(os.path.join(ext_dir, f)).read() for f in sorted(os.listdir(ext_dir)) if f != "frcnn_hip_plate.h")
    assert not any(n in core or n in others for n in names)
    loaded = _lib.load()
    assert loaded.frcnn_plate_version() == version
    assert loaded.frcnn_version() == _lib.ABI_VERSION == int(re.search(r"#define FRCNN_ABI_VERSION (\d+)", core).group(1))
    # the sizes run on the host: the state, then a word per 128 x 8 tile
    size = loaded.frcnn_plate_state_bytes
    assert size(1, 1) == 4 * (4 + 2 + 1) and size(8, 128) == 4 * (4 + 2048 + 1) and size(9, 129) == 4 * (4 + 2 * 9 * 129 + 4)
    assert size(375, 1242) == 4 * (4 + 2 * 375 * 1242 + 47 * 10)
    assert size(0, 5) == size(5, 0) == size(32769, 1) == size(1, 32769) == 0 and size(32768, 1) == 4 * (4 + 2 * 32768 + 4096)
