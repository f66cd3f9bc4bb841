"""Host-only checks of the heat rule's restatement (tests/heat_ref.py) against a hand-worked case, of its properties, of ops.heat_option
and annotate_video's --heatmap parsing and refusals, and of the new header against its ctypes binding.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import heat_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = np.array([0, 1, 1], dtype=np.uint8)               # classes 1 and 2 heat, 0 (the background) does not


# ------------------------------------------------------------------------------------------------------------ the hand-worked literal
# A 6 x 8 frame (h = 6, w = 8), S = 1.  Box A = (1, 1)-(4, 3) covers x 1..4, y 1..3; box B = (3, 2)-(9, 4) crosses the right border and
# covers x 3..7, y 2..4; they overlap on x 3..4, y 2..3.  Frame 1 has A and B, frame 2 has A, frame 3 has B.  By hand, for a pixel under
# A only / under both / under B only:
#   frame 1: decay of 0 is 0; +256 / +512 / +256                                        -> 256 / 512 / 256
#   frame 2: 256 - (257 >> 1) = 128, 512 - (513 >> 1) = 256, 128; +256 / +256 / +0      -> 384 / 512 / 128
#   frame 3: 384 - (385 >> 1) = 192, 512 - 256 = 256, 128 - (129 >> 1) = 64; +0 / +256 / +256 -> 192 / 512 / 320
A_BOX, B_BOX = [1, 1, 4, 3], [3, 2, 9, 4]
LITERAL_MAP = np.array([[0,   0,   0,   0,   0,   0,   0,   0],
                        [0, 192, 192, 192, 192,   0,   0,   0],
                        [0, 192, 192, 512, 512, 320, 320, 320],
                        [0, 192, 192, 512, 512, 320, 320, 320],
                        [0,   0,   0, 320, 320, 320, 320, 320],
                        [0,   0,   0,   0,   0,   0,   0,   0]])
# the draw at A = 160 into a frame of 100s, R, G, B order.  peak = 512:
#   v = 512: t = 255, colour (255, 255, 255), a = 160: (100 * 95 + 255 * 160 + 127) / 255 = 50427 / 255 = 197
#   v = 320: t = 81600 / 512 = 159, 3t = 477: (255, 222, 0), a = 25440 / 255 = 99:
#            R (15600 + 25245 + 127) / 255 = 160, G (15600 + 21978 + 127) / 255 = 147, B (15600 + 127) / 255 = 61
#   v = 192: t = 48960 / 512 = 95, 3t = 285: (255, 30, 0), a = 15200 / 255 = 59:
#            R (19600 + 15045 + 127) / 255 = 136, G (19600 + 1770 + 127) / 255 = 84, B (19600 + 127) / 255 = 77
#   v = 0: unchanged
LITERAL_RGB = {0: (100, 100, 100), 192: (136, 84, 77), 320: (160, 147, 61), 512: (197, 197, 197)}


def literal_state():
    s = R.Heat(6, 8)
    s.update(R.make_packed(4, [A_BOX, B_BOX]), TABLE, decay=1)
    s.update(R.make_packed(4, [A_BOX]), TABLE, decay=1)
    s.update(R.make_packed(4, [B_BOX]), TABLE, decay=1)
    return s


def test_the_hand_worked_literal():
    s = literal_state()
    assert np.array_equal(s.map, LITERAL_MAP)
    assert (s.frames, s.peak, s.saturated) == (3, 512, 0)
    assert s.words().tolist() == [3, 512, 0, 0] + LITERAL_MAP.reshape(-1).tolist()
    frame = np.full((6, 8, 3), 100, dtype=np.uint8)
    want = np.array([[LITERAL_RGB[int(v)] for v in row] for row in LITERAL_MAP], dtype=np.uint8)
    assert np.array_equal(s.draw(frame, 160, rgb=True), want)
    assert np.array_equal(s.draw(frame, 160, rgb=False), want[..., ::-1])
    assert (frame == 100).all()                                             # (a copy: the source is not written)


# ------------------------------------------------------------------------------------------------------------ properties
def test_decay_reaches_zero():
    for S in (1, 4, 15):
        s = R.Heat(3, 5)
        s.update(R.make_packed(2, [[0, 0, 4, 2], [1, 1, 2, 1]]), TABLE, decay=S)
        assert s.peak == 512
        empty, seen = R.make_packed(2, []), []
        for _ in range(600 if S < 15 else 3):
            s.update(empty, TABLE, decay=S)
            seen.append(s.peak)
        assert all(b < a or a == 0 for a, b in zip(seen, seen[1:]))           # every positive value loses at least 1
        assert (s.peak == 0 and not s.map.any()) if S < 15 else s.peak == 512 - 3
    s = R.Heat(3, 5)
    s.update(R.make_packed(2, [[0, 0, 4, 2]]), TABLE)
    s.update(R.make_packed(2, []), TABLE, decay=0)
    assert s.peak == 256 and s.frames == 2                                  # S = 0: none


def test_the_clamp_and_saturated():
    words = np.zeros(4 + 6, dtype=np.int32)
    words[4:] = [R.MAX - 256, R.MAX - 255, R.MAX - 257, R.MAX, 0, 7]
    words[1] = R.MAX
    s = R.Heat(2, 3, words)
    s.update(R.make_packed(2, [[0, 0, 0, 0]]), TABLE)                       # exactly 2^30: not clamped
    assert s.map[0, 0] == R.MAX and s.saturated == 0
    s.update(R.make_packed(2, [[1, 0, 2, 0]]), TABLE)
    assert s.map.reshape(-1).tolist() == [R.MAX, R.MAX, R.MAX - 1, R.MAX, 0, 7] and s.saturated == 1 and s.peak == R.MAX
    s.update(R.make_packed(2, []), TABLE)
    assert s.saturated == 1                                                 # sticky
    assert int(s.words().max()) == R.MAX and s.words().dtype == np.int32


def test_boxes_classes_and_held_rows():
    h, w = 5, 7
    cov = R.coverage(h, w, R.make_packed(6, [[-3, -3, 1, 1], [5, 3, 99, 99], [7, 0, 9, 2], [2, 2, 2, 2], [6, 4, 0, 0], [1, 1, 3, 3]],
                                           cls=[1, 2, 1, 1, 1, 0]), False, TABLE)
    want = np.zeros((h, w), dtype=np.int64)
    want[0:2, 0:2] += 1                                                     # crosses the top left corner
    want[3:5, 5:7] += 1                                                     # crosses the bottom right corner
    want[2, 2] += 1                                                         # (the third lies outside: empty; then one pixel)
    want[0:5, 0:7] += 1                                                     # corners in any order: the full frame
    assert np.array_equal(cov, want)                                        # (and the last row's class is not set)
    assert not R.coverage(h, w, R.make_packed(6, [[0, 0, 6, 4]], cls=[5]), False, TABLE).any()      # a class beyond the table
    assert not R.coverage(h, w, R.make_packed(6, [[0, 0, 6, 4]], n_dets=0), False, TABLE).any()     # rows behind n_dets are not read
    tracked = R.make_tracked(6, 1, [[0, 0, 1, 1], [3, 3, 6, 4]])
    assert R.coverage(h, w, tracked, True, TABLE).sum() == 4                # the held row does not count
    assert R.coverage(h, w, R.make_tracked(6, 9, [[0, 0, 0, 0]]), True, TABLE).sum() == 1             # n_live above the rows: clamped


def test_a_frame_that_is_not_real_changes_nothing():
    s = literal_state()
    before = s.words().copy()
    buf = R.make_packed(4, [A_BOX])
    for kw in (dict(frame_index=1, n_frames=1), dict(frame_index=0, n_frames=0), dict(frame_index=0, n_frames=-1),
               dict(frame_index=0, n_frames=3, gate=0)):
        s.update(buf, TABLE, decay=1, **kw)
        assert np.array_equal(s.words(), before)
    s.update(buf, TABLE, decay=1, frame_index=2, n_frames=3, gate=-1)
    assert s.frames == 4


def test_a_draw_with_zero_weight_leaves_the_bytes():
    rs = np.random.RandomState(2)
    frame = rs.randint(0, 256, (4, 6, 3)).astype(np.uint8)
    assert np.array_equal(R.Heat(4, 6).draw(frame, 255), frame)             # a cold map: peak 0
    s = R.Heat(4, 6)
    s.map[0, 0], s.map[1, 1], s.map[2, 2] = 1000, 3, 4
    s.peak = 1000
    out = s.draw(frame, 1)                                                  # A = 1: a = t // 255 is 0 below t = 255
    assert np.array_equal(out[1:], frame[1:]) and np.array_equal(out[0, 1:], frame[0, 1:])
    out = s.draw(frame, 255)                                                # v = 3: t = 0; v = 4: t = 1, a = 1
    assert np.array_equal(out[1, 1], frame[1, 1]) and s.levels()[1, 1] == 0 and s.levels()[2, 2] == 1
    changed = (out != frame).any(axis=-1)
    assert changed[0, 0] and not changed[1, 1] and changed.sum() <= 2
    assert (s.draw(np.zeros((4, 6, 3), np.uint8), 255, rgb=True)[0, 0] == 255).all()    # the hottest pixel at A = 255: white


def test_levels_in_64_bits():
    s = R.Heat(1, 2)
    s.map[0] = [R.MAX, R.MAX - 1]
    s.peak = R.MAX
    assert s.levels().tolist() == [[255, 254]]                              # (v * 255 does not fit 32 bits)


# ------------------------------------------------------------------------------------------------------------ the option
def test_heat_option():
    from faster_rcnn_amd import ops
    assert (ops.HEAT_ALPHA, ops.HEAT_DECAY, ops.HEAT_MAX) == (R.ALPHA, R.DECAY, R.MAX) == ((1, 255, 160), (0, 15, 0), 1 << 30)
    assert ops.heat_option("all") == ("all", 160, 0) and ops.heat_option(("all",)) == ("all", 160, 0)
    assert ops.heat_option("car", 1, 15) == (("car",), 1, 15) and ops.heat_option(["car", "person"], 255) == (("car", "person"), 255, 0)
    assert ops.heat_option("all", np.int64(7), np.int32(2)) == ("all", 7, 2)
    for bad in (0, 256, -1, True, 160.0, "160"):
        with pytest.raises(ValueError, match=r"heat alpha=.*1\.\.255"):
            ops.heat_option("all", bad)
    for bad in (-1, 16, True, 1.0, "1"):
        with pytest.raises(ValueError, match=r"heat decay=.*0\.\.15"):
            ops.heat_option("all", None, bad)
    for bad in ((), [], 5, None, ("car", ""), ("car", 3)):
        with pytest.raises(ValueError, match="heat classes="):
            ops.heat_option(bad)


MAPPING = {"bg": 0, "car": 1, "person": 2}


def parse(*argv):
    from faster_rcnn_amd import annotate_video
    return annotate_video.heatmap_from_args(annotate_video.build_parser().parse_args(["a.h5", "b.h5", "frames"] + list(argv)), MAPPING)


def test_the_command_line():
    assert parse() == (None, None) and parse("--track") == (None, None)
    assert parse("--heatmap", "all") == (("all", 160, 0), None)
    assert parse("--heatmap", "person, car", "--heatmap_alpha", "255", "--heatmap_decay", "15") == ((("person", "car"), 255, 15), None)
    assert parse("--heatmap", "car", "--heatmap_out", "out/heat.png") == ((("car",), 160, 0), "out/heat.png")
    assert parse("--heatmap", "all", "--no_draw", "--redact", "all", "--track", "--track_trails") == (("all", 160, 0), None)
    for flag, value in (("--heatmap_alpha", "9"), ("--heatmap_decay", "2"), ("--heatmap_out", "x.png")):
        with pytest.raises(ValueError, match=r"%s=%s is a setting of the heat map: it needs --heatmap CLASSES" % (flag, value)):
            parse(flag, value)
    with pytest.raises(ValueError, match=r"--heatmap takes comma-separated class names, or all"):
        parse("--heatmap", " , ")
    with pytest.raises(ValueError, match=r"unknown class name 'tram'; the classes are: car, person"):
        parse("--heatmap", "car,tram")
    with pytest.raises(ValueError, match=r"unknown class name 'bg'"):
        parse("--heatmap", "bg")
    for a in ("0", "256", "-3"):
        with pytest.raises(ValueError, match=r"--heatmap / --heatmap_alpha / --heatmap_decay: heat alpha="):
            parse("--heatmap", "all", "--heatmap_alpha", a)
    for s in ("-1", "16"):
        with pytest.raises(ValueError, match=r"--heatmap / --heatmap_alpha / --heatmap_decay: heat decay="):
            parse("--heatmap", "all", "--heatmap_decay", s)
    with pytest.raises(ValueError, match=r"heatmap_out='heat.jpg': .* a path that ends in .png"):
        parse("--heatmap", "all", "--heatmap_out", "heat.jpg")


def test_the_api_refusals_and_the_file_names():
    from faster_rcnn_amd import annotate_video as av
    assert av._heatmap(None) is None and av._heatmap(("all", None, None)) == ("all", 160, 0)
    assert av._heatmap((["car"], 9, 3)) == (("car",), 9, 3)
    with pytest.raises(ValueError, match=r"heatmap='all': \(classes, alpha, decay\)"):
        av._heatmap("all")
    with pytest.raises(ValueError, match="heat alpha=300"):
        av._heatmap(("all", 300, 0))
    with pytest.raises(ValueError, match="heat decay=16"):
        av._heatmap(("all", 160, 16))
    assert av._heatmap_out(None, None) is None and av._heatmap_out("a.PNG", ("all", 160, 0)) == "a.PNG"
    with pytest.raises(ValueError, match=r"heatmap_out='a.png' is where the heat map is written: it needs heatmap="):
        av._heatmap_out("a.png", None)
    assert av.heatmap_paths("d/heat.png", []) == {}
    assert av.heatmap_paths("d/heat.png", [(375, 1242)]) == {(375, 1242): "d/heat.png"}
    assert av.heatmap_paths("d/heat.png", [(375, 1242), (375, 500)]) == {(375, 500): "d/heat_500x375.png", (375, 1242): "d/heat_1242x375.png"}


def test_heatmap_out_writes_the_levels(tmp_path):
    from PIL import Image as PilImage
    from faster_rcnn_amd import annotate_video as av, ops
    s = literal_state()
    cold = R.Heat(2, 2)
    path = str(tmp_path / "heat.png")
    tail = np.zeros(3, dtype=np.int32)                                      # (a buffer is longer than its state: scratch words behind the map)
    written = av.write_heatmaps(path, {(6, 8): np.concatenate([s.words(), tail]), (2, 2): cold.words()})
    assert written == [path] and sorted(os.listdir(str(tmp_path))) == ["heat.png"]      # (the size that saw no frame is not written)
    with PilImage.open(path) as im:
        assert im.mode == "L" and np.array_equal(np.asarray(im), s.levels().astype(np.uint8))
    assert np.array_equal(ops.heat_levels(cold.words(), 2, 2), np.zeros((2, 2), np.uint8))
    other = R.Heat(2, 2)
    other.update(R.make_packed(1, [[0, 0, 0, 1]]), TABLE)
    written = av.write_heatmaps(path, {(6, 8): s.words(), (2, 2): other.words()})
    assert written == [str(tmp_path / "heat_2x2.png"), str(tmp_path / "heat_8x6.png")]
    with PilImage.open(written[0]) as im:
        assert np.asarray(im).tolist() == [[255, 0], [255, 0]]


def test_the_cache_key_and_the_refusals_in_front_of_any_capture():
    from faster_rcnn_amd import entry
    from faster_rcnn_amd._lib import FrcnnError
    spec = entry.PassSpec(annotate=True, track=(30, 8, 0), track_motion=8, track_trails=(16, 3))
    with_heat = entry.PassSpec(annotate=True, track=(30, 8, 0), track_motion=8, track_trails=(16, 3), heat=("all", 160, 0))
    assert with_heat.key_tail(4) == spec.key_tail(4) + ("heat", "all", 160, 0) and "heat" not in spec.key_tail(4)
    assert entry.PassSpec(annotate=True, heat=(("car",), 9, 2)).key_tail(1) == ("annotate", "heat", ("car",), 9, 2)
    assert entry.PassSpec().heat is None

    class Engine:                                                           # what ``PassSpec.checked`` asks of an engine
        device_preprocess = True
        batch = 4
        class_names = staticmethod(lambda: ["bg", "car", "person"])
        heat_option = entry.DetectionEntry.heat_option

    eng = Engine()
    assert entry.PassSpec.checked(eng, None, annotate=True, heat=("all", None, None)).heat == ("all", 160, 0)
    assert entry.PassSpec.checked(eng, None, annotate=True, heat=(["person"], 200, 4), draw=False).heat == (("person",), 200, 4)
    assert entry.PassSpec.checked(eng, None, annotate=True).key_tail(4) == (4, "annotate")
    with pytest.raises(FrcnnError, match=r"heat= blends the heat map into the frame an ANNOTATING pass returns: pass annotate=True"):
        entry.PassSpec.checked(eng, None, heat=("all", None, None))
    for bad, why in ((("all", 0, 0), "heat alpha=0"), (("all", 160, 16), "heat decay=16"), (("tram", 160, 0), "unknown class name 'tram'"),
                     ("all", r"\(classes, alpha, decay\)"), (((), 1, 1), "heat classes=")):
        with pytest.raises(FrcnnError, match=r"submit_batch: heat=.*%s" % why):
            entry.PassSpec.checked(eng, None, annotate=True, heat=bad)
    eng.device_preprocess = False
    with pytest.raises(FrcnnError, match=r"heat= needs the device-side preprocess: a foreign preprocess_func"):
        entry.PassSpec.checked(eng, None, annotate=True, heat=("all", None, None))


# ------------------------------------------------------------------------------------------------------------ header and binding
def test_header_binding_and_library_agree():
    from faster_rcnn_amd import _lib
    from faster_rcnn_amd.build import build_library
    ext = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_heat.h")).read()
    version = int(re.search(r"#define FRCNN_HEAT_VERSION (\d+)", ext).group(1))
    assert version == _lib.HEAT_VERSION == 1 and re.search(r"^ \*   1 = ", ext, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    names = sorted(set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", code)))
    assert names == sorted(_lib.HEAT_SIGNATURES) == ["frcnn_heat_draw_u8", "frcnn_heat_state_bytes", "frcnn_heat_update", "frcnn_heat_version"]
    build_library(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        m = re.search(r"\b(int|size_t) %s\s*\(([^)]*)\)" % name, code)
        assert m, name
        decls = [d for d in m.group(2).split(",") if d.strip() != "void"]
        restype, argtypes = _lib.HEAT_SIGNATURES[name]
        assert restype is {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[m.group(1)] and len(argtypes) == len(decls), name
        for decl, ct in zip(decls, argtypes):
            assert ("*" in decl) == (ct is ctypes.c_void_p), (name, decl)
            assert ("size_t" in decl) == (ct is ctypes.c_size_t), (name, decl)
        assert hasattr(lib, name), name
    define = lambda k: int(re.search(r"#define FRCNN_HEAT_%s (\d+)" % k, ext).group(1))
    assert (1, 255, define("DEFAULT_ALPHA")) == _lib.HEAT_ALPHA and (0, define("MAX_DECAY"), 0) == _lib.HEAT_DECAY
    assert define("MAX") == _lib.HEAT_MAX == R.MAX and define("MAX_FRAMES") == _lib.HEAT_MAX_FRAMES
    assert (define("TILE_W"), define("TILE_H")) == _lib.HEAT_TILE
    # the core header and the other extensions do not know the new symbols, and no revision but the new one moved
    core = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    ext_dir = os.path.join(ROOT, "include", "ext")
    others = "".join(open(os.path.join(ext_dir, f)).read() for f in sorted(os.listdir(ext_dir)) if f != "frcnn_hip_heat.h")
    assert not any(n in core or n in others for n in names)
    loaded = _lib.load()
    assert loaded.frcnn_heat_version() == version
    assert loaded.frcnn_version() == _lib.ABI_VERSION == int(re.search(r"#define FRCNN_ABI_VERSION (\d+)", core).group(1))
    # the sizes run on the host: the state, then a word per 64 x 16 tile
    size = loaded.frcnn_heat_state_bytes
    assert size(1, 1) == 4 * (4 + 1 + 1) and size(16, 64) == 4 * (4 + 1024 + 1) and size(17, 65) == 4 * (4 + 17 * 65 + 4)
    assert size(375, 1242) == 4 * (4 + 375 * 1242 + 24 * 20)
    assert size(0, 5) == size(5, 0) == size(32769, 1) == size(1, 32769) == 0 and size(32768, 1) == 4 * (4 + 32768 + 2048)
