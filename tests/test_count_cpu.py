"""The count rule on the host (no GPU): the numpy restatement (tests/count_ref.py) against answers written out by hand, the option and
command-line parsing with every refusal, the cache key with and without the option, the CSV rows and the printed totals, and the
header against the binding."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import count_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPPING = {"bg": 0, "car": 1, "person": 2}
ALL = np.ones(4, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("case", R.HAND_CASES, ids=[c[0] for c in R.HAND_CASES])
def test_the_rule_gives_the_hand_answers(case):
    _, (h, w), lines, points, answers = case
    ref = R.Counter(h, w, lines, ALL, capacity=4, expire=9)
    lists = ref.update(R.hand_buffers(points), len(points))
    assert [[ev[:2] for ev in R.events_of(l)] for l in lists] == [[tuple(a) for a in ans] for ans in answers]
    totals = [[0, 0] for _ in range(R.MAX_LINES)]
    for ans in answers:
        for l, d in ans:
            totals[l][d] += 1
    assert ref.totals == totals and ref.frames == len(points) and [e["pt"] for e in ref.entries] == [tuple(points[-1])]
    assert np.array_equal(lists[-1][4:R.HEAD], np.asarray(totals).reshape(-1)) and lists[-1][1] == len(points)


def test_a_32_bit_product_would_be_wrong():
    line, p, q = (-32768, -32768, 65535, 65535), (32767, 0), (0, 32767)
    s = (line[2] - line[0]) * (p[1] - line[1]) - (line[3] - line[1]) * (p[0] - line[0])
    assert s == -98303 * 32767 and abs(s) > 2 ** 31 and (np.int64(s).astype(np.int32) >= 0) != (s >= 0)
    assert R.crossing(line, p, q) == 1 and R.crossing(line, q, p) == 0


def test_once_full_table_expiry_and_the_event_limit():
    line = [(0, 50, 200, 50)]
    ref = R.Counter(120, 200, line, ALL, capacity=2, expire=1)
    at = lambda y, ids: R.make_tracked([(i, 1, (10 * i, y, 10 * i, y)) for i in ids], 8)
    lists = ref.update(np.stack([at(10, (3, 1, 2)), at(90, (3, 1, 2)), at(10, (1,)), at(90, (1,)), at(90, (2,))]), 5)
    # capacity 2: id 2 is dropped twice; 3 and 1 cross (+); 1 goes back (-) and over again (+, counted already); 3 has left, 2 enters
    assert ref.dropped == 2 and ref.totals[0] == [1, 2] and [e["id"] for e in ref.entries] == [1, 2]
    assert [R.events_of(l) for l in lists] == [[], [(0, 1, 3, 1), (0, 1, 1, 1)], [(0, 0, 1, 1)], [], []]
    assert ref.entries[0]["counted"] == 3 and np.array_equal(ref.words()[:6], [2, 5, 2, 0, 1, 2])
    many = R.Counter(120, 200, line, ALL, capacity=128, expire=1)
    ids = range(1, 66)
    lists = many.update(np.stack([R.make_tracked([(i, 1, (2 * i, y, 2 * i, y)) for i in ids], 70) for y in (10, 90)]), 2)
    assert lists[1][0] == 64 and many.events_dropped == 1 and many.totals[0] == [0, 65]
    again = R.Counter(120, 200, line, ALL, capacity=128).load(many.words())
    assert np.array_equal(again.words(), many.words())


def test_classes_id_zero_and_rows_behind_n_live_do_not_count():
    table = np.array([0, 1, 0], dtype=np.uint8)
    rows = lambda y: [(1, 1, (10, y, 10, y)), (2, 2, (20, y, 20, y)), (0, 1, (30, y, 30, y)), (3, 5, (40, y, 40, y)), (4, 1, (50, y, 50, y))]
    ref = R.Counter(120, 200, [(0, 50, 200, 50)], table, capacity=8, expire=3)
    ref.update(np.stack([R.make_tracked(rows(y), 6, n_live=4) for y in (10, 90)]), 2)
    assert [e["id"] for e in ref.entries] == [1] and ref.totals[0] == [0, 1]
    assert not R.Counter(120, 200, [(0, 50, 200, 50)], table).update(np.stack([R.make_tracked(rows(10), 6)]), 1, gate=0).any()


def test_the_label_placement_and_the_draw():
    assert R.label_text(3, (10, 99999)) == "L3 +99999 -10" and R.label_text(0, (-1, 2147483647)) == "L0 +2147483647 -0"
    assert R.label_box((10, 10, 30, 20), "L0 +0 -0", 64, 300) == (20, 15, 96, 16)
    assert R.label_box((250, 60, 290, 62), "L0 +0 -0", 64, 300) == (204, 48, 96, 16)          # shifted inside on both axes
    assert R.label_box((-60, 8, 9, 8), "L0 +0 -0", 12, 60) == (-26, 8, 96, 16)                # fits on neither: stays at the anchor
    frame = np.full((40, 120, 3), 7, dtype=np.uint8)
    out = R.draw(frame, R.make_list(1, [(2, 1)]), [(5, 30, 110, 30)], 3, 1)
    x0, y0, bw, bh = R.label_box((5, 30, 110, 30), "L0 +1 -2", 40, 120)
    box = out[y0:y0 + bh, x0:x0 + bw]
    assert set(map(tuple, box.reshape(-1, 3))) == {(0, 0, 0), R.PALETTE[0]}
    assert (box[1:15, 1] == R.PALETTE[0]).all() and (box[0] == 0).all() and (box[:, 0] == 0).all()      # the stem of the L, the padding
    assert (out[30, 5:x0] == R.PALETTE[0]).all() and (out[28, 5:x0] == 7).all() and (out[29, 6:x0] == R.PALETTE[0]).all()
    assert np.array_equal(R.draw(frame, R.make_list(1, [(2, 1)]), [(5, 30, 110, 30)], 3, 0)[30, 5], R.PALETTE[0][::-1])
    assert np.array_equal(R.draw(frame, R.make_list(0, [(2, 1)]), [(5, 30, 110, 30)], 3, 1), frame)


# ------------------------------------------------------------------------------------------------------------ options and command line
def test_the_option():
    from faster_rcnn_amd import ops
    assert ops.count_option([(0, 0, 5, 5)]) == (((0, 0, 5, 5),), "all", 3)
    assert ops.count_option((1, 2, 3, 4), "car", 9) == (((1, 2, 3, 4),), ("car",), 9)
    assert ops.count_option([[np.int64(-32768), 0, 65535, 1]] * 8, ["car", "person"], np.int32(1)) == (((-32768, 0, 65535, 1),) * 8, ("car", "person"), 1)
    for bad, why in (([], "1..8 are possible"), ([(0, 0, 1, 1)] * 9, "9 of them"), ([(0, 0, 0, 0)], "A = B"), ([(0, 0, 1)], "four integers"),
                     ([(0, 0, 1, 65536)], "four integers"), ([(-32769, 0, 1, 1)], "four integers"), ([(0.5, 0, 1, 1)], "four integers"),
                     (5, "a list of"), ([(True, 0, 1, 1)], "four integers")):
        with pytest.raises(ValueError, match=why):
            ops.count_option(bad)
    for bad in (0, 10, True, 3.0, "3"):
        with pytest.raises(ValueError, match=r"count width=.*1\.\.9"):
            ops.count_option([(0, 0, 1, 1)], "all", bad)
    for bad in ((), 5, ("car", ""), ("car", 3)):
        with pytest.raises(ValueError, match="count classes="):
            ops.count_option([(0, 0, 1, 1)], bad)


def parse(*argv):
    from faster_rcnn_amd import annotate_video
    return annotate_video.count_from_args(annotate_video.build_parser().parse_args(["a.h5", "b.h5", "frames"] + list(argv)), MAPPING)


def test_the_command_line():
    assert parse() == (None, None) and parse("--track") == (None, None)
    assert parse("--track", "--count_line", "0,10,100,10") == ((((0, 10, 100, 10),), "all", 3), None)
    got = parse("--track", "--count_line", "0,10,100,10", "--count_line=-5,0,-5,65535", "--count_classes", "person,car",   # (a leading minus: the = form)
                "--count_width", "9", "--counts_out", "c.csv")
    assert got == ((((0, 10, 100, 10), (-5, 0, -5, 65535)), ("person", "car"), 9), "c.csv")
    assert parse("--track", "--count_line", "1,2,3,4", "--count_classes", "all")[0][1] == "all"
    line = ["--count_line", "0,0,5,5"]
    for argv, why in ((line, "needs --track"), (["--track"] + line * 9, "9 of them"), (["--track", "--count_line", "3,3,3,3"], "A = B"),
                      (["--track", "--count_line", "1,2,3"], "four integers X1,Y1,X2,Y2"), (["--track", "--count_line", "1,2,3,x"], "four integers"),
                      (["--track", "--count_line", "1;2;3;4"], "four integers"), (["--track", "--count_line", "0,0,1,70000"], "four integers"),
                      (["--track"] + line + ["--count_classes", "tram"], "unknown class name 'tram'"),
                      (["--track"] + line + ["--count_classes", ","], "comma-separated class names"),
                      (["--track"] + line + ["--count_width", "0"], r"count width=0.*1\.\.9"), (["--track", "--count_classes", "car"], "needs --count_line"),
                      (["--track", "--count_width", "3"], "needs --count_line"), (["--track", "--counts_out", "c.csv"], "needs --count_line")):
        with pytest.raises(ValueError, match=why):
            parse(*argv)


def test_the_python_arguments_are_checked_in_front_of_any_work():
    from faster_rcnn_amd import annotate_video
    assert annotate_video._count(None, None) is None
    assert annotate_video._count(([(0, 0, 9, 9)], "all", None), (30, 8, 0)) == (((0, 0, 9, 9),), "all", 3)
    with pytest.raises(ValueError, match="needs track="):
        annotate_video._count(([(0, 0, 9, 9)], "all", None), None)
    with pytest.raises(ValueError, match=r"\(lines, classes, width\)"):
        annotate_video._count([(0, 0, 9, 9)], (30, 8, 0))


def test_the_cache_key_and_the_refusals_in_front_of_any_capture():
    from faster_rcnn_amd import entry
    from faster_rcnn_amd._lib import FrcnnError
    count = (((0, 10, 100, 10),), "all", 3)
    spec = entry.PassSpec(annotate=True, track=(30, 8, 0), track_motion=8, track_trails=(16, 3), heat=("all", 160, 0))
    with_count = entry.PassSpec(annotate=True, track=(30, 8, 0), track_motion=8, track_trails=(16, 3), heat=("all", 160, 0), count=count)
    assert with_count.key_tail(4) == spec.key_tail(4) + ("count",) + count and "count" not in spec.key_tail(4)
    assert entry.PassSpec().count is None

    class Engine:                                                           # what ``PassSpec.checked`` asks of an engine
        device_preprocess = True
        batch = 4
        class_names = staticmethod(lambda: ["bg", "car", "person"])
        count_option = entry.DetectionEntry.count_option

        @staticmethod
        def track_option(track):
            return tuple(track)

    eng = Engine()
    got = entry.PassSpec.checked(eng, None, annotate=True, track=(30, 8, 0), count=([(0, 10, 100, 10)], None, None))
    assert got.count == count and got.key_tail(4)[-4:] == ("count",) + count
    assert entry.PassSpec.checked(eng, None, annotate=True, track=(30, 8, 0), draw=False, count=([(0, 0, 1, 1)], ["person"], 9)).count \
        == (((0, 0, 1, 1),), ("person",), 9)
    without = entry.PassSpec.checked(eng, None, annotate=True, track=(30, 8, 0))
    assert without.count is None and without.key_tail(4) == got.key_tail(4)[:-4]
    with pytest.raises(FrcnnError, match=r"count= counts the tracker's ids as they cross a line: pass track="):
        entry.PassSpec.checked(eng, None, annotate=True, count=count)
    for bad, why in ((([(0, 0, 0, 0)], "all", 3), "A = B"), (([(0, 0, 1, 1)] * 9, "all", 3), "9 of them"), (([(0, 0, 1, 1)], "tram", 3), "unknown class name 'tram'"),
                     (([(0, 0, 1, 1)], "all", 10), "count width=10"), ([(0, 0, 1, 1)], r"\(lines, classes, width\)")):
        with pytest.raises(FrcnnError, match=r"submit_batch: count=.*%s" % why):
            entry.PassSpec.checked(eng, None, annotate=True, track=(30, 8, 0), count=bad)


def test_the_csv_rows_and_the_printed_totals(capsys):
    from faster_rcnn_amd import annotate_video as av
    names = ["bg", "car", "person"]
    assert av.COUNTS_HEADER == "frame,line,direction,id,cls"
    assert av.counts_rows(7, [(0, 1, 12, 1), (3, 0, 5, 2), (1, 1, 9, 40)], names) == ["7,0,+,12,car", "7,3,-,5,person", "7,1,+,9,40"]
    assert av.counts_rows(1, [], names) == []
    av.print_counts(2, [(1, 4), (0, 2)] + [(0, 0)] * 6, {"person": [1, 0], "car": [0, 6]}, 0)
    assert capsys.readouterr().out.splitlines() == ["line 0: +4 -1", "line 1: +2 -0", "crossings of car: +6 -0", "crossings of person: +0 -1"]
    av.print_counts(1, [(0, 70)] + [(0, 0)] * 7, {"car": [0, 64]}, 6)
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "line 0: +70 -0" and out[-1].startswith("warning: 6 crossings did not fit") and "the totals are exact" in out[-1]


# ------------------------------------------------------------------------------------------------------------ header and binding
def test_header_binding_and_library_agree():
    from faster_rcnn_amd import _lib, ops
    from faster_rcnn_amd.build import build_library
    ext = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_count.h")).read()
    version = int(re.search(r"#define FRCNN_COUNT_VERSION (\d+)", ext).group(1))
    assert version == _lib.COUNT_VERSION == 1 and re.search(r"^ \*   1 = ", ext, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    names = sorted(set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", code)))
    assert names == sorted(_lib.COUNT_SIGNATURES) == ["frcnn_count_draw_u8", "frcnn_count_list_words", "frcnn_count_state_bytes", "frcnn_count_update",
                                                      "frcnn_count_version"]
    build_library(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        m = re.search(r"\b(int|size_t) %s\s*\(([^)]*)\)" % name, code)
        assert m, name
        decls = [d for d in m.group(2).split(",") if d.strip() != "void"]
        restype, argtypes = _lib.COUNT_SIGNATURES[name]
        assert restype is {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[m.group(1)] and len(argtypes) == len(decls), name
        for decl, ct in zip(decls, argtypes):
            assert ("*" in decl) == (ct is ctypes.c_void_p), (name, decl)
            assert ("long long" in decl) == (ct is ctypes.c_longlong), (name, decl)
        assert hasattr(lib, name), name
    define = lambda k: int(re.search(r"#define FRCNN_COUNT_%s \(?(-?\d+)\)?$" % k, ext, flags=re.M).group(1))
    assert define("MAX_LINES") == _lib.COUNT_MAX_LINES == R.MAX_LINES and define("MAX_EVENTS") == _lib.COUNT_MAX_EVENTS == R.MAX_EVENTS
    assert (define("MIN_COORD"), define("MAX_COORD")) == _lib.COUNT_COORD == R.COORD
    assert (1, define("MAX_WIDTH"), define("DEFAULT_WIDTH")) == _lib.COUNT_WIDTH == R.WIDTH and define("MAX_EXPIRE") == _lib.COUNT_MAX_EXPIRE == R.MAX_EXPIRE
    assert _lib.COUNT_LIST_WORDS == R.LIST_WORDS == 276 and (ops.COUNT_HEAD, ops.COUNT_ENTRY) == (R.HEAD, R.ENTRY)
    core = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    ext_dir = os.path.join(ROOT, "include", "ext")
    others = "".join(open(os.path.join(ext_dir, f)).read() for f in sorted(os.listdir(ext_dir)) if f != "frcnn_hip_count.h")
    assert not any(n in core or n in others for n in names)
    loaded = _lib.load()
    assert loaded.frcnn_count_version() == version and loaded.frcnn_count_list_words() == 276
    assert loaded.frcnn_version() == _lib.ABI_VERSION == int(re.search(r"#define FRCNN_ABI_VERSION (\d+)", core).group(1))
    size = loaded.frcnn_count_state_bytes
    assert size(1) == 4 * 26 and size(128) == 4 * (20 + 6 * 128) and size(0) == size(129) == size(-1) == 0
    # the draw kernels' glyph rows (csrc/overlay.h: the count and the zone labels' glyphs in one table) are the font's
    src = open(os.path.join(ROOT, "faster_rcnn_amd", "csrc", "overlay.h")).read()
    from faster_rcnn_amd import annotate_font
    table = re.search(r"OV_GLYPHS\[16\]\[7\] = \{(.*?)\};", src, flags=re.S).group(1)
    rows = np.array([int(v, 16) for v in re.findall(r"0x[0-9A-Fa-f]{2}", table)]).reshape(16, 7)
    assert np.array_equal(rows, np.stack([annotate_font.glyph(c) for c in " +-/0123456789LZ"]))
    palette = re.search(r"OV_PALETTE\[8\]\[3\] = \{(.*?)\};", src, flags=re.S).group(1)
    assert tuple(map(tuple, np.array(re.findall(r"\d+", palette), dtype=int).reshape(8, 3))) == R.PALETTE


def test_the_counts_log_and_the_one_frame_writer(tmp_path):
    import io
    from faster_rcnn_amd import annotate_video as av
    names = ["bg", "car", "person"]
    log = av.CountsLog(str(tmp_path / "c.csv"), names)
    log.add(1, [(0, 1, 12, 1)])
    log.add(3, [(1, 0, 5, 2), (0, 1, 7, 1)])
    log.close()
    log.close()                                                              # (closing twice is harmless: the error path closes again)
    assert (tmp_path / "c.csv").read_text().splitlines() == ["frame,line,direction,id,cls", "1,0,+,12,car", "3,1,-,5,person", "3,0,+,7,car"]
    assert log.per_class == {"car": [0, 2], "person": [1, 0]}
    silent = av.CountsLog(None, names)
    silent.add(1, [(0, 0, 1, 9)])
    assert silent.per_class == {"9": [1, 0]} and silent.file is None
    out = io.StringIO()
    av._write_counts(out, 4, [(2, 1, 3, 2)], MAPPING)
    av._write_counts(None, 4, [(2, 1, 3, 2)], MAPPING)
    av._write_counts(silent, 2, [(0, 1, 1, 1)], MAPPING)
    assert out.getvalue() == "4,2,+,3,person\n" and silent.per_class["car"] == [0, 1]
    assert "--count_line=-5,0,-5,100" in "".join(av.build_parser().format_help().split())       # (the help says how a leading minus is written)
