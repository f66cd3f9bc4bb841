"""The zone rule without a GPU: the restatement (tests/zone_ref.py) against the hand cases' literal expectations, the header's constants
against the binding's, ``ops.zone_option``'s checks, annotate_video's command line (``--zone`` and its companions, the ``=`` form, the
refusals), the ``--zones_out`` CSV writer, the summary lines printed at the end, and the pass key."""
import os
import re

import numpy as np
import pytest

from tests import zone_ref as R

CLASSES = np.array([0, 1, 0, 1, 1], dtype=np.uint8)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ext", "frcnn_hip_zone.h")


@pytest.mark.parametrize("case", R.HAND_CASES, ids=[c[0] for c in R.HAND_CASES])
def test_the_reference_gives_the_hand_cases_answers(case):
    _, (h, w), zones, anchor, expire, frames, answers, totals = case
    ref = R.Zones(h, w, zones, CLASSES, 4, expire, anchor)
    lists = ref.update(R.hand_buffers(frames), len(frames))
    assert [[(z, k, i, d) for z, k, i, _, d in R.events_of(l)] for l in lists] == [[tuple(a) for a in ans] for ans in answers]
    n = len(zones)
    assert (ref.visitors[:n], ref.stays[:n], ref.dwell[:n], ref.peak[:n]) == totals
    assert all(int(l[1]) == f + 1 for f, l in enumerate(lists))
    words = ref.words()
    assert words.size == R.state_words(4) and not words[R.HEAD + R.ENTRY * len(ref.entries):].any()


def test_the_hand_cases_cover_what_the_rule_promises():
    names = " | ".join(c[0] for c in R.HAND_CASES)
    for what in ("shared edge", "shared vertex", "turns back", "flaps", "first seen inside", "lost inside", "concave", "bow-tie", "beyond the frame",
                 "zone order", "centre:", "bottom:"):
        assert what in names, what
    # exactly one of two abutting zones owns every point of the line they share
    for y in range(10, 20):
        assert R.inside(R.A, (20, y)) + R.inside(R.B, (20, y)) == 1
    # and the whole-frame test is the pixel test
    for zn in (R.A, R.C, R.BOW):
        m = R.inside_mask(zn, 32, 40)
        assert all(m[y, x] == R.inside(zn, (x, y)) for y in range(32) for x in range(40))


def test_the_header_s_constants_are_the_binding_s():
    from faster_rcnn_amd import _lib
    text = open(HEADER).read()
    val = lambda name: re.search(r"#define FRCNN_ZONE_%s \(?(-?\d+)" % name, text).group(1)
    assert int(val("VERSION")) == _lib.ZONE_VERSION == 1
    assert int(val("MAX_ZONES")) == _lib.ZONE_MAX_ZONES == R.MAX_ZONES
    assert (int(val("MIN_VERTS")), int(val("MAX_VERTS"))) == _lib.ZONE_VERTS == (R.MIN_VERTS, R.MAX_VERTS)
    assert int(val("MAX_EVENTS")) == _lib.ZONE_MAX_EVENTS == R.MAX_EVENTS
    assert (int(val("MIN_COORD")), int(val("MAX_COORD"))) == _lib.ZONE_COORD == R.COORD
    assert (1, int(val("MAX_WIDTH")), int(val("DEFAULT_WIDTH"))) == _lib.ZONE_WIDTH == R.WIDTH
    assert int(val("MAX_EXPIRE")) == _lib.ZONE_MAX_EXPIRE == R.MAX_EXPIRE
    assert _lib.ZONE_MAX_DWELL == R.MAX_DWELL == 1 << 30 and "FRCNN_ZONE_MAX_DWELL (1 << 30)" in text
    assert _lib.ZONE_HEAD_WORDS == R.HEAD == 36 and _lib.ZONE_ENTRY_WORDS == R.ENTRY == 13 and _lib.ZONE_LIST_WORDS == R.LIST_WORDS == 364
    assert set(_lib.ZONE_SIGNATURES) == {"frcnn_zone_version", "frcnn_zone_state_bytes", "frcnn_zone_list_words", "frcnn_zone_update", "frcnn_zone_draw_u8"}
    for name in _lib.ZONE_SIGNATURES:
        assert re.search(r"\b%s\(" % name, text), name


def test_zone_option_normalises():
    from faster_rcnn_amd import ops
    tri = ((1, 2), (30, 4), (5, 60))
    assert ops.zone_option([tri]) == ((tri,), "all", 3, 0)
    assert ops.zone_option(tri) == ((tri,), "all", 3, 0)                               # one polygon alone
    assert ops.zone_option([1, 2, 30, 4, 5, 60]) == ((tri,), "all", 3, 0)              # ... and flat
    assert ops.zone_option([[1, 2, 30, 4, 5, 60], tri], ["car"], 9, "bottom") == ((tri, tri), ("car",), 9, 1)
    assert ops.zone_option([tri], "all", np.int64(1), "centre")[2:] == (1, 0) and ops.zone_option([tri], anchor=1)[3] == 1
    assert ops.zone_option([[(-32768, -32768), (65535, 0), (0, 65535)]])[0][0][0] == (-32768, -32768)
    assert len(ops.zone_option([tri] * 8)[0]) == 8 and len(ops.zone_option([[(i, i * i) for i in range(16)]])[0][0]) == 16
    assert ops.ZONE_KINDS == ("exit", "enter", "lost") and ops.ZONE_ANCHORS == ("centre", "bottom")


@pytest.mark.parametrize("bad", [dict(zones=[]), dict(zones=[((1, 2), (3, 4), (5, 6))] * 9), dict(zones=[((1, 2), (3, 4))]), dict(zones=[[(i, i * i) for i in range(17)]]),
                                 dict(zones=[((1, 2), (1, 2), (5, 6))]), dict(zones=[((1, 2), (5, 6), (1, 2))]), dict(zones=[((1, 2), (3, 4), (5, 65536))]),
                                 dict(zones=[((-32769, 2), (3, 4), (5, 6))]), dict(zones=[((1.5, 2), (3, 4), (5, 6))]), dict(zones=[(1, 2, 3, 4, 5, 6, 7)]),
                                 dict(zones=[((1, 2, 3), (3, 4), (5, 6))]), dict(zones=7), dict(classes=[]), dict(classes=[""]), dict(classes=3), dict(width=0),
                                 dict(width=10), dict(width=2.0), dict(width=True), dict(anchor="top"), dict(anchor=2), dict(anchor=True)])
def test_zone_option_refuses(bad):
    from faster_rcnn_amd import ops
    args = dict(zones=[((1, 2), (30, 4), (5, 60))])
    args.update(bad)
    with pytest.raises(ValueError):
        ops.zone_option(**args)


def test_the_five_options_with_classes_read_them_alike_each_under_its_own_name():
    from faster_rcnn_amd import ops
    tri, line = ((1, 2), (30, 4), (5, 60)), (1, 2, 30, 4)
    tail = ': "all", a class name or a list of class names'
    callers = {"heat classes": lambda c: ops.heat_option(c)[0], "remove classes": lambda c: ops.plate_option(c)[0],
               "count classes": lambda c: ops.count_option(line, c)[1], "zone classes": lambda c: ops.zone_option(tri, c)[1],
               "redact moving except_classes": lambda c: ops.redact_moving_option(except_classes=c)[6]}
    for what, call in callers.items():
        assert call("all") == call(["all"]) == "all" and call("car") == ("car",) and call(["car", "all"]) == ("car", "all")
        moving = what.startswith("redact moving")
        for bad, shown in ((3, "3"), (["car", ""], "['car', '']" if moving else "('car', '')"), ([7], "[7]" if moving else "(7,)")):
            with pytest.raises(ValueError) as e:
                call(bad)
            assert str(e.value) == "%s=%s%s" % (what, shown, tail)
    # None: "all" for count and zone, no class for the moving option's exceptions, refused by heat and remove; no name at all likewise
    assert callers["count classes"](None) == callers["zone classes"](None) == "all"
    assert callers["redact moving except_classes"](None) == callers["redact moving except_classes"]([]) == ()
    for what in ("heat classes", "remove classes"):
        for bad, shown in ((None, "None"), ([], "()")):
            with pytest.raises(ValueError) as e:
                callers[what](bad)
            assert str(e.value) == "%s=%s%s" % (what, shown, tail)
    for what in ("count classes", "zone classes"):
        with pytest.raises(ValueError) as e:
            callers[what](())
        assert str(e.value) == "%s=()%s" % (what, tail)


def test_the_lists_and_totals_read_back():
    from faster_rcnn_amd import ops
    case = next(c for c in R.HAND_CASES if c[0].startswith("two ids"))
    ref = R.Zones(*case[1], case[2], CLASSES, 4, case[4], case[3])
    lists = ref.update(R.hand_buffers(case[5]), len(case[5]))
    assert ops.zone_events(lists[1]) == [(0, 1, 1, 3, 0)] and ops.zone_occupancy(lists[1], 2) == [2, 0]
    assert ops.zone_events(lists[3]) == [(0, 2, 2, 1, 3)] and ops.zone_occupancy(lists[3], 2) == [0, 0]
    totals = ops.zone_totals(ref.words())
    assert totals == {"entries": 0, "frames": 4, "dropped": 0, "events_dropped": 0, "visitors": [2] + [0] * 7, "stays": [2] + [0] * 7,
                      "dwell": [4] + [0] * 7, "peak": [2] + [0] * 7}
    assert R.summary_figures(totals, 2) == [(2, 2, 2, 2.0), (0, 0, 0, None)]


MAPPING = {"bg": 0, "car": 1, "person": 2, "bike": 3}


def zone_args(*extra):
    """The parsed command line: the two model files, the frames' directory and ``extra``."""
    from faster_rcnn_amd import annotate_video
    return annotate_video.build_parser().parse_args(["a.h5", "b.h5", "frames"] + list(extra))


def test_the_command_line_gives_the_option():
    from faster_rcnn_amd import annotate_video
    args = zone_args("--track", "--zone", "10,10,20,10,20,20,10,20", "--zone=-5,0,9,0,9,9", "--zone_classes", "car, person", "--zone_width", "5",
                     "--zone_anchor", "bottom", "--zones_out", "z.csv")
    zone, out = annotate_video.zone_from_args(args, MAPPING)
    assert zone == ((((10, 10), (20, 10), (20, 20), (10, 20)), ((-5, 0), (9, 0), (9, 9))), ("car", "person"), 5, 1) and out == "z.csv"
    zone, out = annotate_video.zone_from_args(zone_args("--track", "--zone", "1,2,30,4,5,60"), MAPPING)
    assert zone == ((((1, 2), (30, 4), (5, 60)),), "all", 3, 0) and out is None
    assert annotate_video.zone_from_args(zone_args("--track"), MAPPING) == (None, None)
    assert annotate_video.zone_from_args(zone_args(), MAPPING) == (None, None)


@pytest.mark.parametrize("argv,match", [
    (("--zone", "1,2,30,4,5,60"), "needs --track"),
    (("--track", "--zone_classes", "car"), "needs --zone"), (("--track", "--zone_width", "2"), "needs --zone"),
    (("--track", "--zone_anchor", "bottom"), "needs --zone"), (("--track", "--zones_out", "z.csv"), "needs --zone"),
    (("--track", "--zone", "1,2,30,4"), "three vertices at least"), (("--track", "--zone", "1,2,30,4,5"), "even number"),
    (("--track", "--zone", "1,2,a,4,5,6"), "even number of integers"), (("--track", "--zone", "1,2,1,2,5,6"), "consecutive"),
    (("--track", "--zone", "1,2,3,4,5,70000"), "-32768..65535"), (("--track",) + ("--zone", "1,2,30,4,5,60") * 9, "1..8"),
    (("--track", "--zone", "1,2,30,4,5,60", "--zone_classes", "tram"), "tram"), (("--track", "--zone", "1,2,30,4,5,60", "--zone_classes", ","), "class names"),
    (("--track", "--zone", "1,2,30,4,5,60", "--zone_width", "10"), "1..9")])
def test_the_command_line_refuses(argv, match):
    from faster_rcnn_amd import annotate_video
    with pytest.raises(ValueError, match=match):
        annotate_video.zone_from_args(zone_args(*argv), MAPPING)


def test_the_parser_refuses_an_unknown_anchor_and_a_bare_minus(capsys):
    with pytest.raises(SystemExit):
        zone_args("--track", "--zone", "1,2,30,4,5,60", "--zone_anchor", "top")
    with pytest.raises(SystemExit):
        zone_args("--track", "--zone", "-5,0,9,0,9,9")                       # a leading minus needs the = form
    capsys.readouterr()


def test_the_csv_rows_and_the_log(tmp_path):
    from faster_rcnn_amd import annotate_video
    names = ["bg", "car", "person"]
    events = [(0, 1, 7, 1, 0), (2, 0, 7, 2, 12), (1, 2, 9, 5, 3)]
    rows = annotate_video.zones_rows(4, events, names)
    assert rows == ["4,0,enter,7,car,0", "4,2,exit,7,person,12", "4,1,lost,9,5,3"]
    path = tmp_path / "z.csv"
    log = annotate_video.ZonesLog(str(path), names)
    log.add(4, events)
    log.add(5, [])
    log.add(6, events[:1])
    log.close()
    log.close()
    assert path.read_text().splitlines() == [annotate_video.ZONES_HEADER, *rows, "6,0,enter,7,car,0"] and annotate_video.ZONES_HEADER == "frame,zone,kind,id,cls,dwell"
    annotate_video.ZonesLog(None, names).add(1, events)                      # no file: nothing to write
    import io
    text = io.StringIO()
    annotate_video._write_zones(text, 2, events[:2], {"bg": 0, "car": 1, "person": 2})
    assert text.getvalue().splitlines() == ["2,0,enter,7,car,0", "2,2,exit,7,person,12"]
    annotate_video._write_zones(None, 2, events, {"bg": 0})


def test_the_summary_lines(capsys):
    from faster_rcnn_amd import annotate_video
    totals = {"entries": 1, "frames": 9, "dropped": 0, "events_dropped": 0, "visitors": [3, 0, 1] + [0] * 5, "stays": [4, 0, 0] + [0] * 5,
              "dwell": [10, 0, 0] + [0] * 5, "peak": [2, 0, 1] + [0] * 5}
    annotate_video.print_zones(3, totals)
    assert capsys.readouterr().out.splitlines() == ["zone 0: visitors 3 peak 2 stays 4 mean dwell 2.5 frames", "zone 1: visitors 0 peak 0 stays 0 mean dwell -",
                                                    "zone 2: visitors 1 peak 1 stays 0 mean dwell -"]
    annotate_video.print_zones(1, dict(totals, events_dropped=7))
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 2 and out[1].startswith("warning: 7 zone events did not fit")


def test_the_one_frame_and_list_calls_refuse_by_name():
    from faster_rcnn_amd import annotate_video
    tri = (((1, 2), (30, 4), (5, 60)),)
    with pytest.raises(ValueError, match="needs track="):
        annotate_video._zone((tri, "all", 3, 0), None)
    with pytest.raises(ValueError, match=r"\(zones, classes, width, anchor\)"):
        annotate_video._zone((tri, "all"), (30, 2, 1))
    assert annotate_video._zone((tri, None, None, "bottom"), (30, 2, 1)) == (tri, "all", 3, 1) and annotate_video._zone(None, None) is None


def test_the_pass_key_carries_the_zone_tag_behind_count():
    from faster_rcnn_amd import ops
    from faster_rcnn_amd.entry import PassSpec
    zone = ops.zone_option([((1, 2), (30, 4), (5, 60))], "all", 2, "bottom")
    count = (((20, 0, 20, 47),), "all", 3)
    plain = PassSpec(annotate=True, track=(30, 2, 1), count=count)
    assert PassSpec(annotate=True, track=(30, 2, 1), count=count, zone=zone).key_tail(2) == plain.key_tail(2) + ("zone",) + zone
    assert PassSpec().zone is None
