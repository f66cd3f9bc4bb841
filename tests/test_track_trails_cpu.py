"""Host-only checks of the trail rule's restatement (tests/track_trails_ref.py) against hand-made cases, of ops.track_trails_option and of
annotate_video's --track_trails / --trail_width parsing and refusals.  No GPU."""
import math

import numpy as np
import pytest

from tests import track_trails_ref as R

H, W = 40, 60


def buffer(rows, n_live, boxes, ids, cls=None):
    """A tracked buffer of ``rows`` rows by hand: ``boxes`` / ``ids`` fill rows 0.., ``n_live`` says how many of them are live."""
    b = np.zeros(4 + 8 * rows, dtype=np.int32)
    b[4:4 + 5 * rows] = -1
    b[0], b[1] = len(ids), n_live
    for r, (box, i) in enumerate(zip(boxes, ids)):
        b[4 + 4 * r:8 + 4 * r] = box
        b[4 + 4 * rows + r] = 1 if cls is None else cls[r]
        b[4 + 6 * rows + r] = i
    return b


def box_at(x, y):
    return [x - 2, y - 2, x + 2, y + 2]


def one(t, ids_at, rows=6):
    """One frame with a live row per (id, x, y)."""
    return t.frame(buffer(rows, len(ids_at), [box_at(x, y) for _, x, y in ids_at], [i for i, _, _ in ids_at]))


# ------------------------------------------------------------------------------------------------------------ ring and expiry
def test_the_ring_keeps_the_last_n_points_in_order():
    t = R.Trails(H, W, capacity=4, length=3, expire=2)
    for f in range(7):
        plist = one(t, [(5, 10 + f, 20)])
    assert R.trails_of(plist, 3) == [(5, [(14, 20), (15, 20), (16, 20)])]
    assert t.words()[:4].tolist() == [1, 7, 0, 0] and t.words()[4:8].tolist() == [5, 1, 7, 3]
    assert t.words()[8:14].tolist() == [14, 20, 15, 20, 16, 20] and not t.words()[14:].any()


@pytest.mark.parametrize("gap,kept", [(2, True), (3, False)])
def test_an_id_absent_for_e_frames_keeps_its_trail_and_for_one_more_loses_it(gap, kept):
    t = R.Trails(H, W, capacity=4, length=8, expire=2)
    one(t, [(3, 10, 10)])
    one(t, [(3, 12, 10)])
    for _ in range(gap):
        assert R.trails_of(one(t, []), 8) == []                             # (not live: not in the frame's list)
    got = R.trails_of(one(t, [(3, 20, 10)]), 8)
    assert got == [(3, [(10, 10), (12, 10), (20, 10)] if kept else [(20, 10)])]


def test_the_point_is_the_centre_of_the_clipped_box():
    assert R.point([-10, -10, 5, 6], H, W) == (2, 3)
    assert R.point([50, 30, 200, 100], H, W) == ((50 + W - 1) >> 1, (30 + H - 1) >> 1)
    assert R.point([9, 8, 3, 2], H, W) == (6, 5)                             # (corners in any order)
    assert R.point([W, 0, W + 5, 5], H, W) is None and R.point([0, -9, 5, -1], H, W) is None


# ------------------------------------------------------------------------------------------------------------ input rows
def test_held_backfilled_and_untracked_rows_are_never_read():
    """A widened buffer by hand: two live rows (one untracked), a held row, a back-filled row."""
    rows = 10
    b = buffer(rows, 2, [box_at(10, 10), box_at(30, 10), box_at(20, 30), box_at(40, 30)], [7, 0, 4, 9])
    b[4 + 7 * rows + 2], b[4 + 7 * rows + 3] = 2, -1                        # ages: held, back-filled
    t = R.Trails(H, W, capacity=4, length=4, expire=0)
    assert R.trails_of(t.frame(b), 4) == [(7, [(10, 10)])]
    assert [e["id"] for e in t.entries] == [7] and t.dropped == 0
    # an empty box gets no point either
    b2 = buffer(rows, 2, [[W + 3, 0, W + 9, 5], box_at(30, 10)], [8, 7])
    assert R.trails_of(t.frame(b2), 4) == [(7, [(10, 10), (30, 10)])]


def test_a_full_table_counts_dropped_and_leaves_the_other_trails_alone():
    t = R.Trails(H, W, capacity=2, length=4, expire=5)
    one(t, [(2, 5, 5), (4, 9, 9)])
    plist = one(t, [(2, 6, 5), (3, 20, 20), (4, 10, 9), (9, 30, 30)])
    assert R.trails_of(plist, 4) == [(2, [(5, 5), (6, 5)]), (4, [(9, 9), (10, 9)])]
    assert t.dropped == 2 and t.words()[:4].tolist() == [2, 2, 2, 0]
    # ids are inserted in id order, wherever their rows stand
    t2 = R.Trails(H, W, capacity=4, length=4, expire=5)
    one(t2, [(9, 5, 5), (2, 9, 9), (5, 1, 1)])
    assert [e["id"] for e in t2.entries] == [2, 5, 9]


def test_padding_frames_and_no_frames():
    t = R.Trails(H, W, capacity=3, length=3, expire=1)
    bufs = np.stack([buffer(6, 1, [box_at(10 + f, 10)], [1]) for f in range(4)])
    out = t.update(bufs, 2)
    assert out.shape == (4, R.list_words(3, 3)) and out[0, 0] == 1 and out[1, 0] == 1 and not out[2:].any() and t.frames == 2
    before = t.words().copy()
    for nf in (0, -3):
        assert not t.update(bufs, nf).any() and np.array_equal(t.words(), before)
    assert not t.update(bufs, 4, gate=0).any() and np.array_equal(t.words(), before)      # a gate word of 0: no frame is real
    assert t.update(bufs, 9, gate=-1)[3, 0] == 1 and t.frames == 6           # (more than the call holds: all of them)


def test_one_call_or_two():
    bufs = np.stack([buffer(6, 2, [box_at(10 + 2 * f, 10), box_at(40 - f, 20 + f)], [1, 2 + f // 3]) for f in range(6)])
    a, b = R.Trails(H, W, 4, 3, 1), R.Trails(H, W, 4, 3, 1)
    whole = a.update(bufs, 6)
    parts = np.concatenate([b.update(bufs[:4], 4), b.update(bufs[4:], 2)])
    assert np.array_equal(whole, parts) and np.array_equal(a.words(), b.words())


# ------------------------------------------------------------------------------------------------------------ drawing
CROSSING = [(3, 1, [(2, 5), (50, 30), (55, 8)]), (11, 2, [(5, 35), (52, 4)]), (6, 1, [(30, 0), (30, 39), (10, 20)])]


@pytest.mark.parametrize("rgb", [0, 1])
@pytest.mark.parametrize("width", [1, 3, 9])
def test_highest_id_wins_is_painting_in_ascending_id_order(width, rgb):
    frame = np.random.RandomState(3).randint(0, 256, (H, W, 3)).astype(np.uint8)
    plist = R.make_list(CROSSING, 4, 4)
    a, b = R.draw(frame, plist, 4, width, rgb), R.draw_highest(frame, plist, 4, width, rgb)
    assert np.array_equal(a, b) and (a != frame).any()
    # ids 3 and 11 share id & 7, and so a colour; 6 has another; where 11 and 6 cross, 11 is on top
    top = R.PALETTE[3] if rgb else R.PALETTE[3][::-1]
    crossing = R.segment_mask((5, 35), (52, 4), H, W, width) & R.segment_mask((30, 0), (30, 39), H, W, width)
    assert crossing.any() and (a[crossing] == top).all()
    # the order of the list does not matter either
    assert np.array_equal(R.draw(frame, R.make_list(CROSSING[::-1], 4, 4), 4, width, rgb), a)
    # a trail with one point has no segment
    assert np.array_equal(R.draw(frame, R.make_list([(5, 1, [(9, 9)])], 4, 4), 4, width, rgb), frame)


def float_distance(a, b, px, py):
    dx, dy = b[0] - a[0], b[1] - a[1]
    dd = dx * dx + dy * dy
    t = 0.0 if dd == 0 else min(max(((px - a[0]) * dx + (py - a[1]) * dy) / dd, 0.0), 1.0)
    return math.hypot(px - (a[0] + t * dx), py - (a[1] + t * dy))


# segments on a 40 x 40 grid whose pixels all keep 1e-6 from the capsule's boundary (checked below): axis-parallel, 45 degrees, shallow,
# steep, reversed, a point, and ends outside the grid
SEGMENTS = [((5, 20), (33, 20)), ((20, 3), (20, 36)), ((4, 4), (30, 30)), ((35, 6), (8, 33)), ((2, 10), (37, 17)), ((31, 38), (24, 1)),
            ((17, 17), (17, 17)), ((-6, 12), (14, -5)), ((30, 30), (47, 44))]


@pytest.mark.parametrize("width", [1, 3, 5, 9])
def test_the_capsule_test_against_a_float64_distance(width):
    """``covers`` against the distance to the segment in float64: covered exactly when the distance is at most W / 2.  The rule's three
    comparisons are exact (the squared distance to an end is a whole number, the side's is cross^2 / dd, and a whole number is at most
    floor(q) exactly when it is at most q), so only a pixel ON the boundary could differ, where float64 cannot decide.  With an odd W no
    pixel of these segments is: 4 cross^2 = W^2 dd and 4 |p|^2 = W^2 have no solutions here, and the test checks the margin itself.  (An
    even W always has such pixels -- one W / 2 beyond an end -- which is why they are left to the exact check below.)"""
    n = 40
    for a, b in SEGMENTS:
        compared = 0
        for py in range(n):
            for px in range(n):
                d = float_distance(a, b, px, py)
                assert abs(d - width / 2) >= 1e-6, (a, b, px, py)            # the cases were chosen so
                assert R.covers(a, b, px, py, width) == (d < width / 2), (a, b, px, py, width)
                compared += 1
        assert compared == n * n                                            # no pixel is left out


def test_a_pixel_on_the_boundary_is_covered():
    """W = 2 and 4, exactly: the pixels at distance W / 2 are inside, one further is not."""
    a, b = (10, 10), (20, 10)
    for width, r in ((2, 1), (4, 2)):
        for p in ((10 - r, 10), (20 + r, 10), (15, 10 - r), (15, 10 + r), (10, 10 + r)):
            assert R.covers(a, b, p[0], p[1], width), (width, p)
        for p in ((10 - r - 1, 10), (20 + r + 1, 10), (15, 10 - r - 1), (15, 10 + r + 1)):
            assert not R.covers(a, b, p[0], p[1], width), (width, p)
    assert R.covers((3, 4), (3, 4), 3, 4, 1) and not R.covers((3, 4), (3, 4), 4, 4, 1)     # a point, W = 1: itself


def test_segment_mask_tests_every_pixel_the_segment_can_cover():
    for a, b in SEGMENTS:
        m = R.segment_mask(a, b, 40, 40, 9)
        full = np.array([[R.covers(a, b, x, y, 9) for x in range(40)] for y in range(40)])
        assert np.array_equal(m, full)


# ------------------------------------------------------------------------------------------------------------ the option
def test_track_trails_option():
    from faster_rcnn_amd import ops
    assert ops.TRACK_TRAILS == ((2, 64, 16), (1, 9, 3), 4095) and (R.LENGTH, R.WIDTH, R.MAX_EXPIRE) == ops.TRACK_TRAILS
    assert ops.track_trails_option() == (16, 3) and ops.track_trails_option(None) == (16, 3)
    assert ops.track_trails_option(2) == (2, 3) and ops.track_trails_option((64, 9)) == (64, 9)
    assert ops.track_trails_option((None, 1)) == (16, 1) and ops.track_trails_option([5, None]) == (5, 3)
    assert ops.track_trails_option(np.int64(7)) == (7, 3)
    for bad in (1, 65, 0, -3, True, (16.0, 3), ("16", 3), (1, 3), (65, 3), (True, 3)):
        with pytest.raises(ValueError, match="track trails length="):
            ops.track_trails_option(bad)
    for bad in (0, 10, -1, True, 3.0, "3"):
        with pytest.raises(ValueError, match="track trails width="):
            ops.track_trails_option((16, bad))
    for bad in ((16,), (16, 3, 1), "abc", 16.0):
        with pytest.raises(ValueError, match="track trails"):
            ops.track_trails_option(bad)


def parse(*argv):
    from faster_rcnn_amd import annotate_video
    return annotate_video.track_trails_from_args(annotate_video.build_parser().parse_args(["a.h5", "b.h5", "frames"] + list(argv)))


def test_the_command_line():
    assert parse() is None and parse("--track") is None
    assert parse("--track", "--track_trails") == (16, 3)
    assert parse("--track", "--track_trails", "40") == (40, 3)
    assert parse("--track", "--track_trails", "--trail_width", "1") == (16, 1)
    assert parse("--track", "--track_motion", "--detect_every", "2", "--track_trails", "2", "--trail_width", "9") == (2, 9)
    assert parse("--track", "--track_lookback", "--track_trails", "64") == (64, 3)
    with pytest.raises(ValueError, match=r"--trail_width=5 .* needs --track_trails"):
        parse("--track", "--trail_width", "5")
    with pytest.raises(ValueError, match=r"--track_trails=16 .* needs --track$"):
        parse("--track_trails")
    with pytest.raises(ValueError, match=r"--track_trails together with --no_draw is not supported"):
        parse("--track", "--track_trails", "--no_draw", "--redact", "all")
    for n in ("1", "65", "0", "-4"):
        with pytest.raises(ValueError, match=r"--track_trails / --trail_width: track trails length="):
            parse("--track", "--track_trails", n)
    for w in ("0", "10", "-1"):
        with pytest.raises(ValueError, match=r"--track_trails / --trail_width: track trails width="):
            parse("--track", "--track_trails", "--trail_width", w)


def test_the_api_refusals():
    from faster_rcnn_amd import annotate_video
    assert annotate_video._track_trails(None, None, True) is None
    assert annotate_video._track_trails((5, 2), (30, 8, 0), True) == (5, 2)
    with pytest.raises(ValueError, match=r"track_trails=\(5, 2\) .* needs track="):
        annotate_video._track_trails((5, 2), None, True)
    with pytest.raises(ValueError, match=r"track_trails=.* together with draw=False is not supported"):
        annotate_video._track_trails((5, 2), (30, 8, 0), False)
    with pytest.raises(ValueError, match="track trails length"):
        annotate_video._track_trails((1, 2), (30, 8, 0), True)


def test_the_cache_key_and_the_expiry():
    from faster_rcnn_amd import entry
    spec = entry.PassSpec(annotate=True, track=(30, 8, 0), track_motion=8)
    with_trails = entry.PassSpec(annotate=True, track=(30, 8, 0), track_motion=8, track_trails=(16, 3))
    assert with_trails.key_tail(4) == spec.key_tail(4) + ("trails", 16, 3) and "trails" not in spec.key_tail(4)
    assert entry.PassSpec().track_trails is None
    expire = entry.DetectionEntry.track_trails_expire
    assert expire((30, 8, 0), None) == 9 and expire((30, 8, 0), 4) == 36 and expire((30, 0, 0), None) == 1
    assert expire((30, 255, 0), 16) == 4095                                  # (the rule's largest)
