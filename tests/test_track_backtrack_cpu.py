"""The back-track rule's numpy restatement (tests/track_backtrack_ref.py) on its own: its identities, the order and place of its rows, and
the option parsing and refusals of the layers above it.  No GPU."""
import os
import re

import numpy as np
import pytest

from tests import track_backtrack_ref as BT
from tests import track_lookback_ref as LB
from tests import track_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, ROWS, CAP = 48, 64, 8, 4
R = ROWS + CAP


def crafted(R, live, next_id, held=()):
    """A tracked buffer of R rows: ``live`` = [(box, cls, id)], ``held`` = [(box, cls, id, age)]."""
    buf = np.zeros(4 + 8 * R, dtype=np.int32)
    buf[4:4 + 5 * R] = -1
    rows = [(b, c, i, 0) for b, c, i in live] + list(held)
    for r, (box, cls, tid, age) in enumerate(rows):
        buf[4 + 4 * r:8 + 4 * r] = box
        buf[4 + 4 * R + r], buf[4 + 5 * R + r], buf[4 + 6 * R + r], buf[4 + 7 * R + r] = cls, T.bits(0.75), tid, age
    buf[:4] = (len(rows), len(live), next_id, 0)
    return buf


def seen(o, t):
    """Object 0 from the start, 1 from frame 3, 2 from frame 6 (frame 0 of a second call of 6), 3 from frame 9; object 0 is not seen in
    frame 6 (held there) and matched again in frame 9."""
    return t >= (0, 3, 6, 9)[o] and not (o == 0 and t == 6)


def ids_ages(buf):
    return [(tid, -k) for tid, k, _ in BT.backfilled(buf)]


def test_interval_one_is_the_look_back_rule_byte_for_byte():
    frames, _, tracked = LB.sequence(H, W, 9, 3, ROWS, CAP, objects=2, hold=2, grow=1)
    for B, sizes, lookback, radius in ((4, (4, 4, 1), 4, 4), (4, (4, 2, 3), 3, 1), (2, (2, 2, 2, 2, 1), 2, 0), (3, (3, 3, 3), 1, 4)):
        a, b = LB.Window(B, H, W, ROWS, CAP, 2), BT.Window(B, H, W, ROWS, CAP, 2)
        at, filled = 0, 0
        for n in list(sizes) + [-1]:
            real = max(n, 0)
            fs = list(frames[at:at + real]) + [np.zeros((H, W, 3), dtype=np.uint8)] * (B - real)
            ts = list(tracked[at:at + real]) + [np.zeros(4 + 8 * R, dtype=np.int32)] * (B - real)
            want, got = a.call(fs, ts, n, lookback, radius, 1), b.call(fs, ts, n, lookback, radius, 1, interval=1)
            assert len(want[0]) == len(got[0])
            assert all(np.array_equal(x, y) for x, y in zip(want[0] + want[1], got[0] + got[1]))
            assert np.array_equal(a.state_bytes(), b.state_bytes())
            filled += sum(len(BT.backfilled(buf)) for buf in got[1])
            at += real
        assert filled > 0


@pytest.mark.parametrize("lookback", (2, 3))
@pytest.mark.parametrize("radius", (0, 4))
def test_the_emitted_sequence_does_not_depend_on_the_cut(lookback, radius):
    """12 frames with K = 3 in full calls with L <= F (the identity's conditions): calls of 6 + 6, of 3 + 3 + 3 + 3 and one of 12."""
    K = 3
    frames, tracked = BT.sequence(H, W, 12, K, 5, ROWS, CAP, seen, per_call=6)
    got = [BT.run(BT.Window(F, H, W, ROWS, CAP, 4), frames, tracked, sizes, lookback, radius, 1, K)
           for F, sizes in ((6, (6, 6)), (3, (3, 3, 3, 3)), (12, (12,)))]
    assert all(len(g[1]) == 12 for g in got)
    for other in got[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(got[0][0] + got[0][1], other[0] + other[1]))
    assert all(np.array_equal(a, b) for a, b in zip(got[0][0], frames))
    filled = [ids_ages(b) for b in got[0][1]]
    assert sum(len(f) for f in filled) > 0
    for g in range(9):                                         # every between frame carries a row for every track the next key frame sees
        if g % K:
            t = (g // K + 1) * K
            live = [int(i) for i in T.split(got[0][1][t])[7][:T.split(got[0][1][t])[1]]]
            assert live and set(live) <= {tid for tid, _ in filled[g]}, (g, filled[g], live)
    if radius:
        assert BT.check_shifts(got[0][1], K, H, W, 4, grow=1) > 0


def test_one_frame_padded_calls_are_not_full_calls():
    """12 frames with K = 3 as calls of 6 + 6 and as 12 one-frame calls padded to F = 6.  The identity asks for FULL calls: a one-frame call
    leaves one frame in the window, and its frame is frame 0 of a call, a key frame, so nothing but a birth's k = 1 row can still arrive.
    What the two cuts do share: the frames, untouched and in order, and every row that is not back-filled; the padded cut's back-filled
    rows are the 6 + 6 cut's k = 1 rows of births, in the same order."""
    K, lookback = 3, 4
    frames, tracked = BT.sequence(H, W, 12, K, 5, ROWS, CAP, seen, per_call=6)
    whole = BT.run(BT.Window(6, H, W, ROWS, CAP, 4), frames, tracked, (6, 6), lookback, 4, 1, K)
    padded = BT.run(BT.Window(6, H, W, ROWS, CAP, 4), frames, tracked, (1,) * 12, lookback, 4, 1, K)
    assert len(whole[1]) == len(padded[1]) == 12
    assert all(np.array_equal(a, b) for a, b in zip(whole[0], padded[0]))
    births = set()
    for t in range(1, 12):
        births |= {(int(T.split(tracked[t])[7][r]), t) for r, b in BT.sources(tracked[t], int(tracked[t - 1][2]), CAP) if b}
    assert births == {(2, 3), (3, 6), (4, 9)}                             # (object 0, held in frame 6, is matched again in frame 9)
    for g, (a, b) in enumerate(zip(whole[1], padded[1])):
        n = T.split(tracked[g])[0]
        assert np.array_equal(LB.widen(tracked[g], R + 4)[4:4 + 4 * n], a[4:4 + 4 * n]) and np.array_equal(a[1:4], b[1:4])
        assert BT.backfilled(b) == [row for row in BT.backfilled(a) if row[1] == 1 and (row[0], g + 1) in births], g
    assert sum(len(BT.backfilled(b)) for b in padded[1]) == 3 < sum(len(BT.backfilled(a)) for a in whole[1])


def mixed_call(back, lookback=4):
    """One call of F = 6, K = 3 over crafted buffers: key frame 0 sees tracks 1 and 2; key frame 3 sees a row without a track (id 0), track
    2 again (a correction), new tracks 3 and 4 (births), and holds track 1.  -> (the window, the six buffers after a flush)."""
    box = lambda i: (4 + 6 * i, 5, 14 + 6 * i, 15)
    key0 = crafted(R, [(box(0), 1, 1), (box(1), 1, 2)], 3)
    key3 = crafted(R, [(box(5), 2, 0), (box(3), 1, 3), (box(1), 1, 2), (box(4), 2, 4)], 5, held=[(box(0), 1, 1, 1)])
    after = crafted(R, [(box(3), 1, 3), (box(1), 1, 2), (box(4), 2, 4)], 5, held=[(box(0), 1, 1, 1)])
    tracked = [key0, key0, key0, key3, after, after]
    frames = BT.rolled(H, W, 6, 7, (0, 0))
    win = BT.Window(6, H, W, ROWS, CAP, back)
    assert win.call(frames, tracked, 6, lookback, 0, 2, 3) == ([], [])
    chained = list(win.chained)
    _, out = win.call(frames, tracked, -1, lookback, 0, 2, 3)
    return win, out, chained


def test_order_and_place_of_corrections_and_births():
    win, out, chained = mixed_call(back=4)
    # the sources of key frame 3 in row order: rows 1, 2, 3 (row 0 has no track, the held row 4 is not live)
    assert [(t, r, birth) for t, r, birth, _ in chained] == [(3, 1, True), (3, 2, False), (3, 3, True)]
    assert [reached for _, _, _, reached in chained] == [[2, 1, 0], [2, 1], [2, 1, 0]]
    assert ids_ages(out[2]) == [(3, -1), (2, -1), (4, -1)] and ids_ages(out[1]) == [(3, -2), (2, -2), (4, -2)]
    assert ids_ages(out[0]) == [(3, -3), (4, -3)]             # the correction stopped in front of key frame 0
    assert all(ids_ages(out[g]) == [] for g in (3, 4, 5)) and win.back_overflow == 0
    for g in range(3):                                         # behind the frame's own rows; n_live does not move; grown by grow * k
        n_rows, n_live, _, _, bbox, cls, prob, ids, age = T.split(out[g])
        assert n_live == 2 and n_rows == 2 + len(ids_ages(out[g])) and ids[:2].tolist() == [1, 2] and age[:2].tolist() == [0, 0]
        e = 2 * (3 - g)
        assert bbox[2].tolist() == [4 + 18 - e, 5 - e, 14 + 18 + e, 15 + e] and cls[2] == 1 and prob[2] == T.bits(0.75)


def test_a_correction_stops_in_front_of_the_previous_key_frame_even_with_a_long_look_back():
    _, out, chained = mixed_call(back=4, lookback=6)
    assert [reached for _, _, birth, reached in chained if not birth] == [[2, 1]]
    assert (2, -3) not in ids_ages(out[0]) and [(2, -1)] == [x for x in ids_ages(out[2]) if x[0] == 2]


def test_rows_without_a_track_and_rows_of_between_frames_are_never_sources():
    _, out, chained = mixed_call(back=4)
    assert all(tid != 0 for buf in out for tid, _ in ids_ages(buf))
    assert {t for t, _, _, _ in chained} == {3}                # frames 1, 2, 4, 5 have live tracked rows and chain nothing
    assert BT.sources(crafted(R, [((1, 1, 9, 9), 1, 0), ((1, 1, 9, 9), 1, 7), ((1, 1, 9, 9), 1, 2)], 8), 7, CAP) == [(1, True), (2, False)]
    assert len(BT.sources(crafted(R, [((1, 1, 9, 9), 1, i) for i in range(1, 7)], 7), 1, CAP)) == CAP


def test_drop_order_and_back_overflow_with_one_row_of_room():
    """rows + capacity + back = 13 rows, frames 1 and 2 hold 2: no drop there.  A frame that is full up to its last row takes the first row
    of the order alone."""
    win, out, _ = mixed_call(back=1)
    assert win.back_overflow == 0 and ids_ages(out[2]) == [(3, -1), (2, -1), (4, -1)]
    box = (4, 5, 14, 15)
    full = crafted(R, [(box, 1, 1), (box, 1, 2)], 3, held=[(box, 1, 10 + i, 1) for i in range(R - 2)])       # every row of R in use
    key3 = crafted(R, [(box, 1, 3), (box, 1, 2), (box, 2, 4)], 5)
    key6 = crafted(R, [(box, 1, 3), (box, 1, 2), (box, 2, 4), (box, 1, 5)], 6)
    tracked = [full, full, full, key3, key3, key3]
    frames = BT.rolled(H, W, 6, 7, (0, 0))
    win = BT.Window(6, H, W, ROWS, CAP, 1)
    win.call(frames, tracked, 6, 6, 0, 0, 3)
    assert win.back_overflow == 2 + 2 + 1                      # frames 2 and 1: three rows for one place; frame 0: the two births
    out = win.call(frames, [key6] + [key3] * 5, 6, 6, 0, 0, 3)[1]
    assert [ids_ages(b) for b in out[:3]] == [[(3, -3)], [(3, -2)], [(3, -1)]]                               # the first of the order stays
    # the second call's key frame 6: its corrections reach frames 5 and 4, its birth (id 5) frames 5..0; frames 0..2 are full already
    assert win.back_overflow == 5 + 3
    out2 = win.call(frames, tracked, -1, 6, 0, 0, 3)[1]
    assert ids_ages(out2[0]) == []
    assert ids_ages(out[5]) == [(3, -1), (2, -1), (4, -1), (5, -1)] and ids_ages(out[3]) == [(5, -3)]
    assert all(T.split(b)[0] <= R + 1 for b in out)


def test_header_states_the_rule_and_the_binding_matches_it():
    text = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_track_backtrack.h")).read()
    from faster_rcnn_amd import _lib
    assert int(re.search(r"#define FRCNN_TRACK_BACKTRACK_VERSION (\d+)", text).group(1)) == _lib.TRACK_BACKTRACK_VERSION == 1
    for word in ("KEY", "SOURCE", "BIRTH", "CORRECTION", "CHAIN", "PLACE", "back_overflow", "age = -k", "int interval"):
        assert word in text
    assert "Back-track rule" in open(os.path.join(ROOT, "DESIGN.md")).read()
    look = _lib.TRACK_LOOKBACK_SIGNATURES["frcnn_track_lookback"][1]
    back = _lib.TRACK_BACKTRACK_SIGNATURES["frcnn_track_backtrack"][1]
    assert len(back) == len(look) + 1 and back[:13] == look[:13] and back[14:] == look[13:]


def test_option_checker():
    from faster_rcnn_amd import ops
    opt = ops.track_backtrack_option
    assert opt(None, 4, 8) == 8 and opt(None, 2, 32) == 16 and opt(True, 3, 6) == 6 and opt(3, 4, 8) == 3 and opt(np.int64(8), 4, 8) == 8
    for bad in (0, 17, -1, False, 2.0, "4"):
        with pytest.raises(ValueError, match="track backtrack=.*an integer in 1..16"):
            opt(bad, 2, 8)
    with pytest.raises(ValueError, match="frames no detection reaches would stay uncovered"):
        opt(2, 4, 8)
    with pytest.raises(ValueError, match="a frame would be emitted before its rows are in place"):
        opt(9, 4, 8)
    with pytest.raises(ValueError, match="frames no detection reaches would stay uncovered"):
        opt(None, 16, 8)                                       # min(16, 8) = 8 < K - 1 = 15


def test_parser_and_the_refusals_of_the_command_line():
    from faster_rcnn_amd import annotate_video as A
    parse = lambda *extra: A.build_parser().parse_args(["a.h5", "b.h5", "frames"] + list(extra))
    full = ("--track", "--track_motion", "--detect_every", "4")
    assert A.track_backtrack_from_args(parse(*full)) is None
    assert A.track_backtrack_from_args(parse(*full, "--track_backtrack")) == A.TRACK_BACKTRACK_AUTO
    assert A.track_backtrack_from_args(parse(*full, "--track_backtrack", "3")) == 3
    assert A.track_backtrack_from_args(parse(*full, "--track_backtrack", "16")) == 16
    for missing in (("--track", "--track_motion"), ("--track", "--detect_every", "4"), ("--track_motion", "--detect_every", "4"), ()):
        with pytest.raises(ValueError, match="--track_backtrack=5 .* needs --track --track_motion --detect_every K"):
            A.track_backtrack_from_args(parse(*missing, "--track_backtrack", "5"))
    with pytest.raises(ValueError, match="--track_backtrack together with --track_lookback is not supported"):
        A.track_backtrack_from_args(parse(*full, "--track_lookback", "2", "--track_backtrack"))
    for bad in ("17", "-1"):
        with pytest.raises(ValueError, match="--track_backtrack: .*an integer in 1..16"):
            A.track_backtrack_from_args(parse(*full, "--track_backtrack", bad))
    with pytest.raises(ValueError, match="--track_backtrack: .*frames no detection reaches would stay uncovered"):
        A.track_backtrack_from_args(parse(*full, "--track_backtrack", "2"))
    # the three refusals of --track_lookback + --detect_every stand as they were
    with pytest.raises(ValueError, match="--detect_every together with --track_lookback is not supported"):
        A.detect_every_from_args(parse(*full, "--track_lookback", "2", "--track_backtrack"))
    with pytest.raises(ValueError, match="detect_every=4 together with track_lookback=2 is not supported"):
        A._detect_every(4, (30, 8, 0), 8, 2, object(), 4)


def test_the_refusals_and_defaults_of_annotate_images_and_get_annotated_frame():
    from faster_rcnn_amd import annotate_video as A
    eng = object()
    assert A._backtrack_frames(None, 4, None, eng, 4) is None
    assert A._backtrack_frames(A.TRACK_BACKTRACK_AUTO, 4, None, eng, 2) == 8 and A._backtrack_frames(A.TRACK_BACKTRACK_AUTO, 4, None, eng, 8) == 16
    assert A._backtrack_frames(3, 4, None, eng, 2) == 3 and A._backtrack_frames(8, 4, None, eng, 2) == 8
    with pytest.raises(ValueError, match="it needs track=.*track_motion=R and detect_every=K"):
        A._backtrack_frames(4, None, None, eng, 4)
    with pytest.raises(ValueError, match="track_backtrack=4 together with track_lookback=2 is not supported"):
        A._backtrack_frames(4, 4, 2, eng, 4)
    with pytest.raises(ValueError, match="the eager path .* cannot"):
        A._backtrack_frames(4, 4, None, None, 4)
    with pytest.raises(ValueError, match="frames no detection reaches would stay uncovered"):
        A._backtrack_frames(2, 4, None, eng, 4)
    with pytest.raises(ValueError, match="a frame would be emitted before its rows are in place"):
        A._backtrack_frames(9, 4, None, eng, 2)
    with pytest.raises(ValueError, match="track_backtrack=4 delays the output: get_annotated_frame"):
        A.get_annotated_frame(None, None, None, None, 600, 1000, track_backtrack=4)
    mapping = {"car": 1, "bg": 0}
    det = lambda **kw: dict({"bbox": np.array([1, 2, 11, 22]), "cls_name": "car", "prob": np.float32(0.5), "track_id": 3}, **kw)
    dets = [det(propagated=True), det(track_id=4, held=2), det(track_id=5, backfilled=1)]
    assert A.mot_lines(7, dets, mapping) == ["7,3,1,2,10,20,0.500000,1,-1,-1"]
