"""The look-back rule's numpy restatement (tests/track_lookback_ref.py; DESIGN §8 "Look-back rule") on hand-worked sequences, and the
host-only parts of its binding.  No GPU."""
import os
import re

import numpy as np
import pytest

from tests import track_lookback_ref as LB
from tests import track_ref as T

H, W = 48, 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows_of(buf):
    n_rows, n_live, _, _, bbox, cls, prob, ids, age = T.split(buf)
    return n_rows, n_live, [(tuple(int(v) for v in bbox[r]), int(cls[r]), int(prob[r]), int(ids[r]), int(age[r])) for r in range(n_rows)]


def moving_square(n=6, first_seen=3):
    """A 16 x 16 textured square that moves +3 px a frame over a fixed texture, "detected" from frame ``first_seen`` on."""
    back, patch = LB.texture(H, W, 1), LB.texture(16, 16, 2)
    frames, tracked, tracker = [], [], T.Tracker(4)
    for t in range(n):
        x, y = 10 + 3 * t, 16
        frames.append(LB.paste(back, patch, x, y))
        dets = [(x, y, x + 15, y + 15, 1, 0.9)] if t >= first_seen else []
        tracked.append(tracker.update_packed(LB.packed(dets, 8), np.array([0, 1], dtype=np.uint8), H, W))
    return frames, tracked


@pytest.mark.parametrize("radius, step", [(4, 3), (0, 0)])
def test_moving_square(radius, step):
    frames, tracked = moving_square()
    win = LB.Window(6, H, W, 8, 4, 2)
    assert win.call(frames, tracked, 6, lookback=3, radius=radius) == ([], [])
    out_f, out_t = win.call(frames, tracked, -1, lookback=3, radius=radius)
    assert len(out_f) == 6 and all(np.array_equal(a, b) for a, b in zip(out_f, frames))      # the window is never drawn into
    birth = (19, 16, 34, 31)
    prob = T.bits(0.9)
    for g, k in ((2, 1), (1, 2), (0, 3)):
        n_rows, n_live, rows = rows_of(out_t[g])
        assert (n_rows, n_live) == (1, 0)
        assert rows[0] == ((birth[0] - step * k, birth[1], birth[2] - step * k, birth[3]), 1, prob, 1, -k)
    for g in (3, 4, 5):                                                                      # the birth frame and behind: as tracked
        assert np.array_equal(out_t[g], LB.widen(tracked[g], 14))
    assert (win.count, win.back_overflow) == (0, 0)


def test_lookback_shorter_than_the_gap_and_grow():
    frames, tracked = moving_square()
    win = LB.Window(6, H, W, 8, 4, 2)
    win.call(frames, tracked, 6, lookback=2, radius=4, grow=2)
    _, out_t = win.call(frames, tracked, -1, lookback=2, radius=4, grow=2)
    assert rows_of(out_t[0])[0] == 0                                                         # three frames back: out of reach
    assert rows_of(out_t[2])[2][0][0] == (16 - 2, 16 - 2, 31 + 2, 31 + 2)
    assert rows_of(out_t[1])[2][0][0] == (13 - 4, 16 - 4, 28 + 4, 31 + 4)


def test_no_births_leaves_the_tracked_rows():
    frames, tracked = moving_square(first_seen=0)                     # born in the sequence's first frame: nothing in front to fill
    win = LB.Window(3, H, W, 8, 4, 2)
    out_f, out_t = LB.run(win, frames, tracked, [3, 3], lookback=3, radius=4)
    assert len(out_t) == 6 and win.back_overflow == 0
    for g in range(6):
        assert np.array_equal(out_t[g], LB.widen(tracked[g], 14)) and np.array_equal(out_f[g], frames[g])


@pytest.mark.parametrize("lookback", [1, 4])
def test_partition_independence(lookback):
    frames, _, tracked = LB.sequence(H, W, 16, 11, rows=8, capacity=8, objects=3)
    got = []
    for B, sizes in ((4, [4, 4, 4, 4]), (8, [8, 8])):
        got.append(LB.run(LB.Window(B, H, W, 8, 8, 8), frames, tracked, sizes, lookback, radius=4, grow=1))
    assert len(got[0][1]) == len(got[1][1]) == 16
    assert sum(int((T.split(b)[8] < 0).sum()) for b in got[0][1]) > 0                        # the sequence has births to fill
    for a, b in zip(got[0][0] + got[0][1], got[1][0] + got[1][1]):
        assert np.array_equal(a, b)


def test_flush_and_zero_frames():
    frames, tracked = moving_square()
    win = LB.Window(3, H, W, 8, 4, 2)
    assert win.call(frames[:3], tracked[:3], 3, 3, 4) == ([], [])
    before = win.state_bytes().copy()
    again = [win.call(frames[3:], tracked[3:], 0, 3, 4) for _ in range(2)]                   # warm-up, capture: emits, writes nothing
    assert np.array_equal(win.state_bytes(), before) and win.count == 3
    for out_f, out_t in again:
        assert len(out_f) == 3 and all(np.array_equal(b, LB.widen(t, 14)) for b, t in zip(out_t, tracked[:3]))
    out_f, out_t = win.call(frames[3:], tracked[3:], 3, 3, 4)                                # the real call fills frames 2, 1, 0
    assert [rows_of(b)[0] for b in out_t] == [1, 1, 1] and win.count == 3
    half = win.half
    out_f, out_t = win.call(frames[:3], tracked[:3], -1, 3, 4)                               # flush: the arguments' frames are not read
    assert len(out_f) == 3 and np.array_equal(out_f[0], frames[3]) and (win.count, win.half) == (0, half)
    assert win.call(frames[:3], tracked[:3], -1, 3, 4) == ([], [])


def test_short_call_and_reset():
    frames, _, tracked = LB.sequence(H, W, 7, 5, rows=8, capacity=4)
    win = LB.Window(4, H, W, 8, 4, 2)
    out_f, _ = LB.run(win, frames, tracked, [4, 1, 2], lookback=4, radius=1)
    assert len(out_f) == 7 and all(np.array_equal(a, b) for a, b in zip(out_f, frames))
    win.call(frames[:4], tracked[:4], 4, 1, 0)
    win.reset()
    assert win.call(frames[:4], tracked[:4], -1, 1, 0) == ([], []) and not win.state_bytes()[:LB.HEADER].any()


def test_back_overflow_drops_the_highest_ids():
    rows, cap, back = 2, 2, 2
    R, R2 = rows + cap, rows + cap + back
    full = np.zeros(4 + 8 * R, dtype=np.int32)                       # frame 0: every live and held row in use, ids 1..4
    full[:4] = (R, rows, 5, 0)
    full[4:4 + 4 * R] = np.tile([1, 1, 9, 9], R)
    full[4 + 4 * R:4 + 5 * R] = 1
    full[4 + 6 * R:4 + 7 * R] = np.arange(1, R + 1)
    full[4 + 7 * R + rows:4 + 8 * R] = 1
    born = np.zeros(4 + 8 * R, dtype=np.int32)                       # frame 1: two births, ids 5 and 6 (capacity: two at most)
    born[:4] = (2, 2, 7, 0)
    born[4:4 + 4 * R] = -1
    born[4:12] = (2, 2, 20, 20, 30, 5, 50, 30)
    born[4 + 4 * R:4 + 5 * R] = -1
    born[4 + 4 * R:6 + 4 * R] = 1
    born[4 + 6 * R:6 + 6 * R] = (5, 6)
    born2 = born.copy()                                              # frame 2: one more, id 7, next to id 6 matched again
    born2[:4] = (2, 2, 8, 0)
    born2[4 + 6 * R:6 + 6 * R] = (6, 7)
    frames = [LB.texture(H, W, s) for s in range(3)]
    win = LB.Window(3, H, W, rows, cap, back)
    win.call(frames, [full, born, born2], 3, lookback=2, radius=0)
    _, out_t = win.call(frames, [full, born, born2], -1, lookback=2, radius=0)
    n_rows, n_live, got = rows_of(out_t[0])
    assert (n_rows, n_live) == (R2, rows) and [(r[3], r[4]) for r in got[R:]] == [(5, -1), (6, -1)]       # id 7 did not fit
    assert [(r[3], r[4]) for r in rows_of(out_t[1])[2][2:]] == [(7, -1)]
    assert win.back_overflow == 1


def test_header_states_the_rule_and_the_binding_matches_it():
    text = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_track_lookback.h")).read()
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))
    from faster_rcnn_amd import _lib
    assert define("FRCNN_TRACK_LOOKBACK_VERSION") == _lib.TRACK_LOOKBACK_VERSION
    assert define("FRCNN_TRACK_LOOKBACK_MAX") == _lib.TRACK_LOOKBACK[1] == LB.LOOKBACK[1] and _lib.TRACK_LOOKBACK == LB.LOOKBACK
    assert 8 <= define("FRCNN_TRACK_LOOKBACK_MAX") <= _lib.TRACK_MAX_FRAMES
    assert define("FRCNN_TRACK_LOOKBACK_HEADER") == _lib.TRACK_LOOKBACK_HEADER == LB.HEADER
    assert define("FRCNN_TRACK_LOOKBACK_MAX_BACK") == _lib.TRACK_LOOKBACK_MAX_BACK
    for word in ("BIRTH", "CHAIN", "PLACE", "back_overflow", "age = -k"):
        assert word in text
    assert "Look-back rule" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_option_checker():
    from faster_rcnn_amd import ops
    assert ops.track_lookback_option() == 8 and ops.track_lookback_option(1) == 1 and ops.track_lookback_option(np.int64(16)) == 16
    for bad in (0, 17, -1, True, 2.0, "4"):
        with pytest.raises(ValueError, match="track lookback"):
            ops.track_lookback_option(bad)


def test_parser_and_mot_lines():
    from faster_rcnn_amd import annotate_video as A
    parse = lambda *extra: A.build_parser().parse_args(["a.h5", "b.h5", "frames"] + list(extra))
    with pytest.raises(ValueError) as e:
        A.track_lookback_from_args(parse("--track_lookback", "4"))
    assert "--track_lookback" in str(e.value) and "needs --track" in str(e.value)
    with pytest.raises(ValueError):
        A.track_lookback_from_args(parse("--track_lookback"))
    for bad in ("17", "-1"):
        with pytest.raises(ValueError, match="--track_lookback"):
            A.track_lookback_from_args(parse("--track", "--track_lookback", bad))
    assert A.track_lookback_from_args(parse("--track")) is None
    assert A.track_lookback_from_args(parse("--track", "--track_lookback", "16")) == 16
    assert A.track_lookback_from_args(parse("--track", "--track_lookback")) == A.TRACK_LOOKBACK_AUTO
    assert A._lookback_frames(A.TRACK_LOOKBACK_AUTO, (30, 8, 0), object(), 4) == 4 and A._lookback_frames(A.TRACK_LOOKBACK_AUTO, (30, 8, 0), object(), 16) == 8
    mapping = {"car": 1, "bg": 0}
    det = lambda **kw: dict({"bbox": np.array([1, 2, 11, 22]), "cls_name": "car", "prob": np.float32(0.5), "track_id": 3}, **kw)
    dets = [det(), det(track_id=4, held=2), det(track_id=5, backfilled=1)]
    assert A.mot_lines(7, dets, mapping) == T.mot_lines(7, dets[:1], mapping) == ["7,3,1,2,10,20,0.500000,1,-1,-1"]
