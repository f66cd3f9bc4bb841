"""The motion rule (DESIGN §8 "Motion rule") on its numpy restatement tests/track_motion_ref.py -- the comparand of the GPU tests -- alone:
shifts that a block match must recover exactly, the boundary cases of the grid, the tie order and the gate, the use case (a held box that
follows its object), and the bookkeeping of the kept frame; then the host-only parts of the feature."""
import os

import numpy as np
import pytest

from tests import track_motion_ref as M
from tests import track_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 96, 128
TABLE = np.array([0, 1, 1, 0], dtype=np.uint8)
BOXES = [(10, 40, 12, 50), (20, 90, 30, 70), (0, W - 1, 0, H - 1), (108, 127, 66, 95)]       # (xa, xb, ya, yb); the last sits in the corner


def noise(h=H, w=W, seed=5):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


@pytest.fixture(scope="module")
def photo():
    from PIL import Image
    rgb = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "VOC_test", "JPEGImages", "000005.jpg")).convert("RGB"))
    return np.ascontiguousarray(rgb[:, :, ::-1])


def grey(values):
    """A frame whose luma is ``values`` (h, w): (v, v, v) has luma v."""
    return np.repeat(np.asarray(values, dtype=np.uint8)[:, :, None], 3, axis=2)


def pack(boxes, cls, rows=8):
    p = np.zeros(4 + 7 * rows, dtype=np.int32)
    p[0] = len(cls)
    p[4:4 + 4 * rows] = -1
    p[4 + 4 * rows:4 + 5 * rows] = -1
    for r, (b, c) in enumerate(zip(boxes, cls)):
        p[4 + 4 * r:8 + 4 * r] = b
        p[4 + 4 * rows + r] = c
        p[4 + 5 * rows + r] = T.bits(0.9 - 0.1 * r)
    return p


# ----------------------------------------------------------------------------------------------------------- recovered shifts
@pytest.mark.parametrize("shift,radius", [((3, 2), 8), ((1, 0), 8), ((-8, 8), 8), ((16, -16), 16)])
def test_a_shift_of_noise_is_recovered_exactly(shift, radius):
    prev = noise()
    cur = M.shifted(prev, *shift)
    assert np.array_equal(cur[20 + shift[1], 30 + shift[0]], prev[20, 30])
    for box in BOXES:
        dx, dy, best, zero, n = M.search(prev, cur, box, radius)
        assert (dx, dy) == shift and best + n <= zero, (box, dx, dy, best, zero, n)
    assert M.search(prev, cur, BOXES[1], radius)[2] == 0                 # a box that stays inside meets its own pixels: cost 0


@pytest.mark.parametrize("shift", [(3, 2), (-8, 8)])
def test_a_shift_of_a_photo_is_recovered_exactly(photo, shift):
    h, w = photo.shape[:2]
    assert (h, w) == (375, 500)
    cur = M.shifted(photo, *shift)
    for box in BOXES[:2] + [(0, w - 1, 0, h - 1)]:
        dx, dy, best, zero, n = M.search(photo, cur, box, 8)
        assert (dx, dy) == shift, (box, dx, dy, best, zero, n)
    # the whole frame: strides (500 + 31) // 32 = 16 and (375 + 31) // 32 = 12, from 8 and 6 on
    assert M.samples(0, 499).tolist() == list(range(8, 500, 16)) and M.samples(0, 374).tolist() == list(range(6, 375, 12))
    assert M.search(photo, cur, (0, w - 1, 0, h - 1), 8)[4] == 31 * 31


def test_the_luma_is_symmetric_in_the_outer_channels():
    f = noise(seed=9)
    assert np.array_equal(M.luma(f), M.luma(f[:, :, ::-1]))
    assert M.luma(np.array([[[255, 255, 255], [0, 0, 1], [1, 0, 0], [0, 1, 0], [3, 0, 0]]], dtype=np.uint8)).tolist() == [[255, 0, 0, 1, 1]]
    cur = M.shifted(f, 2, -1)
    assert M.search(f, cur, BOXES[1]) == M.search(f[:, :, ::-1], cur[:, :, ::-1], BOXES[1])


# ----------------------------------------------------------------------------------------------------------- boundary cases
def test_the_sample_grid():
    assert M.samples(10, 10).tolist() == [10]
    assert M.samples(10, 41).tolist() == list(range(10, 42))                 # 32 wide: stride 1
    assert M.samples(10, 42).tolist() == list(range(11, 43, 2))              # 33 wide: stride 2 from xa + 1, 16 samples
    assert M.samples(0, 69).tolist() == list(range(1, 70, 3))                # 70 wide: stride 3
    for width in range(1, 700):
        assert 1 <= len(M.samples(5, 5 + width - 1)) <= 32
    assert len(M.samples(0, 32767)) == 32


def test_identical_and_flat_frames_do_not_move():
    f = noise()
    for box in BOXES:
        dx, dy, best, zero, n = M.search(f, f, box)
        assert (dx, dy, best, zero) == (0, 0, 0, 0) and n >= 16
    flat = np.full((H, W, 3), 77, dtype=np.uint8)
    other = np.full((H, W, 3), 90, dtype=np.uint8)
    cost, n = M.costs(flat, other, BOXES[0], 8)
    assert len(set(cost.values())) == 1 and cost[(0, 0)] == 13 * n            # every cost equal: the norm picks (0, 0), the gate refuses
    assert M.search(flat, other, BOXES[0]) == (0, 0, 13 * n, 13 * n, n)


def test_small_and_empty_boxes_are_skipped():
    prev = noise()
    cur = M.shifted(prev, 3, 2)
    assert M.search(prev, cur, (20, 20, 30, 30)) == (0, 0, 0, 0, 1)         # 1x1
    assert M.search(prev, cur, (20, 22, 30, 34)) == (0, 0, 0, 0, 15)        # 3x5: n = 15 < 16
    assert M.search(prev, cur, (20, 23, 30, 33))[:2] == (3, 2)              # 4x4: n = 16
    assert M.search(prev, cur, (30, 20, 30, 40)) == (0, 0, 0, 0, 0)         # empty


def test_the_tie_order():
    """Period-4 stripes moved by half a period: the candidates 2 to either side (and 4 further on) cost the same."""
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    v = np.array([10, 80, 200, 120])
    box = (40, 71, 30, 61)                                                   # far from every border: no clamped read within radius 8
    for name, phase, want in (("columns", x, (-2, 0)), ("rows", y, (0, -2)), ("diagonal", x + y, (-1, -1)), ("anti-diagonal", x - y, (1, -1))):
        prev = grey(v[phase % 4])
        cur = grey(v[(phase - 2) % 4])                                       # = moved by 2 along the phase
        cost, n = M.costs(prev, cur, box, 8)
        zero = sorted((d for d in cost if cost[d] == 0), key=lambda d: (d[0] ** 2 + d[1] ** 2, d[1], d[0]))
        assert len(zero) > 2 and zero[0] == want, (name, zero[:4])
        assert {d[0] ** 2 + d[1] ** 2 for d in zero[:2]} == {want[0] ** 2 + want[1] ** 2}      # a true tie of cost and norm
        assert M.search(prev, cur, box)[:2] == want, name
    # (1, -1) against (-1, 1): dy decides before dx
    assert M.choose({(0, 0): 99, (1, -1): 5, (-1, 1): 5, (1, 1): 5, (-1, -1): 5}, 16)[:2] == (-1, -1)
    assert M.choose({(0, 0): 99, (1, -1): 5, (-1, 1): 5}, 16)[:2] == (1, -1)
    assert M.choose({(0, 0): 99, (3, 0): 5, (1, 1): 5}, 16)[:2] == (1, 1)        # the norm before both
    assert M.choose({(0, 0): 99, (3, 0): 4, (1, 1): 5}, 16)[:2] == (3, 0)        # the cost before all


def test_the_gate_at_its_edge():
    assert M.choose({(0, 0): 16, (4, 0): 0}, 16) == (4, 0, 0, 16, 16)
    assert M.choose({(0, 0): 16, (4, 0): 1}, 16) == (0, 0, 1, 16, 16)
    # ... and through frames: a 4x4 box (n = 16) of 10s in front of 11s, found 4 to the right
    prev = grey(np.full((H, W), 10))
    lum = np.full((H, W), 11)
    lum[30:34, 44:48] = 10
    box = (40, 43, 30, 33)
    assert M.search(prev, grey(lum), box) == (4, 0, 0, 16, 16)               # cost(best) + n == cost(0, 0): taken
    lum[31, 45] = 11
    assert M.search(prev, grey(lum), box) == (0, 0, 1, 16, 16)               # one above: refused


# ----------------------------------------------------------------------------------------------------------- the use case
def test_a_held_box_follows_its_object(photo):
    h, w = photo.shape[:2]
    frames = [photo]
    for _ in range(5):
        frames.append(M.shifted(frames[-1], 3, 2))
    first = [120, 90, 260, 230]
    dets = pack([first], [1])
    none = pack([], [])
    for motion in (True, False):
        tr = M.MotionTracker(4)
        plain = T.Tracker(4)
        boxes = []
        for k, f in enumerate(frames):
            p = dets if k == 0 else none
            buf = tr.update_call([f], [p], 1, TABLE, h, w, 30, 8, 0, 8)[0] if motion else plain.update_packed(p, TABLE, h, w, 30, 8, 0)
            n_rows, n_live, _, _, bbox, cls, prob, ids, age = T.split(buf)
            if k:
                assert (n_rows, n_live, ids[0], age[0]) == (1, 0, 1, k)
                boxes.append(bbox[0].tolist())
        want = [[first[0] + 3 * k, first[1] + 2 * k, first[2] + 3 * k, first[3] + 2 * k] if motion else first for k in range(1, 6)]
        assert boxes == want
        # the object is found again where it now is: 15 right and 10 down of where it was last SEEN
        again = pack([[first[0] + 18, first[1] + 12, first[2] + 18, first[3] + 12]], [1])
        seventh = M.shifted(frames[-1], 3, 2)
        buf = tr.update_call([seventh], [again], 1, TABLE, h, w, 80, 8, 0, 8)[0] if motion else plain.update_packed(again, TABLE, h, w, 80, 8, 0)
        inter, union = T.inter_union(T.clip(first, h, w), T.clip(again[4:8], h, w))
        assert inter * 100 < 80 * union                                      # (against the standing box: under the threshold)
        assert T.split(buf)[7][0] == (1 if motion else 2)


# ----------------------------------------------------------------------------------------------------------- equivalence, bookkeeping
def sequence(seed, n, h=H, w=W, rows=8):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        k = rs.randint(0, 5)
        xy = rs.randint(-10, [w - 10, h - 10], (k, 2))
        wh = rs.randint(2, 50, (k, 2))
        out.append(pack(np.concatenate([xy, xy + wh], axis=1).tolist(), rs.choice([1, 2, 3], k).tolist(), rows))
    return out


def test_without_a_reference_it_is_the_plain_tracker():
    dets = sequence(3, 12)
    frames = [noise(seed=40 + k) for k in range(12)]
    plain = T.Tracker(5)
    tr = M.MotionTracker(5)
    for f, p in zip(frames, dets):
        tr.reset_motion()                                                    # a zeroed header in front of every one-frame call
        got = tr.update_call([f], [p], 1, TABLE, H, W, 30, 3, 2, 8)[0]
        assert np.array_equal(got, plain.update_packed(p, TABLE, H, W, 30, 3, 2))
        assert np.array_equal(tr.t.words(), plain.words())
    assert tr.moves == [] and plain.events["match"] + plain.events["hold"] > 0
    # ... and the padding frames of a call are the plain tracker's
    tr = M.MotionTracker(5)
    out = tr.update_call(frames[:4], dets[:4], 2, TABLE, H, W, 30, 3, 2, 8)
    assert np.array_equal(out[2], tr.t.padding(8)) and np.array_equal(out[3], tr.t.padding(8)) and tr.t.frames == 2
    assert np.array_equal(tr.frame, frames[1]) and tr.header().tolist() == [2, H, W, 0]


def test_the_header_bookkeeping():
    prev = noise()
    cur = M.shifted(prev, 3, 2)
    box = [20, 30, 90, 70]
    start = lambda: M.MotionTracker(4)
    # a fresh one: no reference; after a call the header is [frames, h, w, 0] and the kept frame the last REAL frame
    tr = start()
    assert tr.header().tolist() == [0, 0, 0, 0] and not tr.motion_bytes(H, W).any()
    tr.update_call([prev, cur, cur], [pack([box], [1])] * 3, 1, TABLE, H, W)
    assert tr.header().tolist() == [1, H, W, 0] and np.array_equal(tr.frame, prev) and tr.moves == []
    assert np.array_equal(tr.motion_bytes(H, W)[16:].reshape(H, W, 3), prev)
    # the next call uses it
    tr.update_call([cur], [pack([], [])], 1, TABLE, H, W)
    assert tr.moves == [(1, 3, 2)] and tr.header().tolist() == [2, H, W, 0] and tr.t.slots[0]["bbox"] == [23, 32, 93, 72]
    # nf = 0: nothing changes
    before = (tr.header().tolist(), tr.frame.copy(), tr.t.words())
    out = tr.update_call([prev], [pack([box], [1])], 0, TABLE, H, W)
    assert np.array_equal(out[0], tr.t.padding(8))
    assert tr.header().tolist() == before[0] and np.array_equal(tr.frame, before[1]) and np.array_equal(tr.t.words(), before[2])
    # a kept count that is not the state's frame count: no reference (the tracker was advanced, or reset, without the motion state)
    for spoil in ("count", "size", "reset"):
        tr = start()
        tr.update_call([prev], [pack([box], [1])], 1, TABLE, H, W)
        if spoil == "count":
            tr.t.update_packed(pack([box], [1]), TABLE, H, W)                # the plain rule saw a frame in between
        elif spoil == "size":
            tr.size = (W, H)
        else:
            tr.reset_motion()
        tr.update_call([cur], [pack([], [])], 1, TABLE, H, W)
        assert tr.moves == [], spoil
        assert tr.header().tolist() == [tr.t.frames, H, W, 0]
    # another frame size: the first frame of the new size has no reference, the second has
    tr = start()
    tr.update_call([prev], [pack([box], [1])], 1, TABLE, H, W)
    big_prev = noise(120, 160, 8)
    tr.update_call([big_prev], [pack([box], [1])], 1, TABLE, 120, 160)
    assert tr.moves == [] and tr.header().tolist() == [2, 120, 160, 0]
    tr.update_call([M.shifted(big_prev, -2, 1)], [pack([], [])], 1, TABLE, 120, 160)
    assert tr.moves == [(1, -2, 1)]


# ----------------------------------------------------------------------------------------------------------- host-only parts
def test_the_radius_check_needs_no_gpu():
    from faster_rcnn_amd import _lib, ops
    assert _lib.TRACK_MOTION_RADIUS == (1, 16, 8) == M.RADIUS == ops.TRACK_MOTION_RADIUS
    assert ops.track_motion_radius() == 8 and ops.track_motion_radius(None) == 8
    assert ops.track_motion_radius(1) == 1 and ops.track_motion_radius(np.int64(16)) == 16
    for bad in (0, 17, -1, True, 8.0, "8"):
        with pytest.raises(ValueError):
            ops.track_motion_radius(bad)


def test_cli_arguments():
    from faster_rcnn_amd import annotate_video
    parse = lambda *extra: annotate_video.build_parser().parse_args(["a.h5", "b.h5", "frames"] + list(extra))
    assert annotate_video.track_motion_from_args(parse()) is None
    assert annotate_video.track_motion_from_args(parse("--track")) is None
    assert annotate_video.track_motion_from_args(parse("--track", "--track_motion")) == 8
    assert annotate_video.track_motion_from_args(parse("--track", "--track_motion", "16")) == 16
    assert annotate_video.track_motion_from_args(parse("--track_motion", "3", "--track")) == 3
    for extra in (("--track_motion",), ("--track_motion", "4")):
        with pytest.raises(ValueError) as e:
            annotate_video.track_motion_from_args(parse(*extra))
        assert "--track_motion" in str(e.value) and "--track" in str(e.value).replace("--track_motion", "")
    for value in ("0", "17", "-1"):
        with pytest.raises(ValueError) as e:
            annotate_video.track_motion_from_args(parse("--track", "--track_motion", value))
        assert value in str(e.value)
    # the tracker's own arguments are read as they were
    assert annotate_video.track_from_args(parse("--track", "--track_motion", "5")) == (30, 8, 0)
