"""The two entry points of the trail extension (include/ext/frcnn_hip_track_trails.h, csrc/track_trails.hip) against the restatement
(tests/track_trails_ref.py), byte for byte: ops.track_trails_update over hand-made tracked buffers -- state, point lists, both row counts
-- and ops.track_trails_draw_u8 over hand-made point lists."""
import numpy as np
import pytest

from tests import track_trails_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

H, W = 48, 64
CAP, N, FRAMES, MAX_ROWS = 4, 3, 5, 6
E_ARG = -1                                                                   # FRCNN_E_ARG


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def buffer(rows, n_live, boxes, ids):
    b = np.zeros(4 + 8 * rows, dtype=np.int32)
    b[4:4 + 5 * rows] = -1
    b[0], b[1] = len(ids), n_live
    for r, (box, i) in enumerate(zip(boxes, ids)):
        b[4 + 4 * r:8 + 4 * r] = box
        b[4 + 4 * rows + r] = 1 + i % 3
        b[4 + 6 * rows + r] = i
    return b


def box_at(x, y):
    return [x - 3, y - 2, x + 3, y + 2]


def sequence(rows):
    """Ten frames (two calls of five): births (1, 2 in frame 0; 3 in 1; 8 and 9 later), frame 1 brings more ids than the table takes (two
    rows dropped), id 2 vanishes for good behind frame 1, id 1 is absent for E = 2 frames and returns with its trail, id 3 is absent for
    E + 1 and returns afresh; id-0 rows, a tracked box outside the frame, and an id (9) that two rows of one frame carry; every frame
    carries a held row (index >= n_live) whose id must never be read."""
    live = [
        [(1, 10, 10), (2, 50, 40)],
        [(2, 49, 38), (1, 12, 11), (3, 30, 5), (20, 5, 40), (22, 40, 20), (21, 44, 22)],
        [(3, 31, 7), (0, 20, 20)],
        [(3, 32, 9)],
        [(1, 18, 14), (3, 33, 11)],
        [(1, 20, 15)],
        [(8, 60, 44), (1, 22, 16), (0, 9, 9)],
        [(1, 24, 17)],
        [(3, 36, 17), (1, 26, 18), (9, 8, 8), (9, 9, 9)],
        [(1, 28, 19), (9, 10, 10)],
    ]
    out = []
    for f, rows_f in enumerate(live):
        boxes = [box_at(x, y) for _, x, y in rows_f] + [box_at(25, 25)]
        ids = [i for i, _, _ in rows_f] + [40 + f]                           # (the held row)
        if f == 7:
            boxes.insert(1, [W + 2, 3, W + 9, 9])                            # live, tracked, and wholly outside the frame
            ids.insert(1, 11)
        out.append(buffer(rows, len(ids) - 1, boxes, ids))
    return np.stack(out)


def run(bufs, calls, cap=CAP, n=N, expire=2, h=H, w=W):
    """``calls``: [(first frame, frames, the n_frames word)] -> [(state, lists) after each call] from the device and from the rule."""
    from faster_rcnn_amd import ops
    state, ref, got, want = ops.track_trails_state(cap, n), R.Trails(h, w, cap, n, expire), [], []
    for first, frames, word, *gate in calls:
        part = bufs[first:first + frames]
        lists = ops.track_trails_update(state, dev(part), dev(np.array([word], dtype=np.int32)), n, expire, h, w,
                                        gate=dev(np.array(gate, dtype=np.int32)) if gate else None)
        torch.cuda.synchronize()
        got.append((state.cpu().numpy().copy(), lists.cpu().numpy()))
        want_lists = ref.update(part, word, *gate)
        want.append((ref.words(), want_lists))
    return got, want, ref


def same(got, want):
    for k, ((gs, gl), (ws, wl)) in enumerate(zip(got, want)):
        assert np.array_equal(gl, wl), ("lists of call", k, np.argwhere(gl != wl)[:5])
        assert np.array_equal(gs, ws), ("state after call", k, np.argwhere(gs != ws)[:8])


# ------------------------------------------------------------------------------------------------------------ update
@pytest.mark.parametrize("rows", [MAX_ROWS + CAP, MAX_ROWS + CAP + 5])       # R, and a widened R2
def test_update_matches_the_rule_over_two_calls_and_over_one(rows):
    bufs = sequence(rows)
    got, want, ref = run(bufs, [(0, FRAMES, FRAMES), (FRAMES, FRAMES, FRAMES)])
    same(got, want)
    # what the sequence was built to show
    assert ref.dropped == 2 and ref.frames == 10
    lists = np.concatenate([w[1] for w in want])
    trails = [dict(R.trails_of(l, N)) for l in lists]
    assert trails[4][1] == [(10, 10), (12, 11), (18, 14)] and trails[8][3] == [(36, 17)]      # re-matched inside E; outside: afresh
    assert set(trails[1]) == {1, 2, 3, 20} and set(trails[6]) == {1, 8} and 2 not in trails[2] and 11 not in trails[7]
    assert trails[8][9] == [(8, 8), (9, 9)] and trails[9][1] == [(24, 17), (26, 18), (28, 19)]
    assert not any(i >= 40 for t in trails for i in t)
    # the same frames in calls of other sizes: the same lists and the same state
    got2, _, _ = run(bufs, [(0, 5, 3), (3, 5, 5), (8, 2, 2)])
    assert np.array_equal(got2[-1][0], got[-1][0])
    assert np.array_equal(np.concatenate([got2[0][1][:3], got2[1][1], got2[2][1]]), np.concatenate([g[1] for g in got]))


@pytest.mark.parametrize("word", [0, 3, 5, -2, 9])
def test_the_n_frames_word(word):
    bufs = sequence(MAX_ROWS + CAP)
    got, want, _ = run(bufs, [(0, FRAMES, 2), (2, FRAMES, word)])
    same(got, want)
    nf = min(max(word, 0), FRAMES)
    assert not got[1][1][nf:].any() and got[1][0][1] == 2 + nf
    if nf == 0:
        assert np.array_equal(got[1][0], got[0][0])


def test_a_gate_word_of_zero_makes_the_call_no_frames():
    bufs = sequence(MAX_ROWS + CAP)
    got, want, _ = run(bufs, [(0, FRAMES, FRAMES, 7), (FRAMES, FRAMES, FRAMES, 0), (FRAMES, FRAMES, FRAMES, -1)])
    same(got, want)
    assert np.array_equal(got[1][0], got[0][0]) and not got[1][1].any() and got[2][0][1] == 10 and got[2][1].any()


def test_ranks_across_waves():
    """capacity 128, N 64, 64 frames, 300 rows: over a hundred ids at once, births and expiries in every frame, more ids than trails."""
    rs = np.random.RandomState(5)
    h, w, rows, frames = 200, 300, 300, 64
    bufs = []
    for f in range(frames):
        ids = rs.permutation(np.arange(1 + f, 150 + f))[:rs.randint(100, 140)]
        ids = np.concatenate([ids, np.zeros(20, dtype=ids.dtype)])
        rs.shuffle(ids)
        boxes = [[x - 4, y - 4, x + 4, y + 4] for x, y in zip(rs.randint(-5, w + 5, len(ids)), rs.randint(-5, h + 5, len(ids)))]
        bufs.append(buffer(rows, len(ids) - 7, boxes, ids.tolist()))
    got, want, ref = run(np.stack(bufs), [(0, frames, frames)], cap=128, n=64, expire=3, h=h, w=w)
    same(got, want)
    assert ref.dropped > 0 and len(ref.entries) > 64 and max(len(e["pts"]) for e in ref.entries) > 40


# ------------------------------------------------------------------------------------------------------------ draw
def noise(h, w, seed=1):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def check_draw(frame, trails, cap, n, width, rgb):
    from faster_rcnn_amd import ops
    plist = R.make_list(trails, cap, n)
    d = dev(frame)
    ops.track_trails_draw_u8(d, dev(plist), n, width, rgb=bool(rgb))
    torch.cuda.synchronize()
    want = R.draw(frame, plist, n, width, rgb)
    got = d.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:6]
    return want


SHAPES = [(1, [(5, 20), (45, 20)]), (2, [(26, 2), (26, 34)]), (3, [(4, 4), (30, 30)]), (4, [(2, 30), (50, 33)]), (5, [(40, 36), (43, 1)]),
          (6, [(17, 17), (17, 17)]), (9, [(-4, 10), (6, 10)]), (10, [(48, 30), (58, 30)]), (11, [(20, -3), (20, 4)]), (12, [(33, 33), (33, 41)])]


@pytest.mark.parametrize("rgb", [0, 1])
@pytest.mark.parametrize("width", [1, 2, 3, 9])
def test_draw_segments_of_every_kind(width, rgb):
    """37 x 53: horizontal, vertical, 45 degrees, shallow, steep, zero-length, and one capsule leaving the frame on each side."""
    frame = noise(37, 53)
    want = check_draw(frame, [(i, 1, pts) for i, pts in SHAPES], 16, 4, width, rgb)
    assert (want != frame).any(axis=2).sum() > 100
    for i, pts in SHAPES:                                                    # every one of them is visible
        assert R.segment_mask(pts[0], pts[1], 37, 53, width).any(), i


@pytest.mark.parametrize("ids", [(3, 11, 19), (3, 12, 6)])                  # sharing id & 7, and not
@pytest.mark.parametrize("rgb", [0, 1])
def test_draw_three_crossing_trails(ids, rgb):
    paths = [[(2, 5), (50, 30), (45, 8)], [(5, 35), (52, 4)], [(30, 0), (30, 36), (10, 20)]]
    for width in (1, 3):
        check_draw(noise(37, 53, 2), [(i, 1, p) for i, p in zip(ids, paths)], 4, 4, width, rgb)
        check_draw(noise(37, 53, 2), [(i, 1, p) for i, p in zip(ids[::-1], paths)], 4, 4, width, rgb)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 70)])
def test_draw_tiny_frames(h, w):
    for width in (1, 2, 9):
        check_draw(noise(h, w), [(1, 1, [(0, 0), (w - 1, 0)]), (2, 1, [(w // 2, 0), (w // 2, 0)])], 4, 2, width, 1)


def test_an_empty_list_and_single_points_write_no_byte():
    from faster_rcnn_amd import ops
    frame = noise(37, 53)
    for trails in ([], [(4, 1, [(10, 10)]), (5, 1, [(20, 20)])]):
        d = dev(frame)
        ops.track_trails_draw_u8(d, dev(R.make_list(trails, 4, 4)), 4, 9)
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy(), frame)


def test_draw_more_segments_than_the_staging_area_holds():
    """64 x 64, 128 trails of 64 points inside one tile's reach: 8064 segments, staged in chunks."""
    rs = np.random.RandomState(9)
    trails = []
    for t in range(128):
        x, y = rs.randint(2, 62), rs.randint(1, 14)
        pts = []
        for _ in range(64):
            x, y = min(max(x + rs.randint(-1, 2), 0), 63), min(max(y + rs.randint(-1, 2), 0), 15)
            pts.append((int(x), int(y)))
        trails.append((t + 1, 1, pts))
    check_draw(noise(64, 64), trails, 128, 64, 1, 0)


def test_draw_one_segment_across_many_tiles():
    want = check_draw(noise(300, 500, 4), [(7, 1, [(0, 0), (499, 299)]), (2, 1, [(499, 0), (0, 299)])], 2, 2, 3, 1)
    assert (want[0, 0] == R.PALETTE[7]).all() and (want[299, 499] == R.PALETTE[7]).all() and (want[0, 499] == R.PALETTE[2]).all()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_frame_and_state_untouched():
    from faster_rcnn_amd import _lib, ops
    lib = _lib.load()
    rows = MAX_ROWS + CAP
    bufs, word = dev(sequence(rows)[:FRAMES]), dev(np.array([FRAMES], dtype=np.int32))
    state, lists = ops.track_trails_state(CAP, N), ops.track_trails_workspace(FRAMES, CAP, N)
    ops.track_trails_update(state, bufs, word, N, 2, H, W, lists=lists)
    torch.cuda.synchronize()
    s0, l0 = state.cpu().numpy().copy(), lists.cpu().numpy().copy()
    p = lambda t: t.data_ptr()
    good = dict(state=p(state), cap=CAP, tracked=p(bufs), stride=4 + 8 * rows, rows=rows, frames=FRAMES, n_frames=p(word), gate=None, length=N, expire=2,
                h=H, w=W, lists=p(lists))
    bad = [dict(state=None), dict(tracked=None), dict(n_frames=None), dict(lists=None), dict(cap=0), dict(cap=129), dict(rows=0), dict(rows=513),
           dict(frames=0), dict(frames=65), dict(stride=4 + 8 * rows - 1), dict(length=1), dict(length=65), dict(expire=-1), dict(expire=4096),
           dict(h=0), dict(w=0), dict(h=32769), dict(w=32769)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.frcnn_track_trails_update(a["state"], a["cap"], a["tracked"], a["stride"], a["rows"], a["frames"], a["n_frames"], a["gate"], a["length"],
                                           a["expire"], a["h"], a["w"], a["lists"], None)
        assert rc == E_ARG, change
    frame = dev(noise(37, 53))
    f0 = frame.cpu().numpy().copy()
    plist = dev(R.make_list([(1, 1, [(2, 2), (40, 30)])], 4, 4))
    gd = dict(frame=p(frame), h=37, w=53, list=p(plist), length=4, width=3)
    for change in [dict(frame=None), dict(list=None), dict(h=0), dict(w=0), dict(h=32769), dict(w=32769), dict(length=1), dict(length=65),
                   dict(width=0), dict(width=10)]:
        a = dict(gd, **change)
        assert lib.frcnn_track_trails_draw_u8(a["frame"], a["h"], a["w"], a["list"], a["length"], a["width"], 0, None) == E_ARG, change
    torch.cuda.synchronize()
    assert np.array_equal(state.cpu().numpy(), s0) and np.array_equal(lists.cpu().numpy(), l0) and np.array_equal(frame.cpu().numpy(), f0)
    assert lib.frcnn_track_trails_state_bytes(0, 3) == 0 and lib.frcnn_track_trails_state_bytes(4, 65) == 0
    assert lib.frcnn_track_trails_state_bytes(CAP, N) == 4 * R.list_words(CAP, N) == 4 * lib.frcnn_track_trails_list_words(CAP, N)
    with pytest.raises(_lib.FrcnnError):
        ops.track_trails_state(129, 3)
    with pytest.raises(_lib.FrcnnError):
        ops.track_trails_workspace(65, 4, 3)
