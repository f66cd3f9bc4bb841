"""The two entry points of the zone extension (include/ext/frcnn_hip_zone.h, csrc/zone.hip) against the restatement (tests/zone_ref.py),
word for word and byte for byte: ops.zone_update over hand-made tracked buffers -- every word of the state and of the zone lists, in
workspaces pre-filled with 0x7f -- and ops.zone_draw_u8 over hand-made zone lists, on whole frames."""
import ctypes

import numpy as np
import pytest

from tests import zone_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

E_ARG = -1                                                                   # FRCNN_E_ARG
POISON = 0x7f7f7f7f
CLASSES = np.array([0, 1, 0, 1, 1], dtype=np.uint8)                          # class 2 is switched off (0 is the background)
H, W = 120, 200
# a rectangle, its neighbour sharing an edge, an "L", a bow-tie, a triangle beyond two borders, 16 vertices of a star, a sliver, the frame
ZONES8 = [[(20, 20), (100, 20), (100, 90), (20, 90)], [(100, 20), (180, 20), (180, 90), (100, 90)],
          [(10, 10), (150, 10), (150, 50), (60, 50), (60, 110), (10, 110)], [(30, 5), (170, 115), (170, 5), (30, 115)],
          [(-60, 40), (120, -50), (90, 140)],
          [(100, 0), (110, 40), (150, 20), (125, 55), (199, 60), (125, 65), (150, 100), (110, 80), (100, 119), (90, 80), (50, 100), (75, 65),
           (1, 60), (75, 55), (50, 20), (90, 40)],
          [(0, 70), (199, 72), (0, 74)], [(0, 0), (200, 0), (200, 120), (0, 120)]]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def word(v):
    return dev(np.array([v], dtype=np.int32))


def walk(seed, h, w, rows, frames, n_ids, absent=0.25):
    """Tracked buffers of ids on a random walk with long steps: a random subset of the ids in a random row order every frame (so ids
    arrive in any order, are absent -- some for long, so entries expire inside zones -- and return), some ids twice in a frame, rows
    with id 0 and a class that does not count among them, the rows behind n_live and every unused word poisoned."""
    rs = np.random.RandomState(seed)
    pos = np.stack([rs.randint(0, w, n_ids), rs.randint(0, h, n_ids)], axis=1)
    cls = rs.randint(1, 5, n_ids)
    away = np.zeros(n_ids, dtype=np.int64)
    out = []
    for f in range(frames):
        pos = np.clip(pos + rs.randint(-30, 31, pos.shape), [-6, -6], [w + 5, h + 5])
        away = np.where(away > 0, away - 1, np.where(rs.rand(n_ids) < 0.08, rs.randint(2, 6, n_ids), 0))
        present = [i for i in rs.permutation(n_ids) if rs.rand() >= absent and away[i] == 0][:rows - 3 if rows > 3 else rows]
        rws = [(int(i) + 1 + (f // 7 if i % 9 == 0 else 0) * n_ids, int(cls[i]), (pos[i][0] - 3, pos[i][1] - 4, pos[i][0] + 3, pos[i][1] + 4)) for i in present]
        if rws and len(rws) < rows and f % 3 == 0:                                            # the same id twice: it steps twice, in row order
            i, c, (x1, y1, x2, y2) = rws[0]
            rws.append((i, c, (x1 + 40, y1 + 25, x2 + 40, y2 + 25)))
        if len(rws) < rows:
            rws.insert(len(rws) // 2, (0, 1, (POISON, POISON, POISON, POISON)))                 # id 0: its box is never read
        n_live = len(rws)
        if len(rws) < rows:
            rws.append((900 + f, 1, (POISON, -POISON, POISON, -POISON)))                      # a held row, behind n_live
        out.append(R.make_tracked(rws, rows, n_live=n_live, fill=POISON))
    return np.stack(out)


def run(bufs, calls, zones, cap, expire, h, w, classes=CLASSES, anchor=0):
    """``calls``: [(first frame, frames, the n_frames word[, the gate word])] -> [(state, lists) after each call] from the device and from
    the rule.  The workspaces are pre-filled with 0x7f."""
    from faster_rcnn_amd import ops
    state, ref, got, want = ops.zone_state(cap), R.Zones(h, w, zones, classes, cap, expire, anchor), [], []
    table = dev(classes)
    for first, frames, n, *gate in calls:
        part = bufs[first:first + frames]
        lists = ops.zone_workspace(len(part))
        lists.fill_(POISON)
        ops.zone_update(state, dev(part), word(n), zones, table, expire, h, w, anchor=anchor, lists=lists, gate=word(gate[0]) if gate else None)
        torch.cuda.synchronize()
        got.append((state.cpu().numpy().copy(), lists.cpu().numpy()))
        want_lists = ref.update(part, n, *gate)
        want.append((ref.words(), want_lists))
    return got, want, ref


def same(got, want):
    for k, ((gs, gl), (ws, wl)) in enumerate(zip(got, want)):
        assert np.array_equal(gl, wl), ("lists of call", k, np.argwhere(gl != wl)[:5])
        assert np.array_equal(gs, ws), ("state after call", k, np.argwhere(gs != ws)[:8])


# ------------------------------------------------------------------------------------------------------------ update
@pytest.mark.parametrize("cap,rows,frames,n_zones", [(1, 1, 1, 1), (2, 63, 2, 8), (63, 64, 64, 1), (64, 65, 2, 8), (65, 512, 2, 1), (128, 512, 64, 8)])
def test_update_matches_the_rule(cap, rows, frames, n_zones):
    n_ids = min(rows, 2 * cap + 8)
    bufs = walk(cap + rows, H, W, rows, frames, n_ids)
    got, want, ref = run(bufs, [(0, frames, frames)], ZONES8[:n_zones], cap, 2, H, W)
    same(got, want)
    assert ref.frames == frames
    if frames == 64:
        kinds = [ev[1] for lst in got[0][1] for ev in R.events_of(lst)]
        assert kinds.count(R.ENTER) > 20 and kinds.count(R.EXIT) > 10 and sum(ref.dwell) > 20
        assert kinds.count(R.LOST) > 3 or ref.events_dropped > 0             # (the lost events are the last of a frame: the first to be left out)
    if (cap, rows, frames) == (128, 512, 64):                                # more ids than entries, more events in a frame than a list holds
        assert ref.dropped > 0 and ref.events_dropped > 0


@pytest.mark.parametrize("anchor", [0, 1])
def test_update_with_both_anchors_on_tall_boxes(anchor):
    bufs = walk(11, H, W, 40, 12, 30)
    got, want, ref = run(bufs, [(0, 12, 12)], ZONES8, 32, 3, H, W, anchor=anchor)
    same(got, want)
    assert sum(ref.visitors) > 10


@pytest.mark.parametrize("case", R.HAND_CASES, ids=[c[0] for c in R.HAND_CASES])
def test_the_hand_cases(case):
    _, (h, w), zones, anchor, expire, frames, answers, totals = case
    got, want, _ = run(R.hand_buffers(frames), [(0, len(frames), len(frames))], zones, 4, expire, h, w, anchor=anchor)
    same(got, want)
    assert [[(z, k, i, d) for z, k, i, _, d in R.events_of(l)] for l in got[0][1]] == [[tuple(a) for a in ans] for ans in answers]
    n = len(zones)
    assert tuple(list(got[0][0][4 + 8 * k:4 + 8 * k + n]) for k in range(4)) == totals


def test_ids_arriving_in_descending_row_order_keep_id_order():
    rows = [(i, 1, (10 * i, 5, 10 * i, 5)) for i in (9, 7, 5, 3, 1)]
    bufs = np.stack([R.make_tracked(rows, 8, fill=POISON), R.make_tracked([(i, c, (x, 50, x, 50)) for i, c, (x, *_) in rows[::2]], 8, fill=POISON)])
    got, want, ref = run(bufs, [(0, 2, 2)], [ZONES8[0]], 8, 5, H, W)
    same(got, want)
    assert [e["id"] for e in ref.entries] == [1, 3, 5, 7, 9] and [ev[2] for ev in R.events_of(got[0][1][1])] == [9, 5]


def test_a_full_table_drops_rows_and_expiry_frees_places():
    frames = [[(i, 1, (5 * i + 20, 30, 5 * i + 20, 30)) for i in (4, 2, 6, 8, 5)],          # capacity 3: 4, 2, 6 enter; 8 and 5 are dropped
              [(8, 1, (60, 30, 60, 30)), (2, 1, (30, 30, 30, 30))],                           # still full: 8 dropped
              [(8, 1, (60, 30, 60, 30)), (2, 1, (10, 5, 10, 5))],                             # still full: 8 dropped; 2 leaves the zone; E = 1: 4 and 6 are lost
              [(8, 1, (60, 30, 60, 30))]]                                                     # 8 enters the table and the zone
    bufs = np.stack([R.make_tracked(f, 6, fill=POISON) for f in frames])
    got, want, ref = run(bufs, [(0, 4, 4)], [ZONES8[0]], 3, 1, H, W)
    same(got, want)
    assert ref.dropped == 4 and [e["id"] for e in ref.entries] == [2, 8] and ref.visitors[0] == 4 and ref.stays[0] == 3 and ref.peak[0] == 3
    assert [(k, i, d) for _, k, i, _, d in R.events_of(got[0][1][2])] == [(R.EXIT, 2, 2), (R.LOST, 4, 1), (R.LOST, 6, 1)]       # the row's, then in id order
    assert [(k, i, d) for _, k, i, _, d in R.events_of(got[0][1][3])] == [(R.ENTER, 8, 0)]


@pytest.mark.parametrize("expire", [0, 1])
def test_expiry(expire):
    """Absent for one frame inside the zone: with E = 0 the entry is lost and the id enters afresh -- two stays, and a visitor twice, for
    the entry that knew it is gone --, with E = 1 the stay goes on."""
    frames = [[(1, 1, (30, 30, 30, 30))], [], [(1, 1, (31, 30, 31, 30))], [(1, 1, (5, 5, 5, 5))]]
    bufs = np.stack([R.make_tracked(f, 2, fill=POISON) for f in frames])
    got, want, ref = run(bufs, [(0, 4, 4)], [ZONES8[0]], 2, expire, H, W)
    same(got, want)
    assert (ref.visitors[0], ref.stays[0], ref.dwell[0]) == ((1, 1, 3) if expire else (2, 2, 2))


def test_65_events_in_one_frame():
    """64 ids inside and one outside; then the one enters and the 64 leave, in descending row order: 65 events."""
    a = [(i, 1, (20 + i, 30, 20 + i, 30)) for i in range(1, 65)] + [(65, 1, (5, 5, 5, 5))]
    b = [(65, 1, (50, 30, 50, 30))] + [(i, 1, (20 + i, 100, 20 + i, 100)) for i in range(64, 0, -1)]
    bufs = np.stack([R.make_tracked(a, 70, fill=POISON), R.make_tracked(b, 70, fill=POISON)])
    got, want, ref = run(bufs, [(0, 2, 2)], [ZONES8[0]], 128, 3, H, W)
    same(got, want)
    state, lists = got[0]
    assert lists[0][0] == 64 and lists[1][0] == 64 and state[3] == 1 and ref.events_dropped == 1
    assert state[4] == 65 and state[12] == 64 and state[20] == 64 and state[28] == 64          # visitors, stays, dwell, peak: exact
    assert [ev[1:3] for ev in R.events_of(lists[1])] == [(R.ENTER, 65)] + [(R.EXIT, i) for i in range(64, 1, -1)]      # (row, zone) order


def test_a_class_switched_off_and_poisoned_rows():
    """Class 2 does not count, a class outside the table neither; id 0, held rows and rows behind n_live carry poison and are never read."""
    f0 = [(1, 1, (30, 30, 30, 30)), (2, 2, (40, 30, 40, 30)), (3, 7, (50, 30, 50, 30)), (0, 1, (POISON,) * 4), (4, -1, (60, 30, 60, 30))]
    bufs = np.stack([R.make_tracked(f0 + [(5, 1, (POISON,) * 4)], 9, n_live=5, fill=POISON)] * 2)
    got, want, ref = run(bufs, [(0, 2, 2)], [ZONES8[0]], 8, 3, H, W)
    same(got, want)
    assert [e["id"] for e in ref.entries] == [1] and R.events_of(got[0][1][0]) == [(0, R.ENTER, 1, 1, 0)] and R.occupancy_of(got[0][1][1], 1) == [1]


@pytest.mark.parametrize("n", [0, -3, 2, 5, 9])
def test_the_n_frames_word(n):
    bufs = walk(3, H, W, 20, 7, 12)
    got, want, _ = run(bufs, [(0, 2, 2), (2, 5, n)], ZONES8, 16, 2, H, W)
    same(got, want)
    nf = min(max(n, 0), 5)
    assert not got[1][1][nf:].any() and got[1][0][1] == 2 + nf
    if nf == 0:
        assert np.array_equal(got[1][0], got[0][0])


def test_a_gate_word_of_zero_makes_the_call_no_frames():
    bufs = walk(4, H, W, 20, 10, 12)
    got, want, _ = run(bufs, [(0, 5, 5, 7), (5, 5, 5, 0), (5, 5, 5, -1)], ZONES8, 16, 2, H, W)
    same(got, want)
    assert np.array_equal(got[1][0], got[0][0]) and not got[1][1].any() and got[2][0][1] == 10 and got[2][1].any()


def test_two_calls_equal_one_call_and_the_same_call_twice_gives_the_same_bytes():
    bufs = walk(6, H, W, 40, 12, 30)
    one, want, _ = run(bufs, [(0, 12, 12)], ZONES8, 24, 2, H, W)
    same(one, want)
    two, _, _ = run(bufs, [(0, 5, 5), (5, 7, 7)], ZONES8, 24, 2, H, W)
    again, _, _ = run(bufs, [(0, 12, 12)], ZONES8, 24, 2, H, W)
    assert np.array_equal(two[1][0], one[0][0]) and np.array_equal(np.concatenate([two[0][1], two[1][1]]), one[0][1])
    assert np.array_equal(again[0][0], one[0][0]) and np.array_equal(again[0][1], one[0][1])
    assert one[0][0][4:28].sum() > 0


def test_a_captured_call_replayed_after_its_inputs_changed_in_place():
    from faster_rcnn_amd import ops
    cap, rows, F = 16, 20, 4
    bufs = walk(8, H, W, rows, 3 * F, 14)
    state, tracked, n, gate, lists, table = ops.zone_state(cap), dev(bufs[:F]), word(0), word(1), ops.zone_workspace(F), dev(CLASSES)
    run_ = lambda: ops.zone_update(state, tracked, n, ZONES8, table, 2, H, W, lists=lists, gate=gate)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run_()
    assert not state.cpu().numpy().any()                                     # 0 frames: warm-up and capture wrote no word of the state
    ref = R.Zones(H, W, ZONES8, CLASSES, cap, 2)
    for k, real in enumerate((F, 2, F)):
        tracked.copy_(dev(bufs[k * F:k * F + F]))
        n.fill_(real)
        lists.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(lists.cpu().numpy(), ref.update(bufs[k * F:k * F + F], real)), k
        assert np.array_equal(state.cpu().numpy(), ref.words()), k
    assert ref.frames == 2 * F + 2 and sum(ref.visitors) > 0


# ------------------------------------------------------------------------------------------------------------ draw
def noise(h, w, seed=1):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def check_draw(frame, zones, occupancy, visitors, width, rgb, frames=1):
    from faster_rcnn_amd import ops
    zlist = R.make_list(frames, occupancy, visitors)
    d = dev(frame)
    ops.zone_draw_u8(d, dev(zlist), zones, width, rgb=bool(rgb))
    torch.cuda.synchronize()
    want = R.draw(frame, zlist, zones, width, rgb)
    got = d.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:6]
    return want


SIZES = [(1, 1), (16, 85), (17, 86), (33, 171), (200, 330)]
OCC = [1, 0, 3, 0, 12, 0]
VIS = [9, 10, 99999, 0, 2147483647, 7]


def kinds(h, w):
    """A rectangle, a concave one clipped by the border, a triangle far beyond the frame, a bow-tie, a sliver and one fully outside: the
    first, third and fifth occupied."""
    return [[(w // 8, h // 8), (w // 2 + 1, h // 8), (w // 2 + 1, h // 2 + 1), (w // 8, h // 2 + 1)],
            [(w // 3, h // 3), (w + 20, h // 3), (w + 20, h + 9), (2 * w // 3 + 2, h + 9), (2 * w // 3 + 2, 2 * h // 3 + 1), (w // 3, 2 * h // 3 + 1)],
            [(-300, h // 2), (w + 500, -200), (w // 2, h + 400)], [(2, 2), (w - 2, h - 2), (w - 2, 2), (2, h - 2)],
            [(0, h - 3), (w, h - 2), (0, h - 1)], [(w + 40, 0), (w + 90, 0), (w + 40, h)]]


@pytest.mark.parametrize("rgb", [0, 1])
@pytest.mark.parametrize("width", [1, 2, 9])
@pytest.mark.parametrize("h,w", SIZES)
def test_draw_whole_frames(h, w, width, rgb):
    frame = noise(h, w)
    want = check_draw(frame, kinds(h, w), OCC, VIS, width, rgb)
    assert (want != frame).any()


def test_draw_eight_overlapping_zones_highest_on_top():
    zones = [[(5 + 9 * z, 3 + 2 * z), (120 + 20 * z, 6 + z), (110 + 20 * z, 50 + z), (9 * z, 40 + 3 * z)] for z in range(8)]
    frame = noise(64, 300, 3)
    want = check_draw(frame, zones, [1, 2, 0, 4, 5, 0, 7, 0], [1, 2, 3, 4, 5, 6, 7, 8], 3, 1)
    x, y = 80, 22                                                            # inside all eight, no outline near, no label: blended once, with 6
    assert all(R.inside(zn, (x, y)) for zn in zones)
    assert (want[y, x] == (3 * frame[y, x].astype(int) + np.array(R.PALETTE[6]) + 2) >> 2).all()
    assert (want[6 + 7, 120 + 140] == R.PALETTE[7]).all()


@pytest.mark.parametrize("zone", [[(-60, 2), (10, 2), (10, 14)], [(290, 2), (380, 2), (380, 14)], [(100, -30), (120, 4), (90, 4)],
                                  [(100, 30), (120, 60), (90, 60)], [(-400, -40), (-300, -20), (-300, -40)]])
def test_draw_a_label_clipped_at_each_border(zone):
    """A label wider or taller than the frame stays at its anchor and is clipped: left, right, top, bottom, and wholly outside."""
    for (h, w), fig in (((12, 250), 2147483647), ((40, 60), 0)):
        check_draw(noise(h, w, 5), [zone], [fig], [fig], 2, 0)


def test_draw_a_zone_wholly_outside_writes_no_byte():
    from faster_rcnn_amd import ops
    frame = noise(12, 60)
    d = dev(frame)
    far = [[(-500, -300), (-400, -320), (-450, -200)]]
    ops.zone_draw_u8(d, dev(R.make_list(3, [1], [1])), far, 9)
    ops.zone_draw_u8(d, dev(R.make_list(0, [5], [5])), [[(0, 0), (59, 0), (59, 11)]], 9)      # the list of a frame that is not real
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), frame)
    assert np.array_equal(R.draw(frame, R.make_list(3, [1], [1]), far, 9, 0), frame)


@pytest.mark.parametrize("occupied", [0, 1])
def test_draw_a_zone_that_covers_the_whole_frame(occupied):
    frame = noise(33, 171, 7)
    zone = [(-32768, -32768), (65535, -32768), (65535, 65535), (-32768, 65535)]             # the cross product's square passes 2^63
    want = check_draw(frame, [zone], [occupied], [3], 3, 1)
    box = R.label_box(zone, R.label_text(0, occupied, 3), 33, 171)
    changed = (want != frame).any(axis=2)
    changed[box[1]:box[1] + box[3], box[0]:box[0] + box[2]] = bool(occupied)
    assert changed.mean() > 0.99 if occupied else not changed.any()          # (a byte the blend maps to itself is no change)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_everything_untouched_and_the_accepted_call_then_runs():
    from faster_rcnn_amd import _lib, ops
    lib = _lib.load()
    cap, rows, F = 16, 20, 4
    bufs_h = walk(9, H, W, rows, F, 14)
    bufs, n, table = dev(bufs_h), word(F), dev(CLASSES)
    state, lists = ops.zone_state(cap), ops.zone_workspace(F)
    lists.fill_(POISON)
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()
    arr = lambda v: np.ascontiguousarray(np.asarray(v, dtype=np.int32).reshape(-1))
    lp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ok_v, ok_nv = arr([v for zn in ZONES8 for v in zn]), arr([len(zn) for zn in ZONES8])
    tri = lambda *pts: dict(verts=lp(keep.setdefault(pts, arr(pts))), nv=lp(three), n_zones=1)
    keep, three = {}, arr([3])
    good = dict(state=p(state), cap=cap, tracked=p(bufs), stride=4 + 8 * rows, rows=rows, frames=F, n_frames=p(n), gate=None, verts=lp(ok_v), nv=lp(ok_nv),
                n_zones=8, classes=p(table), nc=5, anchor=0, expire=2, h=H, w=W, lists=p(lists))
    nv2, nv17, nv_last = arr([2]), arr([17]), arr([len(zn) for zn in ZONES8[:7]] + [17])
    bad_zones = [dict(n_zones=0), dict(n_zones=9), dict(nv=lp(nv2), n_zones=1), dict(nv=lp(nv17), n_zones=1), dict(nv=lp(nv_last)),
                 tri((5, 5), (5, 5), (9, 9)), tri((5, 5), (9, 9), (9, 9)), tri((5, 5), (9, 9), (5, 5)), tri((-32769, 0), (5, 5), (9, 0)),
                 tri((0, 0), (5, 65536), (9, 0))]
    bad = [dict(state=None), dict(tracked=None), dict(n_frames=None), dict(verts=None), dict(nv=None), dict(classes=None), dict(lists=None), dict(cap=0),
           dict(cap=129), dict(rows=0), dict(rows=513), dict(frames=0), dict(frames=65), dict(stride=4 + 8 * rows - 1), dict(nc=0), dict(nc=257),
           dict(anchor=-1), dict(anchor=2), dict(expire=-1), dict(expire=4096), dict(h=0), dict(w=0), dict(h=32769), dict(w=32769)] + bad_zones
    call = lambda a: lib.frcnn_zone_update(a["state"], a["cap"], a["tracked"], a["stride"], a["rows"], a["frames"], a["n_frames"], a["gate"], a["verts"],
                                           a["nv"], a["n_zones"], a["classes"], a["nc"], a["anchor"], a["expire"], a["h"], a["w"], a["lists"], None)
    for change in bad:
        assert call(dict(good, **change)) == E_ARG, change
    frame = dev(noise(37, 53))
    f0 = frame.cpu().numpy().copy()
    zl = R.make_list(1, [1, 0, 2, 0, 1, 1, 0, 0], list(range(8)))
    zlist = dev(zl)
    gd = dict(frame=p(frame), h=37, w=53, list=p(zlist), verts=lp(ok_v), nv=lp(ok_nv), n_zones=8, width=3)
    draw = lambda a: lib.frcnn_zone_draw_u8(a["frame"], a["h"], a["w"], a["list"], a["verts"], a["nv"], a["n_zones"], a["width"], 0, None)
    for change in [dict(frame=None), dict(list=None), dict(verts=None), dict(nv=None), dict(h=0), dict(w=0), dict(h=32769), dict(w=32769), dict(width=0),
                   dict(width=10)] + bad_zones:
        assert draw(dict(gd, **change)) == E_ARG, change
    torch.cuda.synchronize()
    assert not state.cpu().numpy().any() and (lists.cpu().numpy() == POISON).all() and np.array_equal(frame.cpu().numpy(), f0)
    # the accepted calls then run
    assert call(good) == 0 and draw(gd) == 0
    torch.cuda.synchronize()
    ref = R.Zones(H, W, ZONES8, CLASSES, cap, 2)
    assert np.array_equal(lists.cpu().numpy(), ref.update(bufs_h, F)) and np.array_equal(state.cpu().numpy(), ref.words())
    assert np.array_equal(frame.cpu().numpy(), R.draw(f0, zl, ZONES8, 3, 0))
    assert lib.frcnn_zone_state_bytes(0) == 0 and lib.frcnn_zone_state_bytes(129) == 0
    assert lib.frcnn_zone_state_bytes(cap) == 4 * R.state_words(cap) and lib.frcnn_zone_list_words() == R.LIST_WORDS == ops.ZONE_LIST_WORDS
    with pytest.raises(_lib.FrcnnError):
        ops.zone_state(129)
    with pytest.raises(_lib.FrcnnError):
        ops.zone_workspace(65)


def test_reset_keeps_or_clears_the_totals():
    from faster_rcnn_amd import ops
    bufs = walk(6, H, W, 40, 6, 30)
    state = ops.zone_state(24)
    ops.zone_update(state, dev(bufs), word(6), ZONES8, dev(CLASSES), 2, H, W)
    before = ops.zone_totals(state)
    assert before["entries"] > 0 and before["frames"] == 6 and sum(before["visitors"]) > 0 and sum(before["peak"]) > 0
    ops.zone_reset(state, keep_totals=True)
    after = ops.zone_totals(state)
    assert after == dict(before, entries=0) and not state[ops.ZONE_HEAD:].cpu().numpy().any()
    ops.zone_reset(state)
    assert not state.cpu().numpy().any()
