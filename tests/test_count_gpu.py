"""The two entry points of the count extension (include/ext/frcnn_hip_count.h, csrc/count.hip) against the restatement
(tests/count_ref.py), word for word and byte for byte: ops.count_update over hand-made tracked buffers -- every word of the state and of
the count lists, in workspaces pre-filled with 0x7f -- and ops.count_draw_u8 over hand-made count lists, on whole frames."""
import numpy as np
import pytest

from tests import count_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

E_ARG = -1                                                                   # FRCNN_E_ARG
POISON = 0x7f7f7f7f
CLASSES = np.array([0, 1, 0, 1, 1], dtype=np.uint8)                          # class 2 is switched off (0 is the background)
LINES8 = [(40, -10, 40, 130), (0, 50, 200, 50), (10, 10, 150, 110), (150, 5, 20, 100), (80, 0, 80, 60), (80, 60, 80, 120), (-100, 30, 300, 80),
          (120, 119, 120, 0)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def word(v):
    return dev(np.array([v], dtype=np.int32))


def walk(seed, h, w, rows, frames, n_ids, absent=0.2):
    """Tracked buffers of ids on a random walk with long steps: a random subset of the ids in a random row order every frame (so ids
    arrive in any order, are absent and return), rows with id 0 and a class that does not count among them, the rows behind n_live and
    every unused word poisoned."""
    rs = np.random.RandomState(seed)
    pos = np.stack([rs.randint(0, w, n_ids), rs.randint(0, h, n_ids)], axis=1)
    cls = rs.randint(1, 5, n_ids)
    out = []
    for f in range(frames):
        pos = np.clip(pos + rs.randint(-40, 41, pos.shape), [-6, -6], [w + 5, h + 5])
        present = [i for i in rs.permutation(n_ids) if rs.rand() >= absent][:rows - 2 if rows > 2 else rows]
        rws = [(int(i) + 1 + (f // 7 if i % 9 == 0 else 0) * n_ids, int(cls[i]), (pos[i][0] - 3, pos[i][1] - 2, pos[i][0] + 3, pos[i][1] + 2)) for i in present]
        if len(rws) < rows:
            rws.insert(len(rws) // 2, (0, 1, (POISON, POISON, POISON, POISON)))                 # id 0: its box is never read
        n_live = len(rws)
        if len(rws) < rows:
            rws.append((900 + f, 1, (POISON, -POISON, POISON, -POISON)))                      # a held row, behind n_live
        out.append(R.make_tracked(rws, rows, n_live=n_live, fill=POISON))
    return np.stack(out)


def run(bufs, calls, lines, cap, expire, h, w, classes=CLASSES):
    """``calls``: [(first frame, frames, the n_frames word[, the gate word])] -> [(state, lists) after each call] from the device and from
    the rule.  The workspaces are pre-filled with 0x7f."""
    from faster_rcnn_amd import ops
    state, ref, got, want = ops.count_state(cap), R.Counter(h, w, lines, classes, cap, expire), [], []
    table = dev(classes)
    for first, frames, n, *gate in calls:
        part = bufs[first:first + frames]
        lists = ops.count_workspace(len(part))
        lists.fill_(POISON)
        ops.count_update(state, dev(part), word(n), lines, table, expire, h, w, lists=lists, gate=word(gate[0]) if gate else None)
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
@pytest.mark.parametrize("cap,rows,frames,n_lines", [(1, 1, 1, 1), (2, 63, 2, 8), (63, 64, 64, 1), (64, 65, 2, 8), (65, 512, 2, 1), (128, 512, 64, 8),
                                                     (128, 65, 1, 8), (64, 63, 64, 8)])
def test_update_matches_the_rule(cap, rows, frames, n_lines):
    h, w = 120, 200
    n_ids = min(rows, 2 * cap + 8)
    bufs = walk(cap + rows, h, w, rows, frames, n_ids)
    got, want, ref = run(bufs, [(0, frames, frames)], LINES8[:n_lines], cap, 2, h, w)
    same(got, want)
    assert ref.frames == frames
    if frames == 64:
        assert sum(map(sum, ref.totals)) > 20
    if (cap, rows, frames) == (128, 512, 64):                                # more ids than entries, more events in a frame than a list holds
        assert ref.dropped > 0 and ref.events_dropped > 0


@pytest.mark.parametrize("case", R.HAND_CASES, ids=[c[0] for c in R.HAND_CASES])
def test_the_hand_cases(case):
    _, (h, w), lines, points, answers = case
    got, want, _ = run(R.hand_buffers(points), [(0, len(points), len(points))], lines, 4, 9, h, w)
    same(got, want)
    assert [[ev[:2] for ev in R.events_of(l)] for l in got[0][1]] == [[tuple(a) for a in ans] for ans in answers]
    assert all(ev[2:] == (1, 1) for l in got[0][1] for ev in R.events_of(l))


def test_ids_arriving_in_descending_row_order_keep_id_order():
    rows = [(i, 1, (10 * i, 5, 10 * i, 5)) for i in (9, 7, 5, 3, 1)]
    bufs = np.stack([R.make_tracked(rows, 8, fill=POISON), R.make_tracked([(i, c, (x, 90, x, 90)) for i, c, (x, *_) in rows[::2]], 8, fill=POISON)])
    got, want, ref = run(bufs, [(0, 2, 2)], [(0, 50, 200, 50)], 8, 5, 120, 200)
    same(got, want)
    assert [e["id"] for e in ref.entries] == [1, 3, 5, 7, 9] and [ev[2] for ev in R.events_of(got[0][1][1])] == [9, 5, 1]


def test_a_full_table_drops_rows_and_expiry_frees_places():
    frames = [[(i, 1, (5 * i, 5, 5 * i, 5)) for i in (4, 2, 6, 8, 5)],                      # capacity 3: 4, 2, 6 enter; 8 and 5 are dropped
              [(8, 1, (40, 5, 40, 5)), (2, 1, (10, 90, 10, 90))],                             # still full: 8 dropped; 2 crosses (+)
              [(8, 1, (40, 5, 40, 5)), (2, 1, (10, 5, 10, 5))],                               # E = 1: 4 and 6 are still there; 2 crosses (-)
              [(8, 1, (40, 90, 40, 90))]]                                                     # 4 and 6 have left: 8 enters, without a crossing
    bufs = np.stack([R.make_tracked(f, 6, fill=POISON) for f in frames])
    got, want, ref = run(bufs, [(0, 4, 4)], [(0, 50, 200, 50)], 3, 1, 120, 200)
    same(got, want)
    assert ref.dropped == 4 and [e["id"] for e in ref.entries] == [2, 8] and ref.totals[0] == [1, 1]


@pytest.mark.parametrize("expire", [0, 1])
def test_expiry(expire):
    """Absent for one frame: with E = 0 the entry is gone and the id starts afresh (no crossing), with E = 1 it steps from where it was."""
    frames = [[(1, 1, (10, 10, 10, 10))], [], [(1, 1, (10, 90, 10, 90))], [(1, 1, (10, 10, 10, 10))]]
    bufs = np.stack([R.make_tracked(f, 2, fill=POISON) for f in frames])
    got, want, ref = run(bufs, [(0, 4, 4)], [(0, 50, 200, 50)], 2, expire, 120, 200)
    same(got, want)
    assert ref.totals[0] == ([1, 1] if expire else [1, 0])


def test_65_crossings_in_one_frame():
    a = [(i, 1, (2 * i, 10, 2 * i, 10)) for i in range(1, 66)]
    b = [(i, 1, (2 * i, 90, 2 * i, 90)) for i in range(65, 0, -1)]
    bufs = np.stack([R.make_tracked(a, 70, fill=POISON), R.make_tracked(b, 70, fill=POISON)])
    got, want, ref = run(bufs, [(0, 2, 2)], [(0, 50, 200, 50)], 128, 3, 120, 200)
    same(got, want)
    assert got[0][1][1][0] == 64 and got[0][0][3] == 1 and got[0][0][5] == 65 and ref.events_dropped == 1
    assert [ev[2] for ev in R.events_of(got[0][1][1])] == list(range(65, 1, -1))              # (row, line) order


def test_a_class_switched_off_and_poisoned_rows():
    """Class 2 does not count, a class outside the table neither; id 0, held rows and rows behind n_live carry poison and are never read."""
    f0 = [(1, 1, (10, 10, 10, 10)), (2, 2, (20, 10, 20, 10)), (3, 7, (30, 10, 30, 10)), (0, 1, (POISON,) * 4), (4, -1, (40, 10, 40, 10))]
    f1 = [(1, 1, (10, 90, 10, 90)), (2, 2, (20, 90, 20, 90)), (3, 7, (30, 90, 30, 90)), (0, 1, (POISON,) * 4), (4, -1, (40, 90, 40, 90))]
    bufs = np.stack([R.make_tracked(f + [(5, 1, (POISON,) * 4)], 9, n_live=5, fill=POISON) for f in (f0, f1)])
    got, want, ref = run(bufs, [(0, 2, 2)], [(0, 50, 200, 50)], 8, 3, 120, 200)
    same(got, want)
    assert [e["id"] for e in ref.entries] == [1] and R.events_of(got[0][1][1]) == [(0, 1, 1, 1)]


@pytest.mark.parametrize("n", [0, -3, 2, 5, 9])
def test_the_n_frames_word(n):
    bufs = walk(3, 120, 200, 20, 7, 12)
    got, want, _ = run(bufs, [(0, 2, 2), (2, 5, n)], LINES8, 16, 2, 120, 200)
    same(got, want)
    nf = min(max(n, 0), 5)
    assert not got[1][1][nf:].any() and got[1][0][1] == 2 + nf
    if nf == 0:
        assert np.array_equal(got[1][0], got[0][0])


def test_a_gate_word_of_zero_makes_the_call_no_frames():
    bufs = walk(4, 120, 200, 20, 10, 12)
    got, want, _ = run(bufs, [(0, 5, 5, 7), (5, 5, 5, 0), (5, 5, 5, -1)], LINES8, 16, 2, 120, 200)
    same(got, want)
    assert np.array_equal(got[1][0], got[0][0]) and not got[1][1].any() and got[2][0][1] == 10 and got[2][1].any()


def test_two_calls_equal_one_call_and_the_same_call_twice_gives_the_same_bytes():
    bufs = walk(6, 120, 200, 40, 12, 30)
    one, want, _ = run(bufs, [(0, 12, 12)], LINES8, 24, 2, 120, 200)
    same(one, want)
    two, _, _ = run(bufs, [(0, 5, 5), (5, 7, 7)], LINES8, 24, 2, 120, 200)
    again, _, _ = run(bufs, [(0, 12, 12)], LINES8, 24, 2, 120, 200)
    assert np.array_equal(two[1][0], one[0][0]) and np.array_equal(np.concatenate([two[0][1], two[1][1]]), one[0][1])
    assert np.array_equal(again[0][0], one[0][0]) and np.array_equal(again[0][1], one[0][1])
    assert one[0][0][4:20].sum() > 0


def test_a_captured_call_replayed_after_its_inputs_changed_in_place():
    from faster_rcnn_amd import ops
    h, w, cap, rows, F = 120, 200, 16, 20, 4
    bufs = walk(8, h, w, rows, 3 * F, 14)
    state, tracked, n, gate, lists, table = ops.count_state(cap), dev(bufs[:F]), word(0), word(1), ops.count_workspace(F), dev(CLASSES)
    run_ = lambda: ops.count_update(state, tracked, n, LINES8, table, 2, h, w, lists=lists, gate=gate)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run_()
    assert not state.cpu().numpy().any()                                     # 0 frames: warm-up and capture wrote no word of the state
    ref = R.Counter(h, w, LINES8, CLASSES, cap, 2)
    for k, real in enumerate((F, 2, F)):
        tracked.copy_(dev(bufs[k * F:k * F + F]))
        n.fill_(real)
        lists.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(lists.cpu().numpy(), ref.update(bufs[k * F:k * F + F], real)), k
        assert np.array_equal(state.cpu().numpy(), ref.words()), k
    assert ref.frames == 2 * F + 2 and sum(map(sum, ref.totals)) > 0


# ------------------------------------------------------------------------------------------------------------ draw
def noise(h, w, seed=1):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def check_draw(frame, lines, totals, width, rgb, frames=1):
    from faster_rcnn_amd import ops
    clist = R.make_list(frames, totals)
    d = dev(frame)
    ops.count_draw_u8(d, dev(clist), lines, width, rgb=bool(rgb))
    torch.cuda.synchronize()
    want = R.draw(frame, clist, lines, width, rgb)
    got = d.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:6]
    return want


SIZES = [(1, 1), (16, 85), (17, 86), (33, 171), (64, 300)]
TOTALS = [(0, 0), (9, 10), (99999, 0), (2147483647, 2147483647), (10, 99999), (0, 9), (1, 2), (3, 4)]


def kinds(h, w):
    """Horizontal, vertical, diagonal, clipped by the border, two that share pixels, and one fully outside."""
    return [(2, h // 2, w - 3, h // 2), (w // 2, 1, w // 2, h - 2), (0, 0, w, h), (-20, h // 3, w + 30, h // 2), (w // 2 - 4, 1, w // 2 + 4, h - 2),
            (w + 40, 0, w + 40, h)]


@pytest.mark.parametrize("rgb", [0, 1])
@pytest.mark.parametrize("width", [1, 2, 9])
@pytest.mark.parametrize("h,w", SIZES)
def test_draw_whole_frames(h, w, width, rgb):
    frame = noise(h, w)
    want = check_draw(frame, kinds(h, w), TOTALS[:6], width, rgb)
    assert (want != frame).any()


def test_draw_eight_lines_highest_on_top():
    lines = [(5, 5 + 3 * l, 290, 40 + l) for l in range(8)]
    want = check_draw(noise(64, 300, 3), lines, TOTALS, 3, 1)
    assert (want[40 + 7, 290] == R.PALETTE[7]).all()


@pytest.mark.parametrize("line", [(-60, 8, 10, 8), (290, 8, 380, 8), (100, -30, 120, 4), (100, 30, 120, 60), (-400, -40, -300, -20)])
def test_draw_a_label_clipped_at_each_border(line):
    """A label wider or taller than the frame stays at its anchor and is clipped: left, right, top, bottom, and wholly outside."""
    for (h, w), totals in (((12, 300), (2147483647, 2147483647)), ((40, 60), (0, 0))):
        check_draw(noise(h, w, 5), [line], [totals], 2, 0)


def test_draw_lines_and_labels_wholly_outside_write_no_byte():
    from faster_rcnn_amd import ops
    frame = noise(12, 60)
    d = dev(frame)
    ops.count_draw_u8(d, dev(R.make_list(3, [(1, 1)])), [(-500, -300, -400, -320)], 9)
    ops.count_draw_u8(d, dev(R.make_list(0, [(5, 5)])), [(0, 0, 59, 11)], 9)                 # the list of a frame that is not real
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), frame)
    assert np.array_equal(R.draw(frame, R.make_list(3, [(1, 1)]), [(-500, -300, -400, -320)], 9, 0), frame)


def test_draw_long_lines_beyond_the_frame():
    """Ends at the limits of the coordinate range: the cross product's square passes 2^63."""
    check_draw(noise(33, 171, 7), [(-32768, -32768, 65535, 65535), (65535, -32768, -32768, 40000)], [(1, 2), (3, 4)], 3, 1)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_everything_untouched_and_the_accepted_call_then_runs():
    from faster_rcnn_amd import _lib, ops
    lib = _lib.load()
    h, w, cap, rows, F = 120, 200, 16, 20, 4
    bufs_h = walk(9, h, w, rows, F, 14)
    bufs, n, table = dev(bufs_h), word(F), dev(CLASSES)
    state, lists = ops.count_state(cap), ops.count_workspace(F)
    state.fill_(0)
    lists.fill_(POISON)
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()
    import ctypes
    arr = lambda v: np.ascontiguousarray(np.asarray(v, dtype=np.int32))
    ok_lines = arr(LINES8)
    lp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    good = dict(state=p(state), cap=cap, tracked=p(bufs), stride=4 + 8 * rows, rows=rows, frames=F, n_frames=p(n), gate=None, lines=lp(ok_lines), n_lines=8,
                classes=p(table), nc=5, expire=2, h=h, w=w, lists=p(lists))
    same_ab, low, high = arr([(5, 5, 5, 5)]), arr([(-32769, 0, 5, 5)]), arr([(0, 0, 5, 65536)])
    bad = [dict(state=None), dict(tracked=None), dict(n_frames=None), dict(lines=None), dict(classes=None), dict(lists=None), dict(cap=0), dict(cap=129),
           dict(rows=0), dict(rows=513), dict(frames=0), dict(frames=65), dict(stride=4 + 8 * rows - 1), dict(n_lines=0), dict(n_lines=9),
           dict(lines=lp(same_ab), n_lines=1), dict(lines=lp(low), n_lines=1), dict(lines=lp(high), n_lines=1), dict(nc=0), dict(nc=257),
           dict(expire=-1), dict(expire=4096), dict(h=0), dict(w=0), dict(h=32769), dict(w=32769)]
    call = lambda a: lib.frcnn_count_update(a["state"], a["cap"], a["tracked"], a["stride"], a["rows"], a["frames"], a["n_frames"], a["gate"], a["lines"],
                                            a["n_lines"], a["classes"], a["nc"], a["expire"], a["h"], a["w"], a["lists"], None)
    for change in bad:
        assert call(dict(good, **change)) == E_ARG, change
    frame = dev(noise(37, 53))
    f0 = frame.cpu().numpy().copy()
    clist = dev(R.make_list(1, TOTALS))
    gd = dict(frame=p(frame), h=37, w=53, list=p(clist), lines=lp(ok_lines), n_lines=8, width=3)
    draw = lambda a: lib.frcnn_count_draw_u8(a["frame"], a["h"], a["w"], a["list"], a["lines"], a["n_lines"], a["width"], 0, None)
    for change in [dict(frame=None), dict(list=None), dict(lines=None), dict(h=0), dict(w=0), dict(h=32769), dict(w=32769), dict(n_lines=0), dict(n_lines=9),
                   dict(lines=lp(same_ab), n_lines=1), dict(lines=lp(high), n_lines=1), dict(width=0), dict(width=10)]:
        assert draw(dict(gd, **change)) == E_ARG, change
    torch.cuda.synchronize()
    assert not state.cpu().numpy().any() and (lists.cpu().numpy() == POISON).all() and np.array_equal(frame.cpu().numpy(), f0)
    # the accepted calls then run
    assert call(good) == 0 and draw(gd) == 0
    torch.cuda.synchronize()
    ref = R.Counter(h, w, LINES8, CLASSES, cap, 2)
    assert np.array_equal(lists.cpu().numpy(), ref.update(bufs_h, F)) and np.array_equal(state.cpu().numpy(), ref.words())
    assert np.array_equal(frame.cpu().numpy(), R.draw(f0, R.make_list(1, TOTALS), LINES8, 3, 0))
    assert lib.frcnn_count_state_bytes(0) == 0 and lib.frcnn_count_state_bytes(129) == 0
    assert lib.frcnn_count_state_bytes(cap) == 4 * R.state_words(cap) and lib.frcnn_count_list_words() == R.LIST_WORDS == ops.COUNT_LIST_WORDS
    with pytest.raises(_lib.FrcnnError):
        ops.count_state(129)
    with pytest.raises(_lib.FrcnnError):
        ops.count_workspace(65)


def test_reset_keeps_or_clears_the_totals():
    from faster_rcnn_amd import ops
    bufs = walk(6, 120, 200, 40, 6, 30)
    state = ops.count_state(24)
    ops.count_update(state, dev(bufs), word(6), LINES8, dev(CLASSES), 2, 120, 200)
    before = ops.count_totals(state)
    assert before["entries"] > 0 and before["frames"] == 6 and sum(map(sum, before["totals"])) > 0
    ops.count_reset(state, keep_totals=True)
    after = ops.count_totals(state)
    assert after["entries"] == 0 and after["totals"] == before["totals"] and after["frames"] == 6 and not state[ops.COUNT_HEAD:].cpu().numpy().any()
    ops.count_reset(state)
    assert not state.cpu().numpy().any()
