"""The four ``strong=`` tracker calls of ops (csrc/track.hip's WEAK instantiation behind frcnn_track_update_weak and its motion, interval and
cut forms) against the plain-Python restatement of the weak rule in tests/track_weak_ref.py, every word of every tracked buffer and of the
state; each form at strong = 0.0 against its parent entry point, byte for byte; the refusals."""
import numpy as np
import pytest

from tests import track_weak_ref as WR
from tests.test_track_gpu import pack

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

H, W = 120, 160
TABLE = np.array([0, 1, 1, 0, 1], dtype=np.uint8)         # classes 0 and 3 are not tracked
STRONG = 0.5
NAN = float("nan")


def sequence(seed, frames, rows, objects):
    """A seeded sequence of packed buffers: ``objects`` boxes drift, and each frame an object is seen strongly (0.9 / 0.5, the threshold
    itself), weakly (0.3 / 0.0 / NaN) or not at all; a weak sighting now and then comes with a strong row of a smaller overlap, a repeated
    row (a tie) or a stray weak row nothing reaches; rows of untracked and out-of-range classes of both kinds follow."""
    rs = np.random.RandomState(seed)
    pos = rs.randint(0, [W - 30, H - 30], (objects, 2))
    size = rs.randint(10, 36, (objects, 2))
    cls = rs.choice([1, 2, 4], objects)
    out = []
    for f in range(frames):
        pos += rs.randint(-2, 3, pos.shape)
        b, c, p = [], [], []
        for o in rs.permutation(objects):
            how = rs.rand()
            if how < 0.2 and f:
                continue                                              # missed
            box = [pos[o, 0], pos[o, 1], pos[o, 0] + size[o, 0], pos[o, 1] + size[o, 1]]
            if rs.rand() < 0.2:
                box = [box[2], box[3], box[0], box[1]]               # reversed corners
            score = rs.choice([0.9, 0.5]) if how > 0.6 or f == 0 else rs.choice([0.3, 0.0, NAN, 0.49999997])
            b.append(box), c.append(cls[o]), p.append(score)
            if rs.rand() < 0.2:                                      # the same box twice, as weak as it or weaker: a tie
                b.append(list(box)), c.append(cls[o]), p.append(min(score, 0.3) if score == score else 0.3)
            if rs.rand() < 0.2:                                      # a strong row of the class that overlaps less
                b.append([box[0] + 4, box[1] + 3, box[2] + 4, box[3] + 3]), c.append(cls[o]), p.append(0.8)
        b += [[W - 9, H - 9, W + 5, H + 5], [10, 10, 50, 50], [20, 20, 60, 60], [12, 12, 40, 40], [-40, 5, -3, 30], [-40, 5, -3, 30]]
        c += [4, 0, 9, 3, 1, 2]                                      # a stray weak row, untracked strong, out of range weak, ..., outside
        p += [0.2, 0.9, 0.1, 0.2, 0.9, 0.1]
        order = rs.permutation(len(c))[:rows]
        out.append(pack([b[i] for i in order], [c[i] for i in order], len(order), rows, prob=[p[i] for i in order]))
    return out


def run_chunks(frames, chunks, capacity, params, strong, short=0, h=H, w=W):
    """The frames through ops.track_update(strong=) in calls of ``chunks`` frames (cycled), the state carried over, each call and the
    state after it against the restatement; ``short`` padding frames behind each call's real ones.  -> the reference tracker."""
    from faster_rcnn_amd import ops
    rows = (frames[0].size - 4) // 7
    ref = WR.Tracker(capacity)
    state = ops.track_state(capacity)
    table = torch.from_numpy(TABLE).cuda()
    at, k = 0, 0
    while at < len(frames):
        real = frames[at:at + chunks[k % len(chunks)]]
        part = real + [frames[0]] * short
        dev = torch.from_numpy(np.stack(part)).cuda()
        nf = torch.tensor([len(real)], dtype=torch.int32, device="cuda")
        out = torch.full((len(part), 4 + 8 * (rows + capacity)), 77, dtype=torch.int32, device="cuda")
        got = ops.track_update(state, dev if len(part) > 1 else dev[0], nf, table, h, w, *params, out=out, strong=strong).cpu().numpy()
        for i, p in enumerate(part):
            want = ref.update_packed(p, TABLE, h, w, *params, strong=strong) if i < len(real) else ref.padding(rows)
            bad = np.flatnonzero(got[i] != want)
            assert bad.size == 0, (at + i, bad[:8].tolist(), got[i][bad[:8]].tolist(), want[bad[:8]].tolist())
        assert np.array_equal(state.cpu().numpy(), ref.words()), at
        at += len(real)
        k += 1
    return ref


@pytest.mark.parametrize("capacity,rows,objects", [(1, 2, 2), (3, 3, 3), (3, 130, 110), (64, 130, 110), (64, 448, 380), (1, 448, 380)])
def test_sequences_against_the_restatement(capacity, rows, objects):
    """Calls of 1, 2 and 8 frames, with and without padding behind the real frames."""
    params = (30, 2, 3)
    frames = sequence(31 * capacity + rows, 11, rows, objects)
    a = run_chunks(frames, [1, 2, 8], capacity, params, STRONG)
    b = run_chunks(frames, [8, 2, 1], capacity, params, STRONG, short=2)
    assert np.array_equal(a.words(), b.words()) and a.words()[3] == len(frames) and a.events == b.events
    ev = a.events
    assert ev["match"] and ev["birth"] and ev["weak_drop"], ev
    if capacity == 64:                                                   # (the sequences' own check: the full grid exercises every step)
        assert ev["weak_match"] and ev["hold"] and ev["free"] and ev["overflow"], ev


def filler(k):
    return [[10, 100, 20, 110]] * k, [0] * k, [0.9] * k              # rows of an untracked class: strong, kept, never matched


def test_rows_on_both_sides_of_a_wave_boundary():
    """130 rows: a thread owns rows 2t and 2t + 1, so rows 0..127 are the first wave's.  Slot 1's strong row (row 5, the smaller IoU) is in
    the first wave and its weak row (row 129, the larger IoU) in the second: the strong row wins.  Slot 2 has weak rows only, of one
    IoU, in both waves: the lower row wins, and the other is dropped."""
    rows, cap = 130, 3
    fb, fc, fp = filler(130)
    first = pack([[10, 10, 39, 39], [80, 10, 109, 39], [120, 60, 139, 79]], [1, 1, 2], 3, rows, prob=[0.9, 0.9, 0.9])
    b, c, p = list(fb), list(fc), list(fp)
    b[5], c[5], p[5] = [14, 10, 43, 39], 1, 0.7                       # slot 1, strong, IoU 26 / 34
    b[129], c[129], p[129] = [10, 10, 39, 39], 1, 0.3                 # slot 1, weak, IoU 1
    b[128], c[128], p[128] = [82, 10, 111, 39], 1, 0.3                # slot 2, weak
    b[100], c[100], p[100] = [78, 10, 107, 39], 1, 0.2                # slot 2, weak, the same IoU: the lower row
    second = pack(b, c, 130, rows, prob=p)                            # slot 3 (class 2) sees nothing: held
    for chunks in ([2], [1]):
        ref = run_chunks([first, second], chunks, cap, (30, 2, 1), STRONG)
    ids = {t["id"]: t for t in ref.slots}
    assert ids[1]["bbox"] == [14, 10, 43, 39] and ids[2]["bbox"] == [78, 10, 107, 39] and ids[3]["age"] == 1
    assert ref.events["weak_match"] == 1 and ref.events["weak_drop"] == 2 and ref.next_id == 4


def test_small_cases():
    from faster_rcnn_amd import ops
    rows = 8
    frames = [
        pack([[10, 10, 29, 29], [60, 10, 79, 29], [100, 50, 119, 69]], [1, 2, 4], 3, rows, prob=[0.9, 0.8, 0.7]),
        pack([], [], 0, rows, dead_box=(10, 10, 29, 29), dead_cls=1),       # n = 0: everything is held
        pack([[11, 10, 30, 29], [60, 10, 79, 29], [60, 10, 79, 29], [100, 50, 119, 69]], [1, 2, 2, 3], 4, rows,
             prob=[0.3, 0.2, 0.2, 0.1]),                                    # all weak: a tie, and a row of an untracked class
        pack([[11, 10, 30, 29], [0, 90, 19, 109]], [1, 1], 2, rows, prob=[NAN, 0.4]),   # a NaN score continues; a stray weak row births nothing
        pack([[12, 10, 31, 29], [12, 10, 31, 29]], [1, 1], rows + 3, rows, prob=[0.2, 0.9]),   # the strong one of two equal boxes
    ]
    for chunks, cap in (([1], 4), ([5], 4), ([2, 3], 1), ([1], 64)):
        ref = run_chunks(frames, chunks, cap, (30, 3, 2), STRONG)
    assert ref.events["weak_match"] >= 3 and ref.events["weak_drop"] >= 4
    # *n_frames = 0: no word of the state moves, the buffers are padding
    state = ops.track_state(4)
    ref = WR.Tracker(4)
    ref.update_packed(frames[0], TABLE, H, W, strong=STRONG)
    state.copy_(torch.from_numpy(ref.words()).cuda())
    out = ops.track_update(state, torch.from_numpy(np.stack(frames[:2])).cuda(), torch.zeros(1, dtype=torch.int32, device="cuda"),
                           torch.from_numpy(TABLE).cuda(), H, W, strong=STRONG).cpu().numpy()
    assert np.array_equal(out[0], ref.padding(rows)) and np.array_equal(out[1], ref.padding(rows))
    assert np.array_equal(state.cpu().numpy(), ref.words())


def test_no_weak_row_in_reach_is_the_parent_on_the_strong_rows():
    """The rule's second equality: the weak rows of this sequence overlap no slot, so every buffer and the state are what the parent
    entry point makes of the strong rows alone."""
    from faster_rcnn_amd import ops
    rows, cap, params = 8, 4, (30, 2, 1)
    frames = []
    for f in range(6):
        last = [100, 60 - f, 119, 79 - f] if f != 3 else [0, 100, 15, 115]      # frame 3: the third object is seen weakly, elsewhere
        b = [[10 + f, 10, 29 + f, 29], [140, 100, 155, 115], [60, 10 + f, 79, 29 + f], [130, 5, 150, 20], last]
        frames.append(pack(b, [1, 1, 2, 4, 4], 5, rows, prob=[0.9, 0.1, 0.6, 0.3, 0.7 if f != 3 else NAN]))
    table = torch.from_numpy(TABLE).cuda()
    nf = torch.tensor([6], dtype=torch.int32, device="cuda")
    s_weak, s_par = ops.track_state(cap), ops.track_state(cap)
    got = ops.track_update(s_weak, torch.from_numpy(np.stack(frames)).cuda(), nf, table, H, W, *params, strong=STRONG)
    want = ops.track_update(s_par, torch.from_numpy(np.stack([WR.strong_only(p, STRONG) for p in frames])).cuda(), nf, table, H, W, *params)
    assert torch.equal(got, want) and torch.equal(s_weak, s_par) and int(s_weak[1]) == 3
    assert got.cpu().numpy()[:, 1].tolist() == [3, 3, 3, 2, 3, 3] and got.cpu().numpy()[:, 0].tolist() == [3, 3, 3, 3, 3, 3]


# ---------------------------------------------------------------------------------------------- strong = 0.0 is the parent
FH, FW = 32, 48


def film(n, cut_at):
    """``n`` frames of 32 x 48: dark noise that moves a pixel a frame, bright noise from frame ``cut_at`` on."""
    rs = np.random.RandomState(9)
    dark, bright = rs.randint(0, 100, (FH, FW + n, 3)), rs.randint(150, 256, (FH, FW + n, 3))
    return np.stack([(dark if f < cut_at else bright)[:, f:f + FW] for f in range(n)]).astype(np.uint8)


def boxes_at(f, rows=8):
    b = [[4 + f, 4, 19 + f, 19], [30, 8 + f, 43, 23 + f], [10, 20, 25, 30], [2, 2, 12, 12]]
    return pack(b, [1, 2, 4, 0], 4, rows, prob=[0.9, 0.6, 0.2 + 0.1 * f, 0.3])


@pytest.mark.parametrize("form", ["update", "motion", "interval", "cut"])
def test_strong_zero_is_the_parent_entry_byte_for_byte(form):
    from faster_rcnn_amd import ops
    cap, F, K, params = 4, 6, (2 if form in ("interval", "cut") else 1), (30, 1, 2)
    frames = torch.from_numpy(film(F, 4)).cuda()
    keys = -(-F // K)
    packed = torch.from_numpy(np.stack([boxes_at(f) if f != 2 else boxes_at(f)[:] * 0 for f in range(keys)])).cuda()
    table = torch.from_numpy(TABLE).cuda()
    res = []
    for strong in (None, 0.0):
        state, mstate = ops.track_state(cap), ops.track_motion_state(FH, FW)
        outs = []
        for nf in (F, F - 2):                                            # a second call: the kept frame, and a short pass
            n_frames = torch.tensor([nf], dtype=torch.int32, device="cuda")
            if form == "update":
                out = ops.track_update(state, packed, n_frames, table, FH, FW, *params, strong=strong)
            elif form == "motion":
                out = ops.track_update_motion(state, mstate, frames, 3 * FH * FW, packed, n_frames, table, FH, FW, *params, 4, strong=strong)
            elif form == "interval":
                out = ops.track_update_interval(state, mstate, frames, 3 * FH * FW, packed, n_frames, table, FH, FW, *params, 4, K,
                                                strong=strong)
            else:
                out, cuts = ops.track_update_cut(state, mstate, frames, 3 * FH * FW, packed, n_frames, table, FH, FW, *params, 4, K, 40,
                                                 strong=strong)
                outs.append(cuts.clone())
            outs.append(out.clone())
        res.append(outs + [state, mstate])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert int(res[0][-2][1]) >= 3 and int(res[0][-2][3]) == 2 * F - 2      # tracks were born; every real frame counted
    if form == "cut":
        assert res[0][0].cpu().tolist() == [0, 0, 0, 0, 1, 0]               # the one cut of the sequence


def test_bad_arguments_raise_and_write_nothing():
    from faster_rcnn_amd import _lib, ops
    rows, cap, F = 8, 4, 2
    table = torch.from_numpy(TABLE).cuda()
    frames = torch.from_numpy(film(F, 9)).cuda()
    packed = torch.from_numpy(np.stack([boxes_at(0), boxes_at(1)])).cuda()
    nf = torch.full((1,), F, dtype=torch.int32, device="cuda")
    state, mstate = ops.track_state(cap), ops.track_motion_state(FH, FW)
    out = torch.full((F, 4 + 8 * (rows + cap)), 77, dtype=torch.int32, device="cuda")
    calls = {
        "update": lambda strong, thr: ops.track_update(state, packed, nf, table, FH, FW, thr, 1, 0, out=out, strong=strong),
        "motion": lambda strong, thr: ops.track_update_motion(state, mstate, frames, 3 * FH * FW, packed, nf, table, FH, FW, thr, 1, 0, 4, out=out,
                                                              strong=strong),
        "interval": lambda strong, thr: ops.track_update_interval(state, mstate, frames, 3 * FH * FW, packed, nf, table, FH, FW, thr, 1, 0, 4, 1,
                                                                  out=out, strong=strong),
        "cut": lambda strong, thr: ops.track_update_cut(state, mstate, frames, 3 * FH * FW, packed, nf, table, FH, FW, thr, 1, 0, 4, 1, 40, out=out,
                                                        strong=strong),
    }
    for name, call in calls.items():
        with pytest.raises(_lib.FrcnnError, match="strong is NaN"):
            call(NAN, 30)
        with pytest.raises(_lib.FrcnnError, match="_weak: thr=0"):          # what the parent refuses, under the entry's own name
            call(0.5, 0)
    with pytest.raises(_lib.FrcnnError, match="radius"):
        ops.track_update_motion(state, mstate, frames, 3 * FH * FW, packed, nf, table, FH, FW, 30, 1, 0, 17, out=out, strong=0.5)
    with pytest.raises(_lib.FrcnnError, match="pct"):
        ops.track_update_cut(state, mstate, frames, 3 * FH * FW, packed, nf, table, FH, FW, 30, 1, 0, 4, 1, 0, out=out, strong=0.5)
    lib = _lib.load()
    assert lib.frcnn_track_weak_version() == _lib.TRACK_WEAK_VERSION == 1
    assert lib.frcnn_track_update_weak(None, cap, packed.data_ptr(), 0, 1, nf.data_ptr(), rows, table.data_ptr(), 5, 30, 8, 0, FH, FW, 0.5,
                                       out.data_ptr(), 0, None) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 77).all() and not state.cpu().numpy().any() and not mstate.cpu().numpy().any()      # nothing ran
    calls["update"](float("-inf"), 30)                                       # (the same call, well-formed, does; -inf: every row is strong)
    assert out.cpu().numpy()[0, :4].tolist() == [4, 4, 4, 0]
