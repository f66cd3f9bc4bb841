"""ops.track_update (csrc/track.hip) against the plain-Python restatement of the tracking rule in tests/track_ref.py: every word of every
tracked buffer and of the state; and ops.annotate_u8(ids=) against the label helper, byte for byte."""
import numpy as np
import pytest

from tests import track_ref as T

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

H, W = 120, 160
TABLE = np.array([0, 1, 1, 0, 1], dtype=np.uint8)         # classes 0 and 3 are not tracked


def pack(bbox, cls, n, rows, prob=None, dead_box=(-1, -1, -1, -1), dead_cls=-1):
    """The post-process's packed buffer with ``n`` in its count word and len(cls) filled rows; ``dead_*`` behind them."""
    packed = np.zeros(4 + 7 * rows, dtype=np.int32)
    packed[0] = n
    b = packed[4:4 + 4 * rows].reshape(rows, 4)
    b[:] = dead_box
    packed[4 + 4 * rows:4 + 5 * rows] = dead_cls
    k = min(len(cls), rows)
    b[:k] = np.asarray(bbox, dtype=np.int64).reshape(-1, 4)[:k]
    packed[4 + 4 * rows:4 + 4 * rows + k] = np.asarray(cls)[:k]
    p = np.linspace(0.99, 0.2, max(k, 1)).astype(np.float32)[:k] if prob is None else np.asarray(prob, dtype=np.float32)[:k]
    packed[4 + 5 * rows:4 + 5 * rows + k] = p.view(np.int32)
    return packed


def sequence(seed, frames, rows, objects):
    """A seeded sequence: ``objects`` boxes drift; each vanishes for a while now and then (held, then freed when the gap is long) and new
    ones appear; some frames repeat a box (ties) or carry rows of untracked classes, reversed corners and boxes outside the frame."""
    rs = np.random.RandomState(seed)
    pos = rs.randint(0, [W - 30, H - 30], (objects, 2))
    size = rs.randint(8, 40, (objects, 2))
    cls = rs.choice([1, 2, 4], objects)
    gone = np.zeros(objects, dtype=int)
    out = []
    for f in range(frames):
        pos += rs.randint(-3, 4, pos.shape)
        for o in range(objects):
            if gone[o] == 0 and rs.rand() < 0.15:
                gone[o] = rs.randint(1, 6)
            elif gone[o]:
                gone[o] -= 1
        if f == frames // 2:                                      # a new crowd: births (and overflow in a small table)
            pos[: objects // 2] = rs.randint(0, [W - 30, H - 30], (objects // 2, 2))
        b, c = [], []
        for o in rs.permutation(objects):
            if gone[o]:
                continue
            box = [pos[o, 0], pos[o, 1], pos[o, 0] + size[o, 0], pos[o, 1] + size[o, 1]]
            if rs.rand() < 0.2:
                box = [box[2], box[3], box[0], box[1]]               # reversed corners
            b.append(box)
            c.append(cls[o])
            if rs.rand() < 0.15:                                     # the same box twice: a tie
                b.append(list(box))
                c.append(cls[o])
        b += [[-40, 5, -3, 30], [W, H, W + 20, H + 20], [W - 5, H - 5, W + 30, H + 30], [10, 10, 50, 50], [20, 20, 60, 60]]
        c += [1, 2, 4, 0, 9]                                         # outside, outside, across the corner, untracked, out of range
        out.append(pack(b[:rows], c[:rows], min(len(c), rows), rows))
    return out


def run_chunks(frames, chunks, capacity, h, w, params, short=None):
    """The frames through ops.track_update in calls of ``chunks`` frames (cycled), the state carried over, each call and the state
    after it against the restatement.  ``short``: every call gets this many padding frames behind its real ones.  -> the Tracker."""
    from faster_rcnn_amd import ops
    rows = (frames[0].size - 4) // 7
    ref = T.Tracker(capacity)
    state = ops.track_state(capacity)
    assert state.numel() == 4 + 8 * capacity and not state.cpu().numpy().any()
    table = torch.from_numpy(TABLE).cuda()
    at, k = 0, 0
    while at < len(frames):
        real = frames[at:at + chunks[k % len(chunks)]]
        part = real + ([frames[0]] * short if short else [])
        dev = torch.from_numpy(np.stack(part)).cuda()
        nf = torch.tensor([len(real)], dtype=torch.int32, device="cuda")
        out = ops.track_update(state, dev if len(part) > 1 else dev[0], nf, table, h, w, *params)
        got = out.cpu().numpy()
        assert got.shape == (len(part), 4 + 8 * (rows + capacity))
        for i, p in enumerate(part):
            want = ref.update_packed(p, TABLE, h, w, *params) if i < len(real) else ref.padding(rows)
            bad = np.flatnonzero(got[i] != want)
            assert bad.size == 0, (at + i, bad[:8].tolist(), got[i][bad[:8]].tolist(), want[bad[:8]].tolist())
        assert np.array_equal(state.cpu().numpy(), ref.words()), at
        at += len(real)
        k += 1
    return ref


@pytest.mark.parametrize("capacity", [4, 64])
@pytest.mark.parametrize("rows", [8, 300])
def test_sequences_in_calls_of_1_3_and_8_frames(capacity, rows):
    params = (30, 2, 3)
    frames = sequence(7 * capacity + rows, 24, rows, 6 if rows == 8 else 24)
    # the restatement's own run first: the sequence exercises the rule
    ref = T.Tracker(capacity)
    for p in frames:
        ref.update_packed(p, TABLE, H, W, *params)
    ev = ref.events
    assert ev["match"] and ev["hold"] and ev["free"] and ev["birth"], ev
    assert (ev["overflow"] > 0) == (capacity == 4), ev
    a = run_chunks(frames, [1, 3, 8], capacity, H, W, params)
    b = run_chunks(frames, [1], capacity, H, W, params)
    c = run_chunks(frames, [8, 3], capacity, H, W, params, short=2)      # n_frames < B: the padding is ignored
    assert np.array_equal(a.words(), b.words()) and np.array_equal(a.words(), c.words()) and a.words()[3] == len(frames)
    assert a.events == ev


def test_counts_ties_and_odd_boxes():
    from faster_rcnn_amd import ops
    rows = 8
    huge = (-(1 << 30), -(1 << 30), 1 << 30, 1 << 30)
    dup = [[10, 10, 29, 29], [10, 10, 29, 29], [12, 10, 31, 29], [8, 10, 27, 29]]
    frames = [
        pack(dup, [1, 1, 1, 1], 4, rows),                                   # duplicates: births in row order
        pack(dup[::-1], [1, 1, 1, 1], 4, rows),                             # ... matched again, ties to the lowest row
        pack([], [], 0, rows, dead_box=huge, dead_cls=1),                   # *n_dets = 0: nothing behind it is read, everything is held
        pack([[10, 10, 29, 29]] * rows, [1] * rows, rows + 5, rows),        # *n_dets > max_rows
        pack([], [], -3, rows, dead_box=huge, dead_cls=1),                  # ... negative
        pack([[29, 29, 10, 10], [-5, -5, 3, 3], [W, 0, W + 9, 9], [0, -9, 9, -1], [W - 1, H - 1, W + 50, H + 50]], [1, 2, 1, 2, 4], 5, rows),
        pack([[10, 10, 29, 29], [3, 3, -5, -5], [W - 1, H - 1, W - 1, H - 1]], [1, 2, 4], 3, rows),
    ]
    for chunks in ([1], [len(frames)], [2, 3]):
        ref = run_chunks(frames, chunks, 6, H, W, (40, 3, 1))
    assert ref.events["overflow"] and ref.events["hold"] and ref.events["match"]
    # the threshold edge on the device: 10x10 against 10x5 sharing 50 pixels
    for thr, same in ((50, True), (51, False)):
        ref = run_chunks([pack([[0, 0, 9, 9]], [1], 1, rows), pack([[0, 0, 9, 4]], [1], 1, rows)], [2], 4, H, W, (thr, 0, 0))
        assert (ref.next_id == 2) == same
    # hold = 0 and the extremes of the parameters
    run_chunks(frames, [3], 6, H, W, (1, 0, 64))
    run_chunks(frames, [3], 6, H, W, (100, 255, 64))
    run_chunks(frames, [7], 128, H, W, (30, 8, 0))
    assert ops.TRACK_MAX == T.MAX == 128


@pytest.mark.parametrize("capacity", [64, 128])
def test_a_full_frame_of_300_rows(capacity):
    """Every row of a 300-row buffer live: a grid of small boxes, then the grid moved by a pixel, then half of it."""
    rows = 300
    grid = np.array([[8 * (k % 20), 8 * (k // 20), 8 * (k % 20) + 5, 8 * (k // 20) + 5] for k in range(rows)])
    cls = np.array([(1, 2, 4, 3)[k % 4] for k in range(rows)])
    frames = [pack(grid, cls, rows, rows), pack(grid[::-1] + 1, cls[::-1], rows, rows), pack(grid[::2], cls[::2], rows // 2, rows)]
    ref = run_chunks(frames, [3], capacity, H, W, (30, 1, 1))
    assert ref.events["match"] >= capacity and ref.events["overflow"] and len(ref.slots) == capacity


def test_int64_products():
    """Two 30000-pixel-side boxes in a 32768 frame: inter * union passes 2^59."""
    rows = 8
    a, b = [0, 0, 29999, 29999], [2000, 2000, 31999, 31999]
    small = [0, 0, 29999, 14999]                                            # a second track; its IoU with b is 36.9 %
    for thr, ids in ((77, 2), (78, 3)):
        ref = run_chunks([pack([a, small], [1, 1], 2, rows), pack([b], [1], 1, rows)], [2], 4, 32768, 32768, (thr, 1, 0))
        assert ref.next_id - 1 == ids
    frames = [pack([a, b], [1, 1], 2, rows), pack([b, a], [1, 1], 2, rows), pack([[1, 1, 30000, 30000]], [1], 1, rows)]
    ref = run_chunks(frames, [3], 4, 32768, 32768, (30, 1, 64))
    assert ref.events["match"] == 3


def test_captured_and_replayed_with_other_detections():
    from faster_rcnn_amd import ops
    rows, cap, B, params = 8, 6, 3, (30, 2, 2)
    frames = sequence(5, 4 * B, rows, 5)
    table = torch.from_numpy(TABLE).cuda()
    state = ops.track_state(cap)
    dev = torch.zeros((B, 4 + 7 * rows), dtype=torch.int32, device="cuda")
    nf = torch.zeros(1, dtype=torch.int32, device="cuda")                    # 0 frames: warm-up and capture leave the state alone
    out = torch.zeros((B, 4 + 8 * (rows + cap)), dtype=torch.int32, device="cuda")
    run = lambda: ops.track_update(state, dev, nf, table, H, W, *params, out=out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    assert not state.cpu().numpy().any()
    ref = T.Tracker(cap)
    for k, real in enumerate((3, 2, 3, 1)):                                  # full and short passes
        part = frames[k * B:k * B + B]
        dev.copy_(torch.from_numpy(np.stack(part)).cuda())
        nf.fill_(real)
        graph.replay()
        got = out.cpu().numpy()
        for i, p in enumerate(part):
            want = ref.update_packed(p, TABLE, H, W, *params) if i < real else ref.padding(rows)
            assert np.array_equal(got[i], want), (k, i)
        assert np.array_equal(state.cpu().numpy(), ref.words()), k
    assert ref.frames == 9 and ref.events["match"] and ref.events["birth"]
    # two runs from one state: the same bytes
    snap = state.clone()
    graph.replay()
    first, after = out.clone(), state.clone()
    state.copy_(snap)
    graph.replay()
    assert torch.equal(out, first) and torch.equal(state, after)
    ops.track_reset(state)
    assert not state.cpu().numpy().any()


def test_a_list_of_buffers_is_taken_where_it_lies_or_gathered():
    from faster_rcnn_amd import ops
    rows, cap, params = 8, 4, (30, 1, 0)
    frames = sequence(11, 4, rows, 4)
    table = torch.from_numpy(TABLE).cuda()
    nf = torch.tensor([4], dtype=torch.int32, device="cuda")
    ref = T.Tracker(cap)
    want = np.stack([ref.update_packed(p, TABLE, H, W, *params) for p in frames])
    words = frames[0].size
    area = torch.zeros(4 * (words + 12), dtype=torch.int32, device="cuda")
    even = [area[i * (words + 12):i * (words + 12) + words] for i in range(4)]          # evenly spaced views
    scattered = [torch.empty(words + 64 * (i % 2), dtype=torch.int32, device="cuda")[:words] for i in (0, 1, 3, 2)]
    for bufs in (even, scattered):
        for b, p in zip(bufs, frames):
            b.copy_(torch.from_numpy(p).cuda())
        state = ops.track_state(cap)
        assert np.array_equal(ops.track_update(state, bufs, nf, table, H, W, *params).cpu().numpy(), want)
        assert np.array_equal(state.cpu().numpy(), ref.words())


def test_bad_arguments_raise_and_write_nothing():
    from faster_rcnn_amd import _lib, ops
    rows, cap = 8, 4
    table = torch.from_numpy(TABLE).cuda()
    state = ops.track_state(cap)
    dev = torch.from_numpy(pack([[0, 0, 9, 9]], [1], 1, rows)).cuda()
    nf = torch.ones(1, dtype=torch.int32, device="cuda")
    out = torch.full((1, 4 + 8 * (rows + cap)), 77, dtype=torch.int32, device="cuda")
    for params in ((0, 8, 0), (101, 8, 0), (30, -1, 0), (30, 256, 0), (30, 8, -1), (30, 8, 65)):
        with pytest.raises(_lib.FrcnnError):
            ops.track_update(state, dev, nf, table, H, W, *params, out=out)
    for h, w in ((0, W), (H, 0), (32769, W), (H, 32769)):
        with pytest.raises(_lib.FrcnnError):
            ops.track_update(state, dev, nf, table, h, w, out=out)
    with pytest.raises(_lib.FrcnnError):                                    # R = 449 + 64 > 512
        ops.track_update(ops.track_state(64), torch.zeros(4 + 7 * 449, dtype=torch.int32, device="cuda"), nf, table, H, W)
    with pytest.raises(_lib.FrcnnError):                                    # more frames than a call takes
        ops.track_update(state, torch.zeros((65, 4 + 7 * rows), dtype=torch.int32, device="cuda"), nf, table, H, W)
    with pytest.raises(_lib.FrcnnError):
        ops.track_update(state, dev, nf, torch.zeros(257, dtype=torch.uint8, device="cuda"), H, W, out=out)
    for capacity in (0, 129, -1):
        with pytest.raises(_lib.FrcnnError):
            ops.track_state(capacity)
    lib = _lib.load()
    assert lib.frcnn_track_state_bytes(64) == 4 * (4 + 8 * 64) and lib.frcnn_track_state_bytes(0) == 0
    for null in range(5):                                                   # FRCNN_E_ARG (-1) for each null pointer
        ptrs = [state.data_ptr(), dev.data_ptr(), nf.data_ptr(), table.data_ptr(), out.data_ptr()]
        ptrs[null] = None
        assert lib.frcnn_track_update(ptrs[0], cap, ptrs[1], 0, 1, ptrs[2], rows, ptrs[3], 5, 30, 8, 0, H, W, ptrs[4], 0, None) == -1
        assert b"null pointer" in lib.frcnn_last_error()
    with pytest.raises(AssertionError):
        ops.track_update(state, dev, nf, table, H, W, out=out[:, :-1])
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 77).all() and not state.cpu().numpy().any()      # nothing ran
    ops.track_update(state, dev, nf, table, H, W, out=out)                     # (the same call, well-formed, does)
    assert out.cpu().numpy()[0, :4].tolist() == [1, 1, 2, 0] and state.cpu().numpy()[:4].tolist() == [1, 1, 0, 1]


def test_track_table():
    from faster_rcnn_amd import ops
    names = ["bg", "car", "", "person"]
    assert ops.track_table(names, "all").cpu().tolist() == [0, 1, 0, 1]
    assert ops.track_table(names, ("person",)).cpu().tolist() == [0, 0, 0, 1]
    with pytest.raises(ValueError):
        ops.track_table(names, ["dog"])


# ----------------------------------------------------------------------------------------------------------- labels with ids
def test_annotate_ids_against_the_label_helper():
    from faster_rcnn_amd import ops
    names = ["bg", "car", "person", "Misc"]
    h, w = 90, 330
    src = np.random.RandomState(3).randint(0, 256, (h, w, 3)).astype(np.uint8)
    boxes = [[5, 5, 60, 20], [70, 10, 120, 30], [10, 45, 80, 60], [130, 5, 200, 20], [140, 50, 180, 65]]
    cls = [1, 2, 1, 3, 2]
    prob = [0.97, 0.5, 0.123, 0.9, 1.0]
    ids = [7, 0, 2147483647, 5, 1234567890]                                 # an id of 0, a skipped class, ten digits twice
    rows = 8
    packed = pack(boxes, cls, 5, rows, prob=prob)
    dets = [{"bbox": np.array(b), "cls_name": names[c], "prob": np.float32(p), "track_id": i} for b, c, p, i in zip(boxes, cls, prob, ids)]
    tables = ops.annotate_tables(names)
    dev_packed = torch.from_numpy(packed).cuda()
    ids_dev = torch.tensor(ids + [9] * (rows - 5), dtype=torch.int32, device="cuda")
    plain = ops.annotate_u8(torch.from_numpy(src).cuda(), dev_packed, tables).cpu().numpy()
    none = ops.annotate_u8(torch.from_numpy(src).cuda(), dev_packed, tables, ids=None).cpu().numpy()
    got = ops.annotate_u8(torch.from_numpy(src).cuda(), dev_packed, tables, ids=ids_dev).cpu().numpy()
    from tests import annotate_ref
    assert np.array_equal(plain, none) and np.array_equal(plain, annotate_ref.annotate(src, dets))
    want = T.annotate(src, dets)
    assert np.array_equal(got, want) and not np.array_equal(got, plain)
    zero = ops.annotate_u8(torch.from_numpy(src).cuda(), dev_packed, tables, ids=torch.zeros(rows, dtype=torch.int32, device="cuda")).cpu().numpy()
    assert np.array_equal(zero, plain)
    # a tracked buffer in a det_packed's place: the live rows with their ids, the held row not drawn, and redacted
    ref = T.Tracker(4)
    table = np.array([0, 1, 1, 1], dtype=np.uint8)
    ref.update_packed(pack([[200, 40, 260, 70]], [2], 1, rows, prob=[0.8]), table, h, w, 30, 2, 3)
    state = torch.from_numpy(ref.words()).cuda()
    buf = ops.track_update(state, dev_packed, torch.ones(1, dtype=torch.int32, device="cuda"), torch.from_numpy(table).cuda(), h, w, 30, 2, 3)[0]
    want_buf = ref.update_packed(packed, table, h, w, 30, 2, 3)
    assert np.array_equal(buf.cpu().numpy(), want_buf) and want_buf[0] == 6 and want_buf[1] == 5
    live = [dict(d, track_id=int(i)) for d, i in zip(dets, T.split(want_buf)[7])]
    got = ops.annotate_u8(torch.from_numpy(src).cuda(), buf, tables, tracked=True).cpu().numpy()
    assert np.array_equal(got, T.annotate(src, live))
    from tests import redact_ref as R
    n_rows, _, _, _, t_box, t_cls, _, _, _ = T.split(want_buf)
    red = ops.redact_u8(torch.from_numpy(src).cuda(), buf, torch.from_numpy(table).cuda(), "fill", tracked=True).cpu().numpy()
    assert np.array_equal(red, R.redact(src, t_box, t_cls, n_rows, table, "fill"))
    assert not red[40 - 3:70 + 4, 200 - 3:260 + 4].any() and src[37:74, 197:264].any()      # the held box, grown by 3, is hidden
