"""ops.track_update_motion (csrc/track_motion.hip) against the numpy restatement of the motion rule in tests/track_motion_ref.py, byte for
byte: every tracked buffer, the state, the motion state's header and the kept frame."""
import numpy as np
import pytest

from tests import track_motion_ref as M
from tests import track_ref as T

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TABLE = np.array([0, 1, 1, 0, 1], dtype=np.uint8)
ROWS = 24
PARAMS = (30, 3, 2)
SIZES = [(48, 64), (97, 131)]            # 9216-byte frames (16-byte aligned: the keep step's wide copies) and 38121-byte ones (odd)


def pack(boxes, cls, rows=ROWS):
    p = np.zeros(4 + 7 * rows, dtype=np.int32)
    p[0] = len(cls)
    p[4:4 + 4 * rows] = -1
    p[4 + 4 * rows:4 + 5 * rows] = -1
    for r, (b, c) in enumerate(zip(boxes, cls)):
        p[4 + 4 * r:8 + 4 * r] = b
        p[4 + 4 * rows + r] = c
        p[4 + 5 * rows + r] = T.bits(0.95 - 0.01 * r)
    return p


def boxes_for(h, w):
    """Raw boxes: 70x40 where it fits (strides 3 and 2), boxes that touch and cross every border, one wholly outside (never eligible), a
    3x3 one (n = 9 < 16: tracked, never searched), 4x4 (n = 16), 33 wide (stride 2), reversed corners."""
    big = [8, 5, 77, 44] if w >= 90 else [3, 4, 42, 33]
    return [big, [-5, -6, 20, 18], [w - 20, h - 18, w + 9, h + 7], [w // 2 - 10, -9, w // 2 + 12, 14], [-10, h // 2, 12, h // 2 + 20],
            [w - 9, 10, w - 1, 30], [10, h - 7, 40, h - 1], [w + 5, h + 5, w + 30, h + 30], [30, 30, 32, 32], [40, 20, 43, 23],
            [w // 2 + 16, h // 2 + 8, w // 2 - 16, h // 2 - 9], [0, 0, w - 1, h - 1]]


CLS = [1, 2, 4, 1, 2, 4, 1, 2, 4, 1, 2, 4]


def frames_for(h, w, n, seed, step=None):
    """``n`` frames: noise, each moved against the last by a small seeded shift (``step``: by that shift)."""
    rs = np.random.RandomState(seed)
    out = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8)]
    shifts = []
    for _ in range(n - 1):
        d = step or (int(rs.randint(-3, 4)), int(rs.randint(-3, 4)))
        shifts.append(d)
        out.append(np.ascontiguousarray(M.shifted(out[-1], *d)))
    return out, shifts


class Device:
    """The device side of one tracker: the state, the motion state, and a call that checks everything against the restatement."""

    def __init__(self, capacity, h, w):
        from faster_rcnn_amd import ops
        self.ops, self.h, self.w, self.cap = ops, h, w, capacity
        self.state = ops.track_state(capacity)
        self.mstate = ops.track_motion_state(h, w)
        assert self.mstate.numel() == 16 + 3 * h * w and not self.mstate.cpu().numpy().any()
        self.table = torch.from_numpy(TABLE).cuda()
        self.ref = M.MotionTracker(capacity)

    def call(self, frames, packed, nf, radius, params=PARAMS, pad=0):
        """One call of len(frames) frames, the frames ``pad`` bytes apart beyond their size; -> the device's tracked buffers."""
        h, w, B = self.h, self.w, len(frames)
        stride = 3 * h * w + pad
        host = np.full(B * stride, 0xEE, dtype=np.uint8)
        for i, f in enumerate(frames):
            host[i * stride:i * stride + 3 * h * w] = f.reshape(-1)
        dev_frames = torch.from_numpy(host).cuda()
        dev = torch.from_numpy(np.stack(packed)).cuda()
        n_frames = torch.tensor([nf], dtype=torch.int32, device="cuda")
        out = self.ops.track_update_motion(self.state, self.mstate, dev_frames, stride, dev if B > 1 else dev[0], n_frames, self.table, h, w,
                                           *params, radius)
        got = out.cpu().numpy()
        want = self.ref.update_call(frames, packed, nf, TABLE, h, w, *params, radius)
        for i in range(B):
            bad = np.flatnonzero(got[i] != want[i])
            assert bad.size == 0, (i, bad[:8].tolist(), got[i][bad[:8]].tolist(), want[i][bad[:8]].tolist())
        assert np.array_equal(self.state.cpu().numpy(), self.ref.t.words())
        m = self.mstate.cpu().numpy()
        assert m[:16].view(np.int32).tolist() == self.ref.header().tolist()
        if self.ref.frame is not None:
            assert np.array_equal(m[16:], self.ref.frame.reshape(-1))
        assert np.array_equal(dev_frames.cpu().numpy(), host)                # the frames are read only
        return got


@pytest.mark.parametrize("size,capacity,radius", [(0, 1, 8), (0, 3, 1), (0, 128, 16), (1, 1, 16), (1, 3, 8), (1, 128, 1), (1, 128, 8)])
def test_calls_of_1_and_4_frames_against_the_restatement(size, capacity, radius):
    h, w = SIZES[size]
    frames, _ = frames_for(h, w, 12, 10 * capacity + radius)
    boxes = boxes_for(h, w)
    rows = ROWS
    if capacity == 128:                                                      # a crowd: more slots than one wave, most of them held
        rows = 160
        rs = np.random.RandomState(2)
        xy = rs.randint(-8, [w - 8, h - 8], (rows - 10 - len(boxes), 2))
        boxes = boxes + np.concatenate([xy, xy + rs.randint(3, 45, xy.shape)], axis=1).tolist()
    cls = (CLS * 14)[:len(boxes)]
    everything, some, none = pack(boxes, cls, rows), pack(boxes[1::2], cls[1::2], rows), pack([], [], rows)
    d = Device(capacity, h, w)
    d.call(frames[:1], [everything], 1, radius)                              # no reference yet: the plain rule
    assert d.ref.moves == [] and d.ref.header().tolist() == [1, h, w, 0]
    d.call(frames[1:5], [none, some, none, none], 4, radius, pad=5)          # the kept frame, then the call's own frames
    moved = len(d.ref.moves)
    assert moved and d.ref.t.events["hold"]
    d.call(frames[5:9], [none, everything, none, none], 2, radius)           # a short call: two frames of padding
    assert d.ref.t.frames == 7 and np.array_equal(d.ref.frame, frames[6])
    # *n_frames = 0: the tracked buffers are padding, and no byte of the state or the motion state differs
    before = (d.state.clone(), d.mstate.clone())
    got = d.call(frames[9:12], [everything] * 3, 0, radius)
    assert all(np.array_equal(g, d.ref.t.padding(rows)) for g in got)
    assert torch.equal(d.state, before[0]) and torch.equal(d.mstate, before[1])
    d.call(frames[7:8], [some], 1, radius)                                   # ... and the sequence goes on from the kept frame
    assert len(d.ref.moves) > moved
    if capacity == 1:
        assert d.ref.t.events["overflow"]
    if capacity == 128:
        assert len(d.ref.t.slots) > 64 and d.ref.t.events["overflow"]


def test_every_shift_up_to_the_radius_moves_a_held_box():
    """One call of four frames, each moved by the same shift: the held box lands where the pixels went."""
    h, w = SIZES[1]
    for step, radius in (((3, 2), 8), ((-8, 8), 8), ((16, -16), 16), ((1, 0), 1), ((-1, -1), 1)):
        frames, _ = frames_for(h, w, 4, 77, step)
        box = [40, 30, 90, 66]
        d = Device(3, h, w)
        got = d.call(frames, [pack([box], [1])] + [pack([], [])] * 3, 4, radius, params=(30, 8, 0))
        n_rows, n_live, _, _, bbox, _, _, ids, age = T.split(got[3])
        assert (n_rows, n_live, ids[0], age[0]) == (1, 0, 1, 3)
        xa, xb, ya, yb = T.clip([box[0] + 3 * step[0], box[1] + 3 * step[1], box[2] + 3 * step[0], box[3] + 3 * step[1]], h, w)
        assert bbox[0].tolist() == [xa, ya, xb, yb]                          # (a held row's box is the clipped one)
        assert d.ref.moves == [(1,) + step] * 3


def test_hand_made_states_empty_and_tiny_slots():
    """Slots no detection could have made: a raw box wholly outside the frame (empty: skipped), a 3x3 one (skipped), and one that is
    searched, in one state."""
    h, w = SIZES[0]
    frames, _ = frames_for(h, w, 2, 5, (2, -1))
    d = Device(3, h, w)
    d.call(frames[:1], [pack([], [])], 1, 8)
    d.ref.t.slots = [{"id": 1, "cls": 1, "bbox": [w + 4, h + 4, w + 40, h + 40], "prob": T.bits(0.5), "age": 0},
                     {"id": 2, "cls": 2, "bbox": [20, 20, 22, 22], "prob": T.bits(0.6), "age": 1},
                     {"id": 5, "cls": 4, "bbox": [10, 8, 50, 40], "prob": T.bits(0.7), "age": 0}]
    d.ref.t.next_id = 6
    d.state.copy_(torch.from_numpy(d.ref.t.words()).cuda())
    d.call(frames[1:], [pack([], [])], 1, 8)
    assert d.ref.moves == [(5, 2, -1)]
    assert [s["bbox"] for s in d.ref.t.slots] == [[w + 4, h + 4, w + 40, h + 40], [20, 20, 22, 22], [12, 7, 52, 39]]


def test_a_header_of_another_size_or_count_is_no_reference():
    h, w = SIZES[0]
    frames, _ = frames_for(h, w, 2, 9, (2, 1))
    box = [10, 8, 50, 40]
    for word, value in ((0, 5), (0, 0), (0, -1), (1, h + 1), (2, w - 1), (None, None)):
        d = Device(3, h, w)
        d.call(frames[:1], [pack([box], [1])], 1, 8)
        if word is not None:
            head = d.ref.header()
            head[word] = value
            d.mstate[:16].copy_(torch.from_numpy(head.view(np.uint8)).cuda())
            if word == 0:
                d.ref.kept = value
            else:
                d.ref.size = (value, w) if word == 1 else (h, value)
        d.call(frames[1:], [pack([], [])], 1, 8)
        assert d.ref.moves == ([] if word is not None else [(1, 2, 1)]), (word, value)
        assert d.ref.header().tolist() == [2, h, w, 0]
    # ops.track_motion_reset zeroes the header and nothing else
    before = d.mstate.clone()
    d.ops.track_motion_reset(d.mstate)
    assert not d.mstate[:16].cpu().numpy().any() and torch.equal(d.mstate[16:], before[16:])
    # a state advanced by the plain call in between: the counts differ
    d = Device(3, h, w)
    d.call(frames[:1], [pack([box], [1])], 1, 8)
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    d.ops.track_update(d.state, torch.from_numpy(pack([box], [1])).cuda(), one, d.table, h, w, *PARAMS)
    d.ref.t.update_packed(pack([box], [1]), TABLE, h, w, *PARAMS)
    d.call(frames[1:], [pack([], [])], 1, 8)
    assert d.ref.moves == []


@pytest.mark.parametrize("size", [0, 1])
def test_with_no_reference_and_one_frame_it_is_track_update(size):
    from faster_rcnn_amd import ops
    h, w = SIZES[size]
    frames, _ = frames_for(h, w, 6, 3)
    boxes = boxes_for(h, w)
    table = torch.from_numpy(TABLE).cuda()
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    a, b = ops.track_state(5), ops.track_state(5)
    mstate = ops.track_motion_state(h, w)
    for k, f in enumerate(frames):
        p = torch.from_numpy(pack(boxes[k % 3::2], CLS[k % 3::2]) if k % 3 != 2 else pack([], [])).cuda()
        ops.track_motion_reset(mstate)
        got = ops.track_update_motion(a, mstate, torch.from_numpy(f).cuda().view(-1), 0, p, one, table, h, w, *PARAMS, 8)
        want = ops.track_update(b, p, one, table, h, w, *PARAMS)
        assert torch.equal(got, want) and torch.equal(a, b), k
    assert int(a[3]) == 6 and int(a[0]) > 0
    assert mstate[:16].view(torch.int32).cpu().tolist() == [6, h, w, 0]


def test_captured_and_replayed_with_other_detections_and_frames():
    from faster_rcnn_amd import ops
    h, w = SIZES[1]
    cap, B, radius = 6, 3, 8
    frames, _ = frames_for(h, w, 4 * B, 21)
    boxes = boxes_for(h, w)
    packed = [pack(boxes[k % 4::3], CLS[k % 4::3]) if k % 3 == 0 else pack([], []) for k in range(4 * B)]
    table = torch.from_numpy(TABLE).cuda()
    state, mstate = ops.track_state(cap), ops.track_motion_state(h, w)
    stride = 3 * h * w + 3
    dev_frames = torch.zeros(B * stride, dtype=torch.uint8, device="cuda")
    dev = torch.zeros((B, 4 + 7 * ROWS), dtype=torch.int32, device="cuda")
    nf = torch.zeros(1, dtype=torch.int32, device="cuda")                    # 0 frames: warm-up and capture leave every state alone
    out = torch.zeros((B, 4 + 8 * (ROWS + cap)), dtype=torch.int32, device="cuda")
    run = lambda: ops.track_update_motion(state, mstate, dev_frames, stride, dev, nf, table, h, w, *PARAMS, radius, out=out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    assert not state.cpu().numpy().any() and not mstate.cpu().numpy().any()
    ref = M.MotionTracker(cap)
    for k, real in enumerate((3, 2)):                                        # two replays: a full and a short pass
        part_f, part_p = frames[k * B:k * B + B], packed[k * B:k * B + B]
        host = np.zeros(B * stride, dtype=np.uint8)
        for i, f in enumerate(part_f):
            host[i * stride:i * stride + 3 * h * w] = f.reshape(-1)
        dev_frames.copy_(torch.from_numpy(host).cuda())
        dev.copy_(torch.from_numpy(np.stack(part_p)).cuda())
        nf.fill_(real)
        graph.replay()
        want = ref.update_call(part_f, part_p, real, TABLE, h, w, *PARAMS, radius)
        got = out.cpu().numpy()
        for i in range(B):
            assert np.array_equal(got[i], want[i]), (k, i)
        assert np.array_equal(state.cpu().numpy(), ref.t.words()), k
        assert np.array_equal(mstate.cpu().numpy(), ref.motion_bytes(h, w)), k
    assert ref.moves and ref.t.frames == 5


def test_bad_arguments_raise_and_write_nothing():
    from faster_rcnn_amd import _lib, ops
    h, w = SIZES[0]
    cap = 4
    table = torch.from_numpy(TABLE).cuda()
    state = ops.track_state(cap)
    mstate = ops.track_motion_state(h, w)
    frames = torch.from_numpy(frames_for(h, w, 1, 1)[0][0]).cuda().view(-1)
    two = torch.cat([frames, frames])
    dev = torch.from_numpy(pack([[0, 0, 20, 20]], [1])).cuda()
    dev2 = torch.stack([dev, dev])
    nf = torch.ones(1, dtype=torch.int32, device="cuda")
    R = ROWS + cap
    out = torch.full((1, 4 + 8 * R), 77, dtype=torch.int32, device="cuda")
    out2 = torch.full((2, 4 + 8 * R), 77, dtype=torch.int32, device="cuda")
    call = lambda **kw: ops.track_update_motion(state, mstate, frames, 0, dev, nf, table, h, w, **dict(dict(out=out), **kw))
    for radius in (0, 17, -1):
        with pytest.raises(_lib.FrcnnError):
            call(radius=radius)
    for kw in (dict(thr=0), dict(thr=101), dict(hold=-1), dict(hold=256), dict(grow=-1), dict(grow=65)):
        with pytest.raises(_lib.FrcnnError):
            call(**kw)
    lib = _lib.load()
    ptrs = [state.data_ptr(), mstate.data_ptr(), two.data_ptr(), dev2.data_ptr(), nf.data_ptr(), table.data_ptr(), out2.data_ptr()]

    def raw(p=ptrs, capacity=cap, frame_stride=3 * h * w, det_stride=4 + 7 * ROWS, B=1, max_rows=ROWS, classes=5, radius=8, hh=h, ww=w,
            out_stride=4 + 8 * R):
        return lib.frcnn_track_update_motion(p[0], capacity, p[1], p[2], frame_stride, p[3], det_stride, B, p[4], max_rows, p[5], classes,
                                             30, 8, 0, radius, hh, ww, p[6], out_stride, None)

    for null in range(7):                                                   # FRCNN_E_ARG (-1) for each null pointer
        p = list(ptrs)
        p[null] = None
        assert raw(p) == -1 and b"null pointer" in lib.frcnn_last_error()
    for kw in (dict(B=2, frame_stride=3 * h * w - 1), dict(B=2, frame_stride=0), dict(B=2, det_stride=3 + 7 * ROWS), dict(B=2, out_stride=3 + 8 * R),
               dict(B=0), dict(B=65), dict(capacity=0), dict(capacity=129), dict(max_rows=0), dict(max_rows=512 - cap + 1), dict(classes=0),
               dict(classes=257), dict(hh=0), dict(ww=0), dict(hh=32769), dict(ww=32769), dict(radius=0), dict(radius=17)):
        assert raw(**kw) == -1, kw
    assert raw(frame_stride=0, det_stride=0, out_stride=0, B=1) == 0           # (one frame: no stride is read)
    assert lib.frcnn_track_motion_version() == _lib.TRACK_MOTION_VERSION == 1
    assert lib.frcnn_track_motion_state_bytes(h, w) == 16 + 3 * h * w and lib.frcnn_track_motion_state_bytes(0, w) == 0
    assert lib.frcnn_track_motion_state_bytes(h, 32769) == 0 and lib.frcnn_track_motion_state_bytes(32768, 32768) == 16 + 3 * 32768 * 32768
    for bad in ((0, w), (h, 32769)):
        with pytest.raises(_lib.FrcnnError):
            ops.track_motion_state(*bad)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 77).all() and (out2.cpu().numpy()[1] == 77).all()
    # everything refused wrote nothing; the one well-formed raw call above ran frame 0 into out2[0]
    assert out2.cpu().numpy()[0, :4].tolist() == [1, 1, 2, 0] and state.cpu().numpy()[:4].tolist() == [1, 1, 0, 1]
    assert mstate[:16].view(torch.int32).cpu().tolist() == [1, h, w, 0] and torch.equal(mstate[16:], frames)
