"""ops.track_update_interval (csrc/track_interval.hip) against the numpy restatement of the interval rule in tests/track_interval_ref.py,
byte for byte: every frame's tracked buffer, the state, the motion state's header and the kept frame."""
import numpy as np
import pytest

from tests import track_interval_ref as I
from tests import track_ref as T
from tests.test_track_motion_gpu import TABLE, frames_for, pack as pack_rows

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

H, W = 48, 64
ROWS = 8
PARAMS = (30, 3, 2)
# a 40x30 box (strides 2 and 1), three that cross the frame's borders, a 3x3 one (9 samples < 16: tracked, never searched), a 4x4 one
# (16 samples), reversed corners, one wholly outside (never eligible)
BOXES = [[3, 4, 42, 33], [-5, -6, 20, 18], [W - 20, H - 18, W + 9, H + 7], [30, 30, 32, 32], [44, 20, 47, 23], [W - 9, 10, W + 3, 30],
         [50, 40, 30, 36], [W + 5, H + 5, W + 30, H + 30]]
CLS = [1, 2, 4, 1, 2, 4, 1, 2]


def pack(boxes, cls):
    return pack_rows(boxes, cls, ROWS)


EVERYTHING, SOME, NONE = pack(BOXES, CLS), pack(BOXES[1::2], CLS[1::2]), pack([], [])


def upload(frames, stride):
    host = np.full(len(frames) * stride, 0xEE, dtype=np.uint8)
    for i, f in enumerate(frames):
        host[i * stride:i * stride + 3 * H * W] = f.reshape(-1)
    return host


class Device:
    """The device side of one tracker: the state, the motion state, and a call that checks everything against the restatement."""

    def __init__(self, capacity):
        from faster_rcnn_amd import ops
        self.ops, self.cap = ops, capacity
        self.state, self.mstate = ops.track_state(capacity), ops.track_motion_state(H, W)
        self.table = torch.from_numpy(TABLE).cuda()
        self.ref = I.IntervalTracker(capacity)

    def call(self, frames, packed, nf, radius, interval, params=PARAMS, pad=0):
        F, stride = len(frames), 3 * H * W + pad
        host = upload(frames, stride)
        dev_frames = torch.from_numpy(host).cuda()
        dev = torch.from_numpy(np.stack(packed)).cuda()
        n_frames = torch.tensor([nf], dtype=torch.int32, device="cuda")
        out = torch.full((F, 4 + 8 * (ROWS + self.cap)), 77, dtype=torch.int32, device="cuda")
        self.ops.track_update_interval(self.state, self.mstate, dev_frames, stride, dev if len(packed) > 1 else dev[0], n_frames, self.table, H, W,
                                       *params, radius, interval, out=out)
        got = out.cpu().numpy()
        want = self.ref.update_interval(frames, packed, nf, TABLE, H, W, *params, radius, interval)
        for i in range(F):
            bad = np.flatnonzero(got[i] != want[i])
            assert bad.size == 0, (i, bad[:8].tolist(), got[i][bad[:8]].tolist(), want[i][bad[:8]].tolist())
        assert np.array_equal(self.state.cpu().numpy(), self.ref.t.words())
        assert np.array_equal(self.mstate.cpu().numpy(), self.ref.motion_bytes(H, W))
        assert np.array_equal(dev_frames.cpu().numpy(), host)                # the frames are read only
        return got


def keys_for(frames, interval, first=SOME):
    """The key frames' detections of a call: ``first``, then nothing, then everything, ..."""
    return [(first, NONE, EVERYTHING, SOME)[k % 4] for k in range(I.keys_of(frames, interval))]


@pytest.mark.parametrize("capacity", [4, 64])
@pytest.mark.parametrize("interval", [1, 2, 3, 4])
@pytest.mark.parametrize("frames", [1, 2, 5, 8])
def test_the_grid_against_the_restatement(frames, interval, capacity):
    """Every *n_frames and radius of the grid, each on a tracker of its own that one plain frame has filled: the call's frame 0 has the
    kept frame for its reference, its first key frame loses half of the tracks (held slots on the between frames) and a later one brings
    them back (capacity 4: a full table, births that overflow)."""
    held_between = overflowed = moved = 0
    for radius in (1, 8, 16):
        seq, _ = frames_for(H, W, 1 + frames, 100 * frames + 10 * interval + radius, step=None if radius > 1 else (1, -1))
        for nf in sorted({0, 1, interval, interval + 1, frames}):
            d = Device(capacity)
            d.call(seq[:1], [EVERYTHING], 1, radius, 1)
            before = (d.state.clone(), d.mstate.clone())
            got = d.call(seq[1:], keys_for(frames, interval), nf, radius, interval, pad=5 if nf & 1 else 0)
            real = min(nf, frames)
            assert d.ref.t.frames == 1 + real
            if real == 0:                                                    # nothing but the padding frames' buffers is written
                assert torch.equal(d.state, before[0]) and torch.equal(d.mstate, before[1])
            for f in range(real):
                n_rows, n_live = int(got[f][0]), int(got[f][1])
                held_between += f % interval != 0 and n_rows > n_live
            overflowed += d.ref.t.events["overflow"]
            moved += len(d.ref.moves)
    assert moved
    if frames > 1 and interval > 1:
        assert held_between
    if capacity == 4:
        assert overflowed


def test_interval_1_is_track_update_motion():
    from faster_rcnn_amd import ops
    seq, _ = frames_for(H, W, 9, 4)
    table = torch.from_numpy(TABLE).cuda()
    a, b = ops.track_state(4), ops.track_state(4)
    ma, mb = ops.track_motion_state(H, W), ops.track_motion_state(H, W)
    at = 0
    for F, nf in ((1, 1), (4, 4), (3, 2), (1, 0)):
        frames = torch.from_numpy(np.stack(seq[at:at + F])).cuda()
        packed = torch.from_numpy(np.stack([(EVERYTHING, NONE, SOME)[(at + k) % 3] for k in range(F)])).cuda()
        n = torch.tensor([nf], dtype=torch.int32, device="cuda")
        got = ops.track_update_interval(a, ma, frames, 3 * H * W, packed, n, table, H, W, *PARAMS, 8, 1)
        want = ops.track_update_motion(b, mb, frames.view(-1), 3 * H * W, packed, n, table, H, W, *PARAMS, 8)
        assert torch.equal(got, want) and torch.equal(a, b) and torch.equal(ma, mb), at
        at += F
    assert int(a[3]) == 7 and int(a[0]) > 0


def test_two_calls_in_a_row_carry_the_kept_frame():
    """The second call's frame 0 is a key frame whose reference is the first call's last frame, a BETWEEN frame: the held box has followed
    the pixels through both calls."""
    seq, _ = frames_for(H, W, 8, 31, step=(2, 1))
    box = BOXES[0]
    d = Device(4)
    d.call(seq[:4], [pack([box], [1])], 4, 8, 4, params=(30, 8, 0))
    assert d.ref.moves == [(1, 2, 1)] * 3 and d.ref.header().tolist() == [4, H, W, 0]
    got = d.call(seq[4:], [NONE, NONE], 4, 8, 2, params=(30, 8, 0))
    assert d.ref.moves == [(1, 2, 1)] * 7
    n_rows, n_live, _, _, bbox, _, _, ids, age = T.split(got[3])
    assert (n_rows, n_live, ids[0], age[0]) == (1, 0, 1, 2)                  # two key frames without a match: hold counts key frames
    xa, xb, ya, yb = T.clip([box[0] + 14, box[1] + 7, box[2] + 14, box[3] + 7], H, W)
    assert bbox[0].tolist() == [xa, ya, xb, yb]


def test_captured_and_replayed_twice_gives_the_eager_bytes():
    from faster_rcnn_amd import ops
    cap, F, K, radius = 4, 5, 2, 8
    B = I.keys_of(F, K)
    seq, _ = frames_for(H, W, 2 * F, 21)
    keys = [EVERYTHING, SOME, NONE, NONE, EVERYTHING, SOME]
    table = torch.from_numpy(TABLE).cuda()
    state, mstate = ops.track_state(cap), ops.track_motion_state(H, W)
    stride = 3 * H * W + 3
    dev_frames = torch.zeros(F * stride, dtype=torch.uint8, device="cuda")
    dev = torch.zeros((B, 4 + 7 * ROWS), dtype=torch.int32, device="cuda")
    nf = torch.zeros(1, dtype=torch.int32, device="cuda")                    # 0 frames: warm-up and capture leave every state alone
    out = torch.zeros((F, 4 + 8 * (ROWS + cap)), dtype=torch.int32, device="cuda")
    run = lambda: ops.track_update_interval(state, mstate, dev_frames, stride, dev, nf, table, H, W, *PARAMS, radius, K, out=out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    assert not state.cpu().numpy().any() and not mstate.cpu().numpy().any()
    eager = Device(cap)
    for k, real in enumerate((5, 3)):                                        # two replays: a full and a short call
        part_f, part_p = seq[k * F:k * F + F], keys[k * B:k * B + B]
        dev_frames.copy_(torch.from_numpy(upload(part_f, stride)).cuda())
        dev.copy_(torch.from_numpy(np.stack(part_p)).cuda())
        nf.fill_(real)
        graph.replay()
        want = eager.call(part_f, part_p, real, radius, K, pad=3)            # (the eager call, itself held against the restatement)
        assert np.array_equal(out.cpu().numpy(), want), k
        assert torch.equal(state, eager.state) and torch.equal(mstate, eager.mstate), k
    assert eager.ref.moves and eager.ref.t.frames == 8


def test_bad_arguments_raise_and_write_nothing():
    from faster_rcnn_amd import _lib, ops
    cap = 4
    table = torch.from_numpy(TABLE).cuda()
    state, mstate = ops.track_state(cap), ops.track_motion_state(H, W)
    frame = torch.from_numpy(frames_for(H, W, 1, 1)[0][0]).cuda().view(-1)
    four = torch.cat([frame] * 4)
    dev = torch.from_numpy(pack([[0, 0, 20, 20]], [1])).cuda()
    dev2 = torch.stack([dev, dev])
    nf = torch.ones(1, dtype=torch.int32, device="cuda")
    R = ROWS + cap
    out = torch.full((4, 4 + 8 * R), 77, dtype=torch.int32, device="cuda")
    for interval in (0, 17, -1):
        with pytest.raises(_lib.FrcnnError):
            ops.track_update_interval(state, mstate, four, 3 * H * W, dev, nf, table, H, W, *PARAMS, 8, interval, out=out[:1])
    with pytest.raises(_lib.FrcnnError):                                     # four frames every two: two key frames, one buffer
        ops.track_update_interval(state, mstate, four, 3 * H * W, dev, nf, table, H, W, *PARAMS, 8, 2, out=out)
    for kw in (dict(radius=0), dict(radius=17), dict(thr=0), dict(hold=256), dict(grow=65)):
        with pytest.raises(_lib.FrcnnError):
            ops.track_update_interval(state, mstate, four, 3 * H * W, dev2, nf, table, H, W, **dict(dict(interval=2, out=out), **kw))
    lib = _lib.load()
    ptrs = [state.data_ptr(), mstate.data_ptr(), four.data_ptr(), dev2.data_ptr(), nf.data_ptr(), table.data_ptr(), out.data_ptr()]

    def raw(p=ptrs, capacity=cap, frame_stride=3 * H * W, det_stride=4 + 7 * ROWS, frames=4, max_rows=ROWS, classes=5, radius=8, interval=2,
            hh=H, ww=W, out_stride=4 + 8 * R):
        return lib.frcnn_track_update_interval(p[0], capacity, p[1], p[2], frame_stride, p[3], det_stride, frames, p[4], max_rows, p[5], classes,
                                               30, 8, 0, radius, interval, hh, ww, p[6], out_stride, None)

    for null in range(7):                                                   # FRCNN_E_ARG (-1) for each null pointer
        p = list(ptrs)
        p[null] = None
        assert raw(p) == -1 and b"null pointer" in lib.frcnn_last_error()
    for kw in (dict(interval=0), dict(interval=17), dict(interval=-2), dict(det_stride=3 + 7 * ROWS), dict(det_stride=0),
               dict(frames=3, interval=2, det_stride=0), dict(frame_stride=3 * H * W - 1), dict(out_stride=3 + 8 * R), dict(frames=0),
               dict(frames=65), dict(capacity=0), dict(capacity=129), dict(max_rows=0), dict(max_rows=512 - cap + 1), dict(classes=0),
               dict(classes=257), dict(hh=0), dict(ww=32769), dict(radius=0), dict(radius=17)):
        assert raw(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 77).all() and not state.cpu().numpy().any() and not mstate.cpu().numpy().any()
    # one key frame: the packed buffers' distance is not read, whatever the frames
    assert raw(interval=4, det_stride=0) == 0 and raw(frames=1, interval=1, det_stride=0, frame_stride=0, out_stride=0) == 0
    assert lib.frcnn_track_interval_version() == _lib.TRACK_INTERVAL_VERSION == 1
    torch.cuda.synchronize()
    assert int(state[3]) == 2 and out.cpu().numpy()[0, :4].tolist() == [1, 1, 2, 0]
