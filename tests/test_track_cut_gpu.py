"""ops.track_update_cut (csrc/track_cut.hip) against the numpy restatement of the cut rule in tests/track_cut_ref.py, byte for byte: every
frame's tracked buffer, the cuts, the state, the motion state's header and the kept frame."""
import numpy as np
import pytest

from tests import track_cut_ref as C
from tests import track_interval_ref as I
from tests import track_motion_ref as M
from tests.test_track_motion_gpu import CLS, TABLE, boxes_for, pack as pack_rows

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROWS = 16
PARAMS = (30, 3, 2)
SIZES = [(37, 53), (64, 96)]
RADIUS, PCT = 8, 40
_SCENES = {}


def scenes(h, w):
    """(six frames of scene A, six of scene B) for the size, made once: noise with every channel, and so the luma, in 0..120 against
    136..255 -- a cut is D = 2hw --, each frame the last moved one pixel right; inside a scene D stays under a quarter of the threshold."""
    if (h, w) not in _SCENES:
        both = []
        for seed, (lo, hi) in enumerate(((0, 120), (136, 255))):
            rs = np.random.RandomState(1000 * h + 10 * w + seed)
            seq = [rs.randint(lo, hi + 1, (h, w, 3)).astype(np.uint8)]
            for _ in range(5):
                seq.append(np.ascontiguousarray(M.shifted(seq[-1], 1, 0)))
            for x, y in zip(seq[:-1], seq[1:]):                              # (``film`` keeps the frames of a scene in this order)
                assert C.distance(x, y) * 100 * 4 < PCT * 2 * h * w
            both.append(seq)
        assert all(C.distance(x, y) == 2 * h * w for x in both[0] for y in both[1])
        _SCENES[(h, w)] = both
    return _SCENES[(h, w)]


def film(h, w, n, cuts, first=0):
    """``n`` <= 5 frames behind a frame of scene ``first``, which change scene at the positions ``cuts``: frame f is its scene's frame
    f + 1, so two consecutive frames of one scene are one pixel apart (a tracker's first call shows frame 0 of scene A)."""
    a_b, which, out = scenes(h, w), first, []
    for f in range(n):
        which ^= f in cuts
        out.append(a_b[which][f + 1])
    return out


def packs(h, w):
    boxes = boxes_for(h, w)
    return pack_rows(boxes, CLS, ROWS), pack_rows(boxes[1::2], CLS[1::2], ROWS), pack_rows([], [], ROWS)


def upload(frames, stride, h, w):
    host = np.full(len(frames) * stride, 0xEE, dtype=np.uint8)
    for i, f in enumerate(frames):
        host[i * stride:i * stride + 3 * h * w] = f.reshape(-1)
    return host


class Device:
    """The device side of one tracker: the state, the motion state, and a call that checks everything against the restatement."""

    def __init__(self, capacity, h, w):
        from faster_rcnn_amd import ops
        self.ops, self.cap, self.h, self.w = ops, capacity, h, w
        self.state, self.mstate = ops.track_state(capacity), ops.track_motion_state(h, w)
        self.table = torch.from_numpy(TABLE).cuda()
        self.ref = C.CutTracker(capacity)

    def call(self, frames, packed, nf, interval, pct=PCT, params=PARAMS, pad=0):
        h, w = self.h, self.w
        F, stride = len(frames), 3 * h * w + pad
        host = upload(frames, stride, h, w)
        dev_frames = torch.from_numpy(host).cuda()
        dev = torch.from_numpy(np.stack(packed)).cuda()
        n_frames = torch.tensor([nf], dtype=torch.int32, device="cuda")
        out = torch.full((F, 4 + 8 * (ROWS + self.cap)), 77, dtype=torch.int32, device="cuda")
        cuts = torch.full((F,), 77, dtype=torch.int32, device="cuda")
        res = self.ops.track_update_cut(self.state, self.mstate, dev_frames, stride, dev if len(packed) > 1 else dev[0], n_frames, self.table, h, w,
                                        *params, RADIUS, interval, pct, out=out, cuts=cuts)
        assert res[0] is out and res[1] is cuts
        got, got_cuts = out.cpu().numpy(), cuts.cpu().numpy()
        want, want_cuts = self.ref.update_cut(frames, packed, nf, TABLE, h, w, *params, RADIUS, interval, pct)
        assert got_cuts.tolist() == want_cuts.tolist()
        for i in range(F):
            bad = np.flatnonzero(got[i] != want[i])
            assert bad.size == 0, (i, bad[:8].tolist(), got[i][bad[:8]].tolist(), want[i][bad[:8]].tolist())
        assert np.array_equal(self.state.cpu().numpy(), self.ref.t.words())
        assert np.array_equal(self.mstate.cpu().numpy(), self.ref.motion_bytes(h, w))
        assert np.array_equal(dev_frames.cpu().numpy(), host)                # the frames are read only
        return got, got_cuts


def keys_for(h, w, frames, interval):
    """The key frames' detections of a call: everything, half of it (the rest is held), everything, nothing, ..."""
    every, some, none = packs(h, w)
    return [(every, some, every, none)[k % 4] for k in range(I.keys_of(frames, interval))]


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("capacity", [4, 64])
@pytest.mark.parametrize("interval", [1, 3])
@pytest.mark.parametrize("frames", [1, 2, 5])
def test_the_grid_against_the_restatement(frames, interval, capacity, h, w):
    """Every placement of the cuts the call has room for, each on a tracker of its own that one frame of scene A has filled: none, at
    frame 0 (against the kept frame), on a key frame, on a between frame, twice in one call."""
    every = packs(h, w)[0]
    seen = set()
    for places in ((), (0,), (1,), (3,), (4,), (1, 3), (0, 2), (2, 3)):
        places = tuple(p for p in places if p < frames)
        if places in seen:
            continue
        seen.add(places)
        d = Device(capacity, h, w)
        d.call(scenes(h, w)[0][:1], [every], 1, 1)
        ids_before = {s["id"] for s in d.ref.t.slots}
        assert ids_before
        got, cuts = d.call(film(h, w, frames, places), keys_for(h, w, frames, interval), frames, interval, pad=5 if len(places) & 1 else 0)
        assert tuple(np.flatnonzero(cuts).tolist()) == places
        first = places[0] if places else frames
        for f in range(frames):
            n_rows, ids = int(got[f][0]), got[f][4 + 6 * (ROWS + capacity):4 + 7 * (ROWS + capacity)]
            if f >= first:                                                   # behind a cut no id of the scene before lives on
                assert not ids_before & set(ids[:n_rows].tolist())
            if places and first <= f < -(-first // interval) * interval:     # ... and between the cut and the next key frame: nothing
                assert n_rows == 0
        assert d.ref.t.frames == 1 + frames
    kinds = {(p % interval == 0, p == 0) for places in seen for p in places}
    assert (True, True) in kinds
    if frames > 1:
        assert (interval == 1, False) in kinds                               # a cut on a between frame where there is one, else on a key frame


@pytest.mark.parametrize("h,w", [(16, 24), (40, 64)])
def test_the_threshold_edge_on_the_device(h, w):
    """Half of every region's pixels move from bin 2 to bin 12, then the other half: D = hw exactly both times, a cut at 50 and none at
    51."""
    a = np.full((h, w, 3), 20, dtype=np.uint8)
    half, b = a.copy(), np.full((h, w, 3), 100, dtype=np.uint8)
    half[:, 1::2] = 100
    assert C.distance(a, half) == h * w and C.distance(a, b) == 2 * h * w
    none = pack_rows([], [], ROWS)
    for pct, want in ((50, [0, 1, 1]), (51, [0, 0, 0]), (100, [0, 0, 0]), (1, [0, 1, 1])):
        assert Device(4, h, w).call([a, half, b], [none] * 3, 3, 1, pct=pct)[1].tolist() == want
    assert Device(4, h, w).call([a, b, a], [none] * 3, 3, 1, pct=100)[1].tolist() == [0, 1, 1]
    d = Device(4, h, w)                                                      # ... and through the kept frame
    d.call([a], [none], 1, 1)
    assert d.call([half], [none], 1, 1, pct=50)[1].tolist() == [1]
    assert d.call([a], [none], 1, 1, pct=51)[1].tolist() == [0]


@pytest.mark.parametrize("interval", [1, 3])
def test_without_a_cut_every_byte_is_track_update_interval_s(interval):
    from faster_rcnn_amd import ops
    h, w = SIZES[0]
    seq = scenes(h, w)[0] + scenes(h, w)[0][::-1]
    table = torch.from_numpy(TABLE).cuda()
    a, b = ops.track_state(4), ops.track_state(4)
    ma, mb = ops.track_motion_state(h, w), ops.track_motion_state(h, w)
    at = 0
    for F, nf in ((1, 1), (5, 5), (4, 2), (2, 0)):
        frames = torch.from_numpy(np.stack(seq[at:at + F])).cuda()
        packed = torch.from_numpy(np.stack(keys_for(h, w, F, interval))).cuda()
        n = torch.tensor([nf], dtype=torch.int32, device="cuda")
        got, cuts = ops.track_update_cut(a, ma, frames, 3 * h * w, packed, n, table, h, w, *PARAMS, RADIUS, interval, PCT)
        want = ops.track_update_interval(b, mb, frames.view(-1), 3 * h * w, packed, n, table, h, w, *PARAMS, RADIUS, interval,
                                         out=torch.empty_like(got))
        assert not cuts.cpu().numpy().any() and tuple(cuts.shape) == (F,)
        assert torch.equal(got, want) and torch.equal(a, b) and torch.equal(ma, mb), at
        at += F
    assert int(a[3]) == 8 and int(a[0]) > 0


@pytest.mark.parametrize("interval", [1, 3])
def test_frames_behind_n_frames_are_untouched_and_no_cut(interval):
    h, w = SIZES[0]
    every = packs(h, w)[0]
    for nf in (0, 1, 2, 4, -3, 9):
        d = Device(4, h, w)
        d.call(scenes(h, w)[0][:1], [every], 1, 1)
        before = (d.state.clone(), d.mstate.clone())
        frames = film(h, w, 5, (0, 2, 4))                                    # cuts at 0, 2 and 4: the ones at f >= nf are not seen
        got, cuts = d.call(frames, keys_for(h, w, 5, interval), nf, interval, pad=3)
        real = min(max(nf, 0), 5)
        assert cuts.tolist() == [int(f in (0, 2, 4) and f < real) for f in range(5)]
        if real == 0:
            assert torch.equal(d.state, before[0]) and torch.equal(d.mstate, before[1])
        assert d.ref.t.frames == 1 + real


def test_captured_and_replayed_twice_gives_the_eager_bytes():
    from faster_rcnn_amd import ops
    h, w = SIZES[0]
    cap, F, K = 4, 5, 2
    B = I.keys_of(F, K)
    every, some, none = packs(h, w)
    table = torch.from_numpy(TABLE).cuda()
    state, mstate = ops.track_state(cap), ops.track_motion_state(h, w)
    stride = 3 * h * w + 3
    dev_frames = torch.zeros(F * stride, dtype=torch.uint8, device="cuda")
    dev = torch.zeros((B, 4 + 7 * ROWS), dtype=torch.int32, device="cuda")
    nf = torch.zeros(1, dtype=torch.int32, device="cuda")                    # 0 frames: warm-up and capture leave every state alone
    out = torch.zeros((F, 4 + 8 * (ROWS + cap)), dtype=torch.int32, device="cuda")
    cuts, ws = torch.zeros(F, dtype=torch.int32, device="cuda"), ops.track_cut_workspace(F)
    run = lambda: ops.track_update_cut(state, mstate, dev_frames, stride, dev, nf, table, h, w, *PARAMS, RADIUS, K, PCT, out=out, cuts=cuts,
                                       workspace=ws)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    assert not state.cpu().numpy().any() and not mstate.cpu().numpy().any() and not cuts.cpu().numpy().any()
    eager = Device(cap, h, w)
    # two replays with other frames and detections: a full call with a cut on a between frame, a short one with a cut at frame 0 (against
    # the frame the first replay kept) and one behind *n_frames
    parts = ((film(h, w, F, (3,)), [every, some, none], 5), (film(h, w, F, (0, 4), first=1), [some, every, every], 3))
    for k, (part_f, part_p, real) in enumerate(parts):
        dev_frames.copy_(torch.from_numpy(upload(part_f, stride, h, w)).cuda())
        dev.copy_(torch.from_numpy(np.stack(part_p)).cuda())
        nf.fill_(real)
        graph.replay()
        want, want_cuts = eager.call(part_f, part_p, real, K, pad=3)         # (the eager call, itself held against the restatement)
        assert np.array_equal(out.cpu().numpy(), want) and cuts.cpu().numpy().tolist() == want_cuts.tolist(), k
        assert torch.equal(state, eager.state) and torch.equal(mstate, eager.mstate), k
        assert want_cuts.tolist() == [[0, 0, 0, 1, 0], [1, 0, 0, 0, 0]][k]
    assert eager.ref.t.frames == 8


def test_bad_arguments_raise_and_write_nothing():
    from faster_rcnn_amd import _lib, ops
    h, w = SIZES[0]
    cap = 4
    table = torch.from_numpy(TABLE).cuda()
    state, mstate = ops.track_state(cap), ops.track_motion_state(h, w)
    frame = torch.from_numpy(scenes(h, w)[0][0]).cuda().view(-1)
    four = torch.cat([frame] * 4)
    dev = torch.from_numpy(pack_rows([[0, 0, 20, 20]], [1], ROWS)).cuda()
    dev2 = torch.stack([dev, dev])
    nf = torch.ones(1, dtype=torch.int32, device="cuda")
    R = ROWS + cap
    out = torch.full((4, 4 + 8 * R), 77, dtype=torch.int32, device="cuda")
    cuts = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    ws = torch.full((5 * 512,), 77, dtype=torch.int32, device="cuda")
    for pct in (0, 101, -1):
        with pytest.raises(_lib.FrcnnError):
            ops.track_update_cut(state, mstate, four, 3 * h * w, dev2, nf, table, h, w, *PARAMS, RADIUS, 2, pct, out=out, cuts=cuts, workspace=ws)
    for interval in (0, 17, -1):
        with pytest.raises(_lib.FrcnnError):
            ops.track_update_cut(state, mstate, four, 3 * h * w, dev, nf, table, h, w, *PARAMS, RADIUS, interval, PCT, out=out[:1], cuts=cuts[:1],
                                 workspace=ws)
    with pytest.raises(_lib.FrcnnError):                                     # four frames every two: two key frames, one buffer
        ops.track_update_cut(state, mstate, four, 3 * h * w, dev, nf, table, h, w, *PARAMS, RADIUS, 2, PCT, out=out, cuts=cuts, workspace=ws)
    for kw in (dict(radius=0), dict(radius=17), dict(thr=0), dict(hold=256), dict(grow=65)):
        with pytest.raises(_lib.FrcnnError):
            ops.track_update_cut(state, mstate, four, 3 * h * w, dev2, nf, table, h, w,
                                 **dict(dict(interval=2, pct=PCT, out=out, cuts=cuts, workspace=ws), **kw))
    with pytest.raises(_lib.FrcnnError):
        ops.track_cut_workspace(0)
    with pytest.raises(_lib.FrcnnError):
        ops.track_cut_workspace(65)
    lib = _lib.load()
    assert lib.frcnn_track_cut_workspace_bytes(1) == 2 * 2048 and lib.frcnn_track_cut_workspace_bytes(64) == 65 * 2048
    assert lib.frcnn_track_cut_workspace_bytes(0) == 0 and lib.frcnn_track_cut_workspace_bytes(65) == 0
    ptrs = [state.data_ptr(), mstate.data_ptr(), four.data_ptr(), dev2.data_ptr(), nf.data_ptr(), table.data_ptr(), out.data_ptr(),
            ws.data_ptr(), cuts.data_ptr()]

    def raw(p=ptrs, capacity=cap, frame_stride=3 * h * w, det_stride=4 + 7 * ROWS, frames=4, max_rows=ROWS, classes=5, radius=RADIUS, interval=2,
            hh=h, ww=w, out_stride=4 + 8 * R, pct=PCT):
        return lib.frcnn_track_update_cut(p[0], capacity, p[1], p[2], frame_stride, p[3], det_stride, frames, p[4], max_rows, p[5], classes,
                                          30, 8, 0, radius, interval, hh, ww, p[6], out_stride, pct, p[7], p[8], None)

    for null in range(9):                                                   # FRCNN_E_ARG (-1) for each null pointer
        p = list(ptrs)
        p[null] = None
        assert raw(p) == -1 and b"null pointer" in lib.frcnn_last_error()
    for kw in (dict(pct=0), dict(pct=101), dict(pct=-5), dict(interval=0), dict(interval=17), dict(det_stride=3 + 7 * ROWS), dict(det_stride=0),
               dict(frame_stride=3 * h * w - 1), dict(out_stride=3 + 8 * R), dict(frames=0), dict(frames=65), dict(capacity=0),
               dict(capacity=129), dict(max_rows=0), dict(classes=0), dict(classes=257), dict(hh=0), dict(ww=32769), dict(radius=0),
               dict(radius=17)):
        assert raw(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 77).all() and (cuts.cpu().numpy() == 77).all() and (ws.cpu().numpy() == 77).all()
    assert not state.cpu().numpy().any() and not mstate.cpu().numpy().any()
    assert raw() == 0 and lib.frcnn_track_cut_version() == _lib.TRACK_CUT_VERSION == 1
    torch.cuda.synchronize()
    assert int(state[3]) == 1 and cuts.cpu().numpy().tolist() == [0, 0, 0, 0] and out.cpu().numpy()[0, :4].tolist() == [1, 1, 2, 0]
