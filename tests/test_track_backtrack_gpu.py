"""ops.track_backtrack (csrc/track_backtrack.hip) against the numpy restatement of the back-track rule (tests/track_backtrack_ref.py), byte
for byte: the emitted frames, the emitted tracked buffers and the whole window state after every call."""
import numpy as np
import pytest
import torch

from tests import track_backtrack_ref as BT
from tests import track_lookback_ref as LB
from tests import track_ref as T

pytestmark = pytest.mark.gpu

H, W, ROWS, CAP = 48, 64, 8, 4
R = ROWS + CAP


def seen(o, t):
    """Object 0 from the start, 1 from frame 3, 2 from the first key frame at or behind frame 5 (with F = 6 and with F = 4 frame 0 of a
    call: its chain runs into the window), 3 from frame 8; object 0 is not seen in frames 5..7 (held) and matched again behind them."""
    return t >= (0, 3, 5, 8)[o] and not (o == 0 and 5 <= t <= 7)


class Device:
    """A device window with its restatement beside it: ``call`` runs both and compares everything."""

    def __init__(self, F, K, back, h=H, w=W, rows=ROWS, cap=CAP):
        from faster_rcnn_amd import ops
        self.ops, self.F, self.K, self.h, self.w, self.rows, self.cap, self.back = ops, F, K, h, w, rows, cap, back
        self.R, self.R2 = rows + cap, rows + cap + back
        self.window = ops.track_lookback_state(F, h, w, rows, cap, back)
        self.ref = BT.Window(F, h, w, rows, cap, back)
        self.nf = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.frames = torch.zeros((F, h, w, 3), dtype=torch.uint8, device="cuda")
        self.tracked = torch.zeros((F, 4 + 8 * self.R), dtype=torch.int32, device="cuda")
        self.out = (torch.full((F, h, w, 3), 77, dtype=torch.uint8, device="cuda"),
                    torch.full((F, 4 + 8 * self.R2), 77, dtype=torch.int32, device="cuda"), torch.full((1,), 77, dtype=torch.int32, device="cuda"))

    def load(self, frames, tracked, n):
        real = max(n, 0)
        fs = list(frames[:real]) + [np.zeros((self.h, self.w, 3), dtype=np.uint8)] * (self.F - real)
        ts = list(tracked[:real]) + [np.zeros(4 + 8 * self.R, dtype=np.int32)] * (self.F - real)
        self.frames.copy_(torch.from_numpy(np.stack(fs)))
        self.tracked.copy_(torch.from_numpy(np.stack(ts)))
        self.nf.fill_(n)
        return fs, ts

    def launch(self, L, radius, grow):
        return self.ops.track_backtrack(self.window, self.frames, 3 * self.h * self.w, self.tracked, self.nf, self.cap, self.back, self.h, self.w,
                                        L, radius, grow, self.K, out=self.out)

    def check(self, want, where):
        want_f, want_t = want
        got_f, got_t, count = (t.cpu().numpy() for t in self.out)
        assert int(count[0]) == len(want_f), where
        for e in range(self.F):
            if e < len(want_f):
                assert np.array_equal(got_f[e], want_f[e]), (where, e)
                assert np.array_equal(got_t[e], want_t[e]), (where, e, got_t[e], want_t[e])
            else:
                assert not got_t[e][:4].any(), (where, e)
        state = self.window.cpu().numpy()
        assert np.array_equal(state[:BT.HEADER], self.ref.state_bytes()[:BT.HEADER]), (where, state[:BT.HEADER].view(np.int32))
        assert np.array_equal(state, self.ref.state_bytes()), where
        return want

    def call(self, frames, tracked, n, L, radius=0, grow=0, where=None):
        fs, ts = self.load(frames, tracked, n)
        self.launch(L, radius, grow)
        return self.check(self.ref.call(fs, ts, n, L, radius, grow, self.K), where)


def play(dev, frames, tracked, sizes, L, radius, grow):
    """The sequence cut into calls of ``sizes`` real frames and a flush -> every emitted buffer."""
    at, out = 0, []
    for i, n in enumerate(list(sizes) + [-1]):
        out += dev.call(frames[at:at + max(n, 0)], tracked[at:at + max(n, 0)], n, L, radius, grow, where=(i, n))[1]
        at += max(n, 0)
    return out


_made = {}


def material(F, K, move):
    """12 frames and their tracked buffers (calls of F frames), made once."""
    if (F, K, move) not in _made:
        _made[(F, K, move)] = BT.sequence(H, W, 12, K, 5, ROWS, CAP, seen, move=move, per_call=F)
    return _made[(F, K, move)]


@pytest.mark.parametrize("radius", (0, 4))
@pytest.mark.parametrize("F, K, L", [(6, 3, 1), (6, 3, 2), (6, 3, 6), (4, 2, 1), (4, 2, 4)])
def test_rolled_noise_against_the_restatement(F, K, L, radius):
    """A correction and a birth in the same key frame (frame 3 with K = 3, frame 4 with K = 2), a birth in a call's frame 0 chained into the
    window, full calls and a flush; every interior back-filled box is its source box shifted by -k x (3, -2)."""
    frames, tracked = material(F, K, BT.MOVE)
    dev = Device(F, K, 4)
    out = play(dev, frames, tracked, (F,) * (12 // F), L, radius, grow=1)
    assert len(out) == 12 and dev.ref.back_overflow == 0
    assert sum(len(BT.backfilled(b)) for b in out) > 0
    if radius:
        assert BT.check_shifts(out, K, H, W, 4, grow=1) > 0
    born = [(t, tid) for t in range(F, 12, F) for tid, k, _ in BT.backfilled(out[t - 1]) if k == 1 and tid >= int(tracked[t - 1][2])]
    assert born                                                              # a birth in a call's frame 0 reaches the window
    mixed = 3 if K == 3 else 4                                               # a key frame with a correction and a birth
    got = BT.sources(tracked[mixed], int(tracked[mixed - 1][2]), CAP)
    assert {b for _, b in got} == {True, False}


@pytest.mark.parametrize("F, K, L", [(6, 3, 6), (4, 2, 1)])
def test_identical_frames_keep_the_boxes_still(F, K, L):
    frames, tracked = material(F, K, (0, 0))
    dev = Device(F, K, 4)
    out = play(dev, frames, tracked, (F,) * (12 // F), L, 4, grow=0)
    assert BT.check_shifts(out, K, H, W, 0, move=(0, 0)) == sum(len(BT.backfilled(b)) for b in out) > 0


@pytest.mark.parametrize("F, K, L, sizes", [(6, 3, 6, (6, 4, 2)), (4, 2, 2, (4, 4, 3, 1))])
def test_a_short_last_call_and_a_flush(F, K, L, sizes):
    frames, tracked = material(F, K, BT.MOVE)
    dev = Device(F, K, 4)
    out = play(dev, frames, tracked, sizes, L, 4, grow=1)
    assert len(out) == 12 and sum(len(BT.backfilled(b)) for b in out) > 0
    assert dev.call(frames[:F], tracked[:F], -1, L) == ([], []) and dev.ref.count == 0


def test_one_row_of_room_drops_from_the_end_of_the_order():
    frames, tracked = material(6, 3, BT.MOVE)
    dev = Device(6, 3, 1)
    play(dev, frames, tracked, (6, 6), 6, 4, grow=1)
    assert dev.ref.back_overflow == 0                                        # (two rows at most reach a frame with eight free rows)
    full = tracked[0].copy()                                                 # frame 0: every row of R in use
    n = int(full[0])
    for r in range(n, R):
        full[4 + 4 * r:8 + 4 * r] = (3, 3, 20, 20)
        full[4 + 4 * R + r], full[4 + 6 * R + r], full[4 + 7 * R + r] = 1, 50 + r, 1
    full[0] = R
    dev = Device(6, 3, 1)
    dev.call(frames[:6], [full, full, full] + list(tracked[3:6]), 6, 6, 4, grow=1)
    _, out = dev.call(frames[:6], tracked[:6], -1, 6, 4)
    # key frame 3: track 1 (a correction, row 0) and track 2 (a birth, row 1).  Frames 2 and 1 have one place for the two: the first of the
    # order stays, the birth is dropped; frame 0 is reached by the birth alone
    assert BT.sources(tracked[3], int(tracked[2][2]), CAP) == [(0, False), (1, True)] and T.split(tracked[3])[7][:2].tolist() == [1, 2]
    assert dev.ref.back_overflow == 2 and int(dev.window[:12].view(torch.int32).cpu()[2]) == 2
    assert [[tid for tid, _, _ in BT.backfilled(b)] for b in out[:3]] == [[2], [1], [1]]


def test_zero_frames_writes_no_window_byte():
    frames, tracked = material(6, 3, BT.MOVE)
    dev = Device(6, 3, 4)
    dev.call(frames[:6], tracked[:6], 6, 6, 4, grow=1)
    before = dev.window.cpu().numpy().copy()
    for _ in range(2):
        out_f, _ = dev.call(frames[6:], tracked[6:], 0, 6, 4, grow=1)        # emits the window again
        assert len(out_f) == 6 and np.array_equal(dev.window.cpu().numpy(), before)
    dev.ops.track_lookback_reset(dev.window)
    dev.ref.reset()
    assert dev.call(frames[:6], tracked[:6], 0, 6) == ([], [])


def test_interval_one_is_track_lookback_on_the_device():
    from faster_rcnn_amd import ops
    frames, _, tracked = LB.sequence(H, W, 9, 3, ROWS, CAP, objects=3, hold=2, grow=1)
    B, L, radius = 4, 4, 4
    dev = Device(B, 1, 2)
    window = ops.track_lookback_state(B, H, W, ROWS, CAP, 2)
    out = tuple(torch.full_like(t, 77) for t in dev.out)
    at, filled = 0, 0
    for n in (4, 2, 3, -1):
        real = max(n, 0)
        dev.call(frames[at:at + real], tracked[at:at + real], n, L, radius, 1, where=n)
        ops.track_lookback(window, dev.frames, 3 * H * W, dev.tracked, dev.nf, CAP, 2, H, W, L, radius, 1, out=out)
        assert torch.equal(window, dev.window), n
        for a, b in zip(out, dev.out):
            assert torch.equal(a, b), n
        filled += int((dev.out[1][:, 4 + 7 * dev.R2:] < 0).sum())
        at += real
    assert filled > 0


def test_captured_and_replayed():
    frames, tracked = material(6, 3, BT.MOVE)
    dev = Device(6, 3, 4)
    dev.load(frames[:6], tracked[:6], 0)                                     # 0 frames: warm-up and capture leave the window alone
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dev.launch(6, 4, 1)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dev.launch(6, 4, 1)
    assert not dev.window.cpu().numpy().any()
    for k in range(2):
        fs, ts = dev.load(frames[6 * k:6 * k + 6], tracked[6 * k:6 * k + 6], 6)
        graph.replay()
        want = dev.check(dev.ref.call(fs, ts, 6, 6, 4, 1, 3), k)
        assert len(want[0]) == (0 if k == 0 else 6)


def test_bad_arguments_raise_and_write_nothing():
    from faster_rcnn_amd import _lib, ops
    F, K, back = 4, 2, 2
    R2 = R + back
    dev = Device(F, K, back)
    dev.nf.fill_(F)
    good = dict(lookback=2, radius=1, grow=0, interval=K)
    for kw in (dict(lookback=0), dict(lookback=17), dict(radius=-1), dict(radius=17), dict(grow=-1), dict(grow=65), dict(interval=0),
               dict(interval=17), dict(interval=-1)):
        with pytest.raises(_lib.FrcnnError):
            ops.track_backtrack(dev.window, dev.frames, 3 * H * W, dev.tracked, dev.nf, CAP, back, H, W, out=dev.out, **dict(good, **kw))
    lib = _lib.load()
    ptrs = [dev.window.data_ptr(), dev.frames.data_ptr(), dev.tracked.data_ptr(), dev.nf.data_ptr(), dev.out[0].data_ptr(), dev.out[1].data_ptr(),
            dev.out[2].data_ptr()]

    def raw(p=ptrs, frame_stride=3 * H * W, tracked_stride=4 + 8 * R, frames=F, max_rows=ROWS, capacity=CAP, bk=back, L=2, radius=1, grow=0,
            interval=K, hh=H, ww=W, out_frame_stride=3 * H * W, out_tracked_stride=4 + 8 * R2):
        return lib.frcnn_track_backtrack(p[0], p[1], frame_stride, p[2], tracked_stride, frames, p[3], max_rows, capacity, bk, L, radius, grow,
                                         interval, hh, ww, p[4], out_frame_stride, p[5], out_tracked_stride, p[6], None)

    for null in range(7):                                                    # FRCNN_E_ARG (-1) for each null pointer
        p = list(ptrs)
        p[null] = None
        assert raw(p) == -1 and b"null pointer" in lib.frcnn_last_error()
    p = list(ptrs)
    p[0] += 4
    assert raw(p) == -1 and b"aligned" in lib.frcnn_last_error()
    for kw in (dict(frame_stride=3 * H * W - 1), dict(out_frame_stride=0), dict(tracked_stride=3 + 8 * R), dict(out_tracked_stride=3 + 8 * R2),
               dict(frames=0), dict(frames=65), dict(capacity=0), dict(capacity=129), dict(max_rows=0), dict(bk=0), dict(bk=129),
               dict(max_rows=512 - CAP - back + 1), dict(hh=0), dict(ww=0), dict(hh=32769), dict(ww=32769), dict(L=0), dict(L=17),
               dict(radius=-1), dict(radius=17), dict(grow=-1), dict(grow=65), dict(interval=0), dict(interval=17)):
        assert raw(**kw) == -1, kw
        assert b"track_backtrack" in lib.frcnn_last_error()
    assert lib.frcnn_track_backtrack_version() == _lib.TRACK_BACKTRACK_VERSION == 1
    torch.cuda.synchronize()
    assert not dev.window.cpu().numpy().any()                                # everything refused launched nothing
    assert all((t.cpu().numpy() == 77).all() for t in dev.out)
