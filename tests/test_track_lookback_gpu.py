"""ops.track_lookback (csrc/track_lookback.hip) against the numpy restatement of the look-back rule (tests/track_lookback_ref.py), byte for
byte: the emitted frames, the emitted tracked buffers and the whole window state after every call."""
import numpy as np
import pytest
import torch

from tests import track_lookback_ref as LB
from tests import track_ref as T

pytestmark = pytest.mark.gpu

ROWS = 8
SIZES = ((48, 64), (37, 53))
STARTS = (1, 3, 4, 6)                              # the frame each object is first "detected" in


# (x, y, width, height, vx, vy): rows of their own for the objects of one class, so that no track takes another object's detection;
# object 2 starts left of the frame and object 3 runs out of it on the right
OBJECTS = ((2, 2, 12, 10, 2, 0), (30, 14, 12, 10, -3, 0), (-9, 26, 14, 10, 3, 0), (30, 2, 12, 10, 2, 1))


def detected(o, t):
    """Object o is seen from frame STARTS[o] on; object 0 is lost in frames 4..6 (freed at hold = 2) and born again in frame 7."""
    return t >= STARTS[o % 4] and not (o == 0 and 4 <= t <= 6)


class Device:
    """A device window with its restatement beside it: ``call`` runs both and compares everything."""

    def __init__(self, B, h, w, rows, cap, back):
        from faster_rcnn_amd import ops
        self.ops, self.B, self.h, self.w, self.rows, self.cap, self.back = ops, B, h, w, rows, cap, back
        self.R, self.R2 = rows + cap, rows + cap + back
        self.window = ops.track_lookback_state(B, h, w, rows, cap, back)
        self.ref = LB.Window(B, h, w, rows, cap, back)
        self.nf = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.frames = torch.zeros((B, h, w, 3), dtype=torch.uint8, device="cuda")
        self.tracked = torch.zeros((B, 4 + 8 * self.R), dtype=torch.int32, device="cuda")
        self.out = (torch.full((B, h, w, 3), 77, dtype=torch.uint8, device="cuda"),
                    torch.full((B, 4 + 8 * self.R2), 77, dtype=torch.int32, device="cuda"), torch.full((1,), 77, dtype=torch.int32, device="cuda"))

    def load(self, frames, tracked, n):
        real = max(n, 0)
        fs = list(frames[:real]) + [np.zeros((self.h, self.w, 3), dtype=np.uint8)] * (self.B - real)
        ts = list(tracked[:real]) + [np.zeros(4 + 8 * self.R, dtype=np.int32)] * (self.B - real)
        self.frames.copy_(torch.from_numpy(np.stack(fs)))
        self.tracked.copy_(torch.from_numpy(np.stack(ts)))
        self.nf.fill_(n)
        return fs, ts

    def launch(self, L, radius, grow):
        return self.ops.track_lookback(self.window, self.frames, 3 * self.h * self.w, self.tracked, self.nf, self.cap, self.back, self.h, self.w,
                                       L, radius, grow, out=self.out)

    def check(self, want, where):
        want_f, want_t = want
        got_f, got_t, count = (t.cpu().numpy() for t in self.out)
        assert int(count[0]) == len(want_f), where
        for e in range(self.B):
            if e < len(want_f):
                assert np.array_equal(got_f[e], want_f[e]), (where, e)
                assert np.array_equal(got_t[e], want_t[e]), (where, e, got_t[e], want_t[e])
            else:
                assert not got_t[e][:4].any(), (where, e)
        state = self.window.cpu().numpy()
        assert np.array_equal(state[:LB.HEADER], self.ref.state_bytes()[:LB.HEADER]), (where, state[:LB.HEADER].view(np.int32))
        assert np.array_equal(state, self.ref.state_bytes()), where
        return want

    def call(self, frames, tracked, n, L, radius=0, grow=0, where=None):
        fs, ts = self.load(frames, tracked, n)
        self.launch(L, radius, grow)
        return self.check(self.ref.call(fs, ts, n, L, radius, grow), where)


def play(dev, frames, tracked, sizes, L, radius, grow):
    """The sequence cut into calls of ``sizes`` real frames and a flush -> every emitted buffer."""
    at, out = 0, []
    for i, n in enumerate(list(sizes) + [-1]):
        out += dev.call(frames[at:at + max(n, 0)], tracked[at:at + max(n, 0)], n, L, radius, grow, where=(i, n))[1]
        at += max(n, 0)
    return out


CASES = [  # size, capacity, back, frames per call, the calls' real frames, L, radius
    (0, 4, 2, 4, (4, 4, 1), 4, 4),
    (0, 4, 2, 4, (4, 2, 3), 3, 1),                  # a short call in mid-sequence
    (0, 8, 8, 2, (2, 2, 2, 2, 1), 2, 4),
    (0, 8, 8, 1, (1,) * 9, 1, 1),
    (0, 4, 8, 4, (4, 4, 1), 2, 0),
    (1, 4, 2, 4, (4, 4, 1), 4, 1),
    (1, 8, 2, 4, (3, 4, 2), 3, 4),
    (1, 8, 8, 2, (2, 2, 2, 2, 1), 1, 0),
    (1, 4, 8, 1, (1,) * 9, 1, 4),
    (1, 8, 2, 2, (2, 1, 2, 2, 2), 2, 1),
]


@pytest.mark.parametrize("size, cap, back, B, sizes, L, radius", CASES)
def test_sequences_against_the_restatement(size, cap, back, B, sizes, L, radius):
    h, w = SIZES[size]
    frames, _, tracked = LB.sequence(h, w, 9, 3 + size, ROWS, cap, objects=OBJECTS, hold=2, grow=1, detected=detected)
    born = [t for t in range(1, 9) if LB.births(LB.widen(tracked[t], ROWS + cap + back), int(tracked[t - 1][2]), cap)]
    assert born == [1, 3, 4, 6, 7]                                          # with B = 4: every position of a call, first and last included
    dev = Device(B, h, w, ROWS, cap, back)
    out = play(dev, frames, tracked, sizes, L, radius, grow=1)
    assert len(out) == 9
    filled = [int((T.split(b)[8] < 0).sum()) for b in out]
    assert sum(filled) > 0 and filled[0] >= 1 and dev.ref.back_overflow == 0


def crafted(R, live, next_id, held=()):
    """A tracked buffer of R rows: ``live`` = [(box, cls, id)], ``held`` = [(box, cls, id, age)]."""
    buf = np.zeros(4 + 8 * R, dtype=np.int32)
    buf[4:4 + 5 * R] = -1
    rows = [(b, c, i, 0) for b, c, i in live] + list(held)
    for r, (box, cls, tid, age) in enumerate(rows):
        buf[4 + 4 * r:8 + 4 * r] = box
        buf[4 + 4 * R + r], buf[4 + 5 * R + r], buf[4 + 6 * R + r], buf[4 + 7 * R + r] = cls, T.bits(0.75), tid, age
    buf[:4] = (len(rows), len(live), next_id, 0)
    return buf


def square_frames(h, w, n, step=3):
    back, patch = LB.texture(h, w, 1), LB.texture(16, 16, 2)
    return [LB.paste(back, patch, 4 + step * t, 10) for t in range(n)]


def test_boxes_that_are_not_searched_and_one_that_leaves_the_frame():
    """A box leaves the frame only by being outside it already: the search cannot carry a box whose clipped part is not empty across an
    edge.  A shift that would (xb + dx < 0) clamps EVERY sample to column 0, and so does the shift one pixel shorter (xb + dx + 1 <= 0): the
    two cost the same, and BEST takes the smaller norm, so a move ends with xb >= 0 at the latest (likewise at the other three edges).  The
    bbox -1 / skipped-search branch is therefore reached with a crafted box outside the frame; the tracker itself only gives birth to boxes
    that are not empty, and their chains stay not empty."""
    h, w = SIZES[0]
    frames = square_frames(h, w, 4)
    R = ROWS + 4
    x = 4 + 3 * 3
    live = [((-20, 5, -5, 20), 1, 1),               # outside the frame: the clipped box is empty, bbox -1 in every frame
            ((x + 4, 14, x + 6, 16), 1, 2),         # 3 x 3 = 9 samples: fewer than 16, no search, the box stands still on the moving square
            ((x, 10, x + 15, 25), 2, 3),            # the square: followed, 3 px a frame
            ((1, 30, 12, 45), 1, 4)]                # texture that stands still: the best shift is none
    tracked = [crafted(R, [], 1), crafted(R, [], 1), crafted(R, [], 1), crafted(R, live, 5)]
    dev = Device(4, h, w, ROWS, 4, 2)
    dev.call(frames, tracked, 4, 3, radius=4, grow=2)
    _, out_t = dev.call(frames, tracked, -1, 3, radius=4, grow=2)
    for g, k in ((2, 1), (1, 2), (0, 3)):
        n_rows, n_live, _, _, bbox, cls, _, ids, age = T.split(out_t[g])
        e = 2 * k
        assert (n_rows, n_live) == (4, 0) and ids[:4].tolist() == [1, 2, 3, 4] and age[:4].tolist() == [-k] * 4 and cls[:4].tolist() == [1, 1, 2, 1]
        assert bbox[0].tolist() == [-1, -1, -1, -1]
        assert bbox[1].tolist() == [x + 4 - e, 14 - e, x + 6 + e, 16 + e]
        assert bbox[2].tolist() == [x - 3 * k - e, 10 - e, x + 15 - 3 * k + e, 25 + e]
        assert bbox[3].tolist() == [1 - e, 30 - e, 12 + e, 45 + e]
    assert dev.ref.back_overflow == 0


def test_flat_frames_keep_the_box():
    h, w = SIZES[1]
    frames = [np.full((h, w, 3), 128, dtype=np.uint8)] * 3
    R = ROWS + 4
    tracked = [crafted(R, [], 1), crafted(R, [], 1), crafted(R, [((5, 6, 30, 31), 1, 1)], 2)]
    dev = Device(3, h, w, ROWS, 4, 2)
    dev.call(frames, tracked, 3, 2, radius=4)
    _, out_t = dev.call(frames, tracked, -1, 2, radius=4)
    assert [T.split(b)[4][0].tolist() for b in out_t[:2]] == [[5, 6, 30, 31]] * 2


def test_three_births_into_a_full_frame_overflow():
    h, w = SIZES[0]
    rows, cap, back = 3, 4, 2
    R, box = rows + cap, (3, 3, 20, 20)
    full = crafted(R, [(box, 1, 1), (box, 1, 2), (box, 1, 3)], 8, held=[(box, 1, 4 + i, 1) for i in range(4)])
    born = crafted(R, [((2, 2, 22, 22), 1, 8), ((10, 10, 30, 30), 2, 9), ((20, 20, 40, 40), 1, 10)], 11)
    frames = [LB.texture(h, w, s) for s in range(2)]
    dev = Device(2, h, w, rows, cap, back)
    dev.call(frames, [full, born], 2, 4, radius=1)
    _, out_t = dev.call(frames, [full, born], -1, 4, radius=1)
    n_rows, n_live, _, _, _, _, _, ids, age = T.split(out_t[0])
    assert (n_rows, n_live) == (R + back, rows) and ids[R:].tolist() == [8, 9] and age[R:].tolist() == [-1, -1]
    assert dev.ref.back_overflow == 1 and dev.window[:12].view(torch.int32).cpu().tolist() == [0, 1, 1]
    dev.call(frames, [full, born], 2, 4, radius=1)                           # sticky: the next sequence counts on
    assert dev.ref.back_overflow == 2


def test_zero_frames_writes_no_window_byte_and_flush_empties_it():
    h, w = SIZES[1]
    frames, _, tracked = LB.sequence(h, w, 6, 9, ROWS, 4, objects=OBJECTS[:3], hold=2, grow=1, detected=detected)
    dev = Device(3, h, w, ROWS, 4, 2)
    dev.call(frames[:3], tracked[:3], 3, 3, radius=4)
    before = dev.window.cpu().numpy().copy()
    for _ in range(2):
        out_f, out_t = dev.call(frames[3:], tracked[3:], 0, 3, radius=4)     # emits the window again
        assert len(out_f) == 3 and np.array_equal(dev.window.cpu().numpy(), before)
    dev.call(frames[3:], tracked[3:], 3, 3, radius=4)
    out_f, _ = dev.call(frames[:3], tracked[:3], -1, 3, radius=4)
    assert len(out_f) == 3 and np.array_equal(out_f[2], frames[5]) and dev.ref.count == 0
    assert dev.call(frames[:3], tracked[:3], -1, 3, radius=4) == ([], [])
    dev.ops.track_lookback_reset(dev.window)
    dev.ref.reset()
    assert dev.call(frames[:3], tracked[:3], 0, 3) == ([], [])


def test_captured_and_replayed_three_times():
    h, w = SIZES[0]
    B, cap, back, L, radius = 2, 4, 2, 2, 4
    frames, _, tracked = LB.sequence(h, w, 6, 3, ROWS, cap, objects=OBJECTS, hold=2, grow=1, detected=detected)
    dev, eager = Device(B, h, w, ROWS, cap, back), Device(B, h, w, ROWS, cap, back)
    dev.load(frames[:B], tracked[:B], 0)                                     # 0 frames: warm-up and capture leave the window alone
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dev.launch(L, radius, 1)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dev.launch(L, radius, 1)
    assert not dev.window.cpu().numpy().any()
    for k in range(3):
        part = slice(k * B, k * B + B)
        fs, ts = dev.load(frames[part], tracked[part], B)
        graph.replay()
        want = dev.check(dev.ref.call(fs, ts, B, L, radius, 1), k)
        eager.call(frames[part], tracked[part], B, L, radius, 1, where=k)
        for a, b in zip(dev.out, eager.out):
            assert torch.equal(a, b), k
        assert torch.equal(dev.window, eager.window)
        assert len(want[0]) == (0 if k == 0 else B)


def test_bad_arguments_raise_and_write_nothing():
    from faster_rcnn_amd import _lib, ops
    h, w = SIZES[0]
    cap, back, B = 4, 2, 2
    R, R2 = ROWS + cap, ROWS + cap + back
    dev = Device(B, h, w, ROWS, cap, back)
    dev.nf.fill_(B)
    for kw in (dict(lookback=0), dict(lookback=17), dict(radius=-1), dict(radius=17), dict(grow=-1), dict(grow=65)):
        with pytest.raises(_lib.FrcnnError):
            ops.track_lookback(dev.window, dev.frames, 3 * h * w, dev.tracked, dev.nf, cap, back, h, w, out=dev.out, **kw)
    lib = _lib.load()
    ptrs = [dev.window.data_ptr(), dev.frames.data_ptr(), dev.tracked.data_ptr(), dev.nf.data_ptr(), dev.out[0].data_ptr(), dev.out[1].data_ptr(),
            dev.out[2].data_ptr()]

    def raw(p=ptrs, frame_stride=3 * h * w, tracked_stride=4 + 8 * R, frames=B, max_rows=ROWS, capacity=cap, bk=back, L=2, radius=1, grow=0, hh=h,
            ww=w, out_frame_stride=3 * h * w, out_tracked_stride=4 + 8 * R2):
        return lib.frcnn_track_lookback(p[0], p[1], frame_stride, p[2], tracked_stride, frames, p[3], max_rows, capacity, bk, L, radius, grow, hh,
                                        ww, p[4], out_frame_stride, p[5], out_tracked_stride, p[6], None)

    for null in range(7):                                                    # FRCNN_E_ARG (-1) for each null pointer
        p = list(ptrs)
        p[null] = None
        assert raw(p) == -1 and b"null pointer" in lib.frcnn_last_error()
    p = list(ptrs)
    p[0] += 4
    assert raw(p) == -1 and b"aligned" in lib.frcnn_last_error()
    for kw in (dict(frame_stride=3 * h * w - 1), dict(out_frame_stride=0), dict(tracked_stride=3 + 8 * R), dict(out_tracked_stride=3 + 8 * R2),
               dict(frames=0), dict(frames=65), dict(capacity=0), dict(capacity=129), dict(max_rows=0), dict(bk=0), dict(bk=129),
               dict(max_rows=512 - cap - back + 1), dict(hh=0), dict(ww=0), dict(hh=32769), dict(ww=32769), dict(L=0), dict(L=17),
               dict(radius=-1), dict(radius=17), dict(grow=-1), dict(grow=65)):
        assert raw(**kw) == -1, kw
    assert lib.frcnn_track_lookback_version() == _lib.TRACK_LOOKBACK_VERSION == 1
    cell = 16 + 32 * R2 + (3 * h * w + 15) // 16 * 16
    assert lib.frcnn_track_lookback_state_bytes(B, h, w, ROWS, cap, back) == 32 + 2 * B * cell == dev.window.numel()
    for bad in ((0, h, w, ROWS, cap, back), (65, h, w, ROWS, cap, back), (B, 0, w, ROWS, cap, back), (B, h, 32769, ROWS, cap, back),
                (B, h, w, 0, cap, back), (B, h, w, ROWS, 129, back), (B, h, w, ROWS, cap, 0), (B, h, w, 500, cap, 9)):
        assert lib.frcnn_track_lookback_state_bytes(*bad) == 0, bad
        with pytest.raises(_lib.FrcnnError):
            ops.track_lookback_state(*bad)
    torch.cuda.synchronize()
    assert not dev.window.cpu().numpy().any()                                # everything refused launched nothing
    assert all((t.cpu().numpy() == 77).all() for t in dev.out)
