"""The entry points of the heat extension (include/ext/frcnn_hip_heat.h, csrc/heat.hip) against the restatement (tests/heat_ref.py):
ops.heat_update's state and ops.heat_draw_u8's frame, byte for byte -- everything is integer, so there is no tolerance.  The update
kernel's tiles are 64 x 16 pixels and it stages 256 rows a round; the draw kernel's are 256 byte columns x 16 rows."""
import numpy as np
import pytest

from tests import heat_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

E_ARG = -1                                                                   # FRCNN_E_ARG
MAX_ROWS = 512                                                               # FRCNN_REDACT_MAX_ROWS
TABLE = np.array([0, 1, 1, 0], dtype=np.uint8)                               # classes 1 and 2 heat; 0 and 3 do not
SIZES = [(1, 1), (5, 7), (17, 70), (33, 257)]                                # (h, w): one pixel .. tile edges crossed both ways, w % 64 != 0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def noise(h, w, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def state_of(t, h, w):
    """The STATE of a device buffer: its first 4 + h w words (the update kernel's scratch words lie behind them)."""
    return t.cpu().numpy()[:4 + h * w]


def buffer_of(ref, h, w):
    """A device buffer holding the restatement's state, scratch words zeroed."""
    from faster_rcnn_amd import ops
    buf = np.zeros(ops.heat_state_words(h, w), dtype=np.int32)
    buf[:4 + h * w] = ref.words()
    return dev(buf)


def box_sets(h, w):
    """name -> (a frame's buffer, tracked): the cases of the issue for a frame of (h, w)."""
    rs = np.random.RandomState(h * 1000 + w)
    rnd = lambda n: [[int(rs.randint(-8, w + 8)), int(rs.randint(-8, h + 8)), int(rs.randint(-8, w + 8)), int(rs.randint(-8, h + 8))] for _ in range(n)]
    heap = [[max(w - 9, 0) - int(rs.randint(0, 3)), max(h - 5, 0) - int(rs.randint(0, 3)), w - 1 - int(rs.randint(0, 3)) + 4 * (k % 2),
             h - 1 - int(rs.randint(0, 2))] for k in range(MAX_ROWS)]        # every one meets the last tile: two staging rounds there
    return {
        "none": (R.make_packed(300, []), False),
        "all empty after the clip": (R.make_packed(300, [[w, 0, w + 5, h - 1], [0, h, w - 1, h + 9], [-9, -9, -1, -1], [-7, 0, -1, h]]), False),
        "crossing each border": (R.make_packed(300, [[-4, 1, 2, 3], [w - 2, 0, w + 6, 2], [1, -5, 3, 1], [0, h - 2, 4, h + 3], [-3, -3, w + 3, 0]]), False),
        "one-pixel boxes": (R.make_packed(300, [[0, 0, 0, 0], [w - 1, h - 1, w - 1, h - 1], [w // 2, h // 2, w // 2, h // 2], [w - 1, 0, w - 1, 0]]), False),
        "full frame": (R.make_packed(300, [[0, 0, w - 1, h - 1], [w + 50, h + 50, -50, -50]]), False),
        "a heap on one tile": (R.make_packed(MAX_ROWS, heap, cls=[1 + k % 2 for k in range(MAX_ROWS)]), False),
        "a table that filters": (R.make_packed(300, rnd(40), cls=[k % 6 - 1 for k in range(40)]), False),
        "rows behind n_dets": (R.make_packed(300, rnd(30), n_dets=11), False),
        "tracked, held rows": (R.make_tracked(364, 7, rnd(20), cls=[1 + k % 3 for k in range(20)]), True),
        "tracked, widened": (R.make_tracked(428, 25, rnd(40)), True),
    }


@pytest.mark.parametrize("h,w", SIZES)
def test_every_box_set_at_every_decay(h, w):
    """One frame of each box set on a map that is already warm, S in {0, 1, 15}: state after the update, frame after the draw."""
    from faster_rcnn_amd import ops
    table = dev(TABLE)
    warm = R.Heat(h, w).update(R.make_packed(8, [[0, 0, w // 2, h // 2], [w // 3, h // 3, w, h]]), TABLE)
    warm.map[h - 1, w - 1] += 77                                             # (an odd value: the decay's rounding)
    warm.peak = int(warm.map.max())
    frame = noise(h, w, 1)
    for name, (buf, tracked) in box_sets(h, w).items():
        for S in (0, 1, 15):
            ref = R.Heat(h, w, warm.words())
            state = buffer_of(ref, h, w)
            ops.heat_update(state, h, w, dev(buf), table, S, tracked=tracked)
            ref.update(buf, TABLE, S, tracked)
            assert np.array_equal(state_of(state, h, w), ref.words()), (name, S)
            got = ops.heat_draw_u8(dev(frame), state, 160, rgb=bool(S & 1)).cpu().numpy()
            assert np.array_equal(got, ref.draw(frame, 160, rgb=bool(S & 1))), (name, S)
    if h >= 5:                                                               # (the heap: more than one round's rows on one pixel)
        heap, _ = box_sets(h, w)["a heap on one tile"]
        assert R.coverage(h, w, heap, False, TABLE)[h - 3, max(w - 4, 0)] == MAX_ROWS


def test_a_six_frame_sequence_from_a_cold_map():
    """Boxes that move, appear and leave over six frames of 33 x 257, S = 2, alternating packed and tracked buffers; the drawn frame
    of every step."""
    from faster_rcnn_amd import ops
    h, w = 33, 257
    table, ref, state = dev(TABLE), R.Heat(h, w), ops.heat_state(h, w)
    frame = noise(h, w, 2)
    for f in range(6):
        boxes = [[10 + 30 * f, 2 + f, 60 + 30 * f, 20 + f], [200 - 20 * f, 10, 256 - 10 * f, 40], [63, 15, 64, 16]][:1 + f % 3 + (f > 3)]
        tracked = bool(f & 1)
        buf = R.make_tracked(364, len(boxes) - (f == 5), boxes) if tracked else R.make_packed(300, boxes)
        ops.heat_update(state, h, w, dev(buf), table, 2, tracked=tracked)
        ref.update(buf, TABLE, 2, tracked)
        assert np.array_equal(state_of(state, h, w), ref.words()), f
        got = ops.heat_draw_u8(dev(frame), state, rgb=True).cpu().numpy()
        assert np.array_equal(got, ref.draw(frame, 160, rgb=True)), f
    assert ref.frames == 6 and ref.peak > 256 and ref.saturated == 0


def test_the_clamp_and_saturated():
    """A state preset just under 2^30: a pixel that lands exactly on it is not clamped, one that passes it is, and `saturated` sticks.  The
    peak is above 2^24 here, so the draw divides in 64 bits."""
    from faster_rcnn_amd import ops
    h, w = 17, 70
    table = dev(TABLE)
    ref = R.Heat(h, w)
    ref.map[:] = np.random.RandomState(4).randint(0, R.MAX - 512, (h, w))
    ref.map[2, 3], ref.map[16, 69], ref.map[0, 0] = R.MAX - 256, R.MAX - 255, R.MAX - 600
    ref.peak = int(ref.map.max())
    state = buffer_of(ref, h, w)
    frame = noise(h, w, 3)
    steps = [[[3, 2, 3, 2]], [[69, 16, 69, 16], [0, 0, 0, 0], [0, 0, 0, 0]], []]
    for k, boxes in enumerate(steps):
        buf = R.make_packed(300, boxes)
        ops.heat_update(state, h, w, dev(buf), table, 0)
        ref.update(buf, TABLE, 0)
        assert np.array_equal(state_of(state, h, w), ref.words()), k
        assert ref.saturated == (k > 0) and ref.peak == R.MAX
        for A in (1, 160, 255):
            got = ops.heat_draw_u8(dev(frame), state, A).cpu().numpy()
            assert np.array_equal(got, ref.draw(frame, A)), (k, A)
    assert ref.map[2, 3] == R.MAX and ref.map[16, 69] == R.MAX and ref.map[0, 0] == R.MAX - 88


@pytest.mark.parametrize("h,w", SIZES)
def test_the_draw_at_every_alpha_in_both_orders(h, w):
    from faster_rcnn_amd import ops
    ref = R.Heat(h, w)
    ref.map[:] = np.random.RandomState(h + w).randint(0, 5000, (h, w)) * (np.random.RandomState(w).randint(0, 3, (h, w)) > 0)
    ref.map[h - 1, w - 1] = 5000
    ref.peak = int(ref.map.max())
    state = buffer_of(ref, h, w)
    frame = noise(h, w, 5)
    for A in (1, 160, 255):
        for rgb in (False, True):
            got = ops.heat_draw_u8(dev(frame), state, A, rgb=rgb).cpu().numpy()
            want = ref.draw(frame, A, rgb=rgb)
            assert np.array_equal(got, want), (A, rgb)
            assert np.array_equal(got[ref.map == 0], frame[ref.map == 0])    # a == 0: the byte is what it was
    assert (ref.draw(frame, 255) != frame).any()
    cold = ops.heat_state(h, w)                                              # peak == 0: the frame is untouched
    assert np.array_equal(ops.heat_draw_u8(dev(frame), cold, 255).cpu().numpy(), frame)


def test_a_frame_that_is_not_real_writes_no_word():
    from faster_rcnn_amd import ops
    h, w = 17, 70
    table = dev(TABLE)
    ref = R.Heat(h, w).update(R.make_packed(8, [[5, 5, 60, 12]]), TABLE)
    state = buffer_of(ref, h, w)
    state[4 + h * w:] = 12345                                                # (the scratch words too: nothing of the buffer is written)
    before = state.cpu().numpy().copy()
    buf = dev(R.make_packed(300, [[0, 0, w - 1, h - 1]]))
    word = lambda v: dev(np.array([v], dtype=np.int32))
    for f, nf, gate in ((1, 1, None), (0, 0, None), (0, -1, None), (5, 5, None), (0, 3, 0), (2, 3, 0)):
        ops.heat_update(state, h, w, buf, table, 1, f, word(nf), gate=None if gate is None else word(gate))
        assert np.array_equal(state.cpu().numpy(), before), (f, nf, gate)
    ops.heat_update(state, h, w, buf, table, 1, 4, word(5), gate=word(-1))    # the last real frame of five, behind an open gate
    ref.update(R.make_packed(300, [[0, 0, w - 1, h - 1]]), TABLE, 1)
    assert np.array_equal(state_of(state, h, w), ref.words()) and ref.frames == 2


def test_both_calls_captured_and_replayed():
    """One graph: update + draw.  Between replays the device words (n_frames, gate), the boxes and the frame change."""
    from faster_rcnn_amd import ops
    h, w = 33, 257
    table, state = dev(TABLE), ops.heat_state(h, w)
    src = noise(h, w, 6)
    frame, buf = dev(src), dev(R.make_packed(300, []))
    n_frames, gate = dev(np.array([0], dtype=np.int32)), dev(np.array([1], dtype=np.int32))

    def run():
        ops.heat_update(state, h, w, buf, table, 1, 1, n_frames, gate=gate)
        ops.heat_draw_u8(frame, state, 200, rgb=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                               # (n_frames is 0: the warm-up leaves the state alone)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    ref = R.Heat(h, w)
    steps = [(2, 1, [[0, 0, 100, 20]]), (1, 1, [[3, 3, 9, 9]]), (2, 0, [[3, 3, 9, 9]]), (7, -3, [[90, 10, 300, 40], [60, 0, 70, 32]]), (2, 1, [])]
    for k, (nf, g, boxes) in enumerate(steps):
        packed = R.make_packed(300, boxes)
        buf.copy_(dev(packed))
        n_frames.fill_(nf)
        gate.fill_(g)
        frame.copy_(dev(src))
        graph.replay()
        ref.update(packed, TABLE, 1, frame_index=1, n_frames=nf, gate=g)
        assert np.array_equal(state_of(state, h, w), ref.words()), k
        assert np.array_equal(frame.cpu().numpy(), ref.draw(src, 200, rgb=True)), k
    assert ref.frames == 3


def test_bad_arguments_are_refused_and_launch_nothing():
    from faster_rcnn_amd import _lib, ops
    lib = _lib.load()
    h, w = 12, 20
    table, state = dev(TABLE), ops.heat_state(h, w)
    ops.heat_update(state, h, w, dev(R.make_packed(8, [[1, 1, 8, 8]])), table)
    buf, one = dev(R.make_packed(8, [[0, 0, w - 1, h - 1]])), dev(np.array([1], dtype=np.int32))
    frame = dev(noise(h, w, 7))
    torch.cuda.synchronize()
    s0, f0 = state.cpu().numpy().copy(), frame.cpu().numpy().copy()
    p = lambda t: t.data_ptr()
    good = dict(state=p(state), h=h, w=w, det=p(buf), rows=8, tracked=0, table=p(table), C=4, decay=0, f=0, n=p(one), gate=None)
    call = lambda a: lib.frcnn_heat_update(a["state"], a["h"], a["w"], a["det"], a["rows"], a["tracked"], a["table"], a["C"], a["decay"], a["f"],
                                           a["n"], a["gate"], None)
    for change in (dict(state=None), dict(det=None), dict(table=None), dict(n=None), dict(h=0), dict(w=0), dict(h=32769), dict(w=32769),
                   dict(rows=0), dict(rows=MAX_ROWS + 1), dict(C=0), dict(C=257), dict(decay=-1), dict(decay=16), dict(f=-1), dict(f=65536)):
        assert call(dict(good, **change)) == E_ARG, change
    draw = dict(frame=p(frame), h=h, w=w, state=p(state), alpha=160)
    for change in (dict(frame=None), dict(state=None), dict(h=0), dict(w=32769), dict(alpha=0), dict(alpha=256), dict(alpha=-1)):
        a = dict(draw, **change)
        assert lib.frcnn_heat_draw_u8(a["frame"], a["h"], a["w"], a["state"], a["alpha"], 0, None) == E_ARG, change
    torch.cuda.synchronize()
    assert np.array_equal(state.cpu().numpy(), s0) and np.array_equal(frame.cpu().numpy(), f0)
    assert lib.frcnn_heat_state_bytes(0, 3) == 0 and lib.frcnn_heat_state_bytes(3, 32769) == 0
    with pytest.raises(_lib.FrcnnError):
        ops.heat_state(0, 5)
    with pytest.raises(_lib.FrcnnError, match="decay=16"):
        ops.heat_update(state, h, w, buf, table, 16)
    with pytest.raises(_lib.FrcnnError, match="alpha=0"):
        ops.heat_draw_u8(frame, state, 0)
    assert call(good) == 0                                                   # (the call they were all derived from is good)
    torch.cuda.synchronize()
    assert int(state[0]) == 2
