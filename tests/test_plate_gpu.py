"""The plate kernels (csrc/plate.hip) against tests/plate_ref.py, bit for bit: the state proper (the scratch words behind it belong to
no rule) and the frame.  The kernels do not know the channel order: the plate is kept in the frame's bytes as they lie."""
import numpy as np
import pytest
import torch

from tests import plate_ref as R

pytestmark = pytest.mark.gpu

E_ARG = -1                                                                   # FRCNN_E_ARG
MAX_ROWS = 512                                                               # FRCNN_REDACT_MAX_ROWS
TABLE = np.array([0, 1, 1, 0], dtype=np.uint8)                               # classes 1 and 2 fill; 0 and 3 do not, nor a class outside
# (h, w): one pixel, exactly one update tile (128 x 8), one more row, one more column (odd width: the runs of every other row start on
# an odd pixel, and rows start at any byte), several tiles of both kernels with a ragged edge
SIZES = [(1, 1), (8, 128), (9, 128), (8, 129), (37, 130)]
PARAMS = [(1, 0, 0), (255, 255, 64), (3, 10, 8)]                             # (S, T, M)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def noise(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def random_state(h, w, seed):
    """Any state an update can leave: random plate and candidate, V 0 or 1, runs of every length."""
    rng = np.random.default_rng(seed)
    s = R.empty(h, w)
    R.pack(s, h, w, rng.integers(0, 256, (h, w, 3)), rng.integers(0, 2, (h, w)), rng.integers(0, 256, (h, w, 3)),
           rng.choice([0, 1, 2, 7, 254, 255], (h, w)))
    s[0], s[1] = 41, R.known(s, h, w)
    return s


def buffer_of(ref, h, w):
    """A device buffer that holds the reference state, its scratch words made garbage."""
    from faster_rcnn_amd import ops
    t = ops.plate_state(h, w)
    t[:ref.size] = dev(ref)
    t[ref.size:] = -7
    return t


def state_of(t, h, w):
    return t[:4 + 2 * h * w].cpu().numpy()


def box_sets(h, w):
    """(name, buffer, rows, tracked)."""
    rng = np.random.default_rng(h * 1000 + w)

    def some(n, far=8):
        x, y = rng.integers(-far, w + far, (n, 2)), rng.integers(-far, h + far, (n, 2))
        return [(int(x[i, 0]), int(y[i, 0]), int(x[i, 1]), int(y[i, 1]), int(rng.integers(-1, 6))) for i in range(n)]      # reversed ones among them

    edge = [(w - 1, h - 1, w + 50, h + 90, 1), (-60, -60, 0, 0, 2), (w // 2, -9, w // 2, 10 ** 9, 1), (-2 ** 31, h // 2, 2 ** 31 - 1, h // 2, 5),
            (w + 3, 0, w + 70, h, 1), (-70, 0, -5, h, 2), (w + 65, 0, w + 70, 0, 1), (3, 3, 3, 3, 3)]      # crossing, pushed in by a margin, never in
    # many rows, few of which meet a frame this small: those in round two must still arrive
    far = [(10 ** 6 + i, 10 ** 6, 10 ** 6 + i + 5, 10 ** 6 + 5, 1) for i in range(255)] + some(2, 0)
    full = [(-5 * w, -5 * h, -4 * w - 70, -4 * h - 70, 1)] * 500 + some(12, 0)
    return [("none", R.packed(8, []), 8, False),
            ("one", R.packed(1, [(w // 3, h // 3, w // 2, h // 2, 2)]), 1, False),
            ("edges", R.packed(16, edge), 16, False),
            ("two rounds", R.packed(300, far), 300, False),
            ("all rows", R.tracked(MAX_ROWS, full, n_live=3), MAX_ROWS, True),
            ("tracked, held rows", R.tracked(40, some(9, 3), n_live=4), 40, True),            # rows 4..8 are held: they block and fill
            ("widened", R.tracked(200, some(5, 3) + edge, n_live=0), 200, True),
            ("count over the rows", R.tracked(3, some(3, 0) + some(4, 0)), 3, True)]      # n_rows says 7: clamped to 3


@pytest.mark.parametrize("h,w", SIZES)
def test_every_box_set_at_every_setting(h, w):
    """One update and one fill from a random state, for every kind of buffer and every corner of the parameters."""
    from faster_rcnn_amd import ops
    table = dev(TABLE)
    for k, (name, buf, rows, tracked) in enumerate(box_sets(h, w)):
        for S, T, M in PARAMS:
            ref = random_state(h, w, k)
            state = buffer_of(ref, h, w)
            src = noise(h, w, k)
            # half of the pixels near their candidate, so that runs go on as well as start over
            near = R.unpack(ref, h, w)[2] + np.random.default_rng(k).integers(-12, 13, (h, w, 3))
            src = np.where(np.random.default_rng(k + 1).integers(0, 2, (h, w, 1)) == 1, np.clip(near, 0, 255), src).astype(np.uint8)
            ops.plate_update(state, dev(src), dev(buf), S, T, M, tracked=tracked)
            R.update(ref, src, buf, rows, S, T, M)
            assert np.array_equal(state_of(state, h, w), ref), (name, S, T, M)
            for keep in (False, True):
                frame = dev(src)
                ops.plate_fill_u8(frame, state, dev(buf), table, M, keep_unknown=keep, tracked=tracked)
                want, _, _ = R.fill(src.copy(), ref, buf, rows, TABLE, M, keep)
                assert np.array_equal(frame.cpu().numpy(), want), (name, S, T, M, keep)


def sequence(h, w, n):
    """A fixed pattern with a little noise below T = 10, a bright square that moves over it, and the boxes: one on the square, class 1,
    and one that stands still, class 3 (blocks for ever, never fills), in tracked buffers; in the odd frames the square's row is HELD."""
    rng = np.random.default_rng(5)
    pattern = rng.integers(20, 200, (h, w, 3))
    frames, bufs = [], []
    for f in range(n):
        img = pattern + rng.integers(-4, 5, (h, w, 3))                      # at most 8 apart: within T of any anchor
        x0, y0 = 4 + 6 * f, 5 + f
        img[y0:y0 + 12, x0:x0 + 12] = 250
        frames.append(img.astype(np.uint8))
        still = (w - 20, 2, w - 12, 9, 3)
        square = (x0, y0, x0 + 11, y0 + 11, 1)
        bufs.append(R.tracked(24, [still, square], n_live=2 if f % 2 == 0 else 1))
    return frames, bufs


def test_a_sequence_with_a_moving_square():
    from faster_rcnn_amd import ops
    h, w, n, S, T, M = 37, 130, 12, 4, 10, 2
    frames, bufs = sequence(h, w, n)
    ref, state, table = R.empty(h, w), ops.plate_state(h, w), dev(TABLE)
    filled = unknown = 0
    for f in range(n):
        ops.plate_update(state, dev(frames[f]), dev(bufs[f]), S, T, M, tracked=True)
        R.update(ref, frames[f], bufs[f], 24, S, T, M)
        assert np.array_equal(state_of(state, h, w), ref), f
        frame = dev(frames[f])
        ops.plate_fill_u8(frame, state, dev(bufs[f]), table, M, tracked=True)
        want, from_plate, left = R.fill(frames[f].copy(), ref, bufs[f], 24, TABLE, M)
        assert np.array_equal(frame.cpu().numpy(), want), f
        filled, unknown = filled + int(from_plate.sum()), unknown + int(left.sum())
        if f == n - 1:                                                      # the square is gone from where the plate is known
            assert from_plate.any() and (np.abs(want.astype(int) - frames[f])[from_plate].max() > 100)
    P, V, _, _ = R.unpack(ref, h, w)
    # no case is vacuous (checked on the reference): the plate knows something, not everything (the still box), filled both ways
    assert 0 < ref[1] < h * w and ref[0] == n and filled > 0 and unknown > 0
    assert not V[2:10, w - 20:w - 11].any()                                 # under the box that never moves nothing is ever learned
    assert (P[V != 0] < 215).all()                                          # and the square itself never entered the plate
    frames_seen, known, plate, mask = ops.plate_image(state, h, w)
    assert (frames_seen, known) == (n, int(ref[1])) and np.array_equal(mask, V != 0) and np.array_equal(plate, np.where(mask[:, :, None], P, 0))


def test_a_frame_that_is_not_real_writes_no_word_and_the_cut_word():
    from faster_rcnn_amd import ops
    h, w = 9, 131
    ref = random_state(h, w, 3)
    state = buffer_of(ref, h, w)
    before = state.cpu().numpy().copy()
    src = noise(h, w, 4)
    frame, buf = dev(src), dev(R.packed(300, [(0, 0, 40, 4, 1)]))
    word = lambda v: dev(np.array([v], dtype=np.int32))
    for f, nf, gate in ((1, 1, None), (0, 0, None), (0, -1, None), (5, 5, None), (0, 3, 0), (2, 3, 0)):
        ops.plate_update(state, frame, buf, 2, 10, 0, f, word(nf), gate=None if gate is None else word(gate), cut=word(1))
        assert np.array_equal(state.cpu().numpy(), before), (f, nf, gate)
    ops.plate_update(state, frame, buf, 2, 10, 0, 4, word(5), gate=word(-1), cut=word(0))      # the last real frame of five, no cut
    R.update(ref, src, R.packed(300, [(0, 0, 40, 4, 1)]), 300, 2, 10, 0)
    assert np.array_equal(state_of(state, h, w), ref) and ref[0] == 42
    for S in (1, 2):                                                        # a cut: the old plate is gone in the same launch
        ops.plate_update(state, frame, buf, S, 10, 0, 0, word(1), cut=word(-9))
        R.update(ref, src, R.packed(300, [(0, 0, 40, 4, 1)]), 300, S, 10, 0, cut=-9)
        assert np.array_equal(state_of(state, h, w), ref)
        assert ref[1] == (h * w - 41 * 5 if S == 1 else 0)


def test_both_calls_captured_and_replayed():
    """One graph: update + fill.  Between replays the device words (n_frames, gate, cut), the boxes and the frame change."""
    from faster_rcnn_amd import ops
    h, w, S, T, M = 33, 257, 2, 10, 3
    table, state = dev(TABLE), ops.plate_state(h, w)
    base = noise(h, w, 6)
    frame, buf = dev(base), dev(R.packed(300, []))
    n_frames, gate, cut = (dev(np.array([v], dtype=np.int32)) for v in (0, 1, 0))

    def run():
        ops.plate_update(state, frame, buf, S, T, M, 1, n_frames, gate=gate, cut=cut)
        ops.plate_fill_u8(frame, state, buf, table, M)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                               # (n_frames is 0: the warm-up leaves the state alone)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    ref = R.empty(h, w)
    steps = [(2, 1, 0, [(0, 0, 100, 20, 1)]), (2, 1, 0, [(3, 3, 9, 9, 2)]), (2, 0, 0, [(3, 3, 9, 9, 1)]), (7, -3, 0, [(90, 10, 300, 40, 1), (60, 0, 70, 32, 0)]),
             (1, 1, 1, []), (2, 1, 1, [(0, 0, 100, 32, 2)]), (2, 1, 0, [(200, 5, 150, 30, 2)])]
    for k, (nf, g, c, boxes) in enumerate(steps):
        packed = R.packed(300, boxes)
        src = np.clip(base.astype(int) + (k % 3), 0, 255).astype(np.uint8)
        buf.copy_(dev(packed))
        n_frames.fill_(nf)
        gate.fill_(g)
        cut.fill_(c)
        frame.copy_(dev(src))
        graph.replay()
        R.update(ref, src, packed, 300, S, T, M, frame_index=1, n_frames=nf, gate=g, cut=c)
        want, _, _ = R.fill(src.copy(), ref, packed, 300, TABLE, M)
        assert np.array_equal(state_of(state, h, w), ref), k
        assert np.array_equal(frame.cpu().numpy(), want), k
    assert ref[0] == 5 and 0 < ref[1] < h * w


def test_bad_arguments_are_refused_and_launch_nothing():
    from faster_rcnn_amd import _lib, ops
    lib = _lib.load()
    h, w = 12, 20
    table, state = dev(TABLE), ops.plate_state(h, w)
    src = noise(h, w, 7)
    frame = dev(src)
    ops.plate_update(state, frame, dev(R.packed(8, [(1, 1, 8, 8, 1)])), 1, 0, 0)
    buf, one = dev(R.packed(8, [(0, 0, w - 1, h - 1, 1)])), dev(np.array([1], dtype=np.int32))
    torch.cuda.synchronize()
    s0 = state.cpu().numpy().copy()
    p = lambda t: t.data_ptr()
    good = dict(state=p(state), h=h, w=w, frame=p(frame), det=p(buf), rows=8, M=0, S=1, T=0, f=0, n=p(one), gate=None, cut=None)
    call = lambda a: lib.frcnn_plate_update(a["state"], a["h"], a["w"], a["frame"], a["det"], a["rows"], 0, a["M"], a["S"], a["T"], a["f"], a["n"],
                                            a["gate"], a["cut"], None)
    for change in (dict(state=None), dict(frame=None), dict(det=None), dict(n=None), dict(state=p(state) + 4), dict(h=0), dict(w=0),
                   dict(h=32769), dict(w=32769), dict(rows=0), dict(rows=MAX_ROWS + 1), dict(M=-1), dict(M=65), dict(S=0), dict(S=256),
                   dict(T=-1), dict(T=256), dict(f=-1), dict(f=65536)):
        assert call(dict(good, **change)) == E_ARG, change
    fill = dict(frame=p(frame), h=h, w=w, state=p(state), det=p(buf), rows=8, table=p(table), C=4, M=0, keep=0)
    fcall = lambda a: lib.frcnn_plate_fill_u8(a["frame"], a["h"], a["w"], a["state"], a["det"], a["rows"], 0, a["table"], a["C"], a["M"],
                                              a["keep"], None)
    for change in (dict(frame=None), dict(state=None), dict(det=None), dict(table=None), dict(h=0), dict(w=32769), dict(rows=0),
                   dict(rows=MAX_ROWS + 1), dict(C=0), dict(C=257), dict(M=-1), dict(M=65), dict(keep=2), dict(keep=-1)):
        assert fcall(dict(fill, **change)) == E_ARG, change
    torch.cuda.synchronize()
    assert np.array_equal(state.cpu().numpy(), s0) and np.array_equal(frame.cpu().numpy(), src)
    assert lib.frcnn_plate_state_bytes(0, 3) == 0 and lib.frcnn_plate_state_bytes(3, 32769) == 0
    with pytest.raises(_lib.FrcnnError):
        ops.plate_state(0, 5)
    with pytest.raises(_lib.FrcnnError, match="settle=256"):
        ops.plate_update(state, frame, buf, 256)
    with pytest.raises(_lib.FrcnnError, match="margin=65"):
        ops.plate_fill_u8(frame, state, buf, table, 65)
    assert call(good) == 0 and fcall(fill) == 0                              # (the calls they were all derived from are good)
    torch.cuda.synchronize()
    assert int(state[0]) == 2 and not np.array_equal(frame.cpu().numpy(), src)
