"""The re-identify kernels (csrc/track_reid.hip) against tests/track_reid_ref.py: every word of the state, the out buffers, the lists and
the workspace.  The rule is integer: there is no tolerance."""
import numpy as np
import pytest
import torch

from tests import track_reid_ref as ref

pytestmark = pytest.mark.gpu

CLASSES = np.array([0, 1, 1, 0], dtype=np.uint8)        # classes 1 and 2 are tracked; 0 and 3 are not, nor a class outside
SIZES = [(48, 64), (40, 200)]
FILL = -3                                               # what the workspace holds before a call: the words a call leaves alone stay


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def call(state, capacity, frames, tracked, n_frames, pct, keep, rgb, cuts=None):
    """One call on the device and in the reference, from the same state and workspace -> the device's state as a host array, after
    every word of both sides was compared."""
    from faster_rcnn_amd import ops
    F, R = tracked.shape[0], (tracked.shape[1] - 4) // 8
    h, w = frames.shape[1:3]
    d_state = dev(state)
    ws = ops.track_reid_workspace(F, R)
    ws[0].fill_(FILL)
    ws[1].fill_(FILL)
    ws[2].fill_(FILL)
    out, lists = ops.track_reid_update(d_state, dev(frames), 3 * h * w, dev(tracked), dev(np.array([n_frames], dtype=np.int32)), dev(CLASSES), h, w,
                                       pct, keep, rgb=rgb, cuts=None if cuts is None else dev(np.asarray(cuts, dtype=np.int32)),
                                       capacity=capacity, workspace=ws)
    torch.cuda.synchronize()
    want = ref.update(state, capacity, frames, tracked, n_frames, CLASSES, pct, keep, rgb, cuts,
                      ws=np.full((F, R, ref.WS_WORDS), FILL, dtype=np.int32))
    got = (d_state.cpu().numpy(), out.cpu().numpy(), lists.cpu().numpy(), ws[0].cpu().numpy())
    for name, g, e in zip(("state", "out", "lists", "workspace"), got, want):
        assert g.shape == e.shape and np.array_equal(g, e), "%s differs at words %s" % (name, np.argwhere(g != e)[:8].tolist())
    return got


def picture(h, w, seed):
    """Random bytes with flat patches."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    f[4:20, 8:30] = (200, 30, 90)
    f[h - 12:, w - 20:] = (10, 250, 130)
    return f


def edge_boxes(h, w):
    return [(3, 3, 7, 5),                   # 5 x 3: exactly 15 samples, no signature
            (3, 3, 6, 6),                   # 4 x 4: exactly 16
            (5, 9, 30, 9),                  # one pixel high: a single row, band 0
            (2, 2, 41, 20),                 # 40 wide: sx = 2
            (-10, 1, w + 9, 10),            # wider than the frame (and on the 200 frame wider than 64): clipped, sx = 2 or 7
            (70, 3, 139, 13),               # 70 wide where the frame has it; outside the 64 frame altogether
            (-5, -5, 9, 9), (w - 9, h - 9, w + 5, h + 5), (-7, 20, 5, 30), (20, h - 4, 33, h + 20),      # crossing each border
            (30, 4, 12, 30),                # x1 > x2
            (10, 10, 25, 19),               # 10 rows: not a multiple of 3
            (w + 5, 0, w + 30, 20)]         # never in the frame


@pytest.mark.parametrize("hw", SIZES)
def test_signatures_and_first_bindings(hw):
    h, w = hw
    boxes = edge_boxes(h, w)
    live = []
    for k, b in enumerate(boxes):
        live.append((b, 1 + k % 2, k + 1))
        if k % 3 == 0:
            live.append((b, 1, 0))                                          # an untracked row (id 0) ...
        if k % 4 == 0:
            live.append((b, (0, 3, 4, -1)[k // 4 % 4], 100 + k))            # ... and an id of a class that is not tracked
    held = [((4, 4, 30, 30), 1, 90), ((1, 1, 2, 2), 2, 91)]
    R = len(live) + len(held) + 3
    tracked = ref.pack(R, live, held)[None]
    f = picture(h, w, 1)[None]
    got = {}
    for rgb in (True, False):
        # the same pixels in the other byte order give the same signatures, and with them the same everything
        got[rgb] = call(ref.new_state(64), 64, f if rgb else np.ascontiguousarray(f[..., ::-1]), tracked, 1, 25, 250, rgb)
    for a, b in zip(got[True], got[False]):
        assert np.array_equal(a, b)
    ws = got[True][3][0]
    has = {boxes.index(b): int(ws[r, 0]) for r, (b, c, i) in enumerate(live) if 1 <= i < 100}
    assert has[0] == 0 and has[1] == 1 and has[2] == 1 and has[12] == 0 and has[5] == (1 if w >= 140 else 0)
    assert got[True][1].tobytes() == tracked.tobytes()                      # CONSEQUENCE: first bindings change no byte


def sequence(h, w, seed, steps, n_looks=5, R=12):
    """Objects of a few looks come and go -> (frames (steps, h, w, 3), tracked (steps, 4 + 8R), cuts).  A look is a colour next to the bin
    edges plus fresh noise in every frame, so signatures of one look differ a little from frame to frame and those of two looks may be
    near; ids are drawn without order (inserts in the middle of the table) and never used twice; rows are held for a frame when they leave."""
    rng = np.random.default_rng(seed)
    looks = rng.choice([60, 124, 188], size=(n_looks, 3))
    spots = [(4 + 30 * (k % (w // 30)), 3 + 18 * (k // (w // 30))) for k in range(n_looks)]
    sizes = [(int(rng.integers(6, 27)), int(rng.integers(4, 15))) for _ in range(n_looks)]
    free_ids = list(rng.permutation(np.arange(1, 400)))
    alive, frames, bufs, cuts = {}, [], [], []
    for _ in range(steps):
        held = []
        for k in range(n_looks):
            if k in alive and rng.random() < 0.3:
                held.append(k)
            elif k not in alive and rng.random() < 0.5:
                alive[k] = int(free_ids.pop())
        f = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        rows = {}
        for k in alive:
            (x, y), (bw, bh) = spots[k], sizes[k]
            if k not in held:
                patch = f[y:y + bh, x:x + bw]                              # (a box may reach over the frame's edge)
                patch[:] = np.clip(looks[k] + rng.integers(-1, 9, size=patch.shape), 0, 255)
            rows[k] = ((x, y, x + bw - 1, y + bh - 1), 1 + k % 2, alive[k])
        live = [rows[k] for k in sorted(alive) if k not in held]
        live.insert(len(live) // 2, ((0, 0, 20, 20), 1, 0))
        bufs.append(ref.pack(R, live, [rows[k] for k in held]))
        frames.append(f)
        cuts.append(int(rng.random() < 0.08))
        for k in held:
            del alive[k]
    return np.stack(frames), np.stack(bufs), np.array(cuts, dtype=np.int32)


@pytest.mark.parametrize("hw,capacity,keep,with_cuts", [((48, 64), 256, 250, False), ((40, 200), 256, 3, True), ((48, 64), 1, 250, False),
                                                        ((40, 200), 3, 2, False)])
def test_sequences(hw, capacity, keep, with_cuts):
    h, w = hw
    frames, tracked, cuts = sequence(h, w, seed=h + capacity, steps=24)
    state, at, reid = ref.new_state(capacity), 0, 0
    # calls of one frame, of three, of three of which two are real and of three of which none is: the state is untouched
    for F, nf in [(1, 1), (3, 3), (1, 1), (3, 2), (3, 0), (3, 3), (1, 1), (3, 3), (3, 2), (1, 1), (3, 3)]:
        before = state.copy()
        got = call(state, capacity, frames[at:at + F], tracked[at:at + F], nf, 40, keep, bool(at % 2), cuts[at:at + F] if with_cuts else None)
        state = got[0]
        if nf == 0:
            assert np.array_equal(state, before) and np.array_equal(got[1], tracked[at:at + F]) and not got[2].any()
        at += nf
    assert state[1] == at
    if capacity == 256:
        assert state[3] > 0                                                 # (the case is worth something: ids came back)
    if capacity <= 3:
        assert state[2] > 0                                                 # ... and a small table dropped rows


def flat(h, w, patches):
    f = np.zeros((h, w, 3), dtype=np.uint8)
    for (x1, y1, x2, y2), colour in patches:
        f[y1:y2 + 1, x1:x2 + 1] = colour
    return f


def test_hand_cases():
    """The edges of the rule with flat colours: a held tid is no candidate, two returns share no entry, equal distances go to the lowest
    pid, and the pct boundary (tests/test_track_reid_cpu.py works the numbers out)."""
    h, w, R = 48, 64, 6
    A, B, RED = (8, 8, 23, 23), (40, 24, 55, 39), (255, 0, 0)
    both, none = flat(h, w, [(A, RED), (B, RED)]), flat(h, w, [])
    one = lambda live, held=(): ref.pack(R, live, held)

    def play(steps, pct=25):
        frames, tracked = np.stack([s[0] for s in steps]), np.stack([s[1] for s in steps])
        return call(ref.new_state(8), 8, frames, tracked, len(steps), pct, 250, True)

    state, out, lists, _ = play([(both, one([(A, 1, 1)])), (both, one([(B, 1, 2)], [(A, 1, 1)]))])
    assert out[1, 4 + 6 * R:6 + 6 * R].tolist() == [2, 1] and state[3] == 0
    state, out, lists, _ = play([(both, one([(A, 1, 1)])), (none, one([])), (both, one([(A, 1, 2), (B, 1, 3)]))])
    assert out[2, 4 + 6 * R:6 + 6 * R].tolist() == [1, 3] and ref.events(lists[2]) == [(1, 2, 1, 0, 2)]
    state, out, lists, _ = play([(both, one([(A, 1, 1), (B, 1, 2)])), (none, one([])), (both, one([(B, 1, 3)]))])
    assert out[2, 4 + 6 * R] == 1 and ref.events(lists[2]) == [(1, 3, 1, 0, 2)]
    for k, taken in ((64, True), (65, False)):
        part = flat(h, w, [(A, RED)])
        part[8:8 + 5, 8:24][np.arange(80).reshape(5, 16) < k] = 0           # the first k samples are black
        state, out, lists, _ = play([(both, one([(A, 1, 1)])), (none, one([])), (part, one([(A, 1, 2)]))])
        assert (out[2, 4 + 6 * R] == 1) == taken and (ref.events(lists[2]) == [(1, 2, 1, 32 * k, 2)]) == taken


def test_33_events_in_a_frame():
    h, w, n = 40, 200, 34
    boxes = [(2 + 11 * (k % 17), 2 + 12 * (k // 17), 6 + 11 * (k % 17), 5 + 12 * (k // 17)) for k in range(n)]      # 5 x 4: 20 samples
    f = flat(h, w, [(b, (32 + 64 * (k % 4), 32 + 64 * (k // 4 % 4), 32 + 64 * (k // 16))) for k, b in enumerate(boxes)])
    R = n + 2
    tracked = np.stack([ref.pack(R, [(b, 1, k + 1) for k, b in enumerate(boxes)]), ref.pack(R, []),
                        ref.pack(R, [(b, 1, 50 + k) for k, b in enumerate(boxes)])])
    state, out, lists, _ = call(ref.new_state(256), 256, np.stack([f, flat(h, w, []), f]), tracked, 3, 1, 250, False)
    assert state[3] == n and lists[2, 0] == 32 and state[0] == n
    assert out[2, 4 + 6 * R:4 + 6 * R + n].tolist() == list(range(1, n + 1))


def test_refusals():
    from faster_rcnn_amd import ops
    from faster_rcnn_amd._lib import FrcnnError
    h, w, R = 8, 8, 2
    args = lambda: (ops.track_reid_state(4), dev(np.zeros((1, h, w, 3), dtype=np.uint8)), 3 * h * w, dev(ref.pack(R, [])[None]),
                    dev(np.ones(1, dtype=np.int32)), dev(CLASSES), h, w)
    for kw in ({"pct": 0}, {"pct": 101}, {"keep": 0}, {"keep": 4096}):
        with pytest.raises(FrcnnError):
            ops.track_reid_update(*args(), **kw)
    with pytest.raises(FrcnnError):
        ops.track_reid_state(257)
    with pytest.raises(FrcnnError):
        ops.track_reid_workspace(65, 4)
    for bad in ((0, 250), (25, 0), (True, 250), (25.0, 250)):
        with pytest.raises(ValueError):
            ops.track_reid_option(*bad)
    assert ops.track_reid_option() == (25, 250) and ops.track_reid_option(1, 4095) == (1, 4095)
