"""ops.redact_moving_build (csrc/redact_moving.hip) against the restatement of the moving rule in tests/redact_moving_ref.py: the state,
the stats, the plane's header, W and tile flags of every frame of a sequence, byte for byte, no tolerance.  The frames are the smallest at
which the tiling can go wrong (the cell kernel's tiles are 128 x 8 pixels, the weight kernel's 256 byte columns x 16 rows): 8 x 8, one
cell; 9 x 9, one-pixel edge cells; 16 x 85, one apply tile; 17 x 86, one byte and one row over it; 37 x 45; 40 x 200, two plate tiles and
three apply tile columns; 75 x 130 with G + F = 64, whose reach crosses the whole frame.  A sequence is six frames: two that settle the
plate (S = 2), motion, a still frame that the hold hides, a cut, and a frame that is not real.  State and plane are views inside larger
buffers whose bytes before and behind them must survive."""
import functools

import numpy as np
import pytest

from tests import plate_ref as P
from tests import redact_moving_ref as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xA5
PAD = 64                                                                    # (state and plane are 16-byte aligned)
SETTLE, PLATE_TOL = 2, 10
# (h, w, G, F, K, H)
CASES = [(8, 8, 0, 0, 8, 1), (9, 9, 1, 2, 64, 1), (16, 85, 8, 0, 8, 2), (17, 86, 3, 8, 8, 1), (37, 45, 8, 4, 8, 1), (40, 200, 8, 0, 8, 2),
         (40, 200, 0, 32, 1, 0), (75, 130, 32, 32, 8, 1)]


def _ops():
    from faster_rcnn_amd import ops
    return ops


def guarded(nbytes):
    buf = torch.full((PAD + nbytes + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    view = buf[PAD:PAD + nbytes]
    view.zero_()
    return buf, view


def intact(buf):
    host = buf.cpu().numpy()
    return (host[:PAD] == SENTINEL).all() and (host[-PAD:] == SENTINEL).all()


@functools.lru_cache(maxsize=None)
def sequence(h, w):
    """Six frames of (h, w): a noise background twice, a block and two single pixels that differ, the background, the background under a
    cut, the block once more (not real)."""
    rs = np.random.RandomState(31 * h + w)
    back = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    moved = back.copy()
    y, x = h // 3, w // 2
    moved[y:y + 11, x:x + 13] = rs.randint(0, 256, moved[y:y + 11, x:x + 13].shape)
    moved[h - 1, w - 1] ^= 0x80                                             # the corner cell: one pixel
    moved[0, 0, 1] ^= 0x40
    frames = [back, back, moved, back, back, moved]
    for f in frames:
        f.setflags(write=False)
    return frames


def boxes(h, w, n):
    """n EXCEPT candidates: the first covers the moved block, others cross every border, the rest are scattered small boxes."""
    rs = np.random.RandomState(n)
    out = [(w // 2 - 2, h // 3 - 2, w // 2 + 20, h // 3 + 6, 1), (-9, -9, 3, 3, 2), (w - 3, h - 3, w + 40, h + 40, 1), (5, 2, 1, 9, 3)]
    while len(out) < n:
        x, y = int(rs.randint(-8, w)), int(rs.randint(-8, h))
        out.append((x, y, x + int(rs.randint(0, 6)), y + int(rs.randint(0, 6)), int(rs.randint(0, 5))))
    return out[:n]


def run_sequence(h, w, G, F, K, H, unknown=0, dets=(), tracked=False, rows=4, table=(0, 0, 0, 0), margin=2, tol=24):
    """The sequence on the device and in the restatement, compared frame by frame."""
    ops = _ops()
    option = (tol, K, H, G, F, unknown, (), "fill", 0, SETTLE, PLATE_TOL, margin)
    det_host = (P.tracked if tracked else P.packed)(rows, list(dets))
    det = torch.from_numpy(det_host).cuda()
    table_host = np.array(table, dtype=np.uint8)
    table_dev = torch.from_numpy(table_host).cuda()
    plate = ops.plate_state(h, w)
    sbuf, state = guarded(ops.redact_moving_state_bytes(h, w))
    pbuf, plane = guarded(ops.redact_region_plane_bytes(h, w))
    stats = torch.full((6, 4), -7, dtype=torch.int32, device="cuda")
    n_frames = torch.tensor([5], dtype=torch.int32, device="cuda")         # (frame 5 is not real)
    cuts = torch.tensor([0, 0, 0, 0, 1, 1], dtype=torch.int32, device="cuda")
    ref_plate, ref_state = P.empty(h, w), M.empty(h, w)
    tiles = (-(-h // 16), -(-3 * w // 256))
    last_W = np.zeros((h, w), dtype=np.int64)
    seen = []
    for i, frame in enumerate(sequence(h, w)):
        fdev = torch.from_numpy(np.array(frame)).cuda()
        ops.plate_update(plate, fdev, det, SETTLE, PLATE_TOL, margin, i, n_frames, cut=cuts[i:i + 1], tracked=tracked)
        ops.redact_moving_build(state, plane, stats[i], fdev, plate, det, table_dev, option, i, n_frames, cut=cuts[i:i + 1], tracked=tracked)
        P.update(ref_plate, frame, det_host, rows, SETTLE, PLATE_TOL, margin, i, 5, cut=int(cuts[i]))
        want = M.build(ref_state, frame, ref_plate, det_host, rows, table_host, margin, tol, K, H, G, F, unknown, i, 5, cut=int(cuts[i]))
        frames, cells_now, left = ops.redact_moving_left(state, h, w)
        assert (frames, cells_now) == (ref_state[0], ref_state[1]), i
        assert np.array_equal(left, ref_state[2]), i
        assert stats[i].cpu().tolist() == want["stats"], (i, stats[i].cpu().tolist(), want["stats"])
        host = plane.cpu().numpy()
        assert host[:32].view(np.int32).tolist() == want["header"], i
        if want["real"]:
            last_W = want["W"]
        assert np.array_equal(ops.redact_region_weights(host), last_W), i    # (a frame that is not real leaves W as it was)
        at = (32 + 2 * h * w + 15) // 16 * 16
        assert np.array_equal(host[at:at + tiles[0] * tiles[1]].reshape(tiles), want["flags"]), i
        seen.append(want)
    assert intact(sbuf) and intact(pbuf)
    return seen, (state, plane, plate, det, table_dev, option)


@pytest.mark.parametrize("h,w,G,F,K,H", CASES)
def test_sequence_matches_restatement(h, w, G, F, K, H):
    seen, _ = run_sequence(h, w, G, F, K, H)
    assert [s["real"] for s in seen] == [True] * 5 + [False]
    assert seen[2]["stats"][1] > 0 and seen[4]["stats"][1] == 0           # motion was seen; the cut emptied holds and plate
    if H > 0:
        assert seen[3]["stats"][1] > 0                                      # ... and the hold hid the still frame behind it


@pytest.mark.parametrize("unknown", [0, 1])
def test_unknown_shows_or_hides(unknown):
    seen, _ = run_sequence(37, 45, 2, 2, 8, 1, unknown=unknown)
    cells = M.cells(37, 45)
    assert seen[0]["stats"][1] == (cells[0] * cells[1] if unknown else 0)
    assert seen[4]["stats"][1] == (cells[0] * cells[1] if unknown else 0)  # (the cut emptied the plate: nothing is known again)


@pytest.mark.parametrize("n,tracked", [(0, False), (1, False), (1, True), (300, False), (300, True)])
def test_except_boxes(n, tracked):
    h, w = 40, 200
    seen, _ = run_sequence(h, w, 4, 4, 4, 1, dets=boxes(h, w, n), tracked=tracked, rows=max(n, 4), table=(0, 1, 1, 0, 0), margin=3)
    plain, _ = run_sequence(h, w, 4, 4, 4, 1) if n == 1 and not tracked else (None, None)
    if plain is not None:                                                   # the box over the block took cells away
        assert seen[2]["stats"][1] < plain[2]["stats"][1]


def test_plane_equals_region_build_of_dilated_mask():
    ops = _ops()
    h, w, G, F = 37, 45, 5, 7
    seen, (state, plane, *_) = run_sequence(h, w, G, F, 8, 3)
    # the plane as the sequence left it: frame 4's (the cut: empty).  One more real frame with motion
    _, plane2 = guarded(ops.redact_region_plane_bytes(h, w))
    mask = M.dilated_mask(seen[2]["moving"], h, w, G)
    region = ops.redact_region_plane(h, w, ops.redact_region_option(None, mask, "fill", None, F))
    # replay frames 0..2 into a fresh state to get frame 2's plane on the device
    fresh = ops.redact_moving_state(h, w)
    plate = ops.plate_state(h, w)
    det = torch.from_numpy(P.packed(4, [])).cuda()
    table = torch.zeros(4, dtype=torch.uint8, device="cuda")
    stats = torch.zeros(4, dtype=torch.int32, device="cuda")
    option = (24, 8, 3, G, F, 0, (), "fill", 0, SETTLE, PLATE_TOL, 2)
    for i, frame in enumerate(sequence(h, w)[:3]):
        fdev = torch.from_numpy(np.array(frame)).cuda()
        ops.plate_update(plate, fdev, det, SETTLE, PLATE_TOL, 2, 0)
        ops.redact_moving_build(fresh, plane2, stats, fdev, plate, det, table, option)
    assert ops.redact_region_stats(plane2) == ops.redact_region_stats(region)
    assert np.array_equal(ops.redact_region_weights(plane2), ops.redact_region_weights(region))
    a, b = plane2.cpu().numpy(), region.cpu().numpy()
    at = (32 + 2 * h * w + 15) // 16 * 16
    n = -(-h // 16) * -(-3 * w // 256)
    assert np.array_equal(a[:at + n], b[:at + n])                           # header, W and every tile flag
    got = ops.redact_moving_stats(stats)
    assert (got["covered"], got["full"]) == (ops.redact_region_stats(region)["covered"], ops.redact_region_stats(region)["full"])


def test_refusals_launch_nothing():
    ops = _ops()
    from faster_rcnn_amd._lib import FrcnnError
    h, w = 16, 85
    plate = ops.plate_state(h, w)
    sbuf, state = guarded(ops.redact_moving_state_bytes(h, w))
    pbuf, plane = guarded(ops.redact_region_plane_bytes(h, w))
    state.fill_(SENTINEL), plane.fill_(SENTINEL)
    stats = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    frame = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    det = torch.from_numpy(P.packed(4, [])).cuda()
    table = torch.zeros(4, dtype=torch.uint8, device="cuda")
    good = [24, 8, 4, 8, 0, 0, (), "fill", 0, 8, 10, 8]
    bad = [(0, 256), (0, -1), (1, 0), (1, 65), (2, 256), (2, -1), (3, 33), (3, -1), (4, 33), (4, -1), (5, 2), (11, 65), (11, -1)]
    for at, value in bad:
        option = list(good)
        option[at] = value
        with pytest.raises(FrcnnError):
            ops.redact_moving_build(state, plane, stats, frame, plate, det, table, tuple(option))
    with pytest.raises(FrcnnError):
        ops.redact_moving_build(state, plane, stats, frame, plate, det, table, tuple(good), frame_index=65536)
    with pytest.raises(FrcnnError):
        ops.redact_moving_build(state, plane, stats, frame, plate, det, torch.zeros(257, dtype=torch.uint8, device="cuda"), tuple(good))
    # a state, a plane or a plate state that does not start on a 16-byte boundary (views one byte, one word into larger buffers)
    ns, np_, nw = int(state.numel()), int(plane.numel()), int(plate.numel())
    off_state = torch.full((ns + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    off_plane = torch.full((np_ + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    off_plate = torch.zeros(nw + 4, dtype=torch.int32, device="cuda")
    for st, pl, pt in ((off_state[1:1 + ns], plane, plate), (state, off_plane[8:8 + np_], plate), (state, plane, off_plate[1:1 + nw])):
        assert (st.data_ptr() | pl.data_ptr() | pt.data_ptr()) % 16 != 0
        with pytest.raises(FrcnnError) as e:
            ops.redact_moving_build(st, pl, stats, frame, pt, det, table, tuple(good))
        assert "16-byte aligned" in str(e.value)
    torch.cuda.synchronize()
    assert (off_state.cpu().numpy() == SENTINEL).all() and (off_plane.cpu().numpy() == SENTINEL).all()
    assert (state.cpu().numpy() == SENTINEL).all() and (plane.cpu().numpy() == SENTINEL).all() and stats.cpu().tolist() == [-7] * 4
    assert ops.redact_moving_state_bytes(h, w) >= 16 + 2 * 11 and ops.redact_moving_state_bytes(h, w) % 16 == 0
    with pytest.raises(FrcnnError):
        ops.redact_moving_state_bytes(0, 5)
