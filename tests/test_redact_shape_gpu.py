"""ops.redact_shaped_u8 (csrc/redact_shape.hip) against the restatement of the shape rule in tests/redact_shape_ref.py: byte for byte,
no tolerance.  The frames are the smallest that reach every tile path (tiles are 256 byte columns x 16 rows): 37 x 53 has an odd row
length, three tile rows and one tile column; 16 x 300 has 900 bytes a row, four tile columns, and boxes and rings that straddle them;
33 x 20.  Every frame is a view inside a larger buffer whose bytes before and behind it must survive, and so is the workspace."""
import functools

import numpy as np
import pytest

from tests import redact_ref as R
from tests import redact_shape_ref as RS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xA5
PAD = 67                                                                   # (odd: the frame starts at no aligned address)
FRAMES = [(37, 53), (16, 300), (33, 20)]
MODES = [("fill", 0), ("pixelate", 5), ("blur", 3)]
FEATHERS = [0, 1, 5, 32]
TABLE = np.array([1, 0, 1, 1, 0], dtype=np.uint8)                          # classes 1 and 4 are not redacted


@functools.lru_cache(maxsize=None)
def pixels(h, w):
    a = np.random.RandomState(17 * h + w).randint(0, 256, (h, w, 3)).astype(np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def replacement(h, w, mode, size):
    """R of the frame, computed once per (frame, mode) and shared."""
    a = R.replacement(pixels(h, w), mode, size)
    a.setflags(write=False)
    return a


def pack(bbox, cls, n=None, rows=512, dead_box=None, dead_cls=-1):
    """The post-process's packed buffer with ``n`` live rows; the rows behind them hold ``dead_box`` / ``dead_cls``."""
    packed = np.zeros(4 + 7 * rows, dtype=np.int32)
    packed[0] = len(cls) if n is None else n
    b = packed[4:4 + 4 * rows].reshape(rows, 4)
    c = packed[4 + 4 * rows:4 + 5 * rows]
    b[:] = (-1, -1, -1, -1) if dead_box is None else dead_box
    c[:] = dead_cls
    k = len(cls)
    b[:k] = np.asarray(bbox, dtype=np.int64).reshape(-1, 4)
    c[:k] = cls
    return packed


def unpack(packed):
    rows = (packed.size - 4) // 7
    return packed[4:4 + 4 * rows].reshape(rows, 4), packed[4 + 4 * rows:4 + 5 * rows], int(packed[0])


def padded(data):
    """``data`` (uint8 array) on the device inside a buffer of sentinel bytes -> (the buffer, the view of the data)."""
    n = data.size
    buf = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    view = buf[PAD:PAD + n].view(data.shape)
    view.copy_(torch.from_numpy(np.array(data)).cuda())                     # (a copy: ``data`` may be a shared, read-only array)
    return buf, view


def intact(buf, n):
    host = buf.cpu().numpy()
    return bool((host[:PAD] == SENTINEL).all() and (host[PAD + n:] == SENTINEL).all())


def restated(frame, packed, mode, size, margin, shape, F):
    """The rule over the shared R of the frame (tests/redact_shape_ref.py's ``redact``, with R not computed again)."""
    bbox, cls, n = unpack(packed)
    h, w = frame.shape[:2]
    W = RS.weights(h, w, bbox, cls, n, TABLE, margin, shape, F)[:, :, None]
    S, Rep = frame.astype(np.int64), replacement(h, w, mode, size).astype(np.int64)
    return np.where(W > 0, (W * Rep + (256 - W) * S + 128) >> 8, S).astype(np.uint8), W[:, :, 0]


def check(h, w, packed, mode, size, margin, shape, F):
    """ops.redact_shaped_u8 == the restatement; nothing around the frame or the workspace is written.  -> (the result, W)."""
    from faster_rcnn_amd import ops
    frame = pixels(h, w)
    fbuf, fview = padded(frame)
    need = ops.redact_ws_bytes(h, w, mode, size)
    wbuf, wview = padded(np.full(need, SENTINEL, dtype=np.uint8))
    ret = ops.redact_shaped_u8(fview, torch.from_numpy(packed).cuda(), torch.from_numpy(TABLE).cuda(), mode, size, margin, shape, F, workspace=wview)
    assert ret is fview
    got = fview.cpu().numpy()
    want, W = restated(frame, packed, mode, size, margin, shape, F)
    bad = (got != want).any(axis=2)
    assert not bad.any(), ((h, w), mode, size, margin, shape, F, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert intact(fbuf, frame.size) and intact(wbuf, need), ((h, w), mode, size)
    return got, W


def hand_rows(h, w):
    """The issue's row sets but the random and the very large ones, placed relative to the frame -> (bbox, cls)."""
    cx, cy = w // 2, h // 2
    rows = [
        ((3, 3, 3, 3), 0), ((w - 6, 2, w - 5, 2), 2),                      # a 1 x 1 box and a 2 x 1 box
        ((cx + 4, cy + 2, cx - 3, cy - 2), 0),                             # inverted corners
        ((-5, cy, 2, cy + 3), 2), ((w - 3, cy - 4, w + 6, cy), 3),         # across the left border, the right,
        ((cx - 8, -4, cx - 3, 1), 0), ((cx + 5, h - 2, cx + 9, h + 9), 2),     # the top, the bottom
        ((-14, 2, -4, h - 3), 0), ((2, h + 3, w // 3, h + 9), 3),          # wholly outside: only a ring (or a margin) reaches in
        ((3 * w // 4 - 6, 3 * h // 4 - 5, 3 * w // 4 + 5, 3 * h // 4 + 4), 0),       # two overlapping boxes of different size: the
        ((3 * w // 4 - 1, 3 * h // 4 - 1, 3 * w // 4 + 2, 3 * h // 4 + 1), 3),       # max rule
        ((0, 0, w, h), 1), ((0, 0, w, h), 5), ((0, 0, w, h), -3), ((0, 0, w, h), 1 << 20),     # a class not redacted; cls out of range
    ]
    if w > 256 // 3:                                                        # a box and a ring that straddle the tile columns (85 1/3 pixels each)
        rows += [((80, 4, 90, 9), 0), ((160, 1, 175, 14), 2), ((252, 6, 259, 8), 3)]
    return np.array([r[0] for r in rows], dtype=np.int64), np.array([r[1] for r in rows], dtype=np.int64)


# ----------------------------------------------------------------------------------------------------------- the grid
@pytest.mark.parametrize("mode,size", MODES)
@pytest.mark.parametrize("h,w", FRAMES)
def test_hand_rows(h, w, mode, size):
    bbox, cls = hand_rows(h, w)
    packed = pack(bbox, cls)
    for shape in RS.SHAPES:
        for F in FEATHERS:
            for margin in (0, 3):
                got, W = check(h, w, packed, mode, size, margin, shape, F)
                assert (W == 256).any() and (W < 256).any() and (got != pixels(h, w)).any()
                if F:
                    assert ((W > 0) & (W < 256)).any()                      # a ring there is


@pytest.mark.parametrize("h,w", FRAMES)
def test_512_rows_of_small_boxes(h, w):
    rs = np.random.RandomState(h + w)
    x, y = rs.randint(-8, w + 8, 512), rs.randint(-8, h + 8, 512)
    bbox = np.stack([x, y, x + rs.randint(-1, 7, 512), y + rs.randint(-1, 5, 512)], axis=1)
    cls = rs.randint(0, 5, 512)
    packed = pack(bbox, cls)
    for shape, F, mode, size, margin in (("ellipse", 0, "fill", 0, 0), ("ellipse", 1, "blur", 3, 0), ("ellipse", 5, "pixelate", 5, 3),
                                         ("ellipse", 32, "blur", 3, 0), ("box", 5, "blur", 3, 0), ("box", 32, "fill", 0, 3)):
        got, W = check(h, w, packed, mode, size, margin, shape, F)
        assert (W > 0).any()
    _, W = check(h, w, pack(bbox[:300], cls[:300], 300, dead_box=(0, 0, w, h), dead_cls=0), "fill", 0, 0, "ellipse", 1)      # 300 of 512: two rounds,
    assert (W == 0).any()                                                   # and nothing is read behind the live rows


@pytest.mark.parametrize("h,w", [(37, 53), (16, 300)])
def test_very_large_boxes(h, w):
    """A side of 98 001: (A + 2e)^2 (B + 2e)^2 is about 2^66 and the edge of the ellipse crosses the frame -- the 128-bit path.  A side
    above 131 072: the row counts as a box row."""
    d = 34649                                                               # 49 001.5 / sqrt(2): the circle's edge lies on the frame's middle
    x0, y0 = w // 2 + d - 49000, h // 2 + d - 49000
    circle = [[x0, y0, x0 + 98000, y0 + 98000]]
    for F in (0, 5):
        got, W = check(h, w, pack(circle, [0]), "blur", 3, 0, "ellipse", F)
        assert (W == 256).any() and (W == 0).any()
        assert not np.array_equal(W, RS.weights(h, w, circle, [0], 1, TABLE, 0, "box", F))
    flat = [[w // 2 - 2, h // 2 - 49000, w // 2 + 3, h // 2 + 49000]]      # 6 x 98 001: the sides of the ellipse cross every row
    check(h, w, pack(flat, [2]), "fill", 0, 1, "ellipse", 5)
    wide = [[-70000, h // 2 - 3, 70000, h // 2 + 2]]                        # A = 140 001
    got, W = check(h, w, pack(wide, [0]), "pixelate", 5, 0, "ellipse", 5)
    assert np.array_equal(W, RS.weights(h, w, wide, [0], 1, TABLE, 0, "box", 5)) and (W[h // 2] == 256).all()
    lim = np.iinfo(np.int32)                                                # int32 extremes in live rows: the box arithmetic must not wrap
    check(h, w, pack([[lim.min, lim.min, lim.max, lim.max], [lim.max, 0, lim.max, 5], [lim.min, 2, lim.min + 1, 5]], [1, 0, 0]), "fill", 0, 64,
          "ellipse", 32)
    check(h, w, pack([[lim.min, 2, lim.max, 3]], [0]), "blur", 3, 3, "ellipse", 5)


# ----------------------------------------------------------------------------------------------------------- identities
@pytest.mark.parametrize("mode,size", MODES)
@pytest.mark.parametrize("h,w", FRAMES)
def test_box_without_feather_is_redact_u8(h, w, mode, size):
    from faster_rcnn_amd import ops
    bbox, cls = hand_rows(h, w)
    table = torch.from_numpy(TABLE).cuda()
    for margin in (0, 3):
        packed = torch.from_numpy(pack(bbox, cls)).cuda()
        a, b = torch.from_numpy(pixels(h, w).copy()).cuda(), torch.from_numpy(pixels(h, w).copy()).cuda()
        ops.redact_u8(a, packed, table, mode, size, margin)
        ops.redact_shaped_u8(b, packed, table, mode, size, margin, "box", 0)
        assert torch.equal(a, b) and not np.array_equal(a.cpu().numpy(), pixels(h, w))
        ops.redact_shaped_u8(a.copy_(torch.from_numpy(pixels(h, w).copy()).cuda()), packed, table, mode, size, margin)      # the defaults are ("box", 0)
        assert torch.equal(a, b)


@pytest.mark.parametrize("mode,size", MODES)
def test_no_live_rows_leave_a_poisoned_frame_untouched(mode, size):
    h, w = 37, 53
    from faster_rcnn_amd import ops
    table = torch.from_numpy(TABLE).cuda()
    need = ops.redact_ws_bytes(h, w, mode, size)
    for n in (0, -3):
        packed = torch.from_numpy(pack([[0, 0, w, h]] * 4, [0] * 4, n, dead_box=(-(1 << 30), -(1 << 30), 1 << 30, 1 << 30), dead_cls=0)).cuda()
        fbuf, fview = padded(np.full((h, w, 3), 0x5C, dtype=np.uint8))
        wbuf, wview = padded(np.full(need, SENTINEL, dtype=np.uint8))
        ops.redact_shaped_u8(fview, packed, table, mode, size, 2, "ellipse", 32, workspace=wview)
        assert (fview.cpu().numpy() == 0x5C).all() and (wbuf.cpu().numpy() == SENTINEL).all() and intact(fbuf, h * w * 3)


def test_a_tracked_buffer_with_held_rows():
    """``tracked=True``: every row of a tracked buffer of ops.track_update is shaped, the held ones too."""
    from faster_rcnn_amd import ops
    h, w = 37, 53
    table = torch.from_numpy(TABLE).cuda()
    first = pack([[5, 5, 20, 14], [30, 20, 44, 33]], [0, 2], rows=64)
    second = pack([[6, 6, 21, 15]], [0], rows=64)                           # the second object is lost: its track is held
    state = ops.track_state(8)
    out = torch.zeros((1, 4 + 8 * (64 + 8)), dtype=torch.int32, device="cuda")
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    for p in (first, second):
        ops.track_update(state, torch.from_numpy(p).cuda(), one, table, h, w, 30, 8, 2, out=out)
    n, live, _, _, bbox, cls, _, _, age = [t.cpu().numpy() for t in ops.split_tracked(out[0])]
    n = int(n[0])
    assert n == 2 and int(live[0]) == 1 and age[1] > 0                     # the live row and the held one
    dev = torch.from_numpy(pixels(h, w).copy()).cuda()
    ops.redact_shaped_u8(dev, out[0], table, "blur", 3, 1, "ellipse", 5, tracked=True)
    frame = pixels(h, w)
    W = RS.weights(h, w, bbox, cls, n, TABLE, 1, "ellipse", 5)[:, :, None]
    Rep = replacement(h, w, "blur", 3).astype(np.int64)
    want = np.where(W > 0, (W * Rep + (256 - W) * frame.astype(np.int64) + 128) >> 8, frame).astype(np.uint8)
    assert np.array_equal(dev.cpu().numpy(), want)
    assert W[26, 37, 0] == 256 and W[10, 13, 0] == 256                      # both objects are hidden


# ----------------------------------------------------------------------------------------------------------- captured
@pytest.mark.parametrize("mode,size", [("pixelate", 5), ("blur", 3)])
def test_captured_and_replayed_with_other_detections(mode, size):
    from faster_rcnn_amd import ops
    h, w = 37, 53
    frame = pixels(h, w)
    table = torch.from_numpy(TABLE).cuda()
    src = torch.from_numpy(frame.copy()).cuda()
    dev = torch.empty_like(src)
    bbox, cls = hand_rows(h, w)
    packs = [pack(bbox, cls), pack([[10, 5, 40, 20], [50, 0, 99, 9]], [0, 3]), pack(bbox, cls, 0)]
    packed = torch.from_numpy(packs[0]).cuda()
    others = [torch.from_numpy(p).cuda() for p in packs]
    ws = torch.empty(ops.redact_ws_bytes(h, w, mode, size), dtype=torch.uint8, device="cuda")

    def run():
        dev.copy_(src)
        ops.redact_shaped_u8(dev, packed, table, mode, size, 1, "ellipse", 5, workspace=ws)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for k in (1, 2, 0, 1):
        packed.copy_(others[k])                                            # the detections, n_dets included, rewritten on the device
        graph.replay()
        want, W = restated(frame, packs[k], mode, size, 1, "ellipse", 5)
        assert np.array_equal(dev.cpu().numpy(), want), k
        assert (W > 0).any() == (k != 2)


# ----------------------------------------------------------------------------------------------------------- refusals
def test_bad_arguments_raise_and_launch_nothing():
    from faster_rcnn_amd import _lib, ops
    h, w = 12, 20
    frame = pixels(h, w)
    table = torch.from_numpy(TABLE).cuda()
    packed = torch.from_numpy(pack([[0, 0, w, h]], [0])).cuda()
    dev = torch.from_numpy(frame.copy()).cuda()
    for shape, feather in (("box", -1), ("box", 33), ("ellipse", 33), ("ellipse", -1), ("ellipse", 1 << 20)):
        with pytest.raises(_lib.FrcnnError) as e:
            ops.redact_shaped_u8(dev, packed, table, "fill", None, 0, shape, feather)
        assert "feather" in str(e.value)
    with pytest.raises(ValueError):
        ops.redact_shaped_u8(dev, packed, table, "fill", None, 0, "circle", 0)
    lib = _lib.load()
    args = lambda shape, feather: (dev.data_ptr(), h, w, packed[4:].data_ptr(), packed[4 + 4 * 512:].data_ptr(), packed.data_ptr(), 512,
                                   table.data_ptr(), 5, 0, 0, 0, shape, feather, None, 0, None)
    for shape in (-1, 2, 7):                                                # an unknown shape, at the C ABI itself
        assert lib.frcnn_redact_shaped_u8(*args(shape, 0)) == -1 and b"shape" in lib.frcnn_last_error()
    # everything the plain call refuses
    for mode, size in (("pixelate", 1), ("pixelate", 65), ("blur", 0), ("blur", 33), ("fill", 1)):
        with pytest.raises(_lib.FrcnnError):
            ops.redact_shaped_u8(dev, packed, table, mode, size, 0, "ellipse", 4)
    with pytest.raises(ValueError):
        ops.redact_shaped_u8(dev, packed, table, "mosaic", None, 0, "ellipse", 4)
    for mode, size in (("pixelate", 4), ("blur", 2)):
        need = ops.redact_ws_bytes(h, w, mode, size)
        with pytest.raises(_lib.FrcnnError):
            ops.redact_shaped_u8(dev, packed, table, mode, size, 0, "ellipse", 4, workspace=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.FrcnnError):
        ops.redact_shaped_u8(dev, packed, table, "fill", None, -1, "ellipse", 4)
    with pytest.raises(_lib.FrcnnError):
        ops.redact_shaped_u8(dev, torch.zeros(4 + 7 * 513, dtype=torch.int32, device="cuda"), table, "fill", None, 0, "ellipse", 4)      # max_rows 513
    with pytest.raises(AssertionError):
        ops.redact_shaped_u8(dev.view(h, w * 3), packed, table, "fill", None, 0, "ellipse", 4)
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), frame)                         # nothing ran
    ops.redact_shaped_u8(dev, packed, table, "fill", None, 0, "ellipse", 4)       # (the same call, well-formed, does)
    assert not dev.cpu().numpy()[h // 2, w // 2].any() and dev.cpu().numpy()[0, 0].any()
