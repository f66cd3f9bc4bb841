"""ops.redact_u8 (csrc/redact.hip) against the numpy restatement of the redaction rule in tests/redact_ref.py: byte for byte.  Every
frame is a view inside a larger buffer whose bytes before and behind it must survive, and so is the workspace."""
import numpy as np
import pytest

from tests import redact_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xA5
PAD = 67                                                                   # (odd: the frame starts at no aligned address)
SHAPES = [(1, 1), (5, 7), (33, 70), (64, 64)]
MODES = [("fill", 0), ("pixelate", 2), ("pixelate", 5), ("pixelate", 16), ("pixelate", 64), ("blur", 1), ("blur", 12), ("blur", 32)]
TABLE = np.array([1, 0, 1, 1, 0], dtype=np.uint8)                          # classes 1 and 4 are not redacted


def pixels(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def pack(bbox, cls, n, rows=512, dead_box=None, dead_cls=-1):
    """The post-process's packed buffer with ``n`` live rows; the rows behind them hold ``dead_box`` / ``dead_cls``."""
    packed = np.zeros(4 + 7 * rows, dtype=np.int32)
    packed[0] = n
    b = packed[4:4 + 4 * rows].reshape(rows, 4)
    c = packed[4 + 4 * rows:4 + 5 * rows]
    b[:] = (-1, -1, -1, -1) if dead_box is None else dead_box
    c[:] = dead_cls
    k = len(cls)
    b[:k] = np.asarray(bbox, dtype=np.int64).reshape(-1, 4)
    c[:k] = cls
    return packed


def padded(data):
    """``data`` (uint8 array) on the device inside a buffer of sentinel bytes -> (the buffer, the view of the data)."""
    n = data.size
    buf = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    view = buf[PAD:PAD + n].view(data.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(data)).cuda())
    return buf, view


def intact(buf, n):
    host = buf.cpu().numpy()
    return bool((host[:PAD] == SENTINEL).all() and (host[PAD + n:] == SENTINEL).all())


def check(frame, packed, table, mode, size, margin=0):
    """ops.redact_u8 on ``frame`` == the restatement; nothing around the frame or the workspace is written.  -> the result."""
    from faster_rcnn_amd import ops
    h, w = frame.shape[:2]
    rows = (packed.size - 4) // 7
    fbuf, fview = padded(frame)
    need = ops.redact_ws_bytes(h, w, mode, size)
    wbuf, wview = padded(np.full(need, SENTINEL, dtype=np.uint8))
    ret = ops.redact_u8(fview, torch.from_numpy(packed).cuda(), torch.from_numpy(np.asarray(table, dtype=np.uint8)).cuda(), mode, size, margin,
                        workspace=wview)
    assert ret is fview
    got = fview.cpu().numpy()
    n = int(packed[0])
    want = R.redact(frame, packed[4:4 + 4 * rows].reshape(rows, 4), packed[4 + 4 * rows:4 + 5 * rows], n, table, mode, size, margin)
    bad = (got != want).any(axis=2)
    assert not bad.any(), (frame.shape, mode, size, margin, n, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert intact(fbuf, frame.size) and intact(wbuf, need), (frame.shape, mode, size)
    return got


def hand_boxes(h, w):
    """The boxes of the issue's list, placed relative to the frame -> (bbox, cls)."""
    cx, cy = w // 2, h // 2
    rows = [
        ((cx + 3, cy + 2, cx - 2, cy - 1), 0),                             # x1 > x2, y1 > y2: swapped
        ((w // 4, 1, w // 4, h // 3 + 1), 2),                              # zero area: one column
        ((1, h // 4, w // 3 + 1, h // 4), 3),                              # ... one row
        ((-7, -9, 1, 1), 0),                                               # negative corners
        ((-5, cy, 2, cy + 1), 2),                                          # crossing the left border
        ((w - 3, cy - 1, w + 6, cy), 3),                                   # ... the right
        ((cx, -4, cx + 1, 1), 0),                                          # ... the top
        ((cx - 1, h - 2, cx + 2, h + 9), 2),                               # ... the bottom
        ((-20, 0, -1, h), 0), ((w, 0, w + 20, h), 0),                      # wholly outside: left, right (x = w is outside)
        ((0, -20, w, -1), 0), ((0, h, w, h + 20), 0),                      # ... above, below
        ((3 * w // 4 - 2, 3 * h // 4 - 2, 3 * w // 4 + 4, 3 * h // 4 + 3), 1),       # two overlapping boxes of two classes, one of them
        ((3 * w // 4, 3 * h // 4, 3 * w // 4 + 6, 3 * h // 4 + 5), 3),                # ... on the table
        ((0, 0, w, h), 5), ((0, 0, w, h), -3), ((0, 0, w, h), 1 << 20),    # class indices out of range
    ]
    return np.array([r[0] for r in rows], dtype=np.int64), np.array([r[1] for r in rows], dtype=np.int64)


# ----------------------------------------------------------------------------------------------------------- modes x shapes
@pytest.mark.parametrize("mode,size", MODES)
@pytest.mark.parametrize("h,w", SHAPES)
def test_hand_boxes(h, w, mode, size):
    frame = pixels(h, w, 17 * h + w)
    bbox, cls = hand_boxes(h, w)
    got = check(frame, pack(bbox, cls, len(cls)), TABLE, mode, size)
    if (h, w) == (33, 70):
        m = R.mask(h, w, bbox, cls, len(cls), TABLE)
        assert m.any() and not m.all()
        if mode != "pixelate" or size < 64:
            assert (got != frame).any()


@pytest.mark.parametrize("mode,size", MODES)
@pytest.mark.parametrize("h,w", SHAPES)
def test_a_box_over_the_whole_frame(h, w, mode, size):
    frame = pixels(h, w, 3 * h + w)
    got = check(frame, pack([[-2, -2, w + 5, h + 5]], [3], 1), TABLE, mode, size)
    assert np.array_equal(got, R.replacement(frame, mode, size))
    check(frame, pack([[0, 0, w - 1, h - 1]], [0], 1, rows=1), TABLE, mode, size)        # (exactly the frame; a buffer of one row)


@pytest.mark.parametrize("margin", [0, 3, 64])
@pytest.mark.parametrize("mode,size", [("fill", 0), ("pixelate", 5), ("blur", 12)])
@pytest.mark.parametrize("h,w", [(5, 7), (33, 70)])
def test_margins(h, w, mode, size, margin):
    frame = pixels(h, w, 5 * h + w)
    bbox = [[w // 2, h // 2, w // 2 + 2, h // 2 + 1], [-3 - 3, 1, -3, 2], [w + 2, h - 2, w + 9, h - 1]]      # the last two come in with a margin
    check(frame, pack(bbox, [0, 2, 3], 3), TABLE, mode, size, margin)


# ----------------------------------------------------------------------------------------------------------- n_dets
@pytest.mark.parametrize("mode,size", [("fill", 0), ("pixelate", 16), ("pixelate", 5), ("blur", 12), ("blur", 1)])
@pytest.mark.parametrize("h,w", [(33, 70), (64, 64)])
def test_n_dets(h, w, mode, size):
    frame = pixels(h, w, 7 * h + w)
    rs = np.random.RandomState(h + size)
    x = rs.randint(-8, w + 8, (512, 2))
    y = rs.randint(-8, h + 8, (512, 2))
    bbox = np.stack([x[:, 0], y[:, 0], x[:, 0] + rs.randint(-1, 3, 512), y[:, 0] + rs.randint(-1, 2, 512)], axis=1)      # small: they leave gaps
    cls = rs.randint(0, 5, 512)
    huge = (-(1 << 30), -(1 << 30), (1 << 30), (1 << 30))
    # 0 live rows: nothing is read behind them (they would cover the frame) and the frame stays as it is
    got = check(frame, pack(bbox[:0], cls[:0], 0, dead_box=huge, dead_cls=0), TABLE, mode, size)
    assert np.array_equal(got, frame)
    got = check(frame, pack(bbox, cls, 0), TABLE, mode, size)             # (... with 512 would-be boxes behind them)
    assert np.array_equal(got, frame)
    check(frame, pack([[w // 3, h // 3, w // 2, h // 2]], [2], 1, dead_box=huge, dead_cls=0), TABLE, mode, size)
    got = check(frame, pack(bbox, cls, 512), TABLE, mode, size)            # 512 of 512
    assert (got != frame).any()
    m = R.mask(h, w, bbox, cls, 512, TABLE)
    assert m.any() and not m.all()
    got = check(frame, pack(bbox[:3], cls[:3] * 0, 3, dead_box=huge, dead_cls=0), TABLE, mode, size)      # 3 of 512, garbage behind them
    assert not R.mask(h, w, bbox[:3], cls[:3] * 0, 3, TABLE).all()
    # int32 extremes in LIVE rows: the box arithmetic must not wrap
    lim = np.iinfo(np.int32)
    check(frame, pack([[lim.min, lim.min, lim.max, lim.max], [lim.max, 0, lim.max, 5], [lim.min, 0, lim.min + 1, 5]], [1, 0, 0], 3), TABLE, mode, size, 64)
    check(frame, pack([[lim.min, 2, lim.max, 3]], [0], 1), TABLE, mode, size, 3)


def test_a_frame_of_many_tiles_and_odd_row_stride():
    """Larger than one tile both ways (256 byte columns x 16 rows), 3w = 1041 bytes per row."""
    h, w = 50, 347
    frame = pixels(h, w, 11)
    bbox, cls = hand_boxes(h, w)
    for mode, size, margin in (("fill", 0, 0), ("pixelate", 16, 2), ("pixelate", 64, 0), ("blur", 12, 1), ("blur", 32, 0)):
        check(frame, pack(bbox, cls, len(cls)), TABLE, mode, size, margin)
        check(frame, pack([[-1, -1, w, h]], [0], 1), TABLE, mode, size, margin)


# ----------------------------------------------------------------------------------------------------------- captured
@pytest.mark.parametrize("mode,size", [("pixelate", 5), ("blur", 12)])
def test_captured_and_replayed_with_other_detections(mode, size):
    from faster_rcnn_amd import ops
    h, w = 33, 70
    frame = pixels(h, w, 23)
    table = torch.from_numpy(TABLE).cuda()
    src = torch.from_numpy(frame).cuda()
    dev = torch.empty_like(src)
    bbox, cls = hand_boxes(h, w)
    packs = [pack(bbox, cls, len(cls)), pack([[10, 5, 40, 20], [50, 0, 99, 9]], [0, 3], 2), pack(bbox, cls, 0)]
    packed = torch.from_numpy(packs[0]).cuda()
    others = [torch.from_numpy(p).cuda() for p in packs]
    ws = torch.empty(ops.redact_ws_bytes(h, w, mode, size), dtype=torch.uint8, device="cuda")

    def run():
        dev.copy_(src)
        ops.redact_u8(dev, packed, table, mode, size, 1, workspace=ws)

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
        p = packs[k]
        want = R.redact(frame, p[4:4 + 4 * 512].reshape(512, 4), p[4 + 4 * 512:4 + 5 * 512], int(p[0]), TABLE, mode, size, 1)
        assert np.array_equal(dev.cpu().numpy(), want), k
    assert not np.array_equal(R.redact(frame, packs[1][4:2052].reshape(512, 4), packs[1][2052:2564], 2, TABLE, mode, size, 1), frame)


# ----------------------------------------------------------------------------------------------------------- refusals
def test_bad_arguments_raise_and_launch_nothing():
    from faster_rcnn_amd import _lib, ops
    h, w = 12, 20
    frame = pixels(h, w, 3)
    table = torch.from_numpy(TABLE).cuda()
    packed = torch.from_numpy(pack([[0, 0, w, h]], [0], 1)).cuda()
    dev = torch.from_numpy(frame).cuda()
    for mode, size in (("pixelate", 1), ("pixelate", 65), ("blur", 0), ("blur", 33), ("fill", 1), ("fill", 16)):
        with pytest.raises(_lib.FrcnnError):
            ops.redact_u8(dev, packed, table, mode, size)
    with pytest.raises(ValueError):
        ops.redact_u8(dev, packed, table, "mosaic")
    for mode, size, need in (("pixelate", 4, 3 * 5 * 3), ("blur", 2, h * w * 3)):
        assert ops.redact_ws_bytes(h, w, mode, size) == need
        with pytest.raises(_lib.FrcnnError):
            ops.redact_u8(dev, packed, table, mode, size, workspace=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.FrcnnError):
        ops.redact_u8(dev, packed, table, "fill", None, margin=-1)
    with pytest.raises(_lib.FrcnnError):
        ops.redact_u8(dev, torch.zeros(4 + 7 * 513, dtype=torch.int32, device="cuda"), table, "fill")       # max_rows 513 > 512
    wide = torch.from_numpy(pixels(h, 2 * w, 4)).cuda()
    with pytest.raises(AssertionError):
        ops.redact_u8(wide[:, ::2], packed, table, "fill")                  # a non-contiguous frame
    with pytest.raises(AssertionError):
        ops.redact_u8(dev.view(h, w * 3), packed, table, "fill")
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), frame)                         # nothing ran
    ops.redact_u8(dev, packed, table, "fill")                              # (the same call, well-formed, does)
    assert not dev.cpu().numpy()[:h, :w].any()


def test_redact_table():
    from faster_rcnn_amd import ops
    names = ["bg", "car", "", "person"]
    assert ops.redact_table(names, "all").cpu().tolist() == [0, 1, 0, 1]
    assert ops.redact_table(names, ("person",)).cpu().tolist() == [0, 0, 0, 1]
    t = ops.redact_table(names, ["car"])
    assert t.is_cuda and t.dtype == torch.uint8 and t.shape == (4,)
    with pytest.raises(ValueError):
        ops.redact_table(names, ["dog"])
