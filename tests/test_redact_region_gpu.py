"""ops.redact_region_plane / _prepare / _apply_u8 (csrc/redact_region.hip) against the restatement of the region rule in
tests/redact_region_ref.py: the plane, its two counts and the output byte for byte, no tolerance.  The frames are the smallest at which
the kernels can go wrong (tiles are 256 byte columns x 16 rows): 1 x 1; 16 x 85, one tile row, 255 bytes a row, smaller than the largest
feather; 37 x 91, 273 bytes a row -- two tile columns, not dword-aligned -- and a partial tile row; 33 x 200, three tile columns.  Every
frame and every plane is a view inside a larger buffer whose bytes before and behind it must survive, and so is the workspace."""
import functools

import numpy as np
import pytest

from tests import redact_ref as R
from tests import redact_region_ref as RR
from tests import zone_ref as Z

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xA5
PAD = 67                                                                   # (odd: the frame starts at no aligned address)
PLANE_PAD = 64                                                             # (a plane is 16-byte aligned)
FRAMES = [(1, 1), (16, 85), (37, 91), (33, 200)]
MODES = [("fill", 0), ("pixelate", 16), ("blur", 12)]                      # cells cut short by every frame; a blur window that clamps at every edge
FEATHERS = [0, 1, 8, 32]
TRIANGLE = [(3, 2), (60, 9), (20, 30)]
CONCAVE = [(70, 1), (100, 1), (100, 31), (90, 31), (90, 11), (80, 11), (80, 31), (70, 31)]       # a "U" upside down
BOW = [(105, 2), (135, 30), (135, 2), (105, 30)]                           # crosses itself at (120, 16)
LEFT, RIGHT = [(140, 5), (150, 5), (150, 15), (140, 15)], [(150, 5), (165, 5), (165, 15), (150, 15)]      # share the edge x = 150
OUTSIDE = [(-12, 3), (-4, 3), (-8, 12)]                                    # no pixel of it in any frame: only its feather reaches in
SHAPES = [TRIANGLE, CONCAVE, BOW, LEFT, RIGHT, OUTSIDE]


def diamond(h, w):
    """Crosses every border of the frame."""
    return [(w // 2, -6), (w + 6, h // 2), (w // 2, h + 6), (-6, h // 2)]


@functools.lru_cache(maxsize=None)
def pixels(h, w, seed=0):
    a = np.random.RandomState(17 * h + w + 1000 * seed).randint(0, 256, (h, w, 3)).astype(np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def replacement(h, w, mode, size):
    """R of the source frame, computed once per (frame, mode) and shared."""
    a = R.replacement(pixels(h, w), mode, size)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def painted(h, w):
    """A mask: a block, single pixels in two corners, values on both sides of the threshold."""
    m = np.zeros((h, w), dtype=np.uint8)
    m[h // 2:h // 2 + 3, w // 3:w // 3 + 5] = 255
    m[0, 0], m[h - 1, w - 1] = 128, 200
    if w > 2:
        m[0, w - 2] = 127                                                   # under the threshold
    m.setflags(write=False)
    return m


def padded(data, pad=PAD):
    """``data`` (uint8 array) on the device inside a buffer of sentinel bytes -> (the buffer, the view of the data)."""
    n = data.size
    buf = torch.full((pad + n + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    view = buf[pad:pad + n].view(data.shape)
    view.copy_(torch.from_numpy(np.array(data)).cuda())                     # (a copy: ``data`` may be a shared, read-only array)
    return buf, view


def intact(buf, n, pad=PAD):
    host = buf.cpu().numpy()
    return bool((host[:pad] == SENTINEL).all() and (host[pad + n:] == SENTINEL).all())


def build(h, w, regions, mask, F):
    """The plane of (regions, mask, F) inside sentinel bytes, every byte of it a sentinel before the build -> (buffer, plane, W, option)."""
    from faster_rcnn_amd import ops
    option = ops.redact_region_option(regions, mask, None, None, F)
    n = ops.redact_region_plane_bytes(h, w)
    pbuf, pview = padded(np.full(n, SENTINEL, dtype=np.uint8), PLANE_PAD)
    assert ops.redact_region_plane(h, w, option, out=pview) is pview
    return pbuf, pview, ops.redact_region_weights(pview), option


def check(h, w, regions, mask, mode, size, F):
    """The plane and the output == the restatement; nothing around the plane, the frame or the workspace is written.  The frame that is
    edited is NOT the source frame: R must come from the source the prepare call read.  -> (the result, W)."""
    from faster_rcnn_amd import ops
    pbuf, plane, W, _ = build(h, w, regions, mask, F)
    want_W = RR.weights(h, w, regions, mask, F)
    bad = W != want_W
    assert not bad.any(), ((h, w), F, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    st = ops.redact_region_stats(plane)
    assert (st["h"], st["w"], st["feather"]) == (h, w, F) and (st["covered"], st["full"]) == RR.stats(want_W), st
    head = plane[:32].cpu().numpy().view(np.int32)
    assert head[5] == 1 and head[6] == 0 and head[7] == 0
    source, current = pixels(h, w), pixels(h, w, 1)
    sbuf, sview = padded(source)
    cbuf, cview = padded(current)
    need = ops.redact_ws_bytes(h, w, mode, size)
    wbuf, wview = padded(np.full(need, SENTINEL, dtype=np.uint8))
    ops.redact_region_prepare(sview, plane, mode, size, workspace=wview)
    assert ops.redact_region_apply_u8(cview, plane, mode, size, workspace=wview) is cview
    got = cview.cpu().numpy()
    Wb, C, Rep = want_W[:, :, None], current.astype(np.int64), replacement(h, w, mode, size).astype(np.int64)
    want = np.where(Wb > 0, (Wb * Rep + (256 - Wb) * C + 128) >> 8, C).astype(np.uint8)
    bad = (got != want).any(axis=2)
    assert not bad.any(), ((h, w), mode, size, F, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert np.array_equal(sview.cpu().numpy(), source)                      # the prepare call reads its frame
    n = int(plane.numel())
    assert intact(pbuf, n, PLANE_PAD) and intact(sbuf, source.size) and intact(cbuf, current.size) and intact(wbuf, need), ((h, w), mode, F)
    return got, want_W


# ----------------------------------------------------------------------------------------------------------- the grid
@pytest.mark.parametrize("mode,size", MODES)
@pytest.mark.parametrize("h,w", FRAMES)
def test_polygons_masks_and_feathers(h, w, mode, size):
    for F in FEATHERS:
        got, W = check(h, w, SHAPES, None, mode, size, F)                   # a triangle, concave, self-crossing, a shared edge, one outside
        if (h, w) != (1, 1):
            assert (W == 256).any() and (F == 32 or (W == 0).any()) and (got != pixels(h, w, 1)).any()      # (F = 32 reaches every pixel of the small frames)
            if F:
                assert ((W > 0) & (W < 256)).any()                          # a ring there is
        if F >= 8:
            assert W[min(5, h - 1), 0] > 0                                  # the feather of the polygon outside reaches in
        check(h, w, [], painted(h, w), mode, size, F)                       # the mask alone
        got, W = check(h, w, [diamond(h, w), OUTSIDE, TRIANGLE], painted(h, w), mode, size, F)       # across every border, and a mask
        assert W[h // 2, w // 2] == 256 and W[0, 0] == 256


def test_a_shared_edge_is_hidden_exactly_once():
    h, w = 33, 200
    _, _, W, _ = build(h, w, [LEFT, RIGHT], None, 0)
    a, b = Z.inside_mask(LEFT, h, w), Z.inside_mask(RIGHT, h, w)
    assert not (a & b).any() and np.array_equal(W == 256, a | b) and (W[5:15, 140:165] == 256).all() and (W > 0).sum() == 250
    _, _, Wl, _ = build(h, w, [LEFT], None, 0)
    _, _, Wr, _ = build(h, w, [RIGHT], None, 0)
    assert (Wl[5:15, 149] == 256).all() and (Wl[:, 150] == 0).all() and (Wr[5:15, 150] == 256).all()      # a polygon owns its left boundary


def test_the_weight_never_falls_when_the_feather_grows():
    h, w = 37, 91
    last = None
    for F in (0, 1, 2, 8, 31, 32):
        _, _, W, _ = build(h, w, SHAPES, painted(h, w), F)
        if last is not None:
            assert (W >= last).all() and np.array_equal(W == 256, last == 256), F
        last = W


# ----------------------------------------------------------------------------------------------------------- the identities
def pack(box, rows=16):
    """The post-process's packed buffer with one live row of class 0."""
    packed = np.zeros(4 + 7 * rows, dtype=np.int32)
    packed[0] = 1
    packed[4:4 + 4 * rows].reshape(rows, 4)[:] = -1
    packed[4:8] = box
    packed[4 + 4 * rows:4 + 5 * rows] = -1
    packed[4 + 4 * rows] = 0
    return packed


@pytest.mark.parametrize("mode,size", MODES)
@pytest.mark.parametrize("h,w", [(16, 85), (37, 91)])
def test_a_box_polygon_is_the_existing_redaction_on_the_device(h, w, mode, size):
    from faster_rcnn_amd import ops
    table = torch.ones(1, dtype=torch.uint8, device="cuda")
    source = torch.from_numpy(np.array(pixels(h, w))).cuda()
    boxes = [(4, 3, 30, 9), (-5, -4, 6, 5), (w - 8, h - 5, w + 9, h + 7), (-3, 6, w + 2, 8), (80, -2, 88, h + 1), (-9, -9, w + 9, h + 9), (10, 10, 10, 10)]
    for box in boxes:                                                       # inside, across each border, across two tile columns, all of it, a pixel
        packed = torch.from_numpy(pack(box)).cuda()
        for F in FEATHERS:
            plane = ops.redact_region_plane(h, w, ops.redact_region_option([RR.box_polygon(*box)], None, None, None, F))
            got = source.clone()
            ws = ops.redact_region_prepare(got, plane, mode, size)
            ops.redact_region_apply_u8(got, plane, mode, size, workspace=ws)
            want = source.clone()
            if F == 0:
                ops.redact_u8(want, packed, table, mode, size, 0)
            else:
                ops.redact_shaped_u8(want, packed, table, mode, size, 0, "box", F)
            assert torch.equal(got, want), (box, F)
            assert not torch.equal(got, source)


# ----------------------------------------------------------------------------------------------------------- nothing to write
def test_a_plane_with_no_hard_point_and_a_plane_of_another_size_write_nothing():
    from faster_rcnn_amd import ops
    h, w = 37, 91
    far = [(300, 300), (340, 300), (320, 340)]
    for F in (0, 32):
        pbuf, plane, W, _ = build(h, w, [far], np.zeros((h, w), dtype=np.uint8), F)
        st = ops.redact_region_stats(plane)
        assert not W.any() and (st["covered"], st["full"]) == (0, 0)
        fbuf, fview = padded(pixels(h, w))
        ws = ops.redact_region_prepare(fview, plane, "blur", 3)
        ops.redact_region_apply_u8(fview, plane, "blur", 3, workspace=ws)
        assert np.array_equal(fview.cpu().numpy(), pixels(h, w)) and intact(fbuf, pixels(h, w).size)
    # a plane built for 16 x 85 that hides everything, handed to calls over frames of other sizes -- larger, smaller, the sides swapped
    _, small, W, _ = build(16, 85, [RR.box_polygon(-9, -9, 300, 300)], None, 8)
    assert (W == 256).all()
    for fh, fw in ((37, 91), (1, 1), (85, 16)):
        fbuf, fview = padded(pixels(fh, fw))
        for mode, size in MODES[:1] + [("blur", 1)]:
            need = ops.redact_ws_bytes(fh, fw, mode, size)
            wbuf, wview = padded(np.full(need, SENTINEL, dtype=np.uint8))
            ops.redact_region_prepare(fview, small, mode, size, workspace=wview)
            ops.redact_region_apply_u8(fview, small, mode, size, workspace=wview)
            assert np.array_equal(fview.cpu().numpy(), pixels(fh, fw)) and intact(fbuf, pixels(fh, fw).size) and intact(wbuf, need), (fh, fw, mode)
    # ... and over its own size it hides every byte
    fview = torch.from_numpy(np.array(pixels(16, 85))).cuda()
    ws = ops.redact_region_prepare(fview, small)
    ops.redact_region_apply_u8(fview, small, workspace=ws)
    assert not fview.any()


def test_the_calls_replay_in_a_graph():
    """prepare and apply captured once and replayed over other frames: nothing is read on the host, nothing allocated."""
    from faster_rcnn_amd import ops
    h, w = 37, 91
    _, plane, W, _ = build(h, w, SHAPES, painted(h, w), 8)
    frame = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    ws = torch.empty(ops.redact_ws_bytes(h, w, "blur", 12), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.redact_region_prepare(frame, plane, "blur", 12, workspace=ws)   # (warm-up: the code objects are loaded outside the capture)
        ops.redact_region_apply_u8(frame, plane, "blur", 12, workspace=ws)
        graph = torch.cuda.CUDAGraph()
        graph.capture_begin(capture_error_mode="thread_local")
        try:
            ops.redact_region_prepare(frame, plane, "blur", 12, workspace=ws)
            ops.redact_region_apply_u8(frame, plane, "blur", 12, workspace=ws)
        finally:
            graph.capture_end()
        for seed in (2, 3):
            frame.copy_(torch.from_numpy(np.array(pixels(h, w, seed))).cuda())
            graph.replay()
            side.synchronize()
            assert np.array_equal(frame.cpu().numpy(), RR.redact(pixels(h, w, seed), SHAPES, painted(h, w), "blur", 12, 8)), seed
    torch.cuda.current_stream().wait_stream(side)
