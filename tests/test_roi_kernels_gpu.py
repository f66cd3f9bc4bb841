"""Per-kernel parity of the RoI crop / bilinear-resize kernels (custom_layers.RoiResizeConv), all seven entry points of csrc/roi.hip and
csrc/conv_bf16.hip, against the plain numpy references of tests/roi_ref.py (checked on their own by tests/test_roi_ref_cpu.py):

    frcnn_roi_crop_resize_fwd_ex / _fwd_batch (f32 output)     bit for bit fwd_f32
    frcnn_roi_crop_resize_fwd_planes / _fwd_batch (planes)     the widened planes within 2^-23 |f| + 2^-40 max|f| of fwd_f32
    frcnn_roi_crop_resize_fwd_bf16_ex / _fwd_bf16_batch        within the counted bar of fwd_f64 AND bit for bit rne(fwd_f32)
    frcnn_roi_crop_resize_bwd / _bwd_bf16                      bit for bit bwd_seq_f32, within the counted bar of bwd_f64

One RoI list on a 9 x 13 map (every edge a few cells away) serves all forms: the whole map, 1x1 boxes in the four corners, a 1-wide and a
1-tall strip, the extents pool - 1, pool, pool + 1 and 2 pool that fit the map, fractional corners, corners in (-1, 0), x2 = cols, x2 =
cols + 0.9, y2 = rows, three copies of one box, and one rejected box per clause of the validity predicate.  NaN, infinite and beyond-int32
coordinates are left out: (int) of those is undefined and the proposal path cannot produce them.  Output buffers are pre-filled with a
NaN pattern and carry a guard band that must come back untouched.  Every comparison prints `name  max|err|  max err/bound` (pytest -s);
the figures of an MI355X run are in docs/ROI_KERNEL_PARITY.md."""
import ctypes

import numpy as np
import pytest

from tests import roi_ref as R

pytestmark = pytest.mark.gpu

ROWS, COLS = 9, 13
GUARD = 4096                                # elements after the last one a call may write
SENT32, SENT16 = 0x7FC0ABCD, 0x7FCD         # NaN patterns no kernel produces (f32 / bf16)


@pytest.fixture(scope="module")
def G():
    import torch
    from faster_rcnn_amd import _lib, ops

    class _G:
        pass
    g = _G()
    g.torch, g.lib, g.ops = torch, _lib, ops
    g.dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    g.call = lambda name, *a: _lib.call(name, *a, ops._stream())
    g.ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off) if t is not None else None
    return g


# ----------------------------------------------------------------------------- the shared RoI list
def roi_list(pool):
    fixed = [
        [0, 0, 13, 9],                                          # the whole map (x2 = cols, y2 = rows)
        [0, 0, 1, 1], [12, 0, 13, 1],                           # 1x1 boxes in the corners ...
        [3, 4, 9, 4],                                           # REJECTED: h = 0
        [0, 8, 1, 9], [12, 8, 13, 9],                           # ...
        [4, 0, 5, 9], [0, 3, 13, 4],                            # a 1-wide and a 1-tall strip
        [3, 4, 3, 8],                                           # REJECTED: w = 0
        [5.9, 3.2, 8.5, 8.5],                                   # fractional corners: (5, 3, 8, 8)
        [-0.7, -0.7, 3.2, 5.9],                                 # corners in (-1, 0): truncate to 0, accepted
        [8, 7, 2, 1],                                           # REJECTED: inverted
        [6, 2, 13.9, 9],                                        # x2 = cols + 0.9 -> cols; y2 = rows
        [2, 1, 13, 6], [1, 2, 7, 9],                            # x2 = cols; y2 = rows
        [-1, 0, 5, 5],                                          # REJECTED: x1 = -1
        [2, 1, 8, 7], [2, 1, 8, 7], [2, 1, 8, 7],               # three copies of one box
        [0, -1.5, 5, 5],                                        # REJECTED: y1 = -1.5 -> -1
        [0, 0, 14, 9],                                          # REJECTED: x2 = cols + 1
    ]
    ext = []
    for e in sorted({pool - 1, pool, pool + 1, 2 * pool}):     # source extents below / at / above / twice the output's
        if 1 <= e <= COLS - 1:
            ext.append([1, 1, 1 + e, 1 + min(e, ROWS - 2)])
        if 1 <= e <= ROWS:
            ext.append([2, 0, 2 + min(e + 3, COLS - 2), e])
    return np.array(fixed + ext + [[0, 0, 13, 10]], np.float32)                      # ... and REJECTED: y2 = rows + 1


def long_list(n, pool):
    """n RoIs: the shared list again and again, each repetition moved by a few cells -- what sticks out after the move is rejected, so
    accepted and rejected boxes alternate through every 256-RoI chunk."""
    base = roi_list(pool)
    reps = []
    for k in range(-(-n // len(base))):
        dx, dy = (0, 2, -1, 1, 3)[k % 5], (0, 1, -1)[k % 3]
        reps.append(base + np.array([dx, dy, dx, dy], np.float32))
    return np.concatenate(reps)[:n]


def make_rois(n, pool):
    base = roi_list(pool)
    if n == "list":
        return base
    return base[16:17] if n == 1 else long_list(n, pool)


def test_the_list_holds_every_case():
    for pool in (1, 2, 7, 14, 16):
        rois = roi_list(pool)
        ok = np.array([R.accepted(r, ROWS, COLS) for r in rois])
        assert (~ok).sum() == 7 and ok.sum() >= 15
        for n in (256, 257, 600):
            acc = np.array([R.accepted(r, ROWS, COLS) for r in long_list(n, pool)])
            for c0 in range(0, n, 256):
                assert acc[c0:c0 + 256].any() and (n - c0 < 256 or not acc[c0:c0 + 256].all())      # (257: the one RoI of chunk 2 is accepted)


# ----------------------------------------------------------------------------- helpers
def report(name, got, want, bound):
    """|got - want| <= bound everywhere (bound 0: equal), printing the largest share of the bound any element uses."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), want.shape)
    assert got.shape == want.shape, name
    assert np.isfinite(got).all(), "%s: %d elements not finite (never written?)" % (name, int((~np.isfinite(got)).sum()))
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    print("%-58s max|err| %.3e  max err/bound %.3f" % (name, err.max() if err.size else 0.0, share.max() if share.size else 0.0))
    assert (err <= bound).all(), "%s: %d of %d outside the bound, worst err/bound %.3f" % (name, int((err > bound).sum()), err.size, share.max())


def same_bits(name, got, want):
    """Bit equality of two arrays of one dtype (so -0.0 != +0.0), printing how many differ."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, name
    u = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    bad = int((got.view(u) != want.view(u)).sum())
    print("%-58s max|err| %.3e  max err/bound %s" % (name, 0.0 if not bad else float(np.nanmax(np.abs(got.astype(np.float64) - want.astype(np.float64)))),
                                                     "equal" if not bad else "%d of %d differ" % (bad, got.size)))
    assert bad == 0, "%s: %d of %d elements differ" % (name, bad, got.size)


def guarded(G, numel, bf16=False):
    t = G.torch
    if bf16:
        return t.full((numel + GUARD,), SENT16, dtype=t.int16, device="cuda").view(t.bfloat16)
    return t.full((numel + GUARD,), SENT32, dtype=t.int32, device="cuda").view(t.float32)


def take(G, buf, numel, shape):
    """The first ``numel`` elements as numpy (f32, or bf16 bit patterns as uint16); the guard band behind them must be untouched."""
    t = G.torch
    G.torch.cuda.synchronize()
    if buf.dtype == t.bfloat16:
        h = buf.view(t.int16).cpu().numpy().view(np.uint16)
        assert (h[numel:] == SENT16).all(), "guard band written"
        return h[:numel].reshape(shape)
    h = buf.cpu().numpy()
    assert (h[numel:].view(np.uint32) == SENT32).all(), "guard band written"
    return h[:numel].reshape(shape)


def oshape(n, pool, C, layout):
    return (pool, pool, n, C) if layout else (n, pool, pool, C)


def run_fwd(G, feat_d, rois, pool, fill_d, relu, layout, n_per_img=0):
    rows, cols, C = feat_d.shape[-3:]
    n = len(rois)
    buf = guarded(G, n * pool * pool * C)
    rd = G.dev(rois)
    if n_per_img:
        G.call("frcnn_roi_crop_resize_fwd_batch", G.ptr(feat_d), rows, cols, C, G.ptr(rd), n, n_per_img, pool, G.ptr(fill_d), int(relu), layout, G.ptr(buf), None)
    else:
        G.call("frcnn_roi_crop_resize_fwd_ex", G.ptr(feat_d), rows, cols, C, G.ptr(rd), n, pool, G.ptr(fill_d), int(relu), layout, G.ptr(buf))
    return take(G, buf, n * pool * pool * C, oshape(n, pool, C, layout))


def run_fwd_bf16(G, feat_d, rois, pool, fill_d, relu, layout, n_per_img=0):
    rows, cols, C = feat_d.shape[-3:]
    n = len(rois)
    buf = guarded(G, n * pool * pool * C, bf16=True)
    rd = G.dev(rois)
    if n_per_img:
        G.call("frcnn_roi_crop_resize_fwd_bf16_batch", G.ptr(feat_d), feat_d.shape[0], rows, cols, C, G.ptr(rd), n_per_img, pool, G.ptr(fill_d), int(relu), layout, G.ptr(buf))
    else:
        G.call("frcnn_roi_crop_resize_fwd_bf16_ex", G.ptr(feat_d), rows, cols, C, G.ptr(rd), n, pool, G.ptr(fill_d), int(relu), layout, G.ptr(buf))
    return take(G, buf, n * pool * pool * C, oshape(n, pool, C, layout))


def bf16_dev(G, bits16):
    return G.dev(np.asarray(bits16, np.uint16).view(np.int16)).view(G.torch.bfloat16)


# fill, relu, layout: each option both ways, and the fill vector under ReLU (the rejected branch is code of its own)
VARIANTS = [(False, False, 0), (True, True, 1), (True, False, 1), (False, True, 0), (True, True, 0)]


def inputs(seed, shape, C):
    rs = np.random.RandomState(seed)
    feat = rs.randn(*shape, C).astype(np.float32)
    fill = (rs.randn(C) * 1.5).astype(np.float32)                       # both signs
    return feat, fill


# ----------------------------------------------------------------------------- f32 forward
# C4 = C / 4 float4 lanes of a 256-lane workgroup: 1, 16, 256 (one full trip), 257 (a second trip by one lane), 512 (two trips)
FWD_CASES = [(pool, C, "list") for pool in (1, 2, 7, 14) for C in (4, 64, 1024, 1028, 2048)] + \
            [(7, 64, 1), (7, 1028, 1), (14, 4, 1), (7, 64, 300), (14, 64, 300), (2, 2048, 300), (1, 1028, 300)]


@pytest.mark.parametrize("pool,C,n", FWD_CASES)
def test_fwd_f32(G, pool, C, n):
    """frcnn_roi_crop_resize_fwd_ex == fwd_f32 bit for bit (roi.hip is built without contraction: every operation rounds where the
    reference's does)."""
    rois = make_rois(n, pool)
    feat, fill = inputs(pool * 10007 + C, (ROWS, COLS), C)
    fd, fld = G.dev(feat), G.dev(fill)
    for use_fill, relu, layout in VARIANTS:
        got = run_fwd(G, fd, rois, pool, fld if use_fill else None, relu, layout)
        want = R.fwd_f32(feat, rois, pool, fill if use_fill else None, relu, layout)
        same_bits("fwd_f32 pool %d C %d n %d fill %d relu %d layout %d" % (pool, C, len(rois), use_fill, relu, layout), got, want)


@pytest.mark.parametrize("pool,C", [(7, 8), (2, 1028), (7, 64)])
@pytest.mark.parametrize("n", [21, 17])
def test_fwd_f32_batch(G, pool, C, n):
    """frcnn_roi_crop_resize_fwd_batch, f32 output: three maps, seven RoIs per image (17: the last image partly filled), against fwd_f32
    reading image r // 7 -- not against per-image kernel calls.  The maps differ, so a wrong image index shows."""
    rois = long_list(n, pool)
    feat, fill = inputs(pool * 31 + C + n, (3, ROWS, COLS), C)
    fd, fld = G.dev(feat), G.dev(fill)
    for use_fill, relu, layout in VARIANTS:
        got = run_fwd(G, fd, rois, pool, fld if use_fill else None, relu, layout, n_per_img=7)
        want = R.fwd_f32(feat, rois, pool, fill if use_fill else None, relu, layout, n_per_img=7)
        same_bits("fwd_f32_batch pool %d C %d n %d fill %d relu %d layout %d" % (pool, C, n, use_fill, relu, layout), got, want)


# ----------------------------------------------------------------------------- plane form
@pytest.mark.parametrize("batch", [False, True])
@pytest.mark.parametrize("pool,C,fill_scale", [(7, 64, 0.5), (7, 1028, 0.5), (2, 64, 0.5), (7, 64, 40.0)])
def test_fwd_planes(G, batch, pool, C, fill_scale):
    """frcnn_roi_crop_resize_fwd_planes / _fwd_batch with plane output, through ops.roi_crop_resize(planes_out=True) on a map with a
    magnitude record: the widened planes within 2^-23 |f| + 2^-40 max|f| of fwd_f32 (hi and lo carry 11 bits each; the bar
    test_conv_h3_gpu uses), status word 0, and the exponent the one amax_carry derives from max(max|map|, max|fill|) -- also when the
    fill vector is the larger of the two (fill_scale 40)."""
    ops, t = G.ops, G.torch
    n = 21 if batch else "list"
    rois = long_list(n, pool) if batch else make_rois(n, pool)
    feat, fill = inputs(pool + C, (3, ROWS, COLS) if batch else (ROWS, COLS), C)
    fill = (fill * fill_scale).astype(np.float32)
    bound = max(float(np.abs(feat).max()), float(np.abs(fill).max()))
    assert (float(np.abs(fill).max()) > float(np.abs(feat).max())) == (fill_scale > 1)
    with ops.f32_engine("f16x3"):
        fd, fld = G.dev(feat), G.dev(fill)
        fd._amax = ops.amax_of(fd)
        for relu, layout in ((True, 1), (False, 0)):
            pl = ops.roi_crop_resize(fd, G.dev(rois), pool, fill=fld, relu=relu, layout=layout, planes_out=True, n_per_img=7 if batch else 0)
            assert isinstance(pl, ops.PlaneTensor)
            want = R.fwd_f32(feat, rois, pool, fill, relu, layout, n_per_img=7 if batch else 0)
            assert pl.shape == want.shape
            got = pl.float().double().cpu().numpy()
            f = np.abs(want.astype(np.float64))
            report("fwd_planes batch %d pool %d C %d fill x%g relu %d layout %d" % (batch, pool, C, fill_scale, relu, layout), got, want,
                   2.0 ** -23 * f + 2.0 ** -40 * f.max())
            e = int(pl.exponent.item())
            assert int(pl._amax.view(t.int32)[1].item()) == 0, "status word"
            assert float(pl._amax.max()) == bound and 2.0 ** 14 <= bound * 2.0 ** e < 2.0 ** 15


# ----------------------------------------------------------------------------- bf16 forward
def bf16_inputs(seed, shape, C):
    feat, fill = inputs(seed, shape, C)
    bits = R.bf16_bits_rne(feat)
    return bits, R.bf16_bits_to_f32(bits), fill


def check_bf16(name, got_bits, wide, rois, pool, fill, relu, layout, n_per_img=0):
    val, _, err = R.fwd_f64(wide, rois, pool, fill, relu, layout, n_per_img)
    report(name + " vs f64", R.bf16_bits_to_f32(got_bits), val, R.bf16_bar(val, err))
    same_bits(name + " == rne(f32 form)", got_bits, R.bf16_bits_rne(R.fwd_f32(wide, rois, pool, fill, relu, layout, n_per_img)))


@pytest.mark.parametrize("pool,C", [(7, C) for C in (3, 8, 12, 64, 512, 520, 2048)] + [(2, 520), (14, 64), (1, 12)])
def test_fwd_bf16(G, pool, C):
    """frcnn_roi_crop_resize_fwd_bf16_ex on a bf16 map: within the counted bar of the f64 lerp of the widened map (nine f32 roundings on
    the lerp form, half a bf16 ulp), and -- separately -- bit for bit the round-to-nearest-even of the f32 form on the widened map, which
    is what roi.hip, the oracle and tests/vgg_bf16_ref.py all assume (conv_bf16.hip is built with the default contraction)."""
    rois = make_rois("list", pool)
    bits, wide, fill = bf16_inputs(pool * 7 + C, (ROWS, COLS), C)
    fd, fld = bf16_dev(G, bits), G.dev(fill)
    for use_fill, relu, layout in VARIANTS:
        got = run_fwd_bf16(G, fd, rois, pool, fld if use_fill else None, relu, layout)
        check_bf16("fwd_bf16 pool %d C %d fill %d relu %d layout %d" % (pool, C, use_fill, relu, layout), got, wide, rois, pool,
                   fill if use_fill else None, relu, layout)


@pytest.mark.parametrize("pool,C", [(7, C) for C in (8, 64, 512, 520, 2048)] + [(2, 520), (14, 64)])
def test_fwd_bf16_batch(G, pool, C):
    """frcnn_roi_crop_resize_fwd_bf16_batch (eight channels per lane; 64, 128 or 256 lanes by C): the same two bars against the
    references reading image r // 7, and bit for bit the single form per RoI."""
    rois = long_list(21, pool)
    bits, wide, fill = bf16_inputs(pool * 13 + C, (3, ROWS, COLS), C)
    fd, fld = bf16_dev(G, bits), G.dev(fill)
    for use_fill, relu, layout in VARIANTS:
        f = fill if use_fill else None
        got = run_fwd_bf16(G, fd, rois, pool, fld if use_fill else None, relu, layout, n_per_img=7)
        tag = "fwd_bf16_batch pool %d C %d fill %d relu %d layout %d" % (pool, C, use_fill, relu, layout)
        check_bf16(tag, got, wide, rois, pool, f, relu, layout, n_per_img=7)
        single = [run_fwd_bf16(G, fd[i], rois[7 * i:7 * i + 7], pool, fld if use_fill else None, relu, layout) for i in range(3)]
        same_bits(tag + " == single form", got, np.concatenate(single, axis=2 if layout else 0))


# ----------------------------------------------------------------------------- backward
def run_bwd(G, dout_d, rois, pool, C, name="frcnn_roi_crop_resize_bwd"):
    t = G.torch
    buf = t.full((ROWS * COLS * C + GUARD,), float("nan"), dtype=t.float32, device="cuda")
    buf[ROWS * COLS * C:] = t.full((GUARD,), SENT32, dtype=t.int32, device="cuda").view(t.float32)
    rd = G.dev(np.asarray(rois, np.float32).reshape(-1, 4)) if len(rois) else t.zeros((1, 4), dtype=t.float32, device="cuda")
    G.call(name, G.ptr(dout_d), ROWS, COLS, C, G.ptr(rd), len(rois), pool, G.ptr(buf))
    return take(G, buf, ROWS * COLS * C, (ROWS, COLS, C))


def check_bwd(G, tag, rois, pool, C, seed):
    rs = np.random.RandomState(seed)
    n = len(rois)
    dout = rs.randn(max(n, 1), pool, pool, C).astype(np.float32)[:n]
    dd = G.dev(dout) if n else G.torch.zeros(4, device="cuda")
    got = run_bwd(G, dd, rois, pool, C)                                   # dfeat pre-filled with NaN: every cell is written
    val, cnt, mag = R.bwd_f64(dout, rois, ROWS, COLS, pool)
    same_bits(tag + " == sequential f32 scatter", got, R.bwd_seq_f32(dout, rois, ROWS, COLS, pool))
    report(tag + " vs f64", got, val, R.bwd_bar(cnt, mag))
    assert not got[cnt == 0].view(np.uint32).any(), "a cell no accepted RoI covers must be +0.0"
    same_bits(tag + " twice", run_bwd(G, dd, rois, pool, C), got)
    gb = R.bf16_bits_rne(dout)                                            # the bf16 twin on bf16 gradients == the f32 form on the widened ones
    got16 = run_bwd(G, bf16_dev(G, gb) if n else dd, rois, pool, C, "frcnn_roi_crop_resize_bwd_bf16")
    want16 = run_bwd(G, G.dev(R.bf16_bits_to_f32(gb)) if n else dd, rois, pool, C)
    same_bits(tag + " bf16 == f32 form on the widened gradient", got16, want16)
    return cnt


# n: the 256-RoI chunk loop (256: one full chunk, 257: one RoI in the second, 600: three); C: four channels per lane, 1024 per trip of
# the cb loop (1025: one channel in the second trip; 1300: a partial second trip); C % 4 != 0 is allowed here only
BWD_CASES = [(7, 64, n) for n in (0, 1, "list", 256, 257, 600)] + [(14, 64, 600), (16, 64, 257), (1, 64, 600)] + \
            [(7, C, "list") for C in (1, 3, 1024, 1025, 1300)] + [(pool, 3, "list") for pool in (1, 14, 16)] + [(16, 1025, 1), (1, 1300, 257)]


@pytest.mark.parametrize("pool,C,n", BWD_CASES)
def test_bwd(G, pool, C, n):
    """frcnn_roi_crop_resize_bwd and _bwd_bf16 (k_roi_bwd_gather): bit for bit the sequential f32 scatter in TF's order, within
    (taps + 1) U sum|w g| of the f64 sum, +0.0 where no accepted RoI covers the cell, the same bits twice, and the bf16 twin bit for bit
    the f32 form on the widened gradient.  Rejected RoIs sit all through the lists: the gather's `covers` predicate must agree with
    the forward's."""
    rois = make_rois(n, pool) if n else np.zeros((0, 4), np.float32)
    cnt = check_bwd(G, "bwd pool %d C %d n %d" % (pool, C, len(rois)), rois, pool, C, pool * 1009 + C)
    if len(rois) >= 256 and pool >= 7:                                    # many RoIs on one cell: its samples take several 256-sample passes ...
        boxes = [R.trunc_corners(r) for r in rois[:256] if R.accepted(r, ROWS, COLS)]
        assert sum(x1 <= 2 < x2 and y1 <= 1 < y2 for x1, y1, x2, y2 in boxes) * pool * pool > 4 * 256       # ... of the first chunk's list


@pytest.mark.parametrize("C", [5, 64])
def test_bwd_full_tap_list(G, C):
    """Two 1x1 RoIs on one cell at pool 16: each puts all four taps of its 256 samples on that cell, so each pass of 256 samples fills
    the 1024-entry tap list to its last slot; a neighbour RoI keeps a partly filled pass behind them."""
    rois = np.array([[5, 4, 6, 5], [5, 4, 6, 5], [4, 3, 7, 6]], np.float32)
    cnt = check_bwd(G, "bwd full tap list C %d" % C, rois, 16, C, 77 + C)
    assert cnt[4, 5] >= 2 * 1024


# ----------------------------------------------------------------------------- refusals
def test_refusals(G):
    """Every argument check of the seven entry points refuses (FrcnnError) before anything is launched: the outputs keep their
    sentinel."""
    t, lib = G.torch, G.lib
    feat = G.dev(np.ones((3, ROWS, COLS, 24), np.float32))
    feat16 = t.ones((3, ROWS, COLS, 24), dtype=t.bfloat16, device="cuda")
    rois = G.dev(np.array([[2, 1, 8, 7]] * 6, np.float32))
    out, out16 = guarded(G, 6 * 49 * 24), guarded(G, 6 * 49 * 24, bf16=True)
    planes = t.full((2 * 6 * 49 * 24 + 64,), 7.0, dtype=t.float16, device="cuda")
    expo = t.zeros(1, dtype=t.int32, device="cuda")

    def H(off=0):
        return ctypes.byref(lib.H3Planes(planes=planes.data_ptr() + off, exponent=expo.data_ptr(), status=None))

    refused = [
        ("fwd_ex: C % 4", lambda: G.call("frcnn_roi_crop_resize_fwd_ex", G.ptr(feat), ROWS, COLS, 6, G.ptr(rois), 6, 7, None, 0, 0, G.ptr(out))),
        ("fwd_ex: C = 1", lambda: G.call("frcnn_roi_crop_resize_fwd_ex", G.ptr(feat), ROWS, COLS, 1, G.ptr(rois), 6, 7, None, 0, 0, G.ptr(out))),
        ("fwd_planes: C % 4", lambda: G.call("frcnn_roi_crop_resize_fwd_planes", G.ptr(feat), ROWS, COLS, 6, G.ptr(rois), 6, 7, None, 0, 0, H())),
        ("fwd_planes: misaligned planes", lambda: G.call("frcnn_roi_crop_resize_fwd_planes", G.ptr(feat), ROWS, COLS, 24, G.ptr(rois), 6, 7, None, 0, 0, H(8))),
        ("fwd_batch: both outputs", lambda: G.call("frcnn_roi_crop_resize_fwd_batch", G.ptr(feat), ROWS, COLS, 24, G.ptr(rois), 6, 3, 7, None, 0, 0, G.ptr(out), H())),
        ("fwd_batch: neither output", lambda: G.call("frcnn_roi_crop_resize_fwd_batch", G.ptr(feat), ROWS, COLS, 24, G.ptr(rois), 6, 3, 7, None, 0, 0, None, None)),
        ("fwd_batch: n_per_img = 0", lambda: G.call("frcnn_roi_crop_resize_fwd_batch", G.ptr(feat), ROWS, COLS, 24, G.ptr(rois), 6, 0, 7, None, 0, 0, G.ptr(out), None)),
        ("fwd_batch: n_per_img < 0", lambda: G.call("frcnn_roi_crop_resize_fwd_batch", G.ptr(feat), ROWS, COLS, 24, G.ptr(rois), 6, -2, 7, None, 0, 0, G.ptr(out), None)),
        ("fwd_batch: C % 4", lambda: G.call("frcnn_roi_crop_resize_fwd_batch", G.ptr(feat), ROWS, COLS, 6, G.ptr(rois), 6, 3, 7, None, 0, 0, G.ptr(out), None)),
        ("fwd_batch: misaligned planes", lambda: G.call("frcnn_roi_crop_resize_fwd_batch", G.ptr(feat), ROWS, COLS, 24, G.ptr(rois), 6, 3, 7, None, 0, 0, None, H(8))),
        ("bf16_batch: C = 3", lambda: G.call("frcnn_roi_crop_resize_fwd_bf16_batch", G.ptr(feat16), 3, ROWS, COLS, 3, G.ptr(rois), 2, 7, None, 0, 0, G.ptr(out16))),
        ("bf16_batch: C = 12", lambda: G.call("frcnn_roi_crop_resize_fwd_bf16_batch", G.ptr(feat16), 3, ROWS, COLS, 12, G.ptr(rois), 2, 7, None, 0, 0, G.ptr(out16))),
        ("bf16_batch: misaligned map", lambda: G.call("frcnn_roi_crop_resize_fwd_bf16_batch", G.ptr(feat16, 2), 2, ROWS, COLS, 24, G.ptr(rois), 3, 7, None, 0, 0, G.ptr(out16))),
        ("bf16_batch: misaligned output", lambda: G.call("frcnn_roi_crop_resize_fwd_bf16_batch", G.ptr(feat16), 3, ROWS, COLS, 24, G.ptr(rois), 2, 7, None, 0, 0, G.ptr(out16, 2))),
        ("bf16_batch: n_per_img = 0", lambda: G.call("frcnn_roi_crop_resize_fwd_bf16_batch", G.ptr(feat16), 3, ROWS, COLS, 24, G.ptr(rois), 0, 7, None, 0, 0, G.ptr(out16))),
    ]
    for name, fn in refused:
        with pytest.raises(lib.FrcnnError):
            fn()
            pytest.fail(name + ": accepted")
    t.cuda.synchronize()
    assert (out.view(t.int32) == SENT32).all().item() and (out16.view(t.int16) == SENT16).all().item() and (planes == 7).all().item()
    # ... and the accepted neighbours of those calls run: C = 24, aligned, exactly one output
    G.call("frcnn_roi_crop_resize_fwd_batch", G.ptr(feat), ROWS, COLS, 24, G.ptr(rois), 6, 3, 7, None, 0, 0, G.ptr(out), None)
    G.call("frcnn_roi_crop_resize_fwd_bf16_batch", G.ptr(feat16), 3, ROWS, COLS, 24, G.ptr(rois), 2, 7, None, 0, 0, G.ptr(out16))
    assert (take(G, out, 6 * 49 * 24, (6, 7, 7, 24)) == 1).all()
    assert (take(G, out16, 6 * 49 * 24, (6, 7, 7, 24)) == 0x3F80).all()
