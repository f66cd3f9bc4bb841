"""The average pool taken inside the closing 1x1 convolution's epilogue (csrc/conv_f32_common.h x6_epilogue_vec<.., POOL>,
include/ext/frcnn_hip_pool_epilogue.h; ``ops.conv2d_avgpool``): row tile t of the launch starts at row 245 t = 5 RoIs x 49 rows, every
thread (j, c) of the first 640 adds the rows of RoI slot j, column c, in ascending order over the four wave-rows, and stores acc / 49.

Every case compares the fused launch BIT FOR BIT (torch.equal on the int32 view) with the two launches it replaces on the same inputs --
``conv2d`` -> ``pool2d(x, 7, 7, False)`` -> reshape -- after asserting ``conv_takes_pool`` and that the fused entry point was the one
called.  Each fused launch runs twice into buffers of its own: what another tile left in LDS would show in one of them.

  RoIs     3 (147 rows: less than a tile, slots 3 and 4 empty), 5 (245: exactly one tile, rows 245..255 past M), 6 (294: the second tile
           holds one RoI, so rows 245..255 of tile 0 are REAL rows of RoI 5 that must not enter a sum of tile 0), 11 (539: three tiles,
           the last one ragged).
  columns  Cout = 128 and 384 (three column tiles: n0 > 0).
  depth    Cin = 32 (one chunk), 64 and 512.
  with and without a residual; plane input (the fused form has no f32-input instantiation: that is one of the refusals below)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POOL, WINDOW, TILE = 7, 49, 86
N_ROIS = [3, 5, 6, 11]
E_ARG, E_UNSUPPORTED = -1, -4


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def data():
    from faster_rcnn_amd import ops
    rs = np.random.RandomState(49)
    d = {"x": {}, "pc0": {}, "pc": {}, "res": {}}
    for cout in (128, 384):
        d["res"][cout] = torch.from_numpy(rs.randn(11, POOL, POOL, cout).astype(np.float32)).cuda()
    for cin in (32, 64, 512):
        d["x"][cin] = torch.from_numpy(rs.randn(11, POOL, POOL, cin).astype(np.float32)).cuda()
        d["pc0"][cin] = ops.PackedConv((rs.randn(1, 1, cin, cin) * np.sqrt(2.0 / cin)).astype(np.float32))
        for cout in (128, 384):
            wt = (rs.randn(1, 1, cin, cout) * np.sqrt(2.0 / cin)).astype(np.float32)
            d["pc"][cin, cout] = ops.PackedConv(wt, (1 + 0.1 * rs.randn(cout)).astype(np.float32), (0.1 * rs.randn(cout)).astype(np.float32))
    return d


def planes_of(data, n, cin):
    from faster_rcnn_amd import ops
    x = ops.conv2d(data["x"][cin][:n].contiguous(), data["pc0"][cin], 1, "valid", "relu", tile=TILE, planes_out=True)
    assert isinstance(x, ops.PlaneTensor)
    return x


def run_both(x, pc, residual, act="relu", tile=TILE, expect_fused=True, **kw):
    """-> (the unpooled tensor, the reference's pooled tensor, the two results of conv2d_avgpool), after checking which entry point ran."""
    from faster_rcnn_amd import ops
    full = ops.conv2d(x, pc, kw.get("stride", 1), kw.get("padding", "valid"), act, residual=residual, tile=tile)
    n, h, w, c = full.shape
    want = ops.pool2d(full, h, h, False).reshape(n, c)
    ops.CONV_PROFILE = rec = []
    try:
        gots = [ops.conv2d_avgpool(x, pc, kw.get("stride", 1), kw.get("padding", "valid"), act, residual=residual, window=h * w, tile=tile) for _ in range(2)]
    finally:
        ops.CONV_PROFILE = None
    torch.cuda.synchronize()
    fused = [r for r in rec if r.get("pool")]
    assert len(fused) == (2 if expect_fused else 0) and len(rec) == 2
    if expect_fused:
        assert all(r["flops"] == 2.0 * n * h * w * c * pc.cin and r["kernel"] == "k_conv_igemm_h3_db<2,1,4,4,planes>" and r["shape"] == (n * h * w, c, pc.cin, 1, "pool")
                   for r in fused)
    assert gots[0].data_ptr() != gots[1].data_ptr()
    return full, want, gots


def check(data, n, cout, cin, with_res):
    from faster_rcnn_amd import ops
    pc = data["pc"][cin, cout]
    res = data["res"][cout][:n].contiguous() if with_res else None
    with ops.f32_engine("f16x3"):
        x = planes_of(data, n, cin)
        assert ops.conv_takes_pool(x, pc, 1, "valid", "relu", 0, TILE, WINDOW)
        full, want, gots = run_both(x, pc, res)
    assert tuple(want.shape) == (n, cout)
    for got in gots:
        assert tuple(got.shape) == (n, cout) and got.dtype == torch.float32
        print("max |fused - two launches| =", float((got - want).abs().max()))
        assert torch.equal(bits(got), bits(want))
        # the magnitude record holds max |pooled value|, status word clean
        slots = got._amax.view(-1, 32)
        assert float(slots[:, 0].max()) == float(want.abs().max()) and int(bits(got._amax)[1].item()) == 0
    assert bool((full == 0).any()) and bool((full > 0).any())          # the ReLU bit, and not everywhere


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("cin", [64, 512])
@pytest.mark.parametrize("cout", [128, 384])
@pytest.mark.parametrize("n", N_ROIS)
def test_fused_pool_equals_the_two_launches(data, n, cout, cin, with_res):
    check(data, n, cout, cin, with_res)


@pytest.mark.parametrize("n", N_ROIS)
def test_one_chunk_of_reduction(data, n):
    """Cin = 32: the main loop is a single chunk, the epilogue starts right behind the first barrier of the launch."""
    check(data, n, 384, 32, True)


def test_columns_of_zeros_and_of_negative_zeros(data):
    """Columns 0..3: zero filter, scale -1, shift -0.0, no activation: every un-pooled value is -0.0f, and 0.0f + (-0.0f) = +0.0f (a sum
    that STARTED from its first row would give -0.0f).  Columns 4..7 under a ReLU: a shift of -1e6 leaves zeros only."""
    from faster_rcnn_amd import ops
    rs = np.random.RandomState(7)
    cin, cout, n = 64, 128, 6
    wt = (rs.randn(1, 1, cin, cout) * np.sqrt(2.0 / cin)).astype(np.float32)
    wt[..., 0:4] = 0.0
    scale, shift = np.ones(cout, np.float32), (0.1 * rs.randn(cout)).astype(np.float32)
    scale[0:4], shift[0:4], shift[4:8] = -1.0, -0.0, -1e6
    pc = ops.PackedConv(wt, scale, shift)
    with ops.f32_engine("f16x3"):
        x = planes_of(data, n, cin)
        for act in (None, "relu"):
            assert ops.conv_takes_pool(x, pc, 1, "valid", act, 0, TILE, WINDOW)
            full, want, gots = run_both(x, pc, None, act=act)
            if act is None:
                assert bool((bits(full[..., 0:4]) == -2 ** 31).all())      # -0.0f everywhere
                assert bool((bits(want[:, 0:4]) == 0).all())               # and +0.0f pooled
            else:
                assert bool((bits(full[..., 4:8]) == 0).all()) and bool((bits(want[:, 4:8]) == 0).all())
            for got in gots:
                assert torch.equal(bits(got), bits(want))


def _tree_sum(v):
    """Pairwise-tree sum over axis 0 in f32."""
    while v.shape[0] > 1:
        even = v[: v.shape[0] // 2 * 2]
        s = even[0::2] + even[1::2]
        v = np.concatenate([s, v[-1:]], axis=0) if v.shape[0] % 2 else s
    return v[0]


def test_summation_order_matters_and_is_the_pools(data):
    """A residual whose rows alternate between ~2^20 and ~1: the 49 sequential f32 additions and a pairwise tree over the same values
    differ (checked here in numpy, or the case would prove nothing), and the fused launch gives the sequential sum's bits."""
    from faster_rcnn_amd import ops
    rs = np.random.RandomState(11)
    n, cin, cout = 6, 64, 384
    mag = np.where((np.arange(n * WINDOW) % 2 == 0)[:, None], np.float32(2.0 ** 20), np.float32(1.0))
    res_h = ((1.0 + rs.rand(n * WINDOW, cout)) * mag).astype(np.float32).reshape(n, POOL, POOL, cout)
    res = torch.from_numpy(res_h).cuda()
    pc = data["pc"][cin, cout]
    with ops.f32_engine("f16x3"):
        x = planes_of(data, n, cin)
        assert ops.conv_takes_pool(x, pc, 1, "valid", "relu", 0, TILE, WINDOW)
        full, want, gots = run_both(x, pc, res)
    v = full.cpu().numpy().reshape(n, WINDOW, cout).transpose(1, 0, 2)      # [row of the RoI][roi][column]
    seq = np.zeros((n, cout), np.float32)
    for r in range(WINDOW):
        seq = seq + v[r]
    seq = seq / np.float32(WINDOW)
    tree = _tree_sum(v) / np.float32(WINDOW)
    assert (seq.view(np.int32) != tree.view(np.int32)).any()
    assert np.array_equal(seq.view(np.int32), want.cpu().numpy().view(np.int32))
    for got in gots:
        assert torch.equal(bits(got), bits(want))


def test_refusals_fall_back_and_the_entry_point_launches_nothing(data):
    """Every condition of the form (include/ext/frcnn_hip_pool_epilogue.h): ``conv_takes_pool`` answers False, ``conv2d_avgpool`` runs the
    two launches (same bits, no fused record), and the entry point itself returns FRCNN_E_UNSUPPORTED before any launch.  (A paired
    launch has entry points of its own, frcnn_conv2d_fwd_dual*, none of which pools: there is nothing to pass.)"""
    from faster_rcnn_amd import _lib, ops
    rs = np.random.RandomState(3)
    n, cin, cout = 6, 64, 128
    pc = data["pc"][cin, cout]
    pc3 = ops.PackedConv((rs.randn(3, 3, cin, cout) * np.sqrt(2.0 / (9 * cin))).astype(np.float32))
    xf = data["x"][cin][:n].contiguous()
    with ops.f32_engine("f16x3"):
        x = planes_of(data, n, cin)
        # ---- ops: the fallbacks
        assert not ops.conv_takes_pool(xf, pc, 1, "valid", "relu", 0, TILE, WINDOW)              # f32 activations
        _, want, gots = run_both(xf, pc, None, expect_fused=False)
        assert all(torch.equal(bits(g), bits(want)) for g in gots)
        assert not ops.conv_takes_pool(x, pc3, 1, "same", "relu", 0, TILE, WINDOW)               # 3x3
        _, want, gots = run_both(x, pc3, None, expect_fused=False, padding="same")
        assert all(torch.equal(bits(g), bits(want)) for g in gots)
        assert not ops.conv_takes_pool(x, pc, 1, "valid", "relu", 0, 82, WINDOW)                 # 256x128 on eight waves
        _, want, gots = run_both(x, pc, None, tile=82, expect_fused=False)
        assert all(torch.equal(bits(g), bits(want)) for g in gots)
        assert not ops.conv_takes_pool(xf, pc, 2, "valid", "relu", 0, TILE, 16)                  # stride 2
        _, want, gots = run_both(xf, pc, None, expect_fused=False, stride=2)
        assert all(torch.equal(bits(g), bits(want)) for g in gots)
        xl = xf.permute(1, 2, 0, 3).contiguous()                                                  # position-major rows
        assert not ops.conv_takes_pool(xl, pc, 1, "valid", "relu", 1, TILE, WINDOW)
        got = ops.conv2d_avgpool(xl, pc, 1, "valid", "relu", window=WINDOW, tile=TILE, layout=1)
        want = ops.avgpool_pos_major(ops.conv2d(xl, pc, 1, "valid", "relu", tile=TILE, layout=1))
        assert torch.equal(bits(got), bits(want))
        res_planes = ops.conv2d(x, pc, 1, "valid", "relu", tile=TILE, planes_out=True)           # a residual handed over as planes
        assert isinstance(res_planes, ops.PlaneTensor)
        ops.CONV_PROFILE = rec = []
        try:
            got = ops.conv2d_avgpool(x, pc, 1, "valid", "relu", residual=res_planes, window=WINDOW, tile=TILE)
        finally:
            ops.CONV_PROFILE = None
        assert not any(r.get("pool") for r in rec)
        want = ops.pool2d(ops.conv2d(x, pc, 1, "valid", "relu", residual=res_planes, tile=TILE), POOL, POOL, False).reshape(n, cout)
        assert torch.equal(bits(got), bits(want))
        for tile in (81, 84, 87, 184, 181):                                                       # the other tiles, the split-K codes
            assert not ops.conv_takes_pool(x, pc, 1, "valid", "relu", 0, tile, WINDOW), tile
        assert not ops.conv_takes_pool(x, pc, 1, "valid", "relu", 0, TILE, 48)                   # rows not a multiple of the window
        pc130 = ops.PackedConv((rs.randn(1, 1, cin, 130) * 0.1).astype(np.float32))
        assert not ops.conv_takes_pool(x, pc130, 1, "valid", "relu", 0, TILE, WINDOW)            # cout % 4
        # ---- the entry point: real buffers, so a launch that slipped through would be a launch
        lib = _lib.load()
        xp = _lib.H3Planes(planes=x.planes.data_ptr(), exponent=x.exponent.data_ptr(), status=None)
        xa = ops.amax_of(x)
        y = torch.full((n, cout), 7.0, dtype=torch.float32, device="cuda")

        def desc(**kw):
            base = dict(n=n, h=POOL, w=POOL, cin=cin, cout=cout, kh=1, kw=1, stride=1, pad_top=0, pad_left=0, ho=POOL, wo=POOL, act=1, ldy=0, ldres=0,
                        tile=TILE, layout=0)
            base.update(kw)
            return _lib.ConvDesc(**base)

        def call(d, x_f32=None, planes=xp, residual_planes=None, mask=None, window=WINDOW, y_planes=None, w=pc):
            return lib.frcnn_conv2d_fwd_h3_pool(ctypes.byref(d), x_f32, ctypes.byref(planes) if planes is not None else None, xa.data_ptr(),
                                                w.h3_planes().data_ptr(), w.scale.data_ptr() if w.scale is not None else None,
                                                w.shift.data_ptr() if w.shift is not None else None, None, ctypes.byref(residual_planes) if residual_planes is not None else None,
                                                mask, window, y.data_ptr(), None, ctypes.byref(y_planes) if y_planes is not None else None, None)
        other = _lib.H3Planes(planes=res_planes.planes.data_ptr(), exponent=res_planes.exponent.data_ptr(), status=None)
        refused = {
            "3x3": call(desc(kh=3, kw=3, pad_top=1, pad_left=1), w=pc3),
            "stride": call(desc(stride=2, ho=4, wo=4), window=16),
            "layout": call(desc(layout=1)),
            "rows": call(desc(), window=48),
            "split-K": call(desc(tile=184)),
            "tile 81": call(desc(tile=81)), "tile 82": call(desc(tile=82)), "tile 84": call(desc(tile=84)), "tile 87": call(desc(tile=87)),
            "f32 in": call(desc(), x_f32=xf.data_ptr(), planes=None),
            "residual planes": call(desc(), residual_planes=other),
            "mask": call(desc(), mask=xf.data_ptr()),
            "plane output": call(desc(), y_planes=other),
            "cout % 4": call(desc(cout=130), w=pc130),
            "ldy": call(desc(ldy=256)), "ldres": call(desc(ldres=256)),
        }
        assert all(v == E_UNSUPPORTED for v in refused.values()), refused
        assert b"conv2d_fwd_h3_pool" in lib.frcnn_last_error()
        torch.cuda.synchronize()
        assert bool((y == 7.0).all())                                                             # nothing was launched
        assert call(desc()) == 0                                                                  # and the same call without a fault is taken
        torch.cuda.synchronize()
        assert torch.equal(bits(y), bits(ops.pool2d(ops.conv2d(x, pc, 1, "valid", "relu", tile=TILE), POOL, POOL, False).reshape(n, cout)))


@pytest.fixture(scope="module")
def head():
    from faster_rcnn_amd import nets
    from faster_rcnn_amd.weights import synthetic_resnet
    h = nets.ResNetHead(synthetic_resnet(50, anchors_per_loc=9, num_classes=21, seed=4), 50, 21)
    for b in h.blocks:                                      # 588 rows: far below the policy's threshold for the 256x128 tile, so ask for it
        for name in ("2b", "2c"):
            b[name].tile = TILE
    return h


def test_head_is_bit_equal_with_and_without(head, monkeypatch):
    """ResNetHead.forward_batched, two images x six RoIs on a 9 x 12 map: class probabilities and regressions with the pool inside
    res5c_branch2c's launch (one fused record, no k_pool behind it) against the two launches."""
    from faster_rcnn_amd import nets, ops
    rs = np.random.RandomState(21)
    feat = torch.from_numpy(rs.randn(2, 9, 12, 1024).astype(np.float32)).cuda().clamp_(min=0)
    rois = torch.tensor([[0, 0, 5, 4], [2, 1, 7, 6], [4, 3, 6, 5], [1, 2, 9, 5], [3, 0, 4, 8], [6, 2, 5, 6]] * 2, dtype=torch.float32).cuda()
    out = {}
    for knob in (True, False):
        monkeypatch.setattr(nets, "HEAD_POOL_EPI", knob)
        ops.CONV_PROFILE = rec = []
        try:
            with ops.conv_workspace(ops.NO_SPLIT_K), ops.f32_engine("f16x3"):
                cls, reg = head.forward_batched(feat, rois, 6)
        finally:
            ops.CONV_PROFILE = None
        torch.cuda.synchronize()
        assert sum(1 for r in rec if r.get("pool")) == (1 if knob else 0)
        out[knob] = (cls, reg)
    assert tuple(out[True][0].shape) == (12, 21) and tuple(out[True][1].shape) == (12, 80)
    assert torch.equal(bits(out[True][0]), bits(out[False][0])) and torch.equal(bits(out[True][1]), bits(out[False][1]))
    assert bool(torch.isfinite(out[True][0]).all()) and float(out[True][0].sum(dim=1).min()) > 0.99
