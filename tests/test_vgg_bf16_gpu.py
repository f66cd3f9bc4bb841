"""bf16 VGG16 inference on the GPU: the two new kernels (block1_conv1 on the bf16 matrix cores, the bf16 max-pool), the bf16 base /
RPN / head against the f64 oracle and against the oracle under the product's storage model (tests/vgg_bf16_ref.py), the batched
head, the full-size shape against the product's own f32 VGG16, and the entry point's batched captured passes.

Bars: a single bf16 conv is held to tests/test_bf16_gpu.py's criterion (|got - want| / max(|want|, 1) < 1e-2 after the one bf16
store); a bf16 network against unrounded f64 arithmetic to the bars test_resnet101_bf16_network uses for 101 layers (relative RMS
<= 2e-2, max abs <= 5e-2 x max|x|): VGG16's thirteen stored activations stay inside a bound derived for a hundred.  Against the
storage model in f64 what is left is accumulation order and rounding ties: measured first (figures in the tests' docstrings and in
DESIGN), the bars are the observed values x 4."""
import contextlib
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MEAN_BGR = np.array([103.939, 116.779, 123.68])


def pixels(rs, n, h, w):
    """uint8 minus the BGR mean: what vgg.preprocess hands the network."""
    return (rs.randint(0, 256, (n, h, w, 3)).astype(np.float64) - MEAN_BGR).astype(np.float32)


def bf(t):
    return t.to(torch.bfloat16)


def err(a, b):
    a, b = torch.as_tensor(np.asarray(a)).double(), torch.as_tensor(np.asarray(b)).double()
    d = a - b
    return float(d.pow(2).mean().sqrt() / b.pow(2).mean().sqrt()), float(d.abs().max() / b.abs().max())


def within(a, b, rms_bar=2e-2, max_bar=5e-2):
    rms, mx = err(a, b)
    return rms <= rms_bar and mx <= max_bar


# ----------------------------------------------------------------------------- 1, 2: the conv1 kernel
@pytest.mark.parametrize("shape", [(1, 7, 5), (1, 1, 300), (1, 9, 1), (1, 37, 53), (2, 131, 176), (1, 600, 1000)])
def test_conv1_kernel_against_f64(shape):
    """block1_conv1 + bias + ReLU against an f64 convolution of the SAME bf16-rounded pixels and taps: what separates the two is the
    f32 accumulation of 27 products and the one bf16 rounding at the store.  Widths that are no multiple of the wave's 64-pixel run
    or the workgroup's 256, one-pixel-high and one-pixel-wide images (every pixel a border), two different images (batch stride)."""
    from faster_rcnn_amd import ops
    from oracle import keras_ref
    n, h, w = shape
    rs = np.random.RandomState(h * 1000 + w)
    x = torch.from_numpy(pixels(rs, n, h, w))
    k = (rs.randn(3, 3, 3, 64) * np.sqrt(2.0 / 27) / 70.0).astype(np.float32)
    b = (rs.randn(64) * 0.1).astype(np.float32)
    got = ops.vgg_conv1_bf16(x.cuda(), ops.PackedVggConv1Bf16(k, b))
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (n, h, w, 64)
    want = keras_ref.conv2d(bf(x).double(), bf(torch.from_numpy(k)).double(), torch.from_numpy(b).double(), 1, "same", torch.float64).clamp(min=0)
    rel = ((got.cpu().double() - want).abs() / want.abs().clamp(min=1)).max()
    print("conv1 %s: worst |got - want| / max(|want|, 1) = %.3g" % (shape, float(rel)))
    assert float(rel) < 1e-2
    if n > 1:
        one = ops.vgg_conv1_bf16(x[1:].contiguous().cuda(), ops.PackedVggConv1Bf16(k, b))
        assert torch.equal(one[0], got[1])


def test_conv1_same_padding_reads_zeros():
    """A constant-1 image under an all-ones filter with zero bias: 12 at the four corners, 18 on the edges, 27 inside, in every
    channel -- exact in bf16.  Width 300: the run boundary at pixel 256 is interior and must read its neighbours, not zeros."""
    from faster_rcnn_amd import ops
    n, h, w = 2, 5, 300
    got = ops.vgg_conv1_bf16(torch.ones((n, h, w, 3)).cuda(), ops.PackedVggConv1Bf16(np.ones((3, 3, 3, 64), np.float32), np.zeros(64, np.float32)))
    want = torch.full((n, h, w, 64), 27.0)
    want[:, 0, :], want[:, -1, :], want[:, :, 0], want[:, :, -1] = 18.0, 18.0, 18.0, 18.0
    for yy in (0, -1):
        for xx in (0, -1):
            want[:, yy, xx] = 12.0
    assert torch.equal(got.cpu().float(), want)


# ----------------------------------------------------------------------------- 3: the bf16 max-pool
@pytest.mark.parametrize("case", [(1, 600, 1000, 64), (3, 37, 53, 128), (3, 3, 2, 512), (1, 37, 53, 512), (3, 36, 52, 64), (1, 2, 2, 128)])
def test_pool2d_bf16_is_exact(case):
    import torch.nn.functional as F
    from faster_rcnn_amd import ops
    n, h, w, c = case
    rs = np.random.RandomState(h + w + c)
    x = bf(torch.from_numpy(rs.randn(n, h, w, c).astype(np.float32) * 3.0))
    assert not bool((x == 0).any())                                   # (no window holds both zeros)
    got = ops.pool2d_bf16(x.cuda(), 2, 2)
    want = bf(F.max_pool2d(x.float().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous())      # (the maximum of bf16 values is one of them)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (n, h // 2, w // 2, c) and torch.equal(got.cpu(), want)


@pytest.mark.parametrize("bad", [dict(c=12), dict(k=3, stride=3), dict(stride=1)])
def test_pool2d_bf16_refuses_what_it_does_not_support(bad):
    from faster_rcnn_amd import _lib
    from faster_rcnn_amd.ops import _p, _stream
    a = dict(n=1, h=12, w=12, c=64, k=2, stride=2)
    a.update(bad)
    x = torch.zeros((a["n"], a["h"], a["w"], a["c"]), dtype=torch.bfloat16, device="cuda")
    y = torch.full((a["n"], a["h"], a["w"], a["c"]), 7.0, dtype=torch.bfloat16, device="cuda")
    code = _lib.load().frcnn_pool2d_fwd_bf16(_p(x), a["n"], a["h"], a["w"], a["c"], a["k"], a["stride"], _p(y), _stream())
    torch.cuda.synchronize()
    assert code == -4 and _lib.load().frcnn_last_error()              # FRCNN_E_UNSUPPORTED, with a message
    assert bool((y == 7.0).all())


# ----------------------------------------------------------------------------- 4: the network at a reduced size
# Observed against the storage model in f64 (131 x 176, seed 3), (relative RMS, max / max|x|): map (5.34e-3, 6.36e-3), rpn_out_cls
# (1.88e-3, 5.61e-3), rpn_out_bbreg (5.10e-3, 4.80e-3) -- against unrounded f64: (7.56e-3, 9.18e-3), (2.46e-3, 8.34e-3), (7.08e-3,
# 8.27e-3).  Most of a bf16 chain's distance from exact arithmetic is NOT removed by modelling the storage: an f32 sum that lands on
# the other side of a rounding tie moves the stored value by one bf16 unit (2^-9 .. 2^-8 relative), the next layer's sums move with
# it, and after thirteen stored layers most elements sit one unit away from the model's.  Bars = observed x 4 (tie flips differ
# between boxes), capped at the bars against unrounded arithmetic (2e-2, 5e-2).
MODEL_BARS = {"feat": (2e-2, 2.54e-2), "cls": (7.5e-3, 2.24e-2), "reg": (2e-2, 1.92e-2)}


def test_vgg16_bf16_network():
    from faster_rcnn_amd import vgg
    from faster_rcnn_amd.weights import synthetic_vgg16
    from oracle.keras_ref import KerasGraphs
    from tests.vgg_bf16_ref import VggBf16Graphs
    w = synthetic_vgg16(anchors_per_loc=9, seed=3, with_classifier=False)
    base = vgg.vgg16_base(weights=w, dtype="bf16")
    rpn = vgg.vgg16_rpn(base, include_conv=True, anchors_per_loc=9)
    assert base.net.dtype == "bf16" and rpn.head.conv.dtype == "bf16"
    x = pixels(np.random.RandomState(0), 1, 131, 176).astype(np.float64)
    cls, reg, feat = rpn.predict_on_batch(x)
    assert cls.dtype == np.float32 and feat.shape == (1, 8, 11, 512)
    ref = KerasGraphs(w, torch.float64)
    f64 = ref.vgg_base(x)
    c64, r64 = ref.rpn(f64)
    print("bf16 VGG16 against the f64 oracle (rms, max): map %s, cls %s, reg %s" % (err(feat, f64), err(cls, c64), err(reg, r64)))
    assert within(feat, f64) and within(cls, c64) and within(reg, r64)
    model = VggBf16Graphs(w, torch.float64, mixed=True)
    fm = model.vgg_base(x)
    cm, rm = model.rpn(fm)
    figs = {"feat": err(feat, fm), "cls": err(cls, cm), "reg": err(reg, rm)}
    print("bf16 VGG16 against the f64 storage model (rms, max): %s" % figs)
    for k, (rms, mx) in figs.items():
        assert rms <= MODEL_BARS[k][0] and mx <= MODEL_BARS[k][1], (k, rms, mx)


# ----------------------------------------------------------------------------- 5: the head
# Observed against the storage model in f64 (relative RMS, max / max|x|): class probabilities (1.01e-3, 1.63e-3) at 300 RoIs, (9.7e-4,
# 1.63e-3) at 64; regressions (1.61e-3, 1.70e-3) at 300, (1.51e-3, 2.13e-3) at 64.  Bars = the larger observed value x 4.
HEAD_BARS = {"cls": (4.06e-3, 6.5e-3), "reg": (6.46e-3, 8.53e-3)}


def _rois(rs, n, rows, cols):
    """n boxes [x1, y1, x2, y2] inside a rows x cols map, at least one cell each (the crop is [y1:y2, x1:x2])."""
    x1, y1 = rs.randint(0, cols, n), rs.randint(0, rows, n)
    x2, y2 = np.minimum(x1 + rs.randint(1, cols + 1, n), cols), np.minimum(y1 + rs.randint(1, rows + 1, n), rows)
    return np.stack([x1, y1, x2, y2], axis=1).astype(np.float32)


@pytest.fixture(scope="module")
def head_setup():
    from faster_rcnn_amd import vgg
    from faster_rcnn_amd.weights import synthetic_vgg16
    C = 21
    w = synthetic_vgg16(num_classes=C, seed=5)
    det = vgg.vgg16_classifier(64, C, weights=w, dtype="bf16")
    return w, det, C


def test_vgg16_bf16_head_against_the_storage_model(head_setup):
    from faster_rcnn_amd import ops
    from tests.vgg_bf16_ref import VggBf16Graphs
    w, det, C = head_setup
    assert det.head.dtype == "bf16" and det.head.hoist
    rs = np.random.RandomState(8)
    rows, cols = 37, 62
    fmap = bf(torch.from_numpy(np.maximum(rs.randn(1, rows, cols, 512), 0).astype(np.float32)))
    rois = _rois(rs, 300, rows, cols)
    k64, g64 = VggBf16Graphs(w, torch.float64, mixed=True).vgg_classifier(fmap.float(), rois, C)
    for n in (64, 300):
        with ops.conv_workspace(ops.NO_SPLIT_K):
            cls, reg = det.forward_dev(fmap.cuda(), torch.from_numpy(rois[:n]).cuda())
        assert cls.dtype == torch.float32 and tuple(cls.shape) == (n, C) and tuple(reg.shape) == (n, 4 * (C - 1))
        figs = {"cls": err(cls.cpu(), k64[:n]), "reg": err(reg.cpu(), g64[:n])}
        print("bf16 VGG16 head, %d RoIs, against the f64 storage model (rms, max): %s" % (n, figs))
        for k, (rms, mx) in figs.items():
            assert rms <= HEAD_BARS[k][0] and mx <= HEAD_BARS[k][1], (n, k, rms, mx)
    # with split-K (one image alone on the chip: fc1's 392 k-chunks are cut over several workgroups) only the summation order moves
    cls_sk, reg_sk = det.forward_dev(fmap.cuda(), torch.from_numpy(rois).cuda())
    assert within(cls_sk.cpu(), k64, *HEAD_BARS["cls"]) and within(reg_sk.cpu(), g64, *HEAD_BARS["reg"])


def test_vgg16_bf16_head_batched_equals_one_image_calls(head_setup):
    """forward_batched over three images with different maps and RoIs against three one-image calls, both WITHOUT split-K: bit for
    bit (a row's k order does not depend on the GEMM's height).  The f32 head has no batched form."""
    from faster_rcnn_amd import _lib, ops, vgg
    w, det, C = head_setup
    rs = np.random.RandomState(9)
    B, n, rows, cols = 3, 64, 20, 31
    fmap = bf(torch.from_numpy(np.maximum(rs.randn(B, rows, cols, 512), 0).astype(np.float32))).cuda()
    rois = torch.from_numpy(np.concatenate([_rois(rs, n, rows, cols) for _ in range(B)])).cuda()
    with ops.conv_workspace(ops.NO_SPLIT_K):
        cls, reg = det.head.forward_batched(fmap, rois, n)
        for i in range(B):
            c1, r1 = det.head(fmap[i:i + 1].contiguous(), rois[i * n:(i + 1) * n].contiguous())
            assert torch.equal(c1, cls[i * n:(i + 1) * n]) and torch.equal(r1, reg[i * n:(i + 1) * n]), i
    assert not torch.equal(cls[:n], cls[n:2 * n])
    f32_head = vgg.vgg16_classifier(64, C, weights=w).head
    assert f32_head.dtype == "f32" and not f32_head.hoist
    with pytest.raises(_lib.FrcnnError):
        f32_head.forward_batched(fmap.float(), rois, n)


# ----------------------------------------------------------------------------- 6: configs[0]'s shape
def test_vgg16_bf16_full_size_against_the_f32_product():
    """600 x 1000: the bf16 base + RPN against the product's own f32 VGG16 on the native engine (itself held to the oracle at this
    size by tests/test_configs_full_size_gpu.py), under the bars of a bf16 network against unrounded arithmetic.  What only large
    shapes show: tile tails, batch strides, offset width."""
    from faster_rcnn_amd import ops, vgg
    from faster_rcnn_amd.weights import synthetic_vgg16
    w = synthetic_vgg16(seed=4, with_classifier=False)
    x = torch.from_numpy(pixels(np.random.RandomState(4), 1, 600, 1000)).cuda()
    with ops.f32_engine("native"):
        c32, r32, f32map = vgg.vgg16_rpn(vgg.vgg16_base(weights=w), include_conv=True, anchors_per_loc=9).forward_dev(x)
    cls, reg, feat = vgg.vgg16_rpn(vgg.vgg16_base(weights=w, dtype="bf16"), include_conv=True, anchors_per_loc=9).forward_dev(x)
    assert feat.dtype == torch.bfloat16 and tuple(feat.shape) == (1, 37, 62, 512) and cls.dtype == torch.float32
    figs = (err(feat.float().cpu(), f32map.cpu()), err(cls.cpu(), c32.cpu()), err(reg.cpu(), r32.cpu()))
    print("bf16 against f32 VGG16 at 600 x 1000 (rms, max): map %s, cls %s, reg %s" % figs)
    assert all(rms <= 2e-2 and mx <= 5e-2 for rms, mx in figs), figs


def test_conv1_and_pool_at_eight_full_size_images_equal_per_image_launches():
    """n = 8 at 600 x 1000: block 1's bf16 map is 614 MB, its element offsets pass 2^28 -- against one launch per image, bit for bit."""
    from faster_rcnn_amd import ops
    rs = np.random.RandomState(6)
    x = torch.from_numpy(pixels(rs, 8, 600, 1000)).cuda()
    pk = ops.PackedVggConv1Bf16((rs.randn(3, 3, 3, 64) * np.sqrt(2.0 / 27) / 70.0).astype(np.float32), (rs.randn(64) * 0.1).astype(np.float32))
    y = ops.vgg_conv1_bf16(x, pk)
    p = ops.pool2d_bf16(y, 2, 2)
    assert tuple(y.shape) == (8, 600, 1000, 64) and tuple(p.shape) == (8, 300, 500, 64)
    for i in range(8):
        yi = ops.vgg_conv1_bf16(x[i:i + 1].contiguous(), pk)
        assert torch.equal(yi[0], y[i]), i
        assert torch.equal(ops.pool2d_bf16(yi, 2, 2)[0], p[i]), i


# ----------------------------------------------------------------------------- 7: the entry point
def named_image(name, px):
    from faster_rcnn_amd import shapes
    h, w = px.shape[:2]
    return shapes.Image(shapes.Metadata(name, w, h, [], "none"), px)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _pair(w, dtype, anchors):
    from faster_rcnn_amd import vgg
    from faster_rcnn_amd.data.voc_data_helpers import VOC_CLASS_MAPPING
    from faster_rcnn_amd.det_util import DetTrainingManager
    rpn = vgg.vgg16_rpn(vgg.vgg16_base(weights=w, dtype=dtype), include_conv=True, anchors_per_loc=9)
    det = vgg.vgg16_classifier(64, 21, weights=w, dtype=dtype)
    new_mgr = lambda: DetTrainingManager(rpn_model=rpn, class_mapping=VOC_CLASS_MAPPING, preprocess_func=vgg.preprocess, anchor_dims=anchors)
    return rpn, det, new_mgr


def test_entry_batches_the_bf16_vgg16_detector(monkeypatch):
    """voc_dets.get_dets_by_cls with a bf16 VGG16 pair on ten frames of one size at four images per pass (two whole passes, one
    padded): every image's detections equal, bit for bit, those of an engine that runs one image per pass without split-K; replaying
    the captured passes gives the same bits; the f32 VGG16 pair keeps one image per pass."""
    from faster_rcnn_amd import entry, util, vgg, voc_dets
    from faster_rcnn_amd.pipeline import InferencePipeline
    from faster_rcnn_amd.weights import calibrate_classifier, synthetic_vgg16
    monkeypatch.setattr(voc_dets, "CAPTURE_MIN", 1)
    anchors = util.get_anchors([128, 256, 512])
    w = synthetic_vgg16(anchors_per_loc=9, num_classes=21, seed=1)
    rpn, det, new_mgr = _pair(w, "bf16", anchors)
    rs = np.random.RandomState(99)
    # an untrained dense_class puts every RoI in one class: re-centre it on a calibration frame so that several classes fire
    cal = torch.from_numpy(vgg.preprocess(rs.randint(0, 256, (1, 320, 480, 3))).astype(np.float32)).cuda()
    out = InferencePipeline(rpn, det, anchors).forward_dev(cal)
    det.get_layer("dense_class_21").set_weights(calibrate_classifier(w, 21, out["cls"][:int(out["n_rois"].item())].cpu().numpy()))
    images = [named_image("v%02d" % i, rs.randint(0, 256, (320, 480, 3)).astype(np.uint8)) for i in range(10)]
    ratios = [1.0 + 0.01 * i for i in range(10)]

    monkeypatch.setenv("FRCNN_ENTRY_BATCH", "4")
    mgr4 = new_mgr()
    batched = quiet(voc_dets.get_dets_by_cls, mgr4, det, ratios, images, det_threshold=0.0)
    eng4 = entry.for_models(mgr4, det, 64, 16, entry.default_in_flight("bf16"))
    assert eng4.batch == 4 and eng4.stats()["images_per_pass"] == 4
    assert sum(len(v) for c in batched.values() for v in c.values()) > 0

    monkeypatch.setenv("FRCNN_ENTRY_BATCH", "1")
    monkeypatch.setenv("FRCNN_ENTRY_NO_SPLITK", "1")
    mgr1 = new_mgr()
    single = quiet(voc_dets.get_dets_by_cls, mgr1, det, ratios, images, det_threshold=0.0)
    assert entry.for_models(mgr1, det, 64, 16, entry.default_in_flight("bf16")).batch == 1

    def same(a, b):
        assert list(a) == list(b)
        for cls_name in a:
            assert list(a[cls_name]) == list(b[cls_name])
            for img in a[cls_name]:
                da, db = a[cls_name][img], b[cls_name][img]
                assert len(da) == len(db), (cls_name, img)
                for p, q in zip(da, db):
                    assert p["cls_name"] == q["cls_name"] and np.array_equal(p["bbox"], q["bbox"]) and float(p["prob"]) == float(q["prob"]), (p, q)
    same(batched, single)
    monkeypatch.setenv("FRCNN_ENTRY_BATCH", "4")
    same(quiet(voc_dets.get_dets_by_cls, mgr4, det, ratios, images, det_threshold=0.0), batched)       # the captured passes replayed
    assert not any(sl.busy for v in eng4.cache._slots.values() for sl in v)

    # the f32 VGG16 pair: one image per pass, as before
    _, det32, new_mgr32 = _pair(w, "f32", anchors)
    eng32 = entry.for_models(new_mgr32(), det32, 64, 16, entry.default_in_flight("f32"))
    assert eng32 is not None and eng32.batch == 1


# ----------------------------------------------------------------------------- 8: weights change, training refused
def test_set_weights_reaches_the_conv1_kernel_and_training_is_refused():
    from faster_rcnn_amd import _lib, train, vgg
    from faster_rcnn_amd.weights import synthetic_vgg16
    w = synthetic_vgg16(anchors_per_loc=9, seed=2, with_classifier=False)
    rpn = vgg.vgg16_rpn(vgg.vgg16_base(weights=w, dtype="bf16"), include_conv=True, anchors_per_loc=9)
    x = pixels(np.random.RandomState(1), 1, 64, 96)
    before = rpn.predict_on_batch(x)
    again = rpn.predict_on_batch(x)
    assert all(np.array_equal(a, b) for a, b in zip(before, again))
    k, b = rpn.get_layer("block1_conv1").get_weights()
    rpn.get_layer("block1_conv1").set_weights([k * 0.5, b + 0.25])
    after = rpn.predict_on_batch(x)
    assert not np.array_equal(before[2], after[2]) and not np.array_equal(before[0], after[0])
    rpn.get_layer("block1_conv1").set_weights([k, b])
    assert all(np.array_equal(a, c) for a, c in zip(before, rpn.predict_on_batch(x)))
    with pytest.raises(_lib.FrcnnError, match="VGG16 trains in f32; build the model with dtype='f32'"):
        rpn.compile(train.SGD(1e-3, 0.9))
    with pytest.raises(_lib.FrcnnError, match="VGG16 trains in f32; build the model with dtype='f32'"):
        rpn.train_on_batch(x, [np.zeros((1, 4, 6, 18)), np.zeros((1, 4, 6, 72))])
    det = vgg.vgg16_classifier(64, 21, base_model=rpn.base)
    assert det.head.dtype == "bf16"                                    # a classifier built on a base inherits its dtype
    with pytest.raises(_lib.FrcnnError, match="VGG16 trains in f32"):
        det.compile(train.SGD(1e-3, 0.9))
