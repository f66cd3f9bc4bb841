"""VGG16 canvas passes on the GPU: images of different true sizes, each in the corner (offset (0, 0)) of a canvas of fixed shape, with the
true sizes as device values (nets.VggExtents).  The two new kernels against the existing ones on the true-size tensors (bit for bit
inside the extent, exact zeros outside, garbage beyond the extent never read), a canvas pass against the passes of the true sizes
(f32 engines: the bars tests/test_canvas_gpu.py holds the ResNet canvas to; bf16: bit for bit), a canvas pass against the ORACLE at the
true sizes, the entry point on a shuffled list of many sizes, and a weight change reaching the captured canvas pass."""
import contextlib
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MEAN = (103.939, 116.779, 123.68)


def _u8(h, w, seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)).cuda()


def _hw(sizes):
    return torch.tensor([list(s) for s in sizes], dtype=torch.int32, device="cuda")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _poison(shape, dtype):
    """Large values, infinities and NaN bit patterns: anything a kernel lets through from beyond the extent shows."""
    vals = torch.tensor([3.0e38, float("nan"), float("-inf"), -1.0e30, float("inf"), 7.0], dtype=torch.float32, device="cuda").to(dtype)
    n = int(np.prod(shape))
    return vals.repeat(n // vals.numel() + 1)[:n].reshape(shape).contiguous()


def _canvas_of(true_tensors, hc, wc, dtype):
    """A canvas batch whose corners hold the given (h, w, c) tensors and whose every other cell is poison."""
    c = true_tensors[0].shape[-1]
    x = _poison((len(true_tensors), hc, wc, c), dtype)
    for i, t in enumerate(true_tensors):
        x[i, :t.shape[0], :t.shape[1]] = t
    return x


def _pool_true(t, dtype):
    from faster_rcnn_amd import ops
    t = t[None].contiguous()
    return (ops.pool2d_bf16(t, 2, 2) if dtype == torch.bfloat16 else ops.pool2d(t, 2, 2, True))[0]


def _pool_ext(x, hw, dtype):
    from faster_rcnn_amd import ops
    return ops.pool2d_bf16_extents(x, hw) if dtype == torch.bfloat16 else ops.pool2d_extents(x, hw)


def _check_pool(x, sizes, out, dtype):
    n, hc, wc, c = x.shape
    assert tuple(out.shape) == (n, hc // 2, wc // 2, c) and out.dtype == dtype
    for i, (h, w) in enumerate(sizes):
        if h // 2 and w // 2:                                                          # (else: no pooled cell lies inside the true map)
            want = _pool_true(x[i, :h, :w], dtype)
            assert tuple(want.shape) == (h // 2, w // 2, c)
            assert torch.equal(_bits(out[i, :h // 2, :w // 2]), _bits(want)), i       # bit for bit (NaN-safe: compared as integers)
        rest = _bits(out[i]).clone()
        rest[:h // 2, :w // 2] = 0
        assert int(rest.ne(0).sum()) == 0, i                                           # +0.0 everywhere else, odd sides' extra row / column too


# ----------------------------------------------------------------------------- the pool with extents
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", [((2, 20, 24, 64), [(20, 24), (13, 17)]), ((1, 302, 500, 128), [(301, 499)]), ((3, 6, 8, 8), [(0, 0), (1, 8), (6, 1)])],
                         ids=["20x24x64", "302x500x128", "degenerate"])
def test_pool_with_extents_known_answers(case, dtype):
    """Inside floor(h/2) x floor(w/2): torch.equal to the existing pool of the cropped true-size tensor.  Outside: exactly 0, including
    row floor(h/2) / column floor(w/2) of an odd side.  The input beyond the extent is poison (3e38, NaN, +-inf)."""
    shape, sizes = case
    rs = np.random.RandomState(shape[1] * 7 + shape[2])
    true = [torch.from_numpy(rs.randn(h, w, shape[3]).astype(np.float32)).cuda().to(dtype) for h, w in sizes]
    x = _canvas_of(true, shape[1], shape[2], dtype)
    out = _pool_ext(x, _hw(sizes), dtype)
    _check_pool(x, sizes, out, dtype)
    # extents beyond the canvas are clamped to it: the whole canvas is the image
    full = torch.from_numpy(rs.randn(*shape).astype(np.float32)).cuda().to(dtype)
    out = _pool_ext(full, _hw([(10 ** 6, 10 ** 6)] * shape[0]), dtype)
    _check_pool(full, [(shape[1], shape[2])] * shape[0], out, dtype)


def test_pool_with_extents_refuses_what_it_cannot_serve():
    from faster_rcnn_amd import _lib, ops
    hw = _hw([(4, 4)])
    with pytest.raises(_lib.FrcnnError):
        ops.pool2d_bf16_extents(torch.zeros((1, 4, 4, 12), dtype=torch.bfloat16, device="cuda"), hw)      # C % 8
    with pytest.raises(_lib.FrcnnError):
        ops.pool2d_extents(torch.zeros((1, 4, 4, 6), dtype=torch.float32, device="cuda"), hw)             # C % 4
    with pytest.raises(_lib.FrcnnError):
        ops.pool2d_extents(torch.zeros((1, 1, 4, 8), dtype=torch.float32, device="cuda"), hw)             # smaller than the window


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_pool_with_extents_at_eight_full_size_images(dtype):
    """n = 8 at 600 x 1000 x 64 (the shape whose unmasked launch goes a second trip round its capped grid; element offsets pass 2^28):
    eight different extents, against one existing launch per cropped image."""
    sizes = [(600, 1000), (599, 999), (375, 500), (600, 801), (333, 1000), (2, 2), (601 - 2, 3), (450, 600)]
    x = torch.randn((8, 600, 1000, 64), dtype=torch.float32, device="cuda").to(dtype)
    x[5:7] = _poison((2, 600, 1000, 64), dtype)
    for i in (5, 6):
        h, w = sizes[i]
        x[i, :h, :w] = 1.0 + i
    out = _pool_ext(x, _hw(sizes), dtype)
    _check_pool(x, sizes, out, dtype)


# ----------------------------------------------------------------------------- block1_conv1 with extents
@pytest.mark.parametrize("sizes,canvas", [([(37, 53), (48, 64)], (48, 64)), ([(131, 300), (90, 517), (1, 1)], (132, 520))], ids=["48x64", "132x520"])
def test_conv1_with_extents_equals_the_true_size_launch(sizes, canvas):
    """Images of different odd / even sizes in one launch (the second case crosses the workgroup's 256-pixel run twice): inside the
    extent bit-equal to frcnn_vgg_conv1_bf16_fwd on the true-size image, outside exactly zero; the canvas beyond the extent is poison."""
    from faster_rcnn_amd import ops
    rs = np.random.RandomState(17)
    pk = ops.PackedVggConv1Bf16((rs.randn(3, 3, 3, 64) * np.sqrt(2.0 / 27) / 70.0).astype(np.float32), (rs.randn(64) * 0.1).astype(np.float32))
    true = [ops.preprocess_u8(_u8(h, w, 60 + k), MEAN)[0] for k, (h, w) in enumerate(sizes)]
    x = _canvas_of(true, canvas[0], canvas[1], torch.float32)
    out = ops.vgg_conv1_bf16_extents(x, pk, _hw(sizes))
    assert tuple(out.shape) == (len(sizes),) + canvas + (64,) and out.dtype == torch.bfloat16
    for i, (t, (h, w)) in enumerate(zip(true, sizes)):
        want = ops.vgg_conv1_bf16(t[None].contiguous(), pk)[0]
        assert torch.equal(_bits(out[i, :h, :w]), _bits(want)), i
        assert float(want.float().abs().max()) > 0.0
        rest = _bits(out[i]).clone()
        rest[:h, :w] = 0
        assert int(rest.ne(0).sum()) == 0, i
    # the existing entry point is what it was: a canvas of zeros around the image is not masked by it (bias + ReLU outside)
    plain = ops.vgg_conv1_bf16(torch.zeros((1, 8, 8, 3), dtype=torch.float32, device="cuda"), pk)
    assert float(plain.float().abs().max()) > 0.0


# ----------------------------------------------------------------------------- a canvas pass against the passes of the true sizes
PASS_CASES = [([(320, 480), (304, 450)], (320, 480)), ([(321, 479), (289, 451)], (352, 480)), ([(306, 451), (319, 417)], (320, 512))]


@pytest.fixture(scope="module")
def vgg_pairs():
    from faster_rcnn_amd import util, vgg
    from faster_rcnn_amd.weights import synthetic_vgg16
    anchors = util.get_anchors([128, 256, 512])
    w = synthetic_vgg16(anchors_per_loc=9, num_classes=21, seed=11)
    pairs = {}
    for dtype in ("f32", "bf16"):
        rpn = vgg.vgg16_rpn(vgg.vgg16_base(weights=w, dtype=dtype), include_conv=True, anchors_per_loc=9)
        pairs[dtype] = (rpn, vgg.vgg16_classifier(64, 21, weights=w, dtype=dtype))
    return pairs, anchors, w


def _canvases(imgs, sizes, canvas):
    from faster_rcnn_amd import nets, ops
    Hc, Wc = canvas
    x = torch.empty((len(imgs), Hc, Wc, 3), dtype=torch.float32, device="cuda")
    ext = nets.VggExtents(len(imgs))
    for i, (im, (h, w)) in enumerate(zip(imgs, sizes)):
        assert h <= Hc and w <= Wc
        ops.preprocess_u8_canvas(im, MEAN, x[i], offset=nets.VggExtents.offset_of(h, w))
        ext.set(i, h, w)
    ext.upload()
    return x, ext


def _outside_is_zero(feat, R, C):
    outside = torch.cat([feat[R:].reshape(-1), feat[:, C:].reshape(-1)])
    return outside.numel() == 0 or int(_bits(outside).ne(0).sum()) == 0


@pytest.mark.parametrize("engine", ["native", "f16x3"])
@pytest.mark.parametrize("sizes,canvas", PASS_CASES)
def test_f32_canvas_pass_equals_the_passes_of_the_true_sizes(vgg_pairs, engine, sizes, canvas):
    """The VGG16 twin of test_canvas_pass_equals_the_passes_of_the_true_sizes, f32: base + RPN over BOTH canvases in one batch, then --
    the f32 VGG16 detector keeps one image per pass -- one canvas pass per image, against each image's own pass at its true size on
    the same engine without split-K: map and RPN outputs inside the extents to 1e-5 x max(1, max|b|), exact zeros outside, identical
    proposals, boxes and classes, scores to 1e-5; the f16x3 pass's fence word reads 0."""
    from faster_rcnn_amd import nets, ops
    from faster_rcnn_amd.pipeline import InferencePipeline
    pairs, anchors, _ = vgg_pairs
    rpn, det = pairs["f32"]
    imgs = [_u8(h, w, 40 + k) for k, (h, w) in enumerate(sizes)]
    dyn = torch.tensor([[1.0, 0.0], [1.0, 0.0]], dtype=torch.float64, device="cuda")
    close = lambda a, b: float((a - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max()))
    arena = lambda: ops.AmaxArena() if engine == "f16x3" else None
    x2, ext2 = _canvases(imgs, sizes, canvas)
    with ops.f32_engine(engine), ops.conv_workspace(ops.NO_SPLIT_K), ops.amax_arena(arena()):
        ops.amax_begin()
        both = dict(zip(("rpn_cls", "rpn_reg", "feat"), rpn.forward_dev(x2, ext2)))
    for i, (im, (h, w)) in enumerate(zip(imgs, sizes)):
        x1, ext1 = _canvases([im], [(h, w)], canvas)
        with ops.f32_engine(engine), ops.conv_workspace(ops.NO_SPLIT_K), ops.amax_arena(arena()):
            out = InferencePipeline(rpn, det, anchors, max_proposals=300).forward_dev(x1, dyn=dyn[i], extents=ext1)
            if engine == "f16x3":
                assert int(out["h3_status"].item()) == 0
        with ops.f32_engine(engine), ops.conv_workspace(ops.NO_SPLIT_K), ops.amax_arena(arena()):
            one = InferencePipeline(rpn, det, anchors, max_proposals=300).forward_dev(ops.preprocess_u8(im, MEAN), dyn=dyn[i])
            if engine == "f16x3":
                assert int(one["h3_status"].item()) == 0
        R, C = nets.VggExtents.levels_of(h, w)[4]
        assert tuple(one["feat"].shape[1:3]) == (R, C)
        for k in ("feat", "rpn_cls", "rpn_reg"):
            a, a2, b = out[k][0][:R, :C].float(), both[k][i][:R, :C].float(), one[k][0].float()
            print(engine, sizes[i], k, "canvas pass - exact pass: %.3g (batch of two: %.3g), max|b| %.3g" % (float((a - b).abs().max()), float((a2 - b).abs().max()), float(b.abs().max())))
            assert close(a, b) and close(a2, b), (k, i)
        assert _outside_is_zero(out["feat"][0], R, C) and _outside_is_zero(both["feat"][i], R, C)
        n = int(one["n_rois"].item())
        assert int(out["n_rois"].item()) == n > 0
        assert torch.equal(out["rois"][:n], one["rois"][:n])
        nd = int(one["n_dets"].item())
        assert int(out["n_dets"].item()) == nd
        assert torch.equal(out["det_bbox"][:nd], one["det_bbox"][:nd]) and torch.equal(out["det_cls"][:nd], one["det_cls"][:nd])
        assert nd == 0 or float((out["det_prob"][:nd] - one["det_prob"][:nd]).abs().max()) <= 1e-5


@pytest.mark.parametrize("sizes,canvas", PASS_CASES)
def test_bf16_canvas_pass_equals_the_passes_of_the_true_sizes_bit_for_bit(vgg_pairs, sizes, canvas):
    """bf16, two canvases in one batched pass, no split-K, against each image's own one-image pass: BIT FOR BIT -- the map, rpn_cls and
    rpn_reg inside the extents, the proposals, the detections and their scores.  (Each stored cell is one f32 accumulation in a fixed
    k order, rounded once; a canvas changes only M and the tile count, as batching does.)"""
    from faster_rcnn_amd import nets, ops
    from faster_rcnn_amd.pipeline import BatchedInferencePipeline, InferencePipeline
    pairs, anchors, _ = vgg_pairs
    rpn, det = pairs["bf16"]
    imgs = [_u8(h, w, 40 + k) for k, (h, w) in enumerate(sizes)]
    x, ext = _canvases(imgs, sizes, canvas)
    dyn = torch.tensor([[1.0, 0.0], [1.0, 0.0]], dtype=torch.float64, device="cuda")
    with ops.conv_workspace(ops.NO_SPLIT_K):
        out = BatchedInferencePipeline(rpn, det, anchors, 2, max_proposals=300).forward_dev(x, dyn=dyn, extents=ext)
        assert out["feat"].dtype == torch.bfloat16
        for i, (im, (h, w)) in enumerate(zip(imgs, sizes)):
            one = InferencePipeline(rpn, det, anchors, max_proposals=300).forward_dev(ops.preprocess_u8(im, MEAN), dyn=dyn[i])
            R, C = nets.VggExtents.levels_of(h, w)[4]
            assert tuple(one["feat"].shape[1:3]) == (R, C)
            for k in ("feat", "rpn_cls", "rpn_reg"):
                a, b = out[k][i][:R, :C], one[k][0]
                print("bf16", sizes[i], k, "canvas pass - exact pass: %.3g" % float((a.float() - b.float()).abs().max()))
                assert torch.equal(_bits(a), _bits(b)), (k, i)
            assert _outside_is_zero(out["feat"][i], R, C)
            n = int(one["n_rois"].item())
            assert int(out["n_rois"][i].item()) == n > 0
            assert torch.equal(out["rois"][i][:n], one["rois"][:n])
            nd = int(one["n_dets"].item())
            assert int(out["n_dets"][i].item()) == nd
            assert torch.equal(out["det_bbox"][i][:nd], one["det_bbox"][:nd]) and torch.equal(out["det_cls"][i][:nd], one["det_cls"][:nd])
            assert torch.equal(out["det_prob"][i][:nd], one["det_prob"][:nd])


# ----------------------------------------------------------------------------- against the oracle
ORACLE_SIZES, ORACLE_CANVAS = [(131, 176), (120, 151)], (160, 192)


def _oracle_inputs():
    rs = np.random.RandomState(0)
    return [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ORACLE_SIZES]


def test_f32_canvas_pass_against_the_oracle():
    """One canvas pass with two different true sizes; each image's map / cls / reg inside its extent against oracle.keras_ref's VGG16 +
    RPN head in f64 at the image's TRUE size: 1e-4 (north_star, the bar and the error measure of tests/test_nets_gpu.py)."""
    from faster_rcnn_amd import nets, ops, vgg
    from faster_rcnn_amd.weights import synthetic_vgg16
    from oracle.keras_ref import KerasGraphs
    from tests.test_nets_gpu import TOL, rel_err
    w = synthetic_vgg16(anchors_per_loc=9, seed=4, with_classifier=False)
    rpn = vgg.vgg16_rpn(vgg.vgg16_base(weights=w), include_conv=True, anchors_per_loc=9)
    raw = _oracle_inputs()
    x, ext = _canvases([torch.from_numpy(r).cuda() for r in raw], ORACLE_SIZES, ORACLE_CANVAS)
    with ops.f32_engine("native"):
        cls, reg, feat = rpn.forward_dev(x, ext)
    ref = KerasGraphs(w, torch.float64)
    for i, (r, (h, wd)) in enumerate(zip(raw, ORACLE_SIZES)):
        f64 = ref.vgg_base((r.astype(np.float64) - np.array(MEAN))[None])
        c64, r64 = ref.rpn(f64)
        R, C = nets.VggExtents.levels_of(h, wd)[4]
        assert tuple(f64.shape[1:3]) == (R, C)
        figs = [rel_err(t[i, :R, :C].cpu(), want[0]) for t, want in ((feat, f64), (cls, c64), (reg, r64))]
        print("f32 canvas pass against the f64 oracle at %s (map, cls, reg): %s" % ((h, wd), figs))
        assert all(f < TOL for f in figs), (i, figs)
        assert _outside_is_zero(feat[i], R, C)


def test_bf16_canvas_pass_against_the_oracle():
    """The same in bf16: against the f64 oracle under the bars of a bf16 network against unrounded arithmetic (tests/test_vgg_bf16_gpu.py:
    relative RMS <= 2e-2, max <= 5e-2 x max|x|), and against the oracle under the product's storage model (tests/vgg_bf16_ref.py) under
    that file's MODEL_BARS, which were measured at image 0's size and seed."""
    from faster_rcnn_amd import nets, vgg
    from faster_rcnn_amd.weights import synthetic_vgg16
    from oracle.keras_ref import KerasGraphs
    from tests.test_vgg_bf16_gpu import MODEL_BARS, err, within
    from tests.vgg_bf16_ref import VggBf16Graphs
    w = synthetic_vgg16(anchors_per_loc=9, seed=3, with_classifier=False)
    rpn = vgg.vgg16_rpn(vgg.vgg16_base(weights=w, dtype="bf16"), include_conv=True, anchors_per_loc=9)
    raw = _oracle_inputs()
    x, ext = _canvases([torch.from_numpy(r).cuda() for r in raw], ORACLE_SIZES, ORACLE_CANVAS)
    cls, reg, feat = rpn.forward_dev(x, ext)
    ref, model = KerasGraphs(w, torch.float64), VggBf16Graphs(w, torch.float64, mixed=True)
    for i, (r, (h, wd)) in enumerate(zip(raw, ORACLE_SIZES)):
        xi = (r.astype(np.float64) - np.array(MEAN))[None]
        R, C = nets.VggExtents.levels_of(h, wd)[4]
        got = {"feat": feat[i, :R, :C].float().cpu()[None], "cls": cls[i, :R, :C].cpu()[None], "reg": reg[i, :R, :C].cpu()[None]}
        f64 = ref.vgg_base(xi)
        c64, r64 = ref.rpn(f64)
        assert tuple(f64.shape[1:3]) == (R, C)
        print("bf16 canvas pass against the f64 oracle at %s (rms, max): %s" % ((h, wd), {k: err(got[k], v) for k, v in (("feat", f64), ("cls", c64), ("reg", r64))}))
        assert within(got["feat"], f64) and within(got["cls"], c64) and within(got["reg"], r64), i
        fm = model.vgg_base(xi)
        cm, rm = model.rpn(fm)
        figs = {"feat": err(got["feat"], fm), "cls": err(got["cls"], cm), "reg": err(got["reg"], rm)}
        print("bf16 canvas pass against the f64 storage model at %s (rms, max): %s" % ((h, wd), figs))
        for k, (rms, mx) in figs.items():
            assert rms <= MODEL_BARS[k][0] and mx <= MODEL_BARS[k][1], (i, k, rms, mx)
        assert _outside_is_zero(feat[i], R, C)


# ----------------------------------------------------------------------------- the entry point
def named_image(name, px):
    from faster_rcnn_amd import shapes
    h, w = px.shape[:2]
    return shapes.Image(shapes.Metadata(name, w, h, [], "none"), px)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _manager(rpn, anchors):
    from faster_rcnn_amd import vgg
    from faster_rcnn_amd.data.voc_data_helpers import VOC_CLASS_MAPPING
    from faster_rcnn_amd.det_util import DetTrainingManager
    return DetTrainingManager(rpn_model=rpn, class_mapping=VOC_CLASS_MAPPING, preprocess_func=vgg.preprocess, anchor_dims=anchors)


def _calibrated_pair(dtype, seed):
    from faster_rcnn_amd import util, vgg
    from faster_rcnn_amd.pipeline import InferencePipeline
    from faster_rcnn_amd.weights import calibrate_classifier, synthetic_vgg16
    anchors = util.get_anchors([128, 256, 512])
    w = synthetic_vgg16(anchors_per_loc=9, num_classes=21, seed=seed)
    rpn = vgg.vgg16_rpn(vgg.vgg16_base(weights=w, dtype=dtype), include_conv=True, anchors_per_loc=9)
    det = vgg.vgg16_classifier(64, 21, weights=w, dtype=dtype)
    # an untrained dense_class puts every RoI in one class: re-centre it on a calibration frame so that several classes fire
    cal = torch.from_numpy(vgg.preprocess(np.random.RandomState(99).randint(0, 256, (1, 320, 480, 3))).astype(np.float32)).cuda()
    out = InferencePipeline(rpn, det, anchors).forward_dev(cal)
    det.get_layer("dense_class_21").set_weights(calibrate_classifier(w, 21, out["cls"][:int(out["n_rois"].item())].cpu().numpy()))
    return rpn, det, anchors


def _entry_list():
    from tests.test_vgg_canvas_cpu import ENTRY_SIZES
    rs = np.random.RandomState(23)
    images, ratios = [], []
    for k in range(2 * len(ENTRY_SIZES)):
        h, w = ENTRY_SIZES[k % len(ENTRY_SIZES)]
        images.append(named_image("m%02d" % k, rs.randint(0, 256, (h, w, 3)).astype(np.uint8)))
        ratios.append(1.0 + 0.01 * k)
    order = rs.permutation(len(images))
    return [images[i] for i in order], [ratios[i] for i in order]


def _same_lists(a, b, tol):
    assert list(a) == list(b) and sum(len(v) for c in a.values() for v in c.values()) > 0
    by_box = lambda lst: sorted(lst, key=lambda d: tuple(int(v) for v in d["bbox"])) if tol else lst
    for cls_name in a:
        assert list(a[cls_name]) == list(b[cls_name])
        for img in a[cls_name]:
            da, db = by_box(a[cls_name][img]), by_box(b[cls_name][img])
            assert len(da) == len(db), (cls_name, img)
            for p, q in zip(da, db):
                assert p["cls_name"] == q["cls_name"] and np.array_equal(p["bbox"], q["bbox"]), (p, q)
                assert abs(float(p["prob"]) - float(q["prob"])) <= tol, (p, q)


@pytest.mark.parametrize("dtype,engine", [("f32", "f16x3"), ("f32", "native"), ("bf16", "f16x3")])
def test_get_dets_by_cls_serves_a_mixed_vgg16_list_from_canvas_passes(dtype, engine, monkeypatch):
    """voc_dets.get_dets_by_cls on a shuffled list of 14 frames over 7 geometries (even and odd sides): the f32 VGG16 pair at one image
    per pass, the bf16 pair at its eight.  The planner puts the list on at most three canvas classes (asserted on the plan); no image
    takes the eager path; the captures stay within the planned classes' slot allowance; the results equal those of the same list
    with FRCNN_ENTRY_CANVAS=0 (one image per exact pass, no split-K) -- f32: boxes and classes identical, scores to 1e-5 (two
    detections whose scores are closer than that may swap places: compared by box); bf16: bit for bit, in order."""
    from faster_rcnn_amd import entry, voc_dets
    from tests.test_vgg_canvas_cpu import entry_histogram
    monkeypatch.setattr(voc_dets, "CAPTURE_MIN", 1)
    monkeypatch.setenv("FRCNN_ENTRY_NO_SPLITK", "1")
    monkeypatch.setenv("FRCNN_F32_ENGINE", engine)                                     # (read when an engine is built: both lists' engines)
    monkeypatch.setenv("FRCNN_ENTRY_CANVAS", "1")                                      # VGG16 canvases are opt-in
    rpn, det, anchors = _calibrated_pair(dtype, seed=1)
    images, ratios = _entry_list()
    assert len(images) >= 12 and len({im.data.shape[:2] for im in images}) >= 6 and all(im.data.shape[0] <= 330 and im.data.shape[1] <= 512 for im in images)
    plan = entry.plan_canvas_classes(entry_histogram())
    assert 1 <= len(set(plan.values())) <= 3, plan

    eager_seen = []
    real = voc_dets._get_dets_eager
    monkeypatch.setattr(voc_dets, "_get_dets_eager", lambda *a, **k: (eager_seen.append(a[2].name), real(*a, **k))[1])
    mgr = _manager(rpn, anchors)
    fast = quiet(voc_dets.get_dets_by_cls, mgr, det, ratios, images, det_threshold=0.1)
    eng = entry.for_models(mgr, det, 64, 16, entry.default_in_flight(dtype))
    assert eng.canvas_capable and eng.canvas and eng.batch == (8 if dtype == "bf16" else 1) and eng.f32_engine == engine
    assert eager_seen == []                                                            # no image takes the eager path
    keys = eng.cache.keys()
    assert keys and all(k[0] == "canvas" for k in keys), keys
    classes = {k[1:3] for k in keys}
    assert classes <= set(plan.values())
    st = eng.stats()
    allowance = sum(st["canvas_slots"]["%dx%d" % c] for c in set(plan.values()))
    print(dtype, engine, "classes", sorted(classes), "captures", st["captures"], "allowance", allowance, "bytes", st["bytes"])
    assert 1 <= st["captures"] <= allowance and st["images_per_pass"] == eng.batch

    # the same list through exact passes: canvases off, one image per pass
    monkeypatch.setenv("FRCNN_ENTRY_CANVAS", "0")
    monkeypatch.setenv("FRCNN_ENTRY_BATCH", "1")
    mgr0 = _manager(rpn, anchors)
    exact = quiet(voc_dets.get_dets_by_cls, mgr0, det, ratios, images, det_threshold=0.1)
    eng0 = entry.for_models(mgr0, det, 64, 16, entry.default_in_flight(dtype))
    assert not eng0.canvas_capable and not eng0.canvas and eng0.batch == 1 and eager_seen == []
    assert all(k[0] != "canvas" for k in eng0.cache.keys()) and eng0.stats()["captures"] >= 7
    _same_lists(fast, exact, 1e-5 if dtype == "f32" else 0.0)
    eng0.cache.clear()

    # the same call again re-uses the passes and returns the same bits
    again = quiet(voc_dets.get_dets_by_cls, mgr, det, ratios, images, det_threshold=0.1)
    assert eng.stats()["captures"] == st["captures"] and eager_seen == []
    _same_lists(again, fast, 0.0)
    assert not any(sl.busy for v in eng.cache._slots.values() for sl in v)
    eng.cache.clear()


def test_changed_conv1_weights_reach_the_canvas_pass(monkeypatch):
    """get_layer("block1_conv1").set_weights drops the captured canvas passes (weights epoch); the re-captured pass runs the extents
    variant of conv1 on the NEW packed filter: its results change, and equal the exact passes of the changed model bit for bit."""
    from faster_rcnn_amd import entry, voc_dets
    monkeypatch.setattr(voc_dets, "CAPTURE_MIN", 1)
    monkeypatch.setenv("FRCNN_ENTRY_NO_SPLITK", "1")
    rpn, det, anchors = _calibrated_pair("bf16", seed=2)
    images, ratios = _entry_list()
    # opt-in: without FRCNN_ENTRY_CANVAS a VGG16 engine keeps the exact-geometry passes, a ResNet one has canvases by default
    monkeypatch.delenv("FRCNN_ENTRY_CANVAS", raising=False)
    assert not entry.for_models(_manager(rpn, anchors), det, 64, 16, entry.default_in_flight("bf16")).canvas_capable
    from faster_rcnn_amd import nets
    assert nets.ResNetBase.canvas_by_default and not nets.VggBase.canvas_by_default
    monkeypatch.setenv("FRCNN_ENTRY_CANVAS", "1")
    mgr = _manager(rpn, anchors)
    before = quiet(voc_dets.get_dets_by_cls, mgr, det, ratios, images, det_threshold=0.1)
    eng = entry.for_models(mgr, det, 64, 16, entry.default_in_flight("bf16"))
    assert eng.canvas and all(k[0] == "canvas" for k in eng.cache.keys())
    captures = eng.stats()["captures"]
    k, b = rpn.get_layer("block1_conv1").get_weights()
    rpn.get_layer("block1_conv1").set_weights([k * 0.5, b + 0.25])
    after = quiet(voc_dets.get_dets_by_cls, mgr, det, ratios, images, det_threshold=0.1)
    assert eng.stats()["captures"] > captures and all(k_[0] == "canvas" for k_ in eng.cache.keys())
    flat = lambda d: [(c, i, tuple(int(v) for v in x["bbox"]), float(x["prob"])) for c in d for i in d[c] for x in d[c][i]]
    assert flat(before) != flat(after)
    monkeypatch.setenv("FRCNN_ENTRY_CANVAS", "0")
    monkeypatch.setenv("FRCNN_ENTRY_BATCH", "1")
    mgr0 = _manager(rpn, anchors)
    exact = quiet(voc_dets.get_dets_by_cls, mgr0, det, ratios, images, det_threshold=0.1)
    eng0 = entry.for_models(mgr0, det, 64, 16, entry.default_in_flight("bf16"))
    assert not eng0.canvas
    _same_lists(after, exact, 0.0)
    eng0.cache.clear()
    eng.cache.clear()
