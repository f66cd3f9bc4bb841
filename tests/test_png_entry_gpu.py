"""The device PNG encoder inside the detection entry's annotating passes (entry.DetectionEntry.submit_batch(annotate=True, encode="png"))
and behind ``annotate_video --png_encoder device``: the files decode to what the raw annotating pass returns, the dets are the same, the
printed lines are the same, and the existing passes keep their cache keys."""
import contextlib
import io
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
PilImage = pytest.importorskip("PIL.Image")

B = 4


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()) as buf:
        res = fn(*a, **k)
    return res, buf.getvalue()


def same_dets(a, b, tol=1e-4):
    """tests/test_entry_gpu.py's bar: classes and boxes identical, in order; scores within ``tol``."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x["cls_name"] == y["cls_name"] and np.array_equal(x["bbox"], y["bbox"]), (x, y)
        assert abs(float(x["prob"]) - float(y["prob"])) <= tol, (x, y)


def frame_pixels(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


@pytest.fixture(scope="module")
def f32_models():
    """tests/test_annotate_gpu.py's recipe: the small synthetic ResNet-50 with a calibrated classifier, and its manager."""
    from faster_rcnn_amd import resnet, util
    from faster_rcnn_amd.data.voc_data_helpers import VOC_CLASS_MAPPING
    from faster_rcnn_amd.det_util import DetTrainingManager
    from faster_rcnn_amd.pipeline import InferencePipeline
    from faster_rcnn_amd.weights import calibrate_classifier, synthetic_resnet
    anchors = util.get_anchors([128, 256, 512])
    w = synthetic_resnet(50, anchors_per_loc=9, num_classes=21, seed=1)
    rpn = resnet.resnet50_rpn(resnet.resnet50_base(weights=w), include_conv=True, anchors_per_loc=9)
    det = resnet.resnet50_classifier(64, 21, weights=w)
    x = resnet.preprocess(frame_pixels(320, 480, 99))[None].astype(np.float32)
    out = InferencePipeline(rpn, det, anchors).forward_dev(torch.from_numpy(x).cuda())
    n = int(out["n_rois"].item())
    det.get_layer("dense_class_21").set_weights(calibrate_classifier(w, 21, out["cls"][:n].cpu().numpy()))
    mgr = DetTrainingManager(rpn_model=rpn, class_mapping=VOC_CLASS_MAPPING, preprocess_func=resnet.preprocess, anchor_dims=anchors)
    return mgr, det, w


def _named(name, pixels=None, path=None, size=None):
    from faster_rcnn_amd import shapes
    h, w = pixels.shape[:2] if pixels is not None else size
    return shapes.Image(shapes.Metadata(name, w, h, [], path or "none"), pixels)


def _by_image(by_cls):
    return {(c, name): dets for c, per in by_cls.items() for name, dets in per.items()}


def test_encoding_passes(f32_models, tmp_path, monkeypatch):
    """Four 200x330 frames per pass, in memory (BGR) and as files (uploaded RGB): the encoding pass returns the dets of the raw annotating
    pass and files that decode to its frames in RGB order; each kind of pass has a cache key of its own; get_dets_by_cls is undisturbed."""
    from faster_rcnn_amd import entry, ops, util, voc_dets
    monkeypatch.setattr(voc_dets, "CAPTURE_MIN", 1)
    mgr, det, _ = f32_models
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight("f32"))
    assert eng.batch == B
    srcs = [frame_pixels(200, 330, 300 + i) for i in range(B)]
    mem = [_named("m%d" % i, pixels=s) for i, s in enumerate(srcs)]
    files = []
    for i, s in enumerate(srcs):
        p = str(tmp_path / ("f%d.png" % i))
        PilImage.fromarray(s[:, :, ::-1]).save(p)                        # the same BGR frame, as a file
        files.append(_named("f%d" % i, path=p, size=s.shape[:2]))
    for kind, imgs in (("mem", mem), ("file", files)):
        resized, ratios = util.resize_imgs(imgs, min_size=320, max_size=540)
        before, _ = quiet(voc_dets.get_dets_by_cls, mgr, det, ratios, resized)
        pixels = [eng.host_pixels(r) for r in resized]
        assert bool(pixels[0][4] & 2) == (kind == "file")
        raw = eng.collect_batch(eng.submit_batch(resized, ratios, 0.0, pixels, batch=B, annotate=True))
        enc = eng.collect_batch(eng.submit_batch(resized, ratios, 0.0, pixels, batch=B, annotate=True, encode="png"))
        again = eng.collect_batch(eng.submit_batch(resized, ratios, 0.0, pixels, batch=B, annotate=True, encode="png"))
        assert len(raw) == len(enc) == B and all(len(r) == 3 for r in enc)
        drawn_any = False
        for (n0, d0, frame), (n1, d1, png), (_, _, png2), src in zip(raw, enc, again, srcs):
            assert n0 == n1
            same_dets(d1, d0, tol=0.0)
            assert isinstance(png, bytes) and 0 < len(png) <= ops.png_bound(*frame.shape[:2]) and png == png2
            img = PilImage.open(io.BytesIO(png))
            assert img.mode == "RGB" and img.size == (frame.shape[1], frame.shape[0])
            assert np.array_equal(np.asarray(img), frame[:, :, ::-1] if kind == "mem" else frame), kind
            drawn_any |= bool((frame != (src if kind == "mem" else src[:, :, ::-1])).any())
        assert drawn_any
        after, _ = quiet(voc_dets.get_dets_by_cls, mgr, det, ratios, resized)
        a, b = _by_image(after), _by_image(before)
        assert list(a) == list(b)
        for k in a:
            same_dets(a[k], b[k], tol=0.0)
    keys = eng.cache.keys()
    assert sum(k[-1:] == ("annotate",) for k in keys) == 2 and sum(k[-2:] == ("annotate", "png") for k in keys) == 2
    assert any("annotate" not in k for k in keys)


def test_encode_needs_annotate(f32_models):
    from faster_rcnn_amd import entry, util
    from faster_rcnn_amd._lib import FrcnnError
    mgr, det, _ = f32_models
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight("f32"))
    resized, ratios = util.resize_imgs([_named("x", pixels=frame_pixels(200, 330, 1))], min_size=320, max_size=540)
    pixels = [eng.host_pixels(resized[0])]
    captures = eng.cache.captures
    with pytest.raises(FrcnnError):
        eng.submit_batch(resized, ratios, 0.0, pixels, batch=1, encode="png")
    with pytest.raises(FrcnnError):
        eng.submit_batch(resized, ratios, 0.0, pixels, batch=1, annotate=True, encode="jpeg")
    assert eng.cache.captures == captures


def test_main_png_encoder_device(f32_models, tmp_path):
    """``annotate_video --png_encoder device`` against ``--png_encoder host`` on three small PNG files: the same printed lines, the same
    file names, the same pixels."""
    from faster_rcnn_amd import annotate_video
    from faster_rcnn_amd.weights import save_npz
    _, _, w = f32_models
    npz = str(tmp_path / "w.npz")
    save_npz(npz, w)
    d_in = tmp_path / "frames"
    d_in.mkdir()
    names = ["%06d.png" % i for i in range(3)]
    for i, name in enumerate(names):
        PilImage.fromarray(frame_pixels(180, 260, 40 + i)).save(str(d_in / name))
    text = {}
    for enc in ("host", "device"):
        argv = [npz, npz, str(d_in), "--resize_dims", "320,540", "--out_dir", str(tmp_path / enc), "--png_encoder", enc]
        _, text[enc] = quiet(annotate_video.main, argv)
        assert sorted(os.listdir(str(tmp_path / enc))) == names
    assert text["host"] == text["device"] and "{'bbox'" in text["host"]
    for name in names:
        host, dev = PilImage.open(str(tmp_path / "host" / name)), PilImage.open(str(tmp_path / "device" / name))
        assert dev.mode == "RGB" and np.array_equal(np.asarray(host.convert("RGB")), np.asarray(dev)), name
        assert (np.asarray(dev) != np.asarray(PilImage.open(str(d_in / name)))).any(), name      # (something was drawn)
