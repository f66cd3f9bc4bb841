"""Redaction through the detection entry and annotate_video: submit_batch(annotate=True, redact=..., draw=...) hides the detected
objects inside the captured pass, in front of the drawing step and of every encoder.  Each result is held against the restatement of the
rule (tests/redact_ref.py) applied to the SOURCE frame with the detections that pass returned, followed by the drawing rule's restatement
(tests/annotate_ref.py) when the pass draws: byte for byte."""
import contextlib
import io
import os

import numpy as np
import pytest

from tests import redact_ref as R
from tests import y4m_ref as Y
from tests.annotate_ref import annotate as draw_ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RESIZE = (320, 540)
# every VOC class but one, by name (the path "all" does not take); the calibrated classifier fires on many of them
REDACT = (("bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog", "horse", "motorbike", "person",
           "pottedplant", "sheep", "sofa", "train", "tvmonitor"), "blur", 3, 2)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()) as buf:
        res = fn(*a, **k)
    return res, buf.getvalue()


def frame_pixels(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


@pytest.fixture(scope="module")
def f32_models():
    """tests/test_annotate_gpu.py's small synthetic ResNet-50 pair, its classifier calibrated so that many classes fire."""
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


@pytest.fixture(scope="module")
def engine(f32_models):
    from faster_rcnn_amd import entry
    mgr, det, _ = f32_models
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight("f32"))
    assert eng.batch == 4
    return eng


@pytest.fixture(scope="module")
def staged(engine):
    """Four in-memory BGR frames of one size, resized and with their host pixels: what submit_batch takes."""
    from faster_rcnn_amd import shapes, util
    srcs = [frame_pixels(200, 330, 300 + i) for i in range(4)]
    imgs = [shapes.Image(shapes.Metadata("m%d" % i, 330, 200, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=RESIZE[0], max_size=RESIZE[1])
    return srcs, resized, ratios, [engine.host_pixels(r) for r in resized]


def expected(src, dets, mapping, redact, draw):
    out = src if redact is None else R.redact_dets(src, dets, mapping, *redact)
    return draw_ref(out, dets) if draw else out


def submit(engine, staged, B, **kw):
    srcs, resized, ratios, pixels = staged
    return engine.collect_batch(engine.submit_batch(resized[:B], ratios[:B], 0.0, pixels[:B], batch=B, annotate=True, **kw))


# ----------------------------------------------------------------------------------------------------------- captured passes
@pytest.mark.parametrize("B", [1, 4])
def test_captured_passes_redact_in_front_of_drawing_and_every_encoder(engine, staged, f32_models, B):
    from PIL import Image as PilImage
    mapping = f32_models[0].class_mapping
    srcs = staged[0]
    changed = hidden = 0
    for kw in (dict(), dict(encode="png"), dict(encode="y4m", y4m=("444", "full"))):
        res = submit(engine, staged, B, redact=REDACT, **kw)
        assert len(res) == B
        for (n_rois, dets, out), src in zip(res, srcs):
            want = expected(src, dets, mapping, REDACT, True)               # (in-memory frames are uploaded BGR)
            if kw.get("encode") == "png":
                got = np.asarray(PilImage.open(io.BytesIO(out)).convert("RGB"))[:, :, ::-1]
                assert np.array_equal(got, want), kw
            elif kw.get("encode") == "y4m":
                assert out == Y.encode(want, "444", "full", bgr=True), kw
            else:
                assert out.dtype == np.uint8 and np.array_equal(out, want)
            only_drawn = draw_ref(src, dets)
            changed += int((want != src).any())
            hidden += int((want != only_drawn).any())
    assert changed and hidden                                               # the models fire, and some of it on the redacted classes
    keys = engine.cache.keys()
    tail = ("redact",) + REDACT
    assert any(k[-len(tail):] == tail and "annotate" in k for k in keys)


def test_draw_false_and_the_modes(engine, staged, f32_models):
    mapping = f32_models[0].class_mapping
    srcs = staged[0]
    for redact in (("all", "pixelate", 5, 0), ("all", "fill", None, 3), (("person",), "blur", None, 0), None):
        res = submit(engine, staged, 1, redact=redact, draw=False)
        n_rois, dets, out = res[0]
        norm = None if redact is None else (redact[0], redact[1], R.SIZES[redact[1]][2] if redact[2] is None else redact[2], redact[3])
        assert np.array_equal(out, expected(srcs[0], dets, mapping, norm, False)), redact
        if redact is None:
            assert np.array_equal(out, srcs[0])                             # nothing hidden, nothing drawn
        elif redact[0] == "all":
            assert dets and (out != srcs[0]).any()
    assert any(k[-1:] == ("nodraw",) and "redact" in k for k in engine.cache.keys())
    assert any(k[-2:] == ("annotate", "nodraw") for k in engine.cache.keys())


def test_the_plain_annotating_pass_is_untouched(engine, staged, f32_models):
    """Without the arguments: the same pass, the same key and the same bytes before and after a redacting pass on the engine."""
    mapping = f32_models[0].class_mapping
    before = submit(engine, staged, 4)
    keys_before = set(engine.cache.keys())
    captures = engine.cache.captures
    red = submit(engine, staged, 4, redact=("all", "pixelate", 16, 0))
    assert engine.cache.captures == captures + 1                            # a pass of its own
    after = submit(engine, staged, 4)
    redacting = [k for k in engine.cache.keys() if k[-5:] == ("redact", "all", "pixelate", 16, 0)]
    assert len(redacting) == 1                                              # two keys: the annotating key, and it with the redaction appended
    assert redacting[0][:-5] in keys_before and redacting[0][:-5][-1:] == ("annotate",)
    for (na, da, fa), (nb, db, fb), (nr, dr, fr), src in zip(before, after, red, staged[0]):
        assert na == nb == nr and np.array_equal(fa, fb)
        assert len(da) == len(db) and all(np.array_equal(x["bbox"], y["bbox"]) and x["cls_name"] == y["cls_name"] and x["prob"] == y["prob"]
                                          for x, y in zip(da, db))
        assert np.array_equal(fa, draw_ref(src, da))
        assert np.array_equal(fr, expected(src, dr, mapping, ("all", "pixelate", 16, 0), True))


def test_submit_batch_refusals(engine, staged):
    from faster_rcnn_amd._lib import FrcnnError
    srcs, resized, ratios, pixels = staged
    captures = engine.cache.captures
    one = lambda **kw: engine.submit_batch(resized[:1], ratios[:1], 0.0, pixels[:1], batch=1, **kw)
    for kw in (dict(redact=REDACT), dict(draw=False), dict(redact=REDACT, draw=False)):
        with pytest.raises(FrcnnError) as e:
            one(**kw)
        assert "annotate=True" in str(e.value)
    for bad in ((("unicorn",), "blur", 3, 0), ("all", "mosaic", 3, 0), ("all", "blur", 33, 0), ("all", "pixelate", 1, 0), ("all", "fill", 4, 0),
                ("all", "blur", 3, -1), ("all", "blur"), "all"):
        with pytest.raises(FrcnnError):
            one(annotate=True, redact=bad)
    assert engine.cache.captures == captures


# ----------------------------------------------------------------------------------------------------------- annotate_video
def test_get_annotated_frame_eager_equals_captured(engine, f32_models):
    from faster_rcnn_amd import annotate_video, shapes, util, voc_dets
    mgr, det, _ = f32_models
    src = frame_pixels(220, 300, 7)
    redact = ("all", "pixelate", 5, 1)
    outs = {}
    for fast in (True, False):
        voc_dets.FAST_ENTRY = fast
        try:
            frame = src.copy()
            img = shapes.InMemoryImage(data=frame, width=300, height=220)
            ret, text = quiet(annotate_video.get_annotated_frame, mgr, det, frame, img, *RESIZE, redact=redact, draw=False)
        finally:
            voc_dets.FAST_ENTRY = True
        assert ret is frame
        outs[fast] = (frame, text.splitlines())
    assert np.array_equal(outs[True][0], outs[False][0])
    assert outs[True][1][0] == outs[False][1][0] and outs[True][1][0].startswith("num rois: ")
    # the captured pass again, for its detections (all of them: the printed lines hold only the drawable ones)
    img = shapes.InMemoryImage(data=src.copy(), width=300, height=220)
    resized, ratios = util.resize_imgs([img], min_size=RESIZE[0], max_size=RESIZE[1])
    n_rois, dets, out = engine.collect_batch(engine.submit_batch(resized, ratios, 0.0, [engine.host_pixels(resized[0])], batch=1, annotate=True,
                                                                 redact=redact, draw=False))[0]
    assert dets and np.array_equal(out, outs[True][0]) and (out != src).any()
    assert np.array_equal(out, R.redact_dets(src, dets, mgr.class_mapping, *redact))
    # drawing as well, eagerly: the redaction runs first
    voc_dets.FAST_ENTRY = False
    try:
        frame = src.copy()
        quiet(annotate_video.get_annotated_frame, mgr, det, frame, shapes.InMemoryImage(data=frame, width=300, height=220), *RESIZE, redact=redact)
    finally:
        voc_dets.FAST_ENTRY = True
    drawn = engine.collect_batch(engine.submit_batch(resized, ratios, 0.0, [engine.host_pixels(resized[0])], batch=1, annotate=True, redact=redact))[0]
    assert np.array_equal(drawn[2], expected(src, drawn[1], mgr.class_mapping, redact, True)) and np.array_equal(frame, drawn[2])


def test_main_redacts_a_directory(f32_models, tmp_path, monkeypatch):
    """``annotate_video.main`` with --redact all --redact_mode pixelate --redact_size 5 --no_draw on two small PNGs: the files are the
    restatement over ALL detections of each frame's pass, and the run prints what the run without the arguments prints."""
    from PIL import Image as PilImage
    from faster_rcnn_amd import annotate_video, entry
    from faster_rcnn_amd.data.voc_data_helpers import VOC_CLASS_MAPPING
    from faster_rcnn_amd.weights import save_npz
    npz = str(tmp_path / "w.npz")
    save_npz(npz, f32_models[2])
    d_in = tmp_path / "frames"
    d_in.mkdir()
    frames = {}
    for i in range(2):
        frames["%06d.png" % i] = rgb = frame_pixels(150, 200, 40 + i)
        PilImage.fromarray(rgb).save(str(d_in / ("%06d.png" % i)))
    seen = []
    collect = entry.DetectionEntry.collect_batch

    def recording(self, ticket):
        res = collect(self, ticket)
        seen.extend(res)
        return res

    monkeypatch.setattr(entry.DetectionEntry, "collect_batch", recording)
    base = [npz, npz, str(d_in), "--resize_dims", "%d,%d" % RESIZE]
    _, text_plain = quiet(annotate_video.main, base + ["--out_dir", str(tmp_path / "plain")])
    plain_dets = [r[1] for r in seen]
    del seen[:]
    _, text = quiet(annotate_video.main, base + ["--out_dir", str(tmp_path / "out"), "--redact", "all", "--redact_mode", "pixelate",
                                                 "--redact_size", "5", "--no_draw"])
    assert text == text_plain and text.count("processing ") == 2
    assert sorted(os.listdir(tmp_path / "out")) == sorted(frames) and len(seen) == 2
    for (name, rgb), (n_rois, dets, _), plain in zip(sorted(frames.items()), seen, plain_dets):
        out = np.asarray(PilImage.open(str(tmp_path / "out" / name)).convert("RGB"))
        assert dets and len(dets) == len(plain)
        assert np.array_equal(out, R.redact_dets(rgb, dets, VOC_CLASS_MAPPING, "all", "pixelate", 5, 0)), name
        assert (out != rgb).any()
        drawn = np.asarray(PilImage.open(str(tmp_path / "plain" / name)).convert("RGB"))
        assert np.array_equal(drawn, draw_ref(rgb, plain))
