"""The shape rule through the detection entry and annotate_video: submit_batch(annotate=True, redact=..., redact_shape=(shape, feather))
runs ops.redact_shaped_u8 in the redaction's place inside the captured pass.  Each result is held against the restatement of the rule
(tests/redact_shape_ref.py) applied to the SOURCE frame with the detections that pass returned -- the held rows of a tracking pass too --
byte for byte; a pass without the option, next to it on the same engine, is what it was: bytes and key."""
import numpy as np
import pytest

from tests import redact_ref as R
from tests import redact_shape_ref as RS
from tests.annotate_ref import annotate as draw_ref
from tests.test_redact_entry_gpu import RESIZE, engine, f32_models, frame_pixels, quiet, staged      # noqa: F401  (the synthetic ResNet-50 pair, 200x330 frames)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

REDACT = ("all", "blur", 3, 2)
SHAPE = ("ellipse", 4)
TRACK = (30, 2, 3)


def submit(engine, staged, frames, B, threshold=0.0, **kw):
    srcs, resized, ratios, pixels = staged
    return engine.collect_batch(engine.submit_batch([resized[i] for i in frames], [ratios[i] for i in frames], threshold, [pixels[i] for i in frames],
                                                    batch=B, annotate=True, **kw))


def test_a_captured_pass_is_the_restatement(engine, staged, f32_models):
    mapping = f32_models[0].class_mapping
    srcs = staged[0]
    res = submit(engine, staged, [0, 1, 2, 3], 4, redact=REDACT, draw=False, redact_shape=SHAPE)
    assert len(res) == 4
    softer = 0
    for (n_rois, dets, out), src in zip(res, srcs):
        assert dets and out.dtype == np.uint8
        assert np.array_equal(out, RS.redact_dets(src, dets, mapping, *REDACT, *SHAPE))
        hard = R.redact_dets(src, dets, mapping, *REDACT)
        assert (out != src).any()
        softer += int((out != hard).any())
    assert softer                                                           # the option shows
    tail = ("redact",) + REDACT + ("shape",) + SHAPE + ("nodraw",)
    assert sum(k[-len(tail):] == tail and "annotate" in k for k in engine.cache.keys()) == 1
    # drawing as well: the boxes and labels lie over the shaped redaction, and a box with a feather goes the same way
    n_rois, dets, out = submit(engine, staged, [0], 1, redact=REDACT, redact_shape=("box", 9))[0]
    assert np.array_equal(out, draw_ref(RS.redact_dets(srcs[0], dets, mapping, *REDACT, "box", 9), dets))


def test_held_rows_are_shaped(engine, staged, f32_models):
    """Four frames, then four at a threshold no probability passes: every track is held, its box growing, and hidden as an ellipse."""
    mapping = f32_models[0].class_mapping
    src = staged[0][0]
    kw = dict(redact=REDACT, draw=False, redact_shape=SHAPE, track=TRACK)
    engine.track_reset()
    passes = [submit(engine, staged, [0, 0, 0, 0], 4, **kw), submit(engine, staged, [0, 0, 0, 0], 4, threshold=2.0, **kw)]
    engine.track_reset()
    held_frames = 0
    for res in passes:
        for n_rois, dets, out in res:
            held = [d for d in dets if "held" in d]
            assert np.array_equal(out, RS.redact_dets(src, dets, mapping, *REDACT, *SHAPE))       # live and held rows alike
            if held and len(held) == len(dets):
                held_frames += 1
                assert (out != src).any() and (out != R.redact_dets(src, dets, mapping, *REDACT)).any()
    assert held_frames == 2
    assert any("shape" in k and "track" in k for k in engine.cache.keys())


def test_the_eager_path_gives_the_captured_bytes(engine, staged, f32_models):
    from faster_rcnn_amd import annotate_video
    mapping = f32_models[0].class_mapping
    src = staged[0][1]
    for draw in (False, True):
        n_rois, dets, out = submit(engine, staged, [1], 1, redact=REDACT, draw=draw, redact_shape=SHAPE)[0]
        frame = src.copy()
        plain = [{k: d[k] for k in ("bbox", "cls_name", "prob")} for d in dets]
        ret = annotate_video.draw_eager(frame, plain, mapping, redact=REDACT, draw=draw, redact_shape=SHAPE)
        assert ret is frame and np.array_equal(frame, out) and (out != src).any()
    # ("box", 0) on the eager path is the call without it
    a, b = src.copy(), src.copy()
    annotate_video.draw_eager(a, plain, mapping, redact=REDACT, draw=False, redact_shape=("box", 0))
    annotate_video.draw_eager(b, plain, mapping, redact=REDACT, draw=False)
    assert np.array_equal(a, b) and np.array_equal(a, R.redact_dets(src, plain, mapping, *REDACT))


def test_the_pass_without_the_option_is_untouched(engine, staged, f32_models):
    """Without the option, and with ("box", 0): the same pass, the same key and the same bytes before and after a shaped pass."""
    mapping = f32_models[0].class_mapping
    before = submit(engine, staged, [0, 1, 2, 3], 4, redact=REDACT)
    keys_before = set(engine.cache.keys())
    captures = engine.cache.captures
    shaped = submit(engine, staged, [0, 1, 2, 3], 4, redact=REDACT, redact_shape=SHAPE)
    assert engine.cache.captures == captures + 1                            # a pass of its own
    new = set(engine.cache.keys()) - keys_before
    assert len(new) == 1
    key = new.pop()
    assert key[-3:] == ("shape",) + SHAPE and key[:-3] in keys_before and key[:-3][-5:] == ("redact",) + REDACT
    captures = engine.cache.captures
    after = submit(engine, staged, [0, 1, 2, 3], 4, redact=REDACT)
    stated = submit(engine, staged, [0, 1, 2, 3], 4, redact=REDACT, redact_shape=("box", 0))
    assert engine.cache.captures == captures and set(engine.cache.keys()) == keys_before | {key}      # today's pass, today's key
    for (na, da, fa), (nb, db, fb), (nc, dc, fc), (ns, ds, fs), src in zip(before, after, stated, shaped, staged[0]):
        assert na == nb == nc == ns and np.array_equal(fa, fb) and np.array_equal(fa, fc)
        assert np.array_equal(fa, draw_ref(R.redact_dets(src, da, mapping, *REDACT), da))
        assert np.array_equal(fs, draw_ref(RS.redact_dets(src, ds, mapping, *REDACT, *SHAPE), ds))


def test_submit_batch_refusals(engine, staged):
    from faster_rcnn_amd._lib import FrcnnError
    srcs, resized, ratios, pixels = staged
    captures = engine.cache.captures
    one = lambda **kw: engine.submit_batch(resized[:1], ratios[:1], 0.0, pixels[:1], batch=1, annotate=True, **kw)
    with pytest.raises(FrcnnError) as e:
        one(redact_shape=SHAPE)
    assert "redact=" in str(e.value)
    for bad, word in ((("circle", 0), "shape"), (("ellipse", 33), "feather"), (("box", -1), "feather"), ("ellipse", "(shape, feather)")):
        with pytest.raises(FrcnnError) as e:
            one(redact=REDACT, redact_shape=bad)
        assert word in str(e.value)
    assert engine.cache.captures == captures


def test_get_annotated_frame_takes_the_keyword(engine, f32_models):
    from faster_rcnn_amd import annotate_video, shapes, voc_dets
    mgr, det, _ = f32_models
    src = frame_pixels(220, 300, 7)
    outs = {}
    for fast in (True, False):
        voc_dets.FAST_ENTRY = fast
        try:
            frame = src.copy()
            img = shapes.InMemoryImage(data=frame, width=300, height=220)
            quiet(annotate_video.get_annotated_frame, mgr, det, frame, img, *RESIZE, redact=REDACT, draw=False, redact_shape=SHAPE)
        finally:
            voc_dets.FAST_ENTRY = True
        outs[fast] = frame
    assert np.array_equal(outs[True], outs[False]) and (outs[True] != src).any()
    hard = src.copy()
    quiet(annotate_video.get_annotated_frame, mgr, det, hard, shapes.InMemoryImage(data=hard, width=300, height=220), *RESIZE, redact=REDACT, draw=False)
    assert (hard != outs[True]).any()
