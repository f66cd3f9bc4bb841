"""The region rule through the detection entry, the editing chain and annotate_video: submit_batch(annotate=True, redact_region=(regions,
mask, mode, size, feather)) prepares from the untouched frame and blends behind the plate fill inside the captured pass.  Each result is
held against the restatement of the rule (tests/redact_region_ref.py) applied to the SOURCE frame -- over the restated redaction where the
pass redacts too -- byte for byte; a pass without the option, next to it on the same engine, is what it was: bytes and key."""
import numpy as np
import pytest

from tests import redact_ref as R
from tests import redact_region_ref as RR
from tests.annotate_ref import annotate as draw_ref
from tests.test_redact_entry_gpu import RESIZE, engine, f32_models, frame_pixels, quiet, staged      # noqa: F401  (the synthetic ResNet-50 pair, 200x330 frames)
from tests.test_track_gpu import pack

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

H, W = 200, 330                                                            # the staged frames
POLYS = [[(20, 30), (140, 12), (90, 120)], [(250, -20), (400, 60), (300, 150), (280, 60)]]      # a triangle; a concave polygon across two borders
REDACT = ("all", "blur", 12, 0)
TRACK = (30, 2, 3)


def the_mask():
    m = np.zeros((H, W), dtype=np.uint8)
    m[170:190, 10:120] = 255                                                # a burnt-in timestamp
    return m


REGION = (POLYS, the_mask(), "blur", 5, 6)
POLYGONS_ONLY = (POLYS, None, "pixelate", 8, 0)


def restated(current, source, option):
    regions, mask, mode, size, feather = option
    return RR.apply(current, source, regions, mask, mode, size, feather)


def submit(engine, staged, frames, B, threshold=0.0, **kw):
    srcs, resized, ratios, pixels = staged
    return engine.collect_batch(engine.submit_batch([resized[i] for i in frames], [ratios[i] for i in frames], threshold, [pixels[i] for i in frames],
                                                    batch=B, annotate=True, **kw))


def test_a_captured_pass_is_the_restatement(engine, staged, f32_models):
    mapping = f32_models[0].class_mapping
    srcs = staged[0]
    # alone: no redaction, no tracker, nothing drawn
    for option in (REGION, POLYGONS_ONLY):
        res = submit(engine, staged, [0, 1, 2, 3], 4, draw=False, redact_region=option)
        assert len(res) == 4
        for (n_rois, dets, out), src in zip(res, srcs):
            assert out.dtype == np.uint8 and np.array_equal(out, restated(src, src, option)) and (out != src).any()
    tail = ("nodraw", "region", tuple(tuple(p) for p in POLYS), None, "pixelate", 8, 0)
    assert sum(k[-len(tail):] == tail and "annotate" in k for k in engine.cache.keys()) == 1
    # with the redaction: the region goes over it, and its R comes from the UNTOUCHED frame, not from the redacted one
    res = submit(engine, staged, [0, 1, 2, 3], 4, redact=REDACT, draw=False, redact_region=REGION)
    differs = 0
    for (n_rois, dets, out), src in zip(res, srcs):
        redacted = R.redact_dets(src, dets, mapping, *REDACT)
        assert dets and np.array_equal(out, restated(redacted, src, REGION))
        differs += int((out != restated(redacted, redacted, REGION)).any())
    assert differs
    # drawing as well: boxes and labels stay legible on top of a region
    n_rois, dets, out = submit(engine, staged, [0], 1, redact_region=REGION)[0]
    assert np.array_equal(out, draw_ref(restated(srcs[0], srcs[0], REGION), dets))


def test_the_pass_without_the_option_is_untouched(engine, staged, f32_models):
    mapping = f32_models[0].class_mapping
    before = submit(engine, staged, [0, 1, 2, 3], 4, redact=REDACT)
    keys_before = set(engine.cache.keys())
    captures = engine.cache.captures
    with_region = submit(engine, staged, [0, 1, 2, 3], 4, redact=REDACT, redact_region=POLYGONS_ONLY)
    assert engine.cache.captures == captures + 1                            # a pass of its own
    new = set(engine.cache.keys()) - keys_before
    assert len(new) == 1
    key = new.pop()
    assert key[-6:-5] == ("region",) and key[:-6] in keys_before and key[:-6][-5:] == ("redact",) + REDACT      # the parent's key + the tag, last
    captures = engine.cache.captures
    after = submit(engine, staged, [0, 1, 2, 3], 4, redact=REDACT)
    assert engine.cache.captures == captures and set(engine.cache.keys()) == keys_before | {key}
    for (na, da, fa), (nb, db, fb), (nr, dr, fr), src in zip(before, after, with_region, staged[0]):
        assert na == nb == nr and len(da) == len(db) == len(dr) and np.array_equal(fa, fb)
        assert np.array_equal(fa, draw_ref(R.redact_dets(src, da, mapping, *REDACT), da))
        assert np.array_equal(fr, draw_ref(restated(R.redact_dets(src, dr, mapping, *REDACT), src, POLYGONS_ONLY), dr))


def test_a_delayed_pass_hides_the_region_in_every_emitted_frame(engine, staged):
    srcs = staged[0]
    kw = dict(draw=False, track=TRACK, track_lookback=2, redact_region=REGION)
    engine.track_reset()
    first = engine.submit_batch(staged[1][:2], staged[2][:2], 0.0, staged[3][:2], batch=2, annotate=True, **kw)
    assert engine.collect_batch(first) == []
    second = engine.submit_batch(staged[1][2:4], staged[2][2:4], 0.0, staged[3][2:4], batch=2, annotate=True, **kw)
    emitted = engine.collect_batch(second)
    flush = engine.submit_batch([], [], 0.0, [], batch=2, annotate=True, **kw)
    emitted += engine.collect_batch(flush)
    engine.track_reset()
    assert len(emitted) == 4
    for (n_rois, dets, out), src in zip(emitted, srcs):
        assert np.array_equal(out, restated(src, src, REGION)) and (out != src).any()


def test_the_eager_path_gives_the_captured_bytes(engine, staged, f32_models):
    from faster_rcnn_amd import annotate_video
    mapping = f32_models[0].class_mapping
    src = staged[0][1]
    for draw in (False, True):
        n_rois, dets, out = submit(engine, staged, [1], 1, redact=REDACT, draw=draw, redact_region=REGION)[0]
        frame = src.copy()
        plain = [{k: d[k] for k in ("bbox", "cls_name", "prob")} for d in dets]
        ret = annotate_video.draw_eager(frame, plain, mapping, redact=REDACT, draw=draw, redact_region=REGION)
        assert ret is frame and np.array_equal(frame, out) and (out != src).any()
    # without a detection the eager path still hides the place
    frame = src.copy()
    annotate_video.draw_eager(frame, [], mapping, redact_region=REGION)
    assert np.array_equal(frame, restated(src, src, REGION))


def test_submit_batch_refusals(engine, staged):
    from faster_rcnn_amd._lib import FrcnnError
    srcs, resized, ratios, pixels = staged
    captures = engine.cache.captures
    one = lambda **kw: engine.submit_batch(resized[:1], ratios[:1], 0.0, pixels[:1], batch=1, **kw)
    with pytest.raises(FrcnnError) as e:
        one(redact_region=POLYGONS_ONLY)
    assert "annotate=True" in str(e.value)
    bad_mask = np.zeros((W, H), dtype=np.uint8)
    for bad, word in (((None, None, None, None, None), "neither"), ((POLYS, None, "fill", 0, 33), "feather"), ((POLYS, None, "blur", 40, 0), "size"),
                      ((POLYS, None, "smear", None, 0), "mode"), (([[(0, 0), (0, 0), (5, 5)]], None, None, None, None), "consecutive"),
                      ((POLYS, None), "(regions, mask, mode, size, feather)"), ((None, bad_mask, None, None, None), "%dx%d" % (H, W))):
        with pytest.raises(FrcnnError) as e:
            one(annotate=True, redact_region=bad)
        assert word in str(e.value) and "redact" in str(e.value), bad
    assert engine.cache.captures == captures


# ----------------------------------------------------------------------------------------------------------- the chain, without a model
def test_a_remove_box_over_a_region_shows_R_not_the_plate():
    """An EditChain driven with synthetic rows: the plate learns picture A from frames without rows, then picture B comes with a box of a
    remove class that lies over a region.  Behind the plate fill the region's pixels show R of B -- the untouched frame --, the rest of
    the box does not show B, and the same chain without the option shows no R there."""
    from faster_rcnn_amd import ops
    from faster_rcnn_amd.entry import PassSpec
    from faster_rcnn_amd.frame_edit import EditChain, EditStates
    h, w, rows = 48, 64, 8
    names = ["bg", "car", "person"]
    remove = ("all", 1, 255, 0)
    region = ([[(10, 8), (30, 8), (30, 24), (10, 24)]], None, "blur", 3, 0)       # x 10..29, y 8..23
    box = [4, 4, 40, 30]                                                    # covers the region
    A, B = frame_pixels(h, w, 1), frame_pixels(h, w, 2)
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    outs = {}
    for name, option in (("with", region), ("without", None)):
        spec = PassSpec(annotate=True, draw=False, remove=remove, redact_region=None if option is None else ops.redact_region_option(*option))
        chain = EditChain(EditStates(names, 4, 8), spec, 1, 1, (h, w), False)
        for k in range(3):                                                  # the plate learns A
            frame = torch.from_numpy(A.copy()).cuda()
            chain.update(frame.view(-1), 0, torch.from_numpy(pack([], [], 0, rows)).cuda(), one)
            chain.edit(0, frame)
            if option is not None:
                assert np.array_equal(frame.cpu().numpy(), restated(A, A, option))       # no row anywhere: the region is hidden all the same
        frame = torch.from_numpy(B.copy()).cuda()
        chain.update(frame.view(-1), 0, torch.from_numpy(pack([box], [1], 1, rows)).cuda(), one)
        chain.edit(0, frame)
        outs[name] = frame.cpu().numpy()
    Wt = RR.weights(h, w, region[0], None, 0)
    Rep = R.blurred(B, 3)
    inside = np.zeros((h, w), dtype=bool)
    inside[4:31, 4:41] = True
    assert (Wt == 256).sum() == 20 * 16 and inside[Wt == 256].all()
    assert np.array_equal(outs["with"][Wt == 256], Rep[Wt == 256])          # R of the untouched frame, not the plate
    assert (outs["without"][Wt == 256] != Rep[Wt == 256]).any()
    rest = inside & (Wt == 0)
    assert np.array_equal(outs["with"][rest], outs["without"][rest]) and (outs["with"][rest] != B[rest]).any()       # the remove step ran
    assert np.array_equal(outs["with"][~inside], B[~inside])


def test_get_annotated_frame_takes_the_keyword(engine, f32_models):
    from faster_rcnn_amd import annotate_video, shapes, voc_dets
    mgr, det, _ = f32_models
    src = frame_pixels(220, 300, 7)
    option = (POLYS, None, "blur", 5, 6)
    outs = {}
    for fast in (True, False):
        voc_dets.FAST_ENTRY = fast
        try:
            frame = src.copy()
            img = shapes.InMemoryImage(data=frame, width=300, height=220)
            quiet(annotate_video.get_annotated_frame, mgr, det, frame, img, *RESIZE, draw=False, redact_region=option)
        finally:
            voc_dets.FAST_ENTRY = True
        outs[fast] = frame
    assert np.array_equal(outs[True], outs[False]) and np.array_equal(outs[True], restated(src, src, option))
