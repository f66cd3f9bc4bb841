"""track_scene_cut through the detection entry and annotate_video: submit_batch(annotate=True, track=..., track_motion=R,
track_scene_cut=PCT), with or without detect_every=K, runs ops.track_update_cut inside the captured pass in the place of the motion or
interval call.  Every result is held against the restatements: tests/track_cut_ref.py over the source frames and the live rows the key
frames returned, then tests/redact_ref.py over the live and the held rows, then the drawing rule with ids -- byte for byte."""
import io

import numpy as np
import pytest

from tests import track_cut_ref as C
from tests import track_motion_ref as M
from tests import track_ref as T
from tests.test_redact_entry_gpu import RESIZE, engine, f32_models, frame_pixels, quiet      # noqa: F401  (the synthetic ResNet-50 pair)
from tests.test_track_entry_gpu import same_det, split_dets
from tests.test_track_motion_entry_gpu import H, RADIUS, REDACT, SHIFT, TRACK, W, check_against_rule, expected

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PCT = 40
CUT = 3                                  # the first frame of scene B
NAMES = ["s_%02d.png" % (5 * k) for k in range(6)]                          # (names that are not their positions)


@pytest.fixture(scope="module")
def footage(tmp_path_factory):
    """Three frames of scene A, then three of scene B, as a directory of PNG files: noise with the luma in 0..127 against 128..255 -- the
    cut is D = 2hw --, inside a scene each frame the last moved by (3, 2): far from the decision.  -> (the directory, the frames)."""
    from PIL import Image as PilImage
    a, b = frame_pixels(H, W, 71) // 2, 128 + frame_pixels(H, W, 72) // 2
    srcs = [np.ascontiguousarray(M.shifted(s, k * SHIFT[0], k * SHIFT[1])) for s in (a, b) for k in range(3)]
    for x, y in zip(srcs[:-1], srcs[1:]):
        d = C.distance(x, y)
        assert d == 2 * H * W if y is srcs[CUT] else d * 100 * 4 < PCT * 2 * H * W
    d_in = tmp_path_factory.mktemp("cut") / "in"
    d_in.mkdir()
    for name, rgb in zip(NAMES, srcs):
        PilImage.fromarray(rgb).save(str(d_in / name))
    return d_in, srcs


def annotate(f32_models, footage, d_out, monkeypatch, **kw):
    """``annotate_images`` over the footage -> (the results its passes returned, the printed text, the MOT text, {name: file bytes})."""
    from faster_rcnn_amd import annotate_video, entry
    mgr, det, _ = f32_models
    seen, collect = [], entry.DetectionEntry.collect_batch

    def recording(self, ticket):
        res = collect(self, ticket)
        seen.extend(res)
        return res

    monkeypatch.setattr(entry.DetectionEntry, "collect_batch", recording)
    tracks = io.StringIO()
    try:
        _, text = quiet(annotate_video.annotate_images, mgr, det, str(footage[0]), str(d_out), NAMES, *RESIZE, png_encoder="host", redact=REDACT,
                        track=TRACK, tracks_out=tracks, track_motion=RADIUS, **kw)
    finally:
        monkeypatch.setattr(entry.DetectionEntry, "collect_batch", collect)
    return seen, text, tracks.getvalue(), {p.name: p.read_bytes() for p in d_out.iterdir()}


def check_frames(tracker, srcs, results, mapping, every):
    """The results of the six frames, key and between, against the restatements -> [(live, held, cut)]."""
    seen = []
    for f, (src, (n_rois, dets, out, marks)) in enumerate(zip(srcs, results)):
        cut = tracker.cut_step(src, PCT)
        assert marks == ({"scene_cut": True} if cut else {}), f
        if f % every == 0:
            live, held = check_against_rule(tracker, src, dets, mapping, True)
            assert n_rois > 0 and not any("propagated" in d for d in dets)
        else:
            live, held = split_dets(dets)
            want_live, want_held = tracker.track_between(src, mapping, TRACK[2], RADIUS)
            assert n_rois == 0 and all(d.get("propagated") is True and d["track_id"] > 0 for d in live)
            assert len(live) == len(want_live) and all(same_det(a, b) for a, b in zip(live, want_live)), f
            assert len(held) == len(want_held) and all(same_det(a, b) for a, b in zip(held, want_held)), f
        assert np.array_equal(out, expected(src, live, held, mapping)), f
        seen.append((live, held, cut))
    return seen


@pytest.mark.parametrize("every", [1, 2])
def test_annotate_images_ends_every_track_at_the_cut(engine, f32_models, footage, monkeypatch, tmp_path, every):
    """Plain: a pass of frames 0-3 and a padded one of 4-5, the cut on a key frame.  detect_every 2: one pass of six frames, the cut on a
    between frame."""
    from PIL import Image as PilImage
    mapping = f32_models[0].class_mapping
    d_in, srcs = footage
    kw = {} if every == 1 else {"detect_every": every}
    results, text, lines, files = annotate(f32_models, footage, tmp_path / "out", monkeypatch, track_scene_cut=PCT, **kw)
    assert len(results) == 6 and all(len(r) == 4 for r in results)
    # the pass's outputs: the restatement replayed on the pass's own detections
    tracker = C.CutTracker(64)
    per_frame = check_frames(tracker, srcs, results, mapping, every)
    assert [cut for _, _, cut in per_frame] == [f == CUT for f in range(6)]
    assert np.array_equal(engine.track_state().cpu().numpy(), tracker.t.words()) and tracker.t.frames == 6
    assert [r[3] for r in results] == [{"scene_cut": True} if f == CUT else {} for f in range(6)]
    # ids never continue across the cut, no held row crosses it, and behind a cut on a between frame nothing is shown
    ids = [{d["track_id"] for d in live + held if d["track_id"] > 0} for live, held, _ in per_frame]
    before, after = set().union(*ids[:CUT]), set().union(*ids[CUT:])
    assert before and after and max(before) < min(after)
    assert not per_frame[CUT][1]
    if every == 2:
        assert not per_frame[CUT][0] and ids[CUT] == set() and ids[CUT - 1]
    # the printed lines: the mark exactly once, in front of the cut frame's lines
    out_lines = text.splitlines()
    marks = [i for i, x in enumerate(out_lines) if x.startswith("scene cut:")]
    assert len(marks) == 1 and out_lines[marks[0]] == "scene cut: " + str(d_in / NAMES[CUT])
    assert out_lines[marks[0] + 1] == "processing " + str(d_in / NAMES[CUT])
    assert [x for x in out_lines if x.startswith("processing")] == ["processing " + str(d_in / n) for n in NAMES]
    # the files and the MOT lines (their format is unchanged)
    want_lines = []
    for k, (live, held, _) in enumerate(per_frame):
        want_lines += T.mot_lines(k + 1, live, mapping)
        got = np.asarray(PilImage.open(io.BytesIO(files[NAMES[k]])).convert("RGB"))
        assert np.array_equal(got, expected(srcs[k], live, held, mapping)), NAMES[k]
    assert want_lines and lines == "".join(x + "\n" for x in want_lines)
    tail = ("motion", RADIUS) + (("every", every) if every > 1 else ()) + ("cut", PCT)
    assert any(k[-len(tail):] == tail for k in engine.cache.keys())


@pytest.mark.parametrize("every", [1, 2])
def test_without_the_option_nothing_changes(engine, f32_models, footage, monkeypatch, tmp_path, every):
    """The run without the option before and after a run with it: the same files, lines and MOT text, three-element results, and no cache
    key but the new passes' own carries the tag."""
    kw = {} if every == 1 else {"detect_every": every}
    before = annotate(f32_models, footage, tmp_path / "a", monkeypatch, **kw)
    keys = set(engine.cache.keys())
    with_cut = annotate(f32_models, footage, tmp_path / "b", monkeypatch, track_scene_cut=PCT, **kw)
    after = annotate(f32_models, footage, tmp_path / "c", monkeypatch, **kw)
    now = set(engine.cache.keys())
    cut = {k for k in now if "cut" in k}
    assert cut and now - cut == keys - cut
    assert before[1:] == after[1:] and "scene cut" not in before[1] and all(len(r) == 3 for r in before[0] + after[0])
    assert sorted(before[3]) == sorted(NAMES)
    assert with_cut[1].count("scene cut:") == 1 and all(len(r) == 4 for r in with_cut[0])


@pytest.mark.parametrize("fast", [True, False])
def test_get_annotated_frame_gives_the_same_ids(engine, f32_models, footage, monkeypatch, tmp_path, fast):
    """The one-frame paths, captured and eager, over the same six frames: the kept frame is the reference of every call."""
    from faster_rcnn_amd import annotate_video, shapes, voc_dets
    mgr, det, _ = f32_models
    _, _, want, _ = annotate(f32_models, footage, tmp_path / "out", monkeypatch, track_scene_cut=PCT)
    tracks, texts = io.StringIO(), []
    voc_dets.FAST_ENTRY = fast
    try:
        annotate_video.reset_tracks(mgr, det, 1)
        for k, src in enumerate(footage[1]):
            frame = np.ascontiguousarray(src[:, :, ::-1])                    # (the file's R,G,B as the one-frame path takes it: B,G,R)
            img = shapes.InMemoryImage(data=frame, width=W, height=H)
            texts.append(quiet(annotate_video.get_annotated_frame, mgr, det, frame, img, *RESIZE, redact=REDACT, track=TRACK, tracks_out=tracks,
                               frame_no=k + 1, track_motion=RADIUS, track_scene_cut=PCT)[1])
    finally:
        voc_dets.FAST_ENTRY = True
    rows = lambda text: [x.split(",")[:6] + x.split(",")[7:] for x in text.splitlines()]      # (everything but the prob's decimals)
    assert rows(want) and rows(tracks.getvalue()) == rows(want)
    assert ["scene cut: %d" % (k + 1) in t for k, t in enumerate(texts)] == [k == CUT for k in range(6)]


def test_submit_batch_refusals(engine, f32_models, footage):
    from faster_rcnn_amd import entry, resnet, shapes, util
    from faster_rcnn_amd._lib import FrcnnError
    from faster_rcnn_amd.det_util import DetTrainingManager
    imgs = [shapes.Image(shapes.Metadata("c%d" % i, W, H, [], "none"), s) for i, s in enumerate(footage[1][:2])]
    resized, ratios = util.resize_imgs(imgs, min_size=RESIZE[0], max_size=RESIZE[1])
    pixels = [engine.host_pixels(r) for r in resized]
    captures = engine.cache.captures
    two = lambda eng=engine, px=pixels, **kw: eng.submit_batch(resized, ratios, 0.0, px, batch=2, annotate=True, **kw)
    with pytest.raises(FrcnnError, match="track_scene_cut=.*track_motion=R"):
        two(track=TRACK, track_scene_cut=PCT)
    with pytest.raises(FrcnnError, match="track_scene_cut=.*track_motion=R"):
        two(track_scene_cut=PCT)
    with pytest.raises(FrcnnError, match="track_scene_cut= together with track_lookback= is not supported"):
        two(track=TRACK, track_motion=RADIUS, track_lookback=2, track_scene_cut=PCT)
    with pytest.raises(FrcnnError, match="track_scene_cut= together with track_backtrack= is not supported"):
        engine.submit_batch(resized[:1], ratios[:1], 0.0, pixels, batch=1, annotate=True, track=TRACK, track_motion=RADIUS, detect_every=2,
                            track_backtrack=2, track_scene_cut=PCT)
    for bad in (0, 101, -1, True, 40.0, "40", (40,)):
        with pytest.raises(FrcnnError, match="track_scene_cut"):
            two(track=TRACK, track_motion=RADIUS, track_scene_cut=bad)
    assert engine.cache.captures == captures
    mgr, det, _ = f32_models
    mgr2 = DetTrainingManager(rpn_model=mgr.rpn_model, class_mapping=mgr.class_mapping, preprocess_func=lambda d: resnet.preprocess(d),
                              anchor_dims=mgr.anchor_dims)
    foreign = entry.for_models(mgr2, det, 64, 16, 1)
    assert foreign is not None and not foreign.device_preprocess
    with pytest.raises(FrcnnError, match=r"track_scene_cut= needs the device-side preprocess.*foreign preprocess_func.*float"):
        two(foreign, [foreign.host_pixels(r) for r in resized], track=TRACK, track_motion=RADIUS, track_scene_cut=PCT)
    assert foreign.cache.captures == 0
