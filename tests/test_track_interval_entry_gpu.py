"""detect_every through the detection entry and annotate_video: submit_batch(annotate=True, track=..., track_motion=R, detect_every=K)
stages B * K source frames, runs the network on every K-th and ops.track_update_interval over all of them inside the captured pass, in
front of the redaction and the drawing step.  Every result is held against the restatements: tests/track_interval_ref.py over the source
frames and the live rows the key frames returned, then tests/redact_ref.py over the live and the held rows, then the drawing rule with
ids -- byte for byte."""
import io

import numpy as np
import pytest

from tests import track_interval_ref as I
from tests import track_motion_ref as M
from tests import track_ref as T
from tests.test_redact_entry_gpu import RESIZE, engine, f32_models, frame_pixels, quiet      # noqa: F401  (the synthetic ResNet-50 pair)
from tests.test_track_entry_gpu import same_det, split_dets
from tests.test_track_motion_entry_gpu import H, RADIUS, REDACT, SHIFT, TRACK, W, check_against_rule, expected, moving, run_sequence      # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

B, K = 2, 2
TAIL = ("track",) + TRACK + ("motion", RADIUS, "every", K)


@pytest.fixture(scope="module")
def clip(engine):
    """Eight in-memory BGR frames, frame k moved by k * (3, 2) against frame 0, resized and with their host pixels."""
    from faster_rcnn_amd import shapes, util
    a = frame_pixels(H, W, 300)
    srcs = [np.ascontiguousarray(M.shifted(a, k * SHIFT[0], k * SHIFT[1])) for k in range(8)]
    imgs = [shapes.Image(shapes.Metadata("c%d" % i, W, H, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=RESIZE[0], max_size=RESIZE[1])
    return srcs, resized, ratios, [engine.host_pixels(r) for r in resized]


def submit_every(engine, clip, frames, threshold=0.0, batch=B, every=K, **kw):
    """One pass over ``frames`` of the clip: all of them go up, every K-th is a key frame."""
    srcs, resized, ratios, pixels = clip
    keys = frames[::every]
    kw = dict(dict(redact=REDACT, track=TRACK, track_motion=RADIUS, detect_every=every), **kw)
    return engine.submit_batch([resized[i] for i in keys], [ratios[i] for i in keys], threshold, [pixels[i] for i in frames], batch=batch,
                               annotate=True, **kw)


def check_frames(tracker, srcs, results, mapping, first=0, every=K):
    """The results of consecutive frames, key and between, against the restatements -> [(live, held)]."""
    seen = []
    for f, (src, (n_rois, dets, out)) in enumerate(zip(srcs, results), first):
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
        seen.append((live, held))
    return seen


def test_two_passes_of_four_frames_against_the_restatements(engine, clip, f32_models):
    mapping = f32_models[0].class_mapping
    srcs = clip[0]
    engine.track_reset()
    tickets = [submit_every(engine, clip, [0, 1, 2, 3]), submit_every(engine, clip, [4, 5, 6, 7], threshold=2.0)]
    assert [t.frames for t in tickets] == [4, 4] and [len(t.image) for t in tickets] == [2, 2]
    results = engine.collect_batch(tickets[0]) + engine.collect_batch(tickets[1])
    assert len(results) == 8
    tracker = I.IntervalTracker(64)
    seen = check_frames(tracker, srcs, results, mapping)
    assert np.array_equal(engine.track_state().cpu().numpy(), tracker.t.words()) and tracker.t.frames == 8
    mstate = engine.track_motion_state(H, W).cpu().numpy()
    assert mstate[:16].view(np.int32).tolist() == [8, H, W, 0] and np.array_equal(mstate[16:].reshape(H, W, 3), srcs[7])
    # a between frame shows the tracks of its key frame: the same ids in the same order, and some box moved by exactly the shift
    for f in (1, 3):
        ids = sorted(d["track_id"] for d in seen[f - 1][0] if d["track_id"] > 0)
        assert ids and [d["track_id"] for d in seen[f][0]] == ids
        assert [(d["track_id"], d["held"]) for d in seen[f][1]] == [(d["track_id"], d["held"]) for d in seen[f - 1][1]]
    assert any((dx, dy) == SHIFT for _, dx, dy in tracker.moves)
    # threshold 2.0: the second pass detects nothing; hold counts KEY frames: a between frame shows its key frame's ages, and from one
    # key frame to the next every track that is still held has aged by one
    ages = [{d["track_id"]: d["held"] for d in seen[f][1]} for f in range(8)]
    for f in (4, 5, 6, 7):
        assert not seen[f][0] and ages[f] and (results[f][2] != srcs[f]).any()
    assert ages[5] == ages[4] and ages[7] == ages[6] and 1 in ages[4].values()
    assert ages[6] == {i: a + 1 for i, a in ages[4].items() if a + 1 <= TRACK[1]}
    assert any(k[-len(TAIL):] == TAIL for k in engine.cache.keys())
    # the key frames' live rows are those of a plain tracking pass over the key frames alone
    engine.track_reset()
    srcs_, resized, ratios, pixels = clip
    plain = engine.collect_batch(engine.submit_batch([resized[0], resized[2]], [ratios[0], ratios[2]], 0.0, [pixels[0], pixels[2]], batch=B,
                                                     annotate=True, redact=REDACT, track=TRACK, track_motion=RADIUS))
    for f, (_, dets, _) in zip((0, 2), plain):
        rows = lambda ds: [(d["bbox"].tolist(), d["cls_name"], float(d["prob"])) for d in ds if "held" not in d]
        assert rows(dets) == rows(results[f][1]) and rows(dets)


def test_a_short_last_pass_of_three_frames(engine, clip, f32_models):
    mapping = f32_models[0].class_mapping
    engine.track_reset()
    first = engine.collect_batch(submit_every(engine, clip, [0, 1, 2, 3]))
    ticket = submit_every(engine, clip, [4, 5, 6])
    assert ticket.frames == 3 and len(ticket.image) == 2
    last = engine.collect_batch(ticket)
    assert len(first) == 4 and len(last) == 3
    tracker = I.IntervalTracker(64)
    check_frames(tracker, clip[0], first + last, mapping)
    assert tracker.t.frames == 7 and np.array_equal(engine.track_state().cpu().numpy(), tracker.t.words())
    assert engine.track_motion_state(H, W)[:16].view(torch.int32).cpu().tolist() == [7, H, W, 0]


def test_passes_without_the_option_are_what_they_were(engine, clip, moving, f32_models):
    """The motion sequence of tests/test_track_motion_entry_gpu.py before and after a detect_every sequence: the same bytes, and no
    cache key but the new passes' own carries the tail."""
    mapping = f32_models[0].class_mapping
    before, _ = run_sequence(engine, moving, mapping, True)
    keys = set(engine.cache.keys())
    engine.track_reset()
    engine.collect_batch(submit_every(engine, clip, [0, 1, 2, 3]))
    after, _ = run_sequence(engine, moving, mapping, True)
    now = set(engine.cache.keys())
    every = {k for k in now if "every" in k}
    assert every and all(k[-len(TAIL):] == TAIL for k in every) and now - every == keys - every
    for (_, live_a, held_a, out_a), (_, live_b, held_b, out_b) in zip(before, after):
        assert np.array_equal(out_a, out_b)
        assert len(live_a) == len(live_b) and all(same_det(a, b) for a, b in zip(live_a + held_a, live_b + held_b))


def test_submit_batch_refusals(engine, clip):
    from faster_rcnn_amd._lib import FrcnnError
    captures = engine.cache.captures
    with pytest.raises(FrcnnError, match="track_motion"):
        submit_every(engine, clip, [0, 1], track_motion=None)
    with pytest.raises(FrcnnError, match="track_motion"):
        submit_every(engine, clip, [0, 1], track=None, track_motion=None)
    with pytest.raises(FrcnnError, match="track_lookback"):
        submit_every(engine, clip, [0, 1, 2, 3], track_lookback=2)
    for bad in (1, 0, 17, -2, True, 2.0, "2", (2,)):
        with pytest.raises(FrcnnError, match="detect_every"):
            submit_every(engine, clip, [0, 1], every=2, detect_every=bad)
    with pytest.raises(FrcnnError, match="at most 64"):                        # 5 * 13 = 65 frames in one tracker call
        submit_every(engine, clip, [0, 1], batch=5, every=13)
    srcs, resized, ratios, pixels = clip
    kw = dict(batch=B, annotate=True, redact=REDACT, track=TRACK, track_motion=RADIUS, detect_every=K)
    for images, frames in (([0, 1, 2], [0, 1, 2]), ([0], [0, 1, 2]), ([0, 2, 4], [0, 1, 2, 3, 4]), ([0, 2], [])):
        with pytest.raises(FrcnnError, match="key frames"):
            engine.submit_batch([resized[i] for i in images], [ratios[i] for i in images], 0.0, [pixels[i] for i in frames], **kw)
    with pytest.raises(FrcnnError, match="ANNOTATING"):
        engine.submit_batch(resized[:1], ratios[:1], 0.0, pixels[:2], batch=B, track=TRACK, track_motion=RADIUS, detect_every=K)
    assert engine.cache.captures == captures


def test_a_foreign_preprocess_is_refused(clip, f32_models):
    """An engine whose manager carries a preprocess function the entry does not know uploads float pixels of the network images: there
    are no uint8 source frames for the block match.  The refusal names the option and the reason, in front of any capture."""
    from faster_rcnn_amd import entry, resnet
    from faster_rcnn_amd._lib import FrcnnError
    from faster_rcnn_amd.det_util import DetTrainingManager
    mgr, det, _ = f32_models
    mgr2 = DetTrainingManager(rpn_model=mgr.rpn_model, class_mapping=mgr.class_mapping, preprocess_func=lambda d: resnet.preprocess(d),
                              anchor_dims=mgr.anchor_dims)
    foreign = entry.for_models(mgr2, det, 64, 16, 1)
    assert foreign is not None and not foreign.device_preprocess
    _, resized, ratios, _ = clip
    pixels = [foreign.host_pixels(r) for r in resized[:4]]
    assert all(p[0].dtype != np.uint8 for p in pixels)                          # (what such an engine stages: the preprocessed floats)
    kw = dict(batch=B, annotate=True, redact=REDACT, track=TRACK, track_motion=RADIUS)
    with pytest.raises(FrcnnError, match=r"detect_every= needs the device-side preprocess.*foreign preprocess_func.*float"):
        foreign.submit_batch([resized[0], resized[2]], [ratios[0], ratios[2]], 0.0, pixels, detect_every=K, **kw)
    with pytest.raises(FrcnnError, match="annotating passes need the device-side preprocess"):        # (as without the option)
        foreign.submit_batch(resized[:2], ratios[:2], 0.0, pixels[:2], **kw)
    assert foreign.cache.captures == 0 and not list(foreign.cache.keys())


def test_an_annotating_key_is_never_a_canvas_key(engine, clip, monkeypatch):
    """detect_every goes with annotating passes only, and those take the exact geometry for their key: with canvas passes switched on, a
    detecting pass over these frames is a canvas pass, and the detect_every pass is the one it was -- the same key, no capture."""
    engine.track_reset()
    want = engine.collect_batch(submit_every(engine, clip, [0, 1, 2, 3]))
    captures, keys = engine.cache.captures, set(engine.cache.keys())
    monkeypatch.setattr(engine, "canvas_capable", True)
    monkeypatch.setattr(engine, "canvas", True)
    pixels = clip[3]
    assert engine.geometry(pixels[0])[0] == "canvas" and engine.geometry_of(pixels[0])[0] != "canvas"
    engine.track_reset()
    got = engine.collect_batch(submit_every(engine, clip, [0, 1, 2, 3]))
    assert engine.cache.captures == captures and set(engine.cache.keys()) == keys
    every = [k for k in keys if "every" in k]
    assert every and all(k[0] != "canvas" and "annotate" in k for k in every)
    assert len(got) == len(want) == 4
    for (n_a, dets_a, out_a), (n_b, dets_b, out_b) in zip(want, got):
        assert n_a == n_b and len(dets_a) == len(dets_b) and all(same_det(a, b) for a, b in zip(dets_a, dets_b))
        assert np.array_equal(out_a, out_b)


# ----------------------------------------------------------------------------------------------------------- annotate_images
def test_annotate_images_writes_every_frame_of_a_pass_in_order(engine, f32_models, monkeypatch, tmp_path):
    """A directory of eleven PNG frames through ``annotate_images`` with the engine's passes of four images and detect_every 2: a full
    pass of eight frames and a padded one of three.  Every file, under its own name, and every MOT line is the restatement's."""
    from PIL import Image as PilImage
    from faster_rcnn_amd import annotate_video, entry
    mgr, det, _ = f32_models
    mapping = mgr.class_mapping
    a = frame_pixels(H, W, 71)
    srcs = [np.ascontiguousarray(M.shifted(a, k * SHIFT[0], k * SHIFT[1])) for k in range(11)]
    names = ["f_%02d.png" % (7 * k) for k in range(len(srcs))]               # (names that are not their positions)
    d_in, d_out = tmp_path / "in", tmp_path / "out"
    d_in.mkdir()
    for name, rgb in zip(names, srcs):
        PilImage.fromarray(rgb).save(str(d_in / name))
    seen, tickets, collect = [], [], entry.DetectionEntry.collect_batch

    def recording(self, ticket):
        res = collect(self, ticket)
        tickets.append((ticket.frames, len(ticket.image), ticket.slot.batch))
        seen.extend(res)
        return res

    monkeypatch.setattr(entry.DetectionEntry, "collect_batch", recording)
    tracks = io.StringIO()
    _, text = quiet(annotate_video.annotate_images, mgr, det, str(d_in), str(d_out), names, *RESIZE, png_encoder="host", redact=REDACT,
                    track=TRACK, tracks_out=tracks, track_motion=RADIUS, detect_every=K)
    assert tickets == [(8, 4, 4), (3, 2, 4)] and len(seen) == 11
    assert sorted(p.name for p in d_out.iterdir()) == sorted(names)
    assert [x for x in text.splitlines() if x.startswith("processing")] == ["processing " + str(d_in / n) for n in names]
    tracker = I.IntervalTracker(64)
    # (the files hold R,G,B as PIL delivers it and the passes draw into them as they came: the restatement sees the same arrays)
    per_frame = check_frames(tracker, srcs[:8], seen[:8], mapping) + check_frames(tracker, srcs[8:], seen[8:], mapping)
    want_lines = []
    for k, (live, held) in enumerate(per_frame):
        want_lines += T.mot_lines(k + 1, live, mapping)
        got = np.asarray(PilImage.open(str(d_out / names[k])).convert("RGB"))
        assert np.array_equal(got, expected(srcs[k], live, held, mapping)), names[k]
    assert tracks.getvalue() == "".join(x + "\n" for x in want_lines)
    between = [ln for ln in want_lines if int(ln.split(",")[0]) % K == 0]     # (MOT frame numbers start at 1: the even ones are between frames)
    assert between and tracker.t.frames == 11
