"""The motion step through the detection entry and annotate_video: submit_batch(annotate=True, track=..., track_motion=R) runs
ops.track_update_motion inside the captured pass, on the frames as they were uploaded, in front of the redaction and the drawing step.
Every result is held against the restatements: tests/track_motion_ref.py over the source frames and the live rows the passes returned,
then tests/redact_ref.py over the live and the held rows, then the drawing rule with ids -- byte for byte."""
import io

import numpy as np
import pytest

from tests import redact_ref as R
from tests import track_motion_ref as M
from tests import track_ref as T
from tests import y4m_cases as C
from tests import y4m_ref as Y
from tests.test_redact_entry_gpu import RESIZE, engine, f32_models, frame_pixels, quiet      # noqa: F401  (the synthetic ResNet-50 pair)
from tests.test_track_entry_gpu import same_det, split_dets, tracked_classes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TRACK = (30, 4, 0)                       # grow 0: a held row's box is the slot's clipped box
RADIUS = 8
REDACT = ("all", "pixelate", 5, 1)
H, W = 200, 330
SHIFT = (3, 2)


@pytest.fixture(scope="module")
def moving(engine):
    """Frame A twice, then A moved by (3, 2) and by (6, 4): four in-memory BGR frames, resized and with their host pixels."""
    from faster_rcnn_amd import shapes, util
    a = frame_pixels(H, W, 300)
    srcs = [a, a, np.ascontiguousarray(M.shifted(a, *SHIFT)), np.ascontiguousarray(M.shifted(a, 2 * SHIFT[0], 2 * SHIFT[1]))]
    imgs = [shapes.Image(shapes.Metadata("m%d" % i, W, H, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=RESIZE[0], max_size=RESIZE[1])
    return srcs, resized, ratios, [engine.host_pixels(r) for r in resized]


def submit(engine, staged, frames, threshold=0.0, **kw):
    srcs, resized, ratios, pixels = staged
    return engine.submit_batch([resized[i] for i in frames], [ratios[i] for i in frames], threshold, [pixels[i] for i in frames],
                               batch=len(frames), annotate=True, **kw)


def check_against_rule(tracker, frame, dets, mapping, motion):
    """One frame's returned dets == the restatement over the frame and its live rows.  -> (live, held)."""
    live, held = split_dets(dets)
    plain = [{k: d[k] for k in ("bbox", "cls_name", "prob")} for d in live]
    h, w = frame.shape[:2]
    if motion:
        want_live, want_held = tracker.track_dets(frame, plain, mapping, tracked_classes(mapping), *TRACK, RADIUS)
    else:
        want_live, want_held = T.track_dets(tracker, plain, mapping, tracked_classes(mapping), h, w, *TRACK)
    assert len(live) == len(want_live) and all(same_det(a, b) for a, b in zip(live, want_live))
    assert len(held) == len(want_held) and all(same_det(a, b) for a, b in zip(held, want_held)), (held, want_held)
    return live, held


def expected(src, live, held, mapping, draw=True):
    out = R.redact_dets(src, live + held, mapping, *REDACT)
    return T.annotate(out, live) if draw else out


def run_sequence(engine, moving, mapping, motion, draw=True):
    """The two passes, both in flight at once -> [(src, live, held, out)] of the four frames, each checked against the restatements."""
    kw = dict(redact=REDACT, track=TRACK, draw=draw)
    if motion:
        kw["track_motion"] = RADIUS
    engine.track_reset()
    tickets = [submit(engine, moving, [0, 1], **kw), submit(engine, moving, [2, 3], threshold=2.0, **kw)]
    passes = [engine.collect_batch(t) for t in tickets]
    tracker = M.MotionTracker(64) if motion else T.Tracker(64)
    frames = []
    for src, (n_rois, dets, out) in zip(moving[0], passes[0] + passes[1]):
        live, held = check_against_rule(tracker, src, dets, mapping, motion)
        assert np.array_equal(out, expected(src, live, held, mapping, draw)), len(frames)
        frames.append((src, live, held, out))
    return frames, tracker


@pytest.mark.parametrize("draw", [True, False])
def test_held_boxes_follow_the_pixels(engine, moving, f32_models, draw):
    mapping = f32_models[0].class_mapping
    frames, tracker = run_sequence(engine, moving, mapping, True, draw)
    assert np.array_equal(engine.track_state().cpu().numpy(), tracker.t.words())
    mstate = engine.track_motion_state(H, W).cpu().numpy()
    assert mstate[:16].view(np.int32).tolist() == [4, H, W, 0] and np.array_equal(mstate[16:].reshape(H, W, 3), moving[0][3])
    seen = {d["track_id"]: d["bbox"] for d in frames[1][1] if d["track_id"] > 0}
    assert seen and not frames[0][2] and not frames[1][2]
    assert any((dx, dy) == SHIFT for _, dx, dy in tracker.moves)             # (identical frames move nothing; noise moved by (3, 2) is found)
    for k in (2, 3):                                                         # threshold 2.0: nothing is detected, everything is held
        src, live, held, out = frames[k]
        assert not live and len(held) == len(seen) and all(d["held"] == k - 1 for d in held)
        exact = 0
        for d in held:
            x1, y1, x2, y2 = [int(v) for v in seen[d["track_id"]]]
            s = (k - 1) * SHIFT[0], (k - 1) * SHIFT[1]
            xa, xb, ya, yb = T.clip([x1 + s[0], y1 + s[1], x2 + s[0], y2 + s[1]], H, W)
            stood = T.clip([x1, y1, x2, y2], H, W)
            exact += d["bbox"].tolist() == [xa, ya, xb, yb] and (xa, xb, ya, yb) != stood
        assert exact >= 1, "no held box moved by exactly the shift"
        assert (out != src).any()
    tail = ("track",) + TRACK + ("motion", RADIUS)
    assert any(k[-len(tail):] == tail and "redact" in k for k in engine.cache.keys())


def test_without_the_argument_held_boxes_stand_still(engine, moving, f32_models):
    mapping = f32_models[0].class_mapping
    keys_before = set(engine.cache.keys())
    frames, tracker = run_sequence(engine, moving, mapping, False)
    seen = {d["track_id"]: d["bbox"] for d in frames[1][1] if d["track_id"] > 0}
    for k in (2, 3):
        _, live, held, _ = frames[k]
        assert not live and len(held) == len(seen)
        for d in held:
            xa, xb, ya, yb = T.clip(seen[d["track_id"]], H, W)
            assert d["bbox"].tolist() == [xa, ya, xb, yb]
    new = set(engine.cache.keys()) - keys_before
    assert all("motion" not in k for k in new) and all(k[-4:] == ("track",) + TRACK for k in new)      # a plain tracking key: as it was


def test_track_reset_clears_the_headers(engine, moving, f32_models):
    engine.collect_batch(submit(engine, moving, [0, 1], track=TRACK, track_motion=RADIUS, redact=REDACT))
    torch.cuda.synchronize()
    m = engine.track_motion_state(H, W)
    assert int(m[:16].view(torch.int32)[0]) >= 1
    body = m[16:].clone()
    engine.track_reset()
    torch.cuda.synchronize()
    assert not m[:16].cpu().numpy().any() and torch.equal(m[16:], body) and not engine.track_state().cpu().numpy().any()
    assert engine.track_motion_state(H, W) is m


def test_submit_batch_refusals(engine, moving):
    from faster_rcnn_amd._lib import FrcnnError
    srcs, resized, ratios, pixels = moving
    captures = engine.cache.captures
    one = lambda **kw: engine.submit_batch(resized[:1], ratios[:1], 0.0, pixels[:1], batch=1, annotate=True, **kw)
    with pytest.raises(FrcnnError) as e:
        one(track_motion=RADIUS)
    assert "track=" in str(e.value)
    for bad in (0, 17, -1, True, 8.0, "8", (8,)):
        with pytest.raises(FrcnnError):
            one(track=TRACK, track_motion=bad)
    assert engine.cache.captures == captures


# ----------------------------------------------------------------------------------------------------------- annotate_video
def test_annotate_stream_moves_held_boxes_in_a_y4m_stream(engine, f32_models, monkeypatch):
    from faster_rcnn_amd import annotate_video, entry, y4m
    mgr, det, _ = f32_models
    mapping = mgr.class_mapping
    h, w, n = 96, 128, 5                                                     # a pass of four and a one-frame pass
    base = frame_pixels(h, w, 71)
    moved = [np.ascontiguousarray(M.shifted(base, k * SHIFT[0], k * SHIFT[1])) for k in range(n)]
    records = [Y.encode(f, "444", "full") for f in moved]
    data = C.stream(records, h, w, "444", "full", tags="F25:1 Ip A1:1")
    seen = []
    collect = entry.DetectionEntry.collect_batch

    def recording(self, ticket):
        res = collect(self, ticket)
        seen.extend(res)
        return res

    monkeypatch.setattr(entry.DetectionEntry, "collect_batch", recording)

    def run():
        del seen[:]
        reader = y4m.Y4mReader(io.BytesIO(data), name="clip.y4m")
        sink, tracks = io.BytesIO(), io.StringIO()
        writer = y4m.Y4mWriter(sink, w, h, "444", "full", reader.plan.tags)
        quiet(annotate_video.annotate_stream, mgr, det, reader, writer, *RESIZE, redact=REDACT, track=TRACK, tracks_out=tracks,
              track_motion=RADIUS)
        return sink.getvalue(), tracks.getvalue()

    got, lines = run()
    assert len(seen) == n
    tracker = M.MotionTracker(64)
    want_frames, want_lines = [], []
    for k, ((n_rois, dets, _), record) in enumerate(zip(seen, records)):
        src = Y.decode(record, h, w, "444", "full")
        live, held = check_against_rule(tracker, src, dets, mapping, True)
        want_frames.append(Y.encode(expected(src, live, held, mapping), "444", "full"))
        want_lines += T.mot_lines(k + 1, live, mapping)
    assert got == C.stream(want_frames, h, w, "444", "full", tags="F25:1 Ip A1:1")
    assert want_lines and lines == "".join(x + "\n" for x in want_lines)
    assert tracker.moves and tracker.t.frames == n
    assert run() == (got, lines)                                             # a second run starts a new sequence: the same bytes
    with pytest.raises(ValueError):
        annotate_video.annotate_stream(mgr, det, y4m.Y4mReader(io.BytesIO(data), name="clip.y4m"), None, *RESIZE, track_motion=RADIUS)


def test_the_parser_refuses_the_flag_without_track():
    from faster_rcnn_amd import annotate_video
    parse = lambda *extra: annotate_video.build_parser().parse_args(["a.h5", "b.h5", "frames"] + list(extra))
    with pytest.raises(ValueError) as e:
        annotate_video.track_motion_from_args(parse("--track_motion", "8"))
    assert "--track_motion" in str(e.value) and "needs --track" in str(e.value)
    assert annotate_video.track_motion_from_args(parse("--track", "--track_motion")) == 8
