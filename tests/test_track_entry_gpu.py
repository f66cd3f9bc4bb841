"""Tracking through the detection entry and annotate_video: submit_batch(annotate=True, track=(thr, hold, grow)) runs the engine's
tracker inside the captured pass, behind the post-process; the redaction then hides the held boxes too and the drawing step labels the
live rows with their ids.  Every result is held against the restatements: tests/track_ref.py over the live rows the passes returned, in
order, then tests/redact_ref.py over the live and the held rows, then the drawing rule with ids -- byte for byte."""
import io

import numpy as np
import pytest

from tests import redact_ref as R
from tests import track_ref as T
from tests import y4m_cases as C
from tests import y4m_ref as Y
from tests.annotate_ref import annotate as draw_ref
from tests.test_redact_entry_gpu import RESIZE, engine, f32_models, frame_pixels, quiet, staged      # noqa: F401  (the synthetic ResNet-50 pair, 200x330 frames)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TRACK = (30, 2, 3)
REDACT = ("all", "pixelate", 5, 1)
H, W = 200, 330


def tracked_classes(mapping):
    return tuple(n for n in mapping if n != "bg")                             # VOC: every class is drawable


def split_dets(dets):
    live = [d for d in dets if "held" not in d]
    held = [d for d in dets if "held" in d]
    assert ["held" in d for d in dets] == [False] * len(live) + [True] * len(held)      # the held rows follow the live ones
    return live, held


def same_det(a, b):
    return (np.array_equal(a["bbox"], b["bbox"]) and a["cls_name"] == b["cls_name"] and np.float32(a["prob"]) == np.float32(b["prob"])
            and a.get("track_id", 0) == b.get("track_id", 0) and a.get("held", 0) == b.get("held", 0))


def check_against_rule(tracker, dets, mapping, h, w, track=TRACK):
    """One frame's returned dets == the restatement over its live rows (the tracker carries the sequence).  -> (live, held)."""
    live, held = split_dets(dets)
    plain = [{k: d[k] for k in ("bbox", "cls_name", "prob")} for d in live]
    want_live, want_held = T.track_dets(tracker, plain, mapping, tracked_classes(mapping), h, w, *track)
    assert len(live) == len(want_live) and all(same_det(a, b) for a, b in zip(live, want_live))
    assert len(held) == len(want_held) and all(same_det(a, b) for a, b in zip(held, want_held)), (held, want_held)
    return live, held


def expected(src, live, held, mapping, redact=REDACT, draw=True):
    out = src if redact is None else R.redact_dets(src, live + held, mapping, *redact)
    return T.annotate(out, live) if draw else out


def submit(engine, staged, frames, B, threshold=0.0, **kw):
    srcs, resized, ratios, pixels = staged
    return engine.submit_batch([resized[i] for i in frames], [ratios[i] for i in frames], threshold, [pixels[i] for i in frames], batch=B,
                               annotate=True, **kw)


def decode(out, encode):
    if encode == "png":
        from PIL import Image as PilImage
        return np.asarray(PilImage.open(io.BytesIO(out)).convert("RGB"))[:, :, ::-1]
    return out


@pytest.mark.parametrize("encode", [None, "png", "y4m"])
def test_a_sequence_of_three_passes(engine, staged, f32_models, encode):
    """B = 4 of one frame; the same at threshold 2.0, which no probability passes: every track is held for two frames, its box growing
    by 3 pixels a frame, and is then freed; a pass of one."""
    mapping = f32_models[0].class_mapping
    src = staged[0][0]
    assert engine.in_flight > 1
    kw = dict(redact=REDACT, track=TRACK)
    if encode == "png":
        kw["encode"] = "png"
    elif encode == "y4m":
        kw.update(encode="y4m", y4m=("444", "full"))
    engine.track_reset()
    tickets = [submit(engine, staged, [0, 0, 0, 0], 4, **kw), submit(engine, staged, [0, 0, 0, 0], 4, threshold=2.0, **kw),
               submit(engine, staged, [0], 1, **kw)]                         # all three in flight: the tracking stream keeps their order
    passes = [engine.collect_batch(t) for t in tickets]
    assert [len(p) for p in passes] == [4, 4, 1]
    tracker = T.Tracker(64)
    frames = []
    for res in passes:
        for n_rois, dets, out in res:
            live, held = check_against_rule(tracker, dets, mapping, H, W)
            frames.append((live, held, out))
    first = frames[0][0]
    redacted = set(tracked_classes(mapping))
    assert any(d["track_id"] > 0 and d["cls_name"] in redacted for d in first), "no tracked detection: the test would show nothing"
    for live, held, _ in frames[1:4]:                                        # stable ids across the four identical frames
        assert [d["track_id"] for d in live] == [d["track_id"] for d in first] and not held
    n_tracks = len({d["track_id"] for d in first if d["track_id"] > 0})
    for k, (live, held, out) in enumerate(frames):
        want = expected(src, live, held, mapping)
        if encode == "y4m":
            assert out == Y.encode(want, "444", "full", bgr=True), k
        else:
            assert np.array_equal(decode(out, encode), want), k
    # pass 2: nothing detected; two frames of held, grown boxes with nothing drawn, then the untouched source
    for k, age in ((4, 1), (5, 2)):
        live, held, out = frames[k]
        assert not live and len(held) == n_tracks and all(d["held"] == age for d in held)
        if encode is None:
            only_hidden = R.redact_dets(src, held, mapping, *REDACT)
            assert np.array_equal(out, only_hidden) and (out != src).any()
            by_id = {d["track_id"]: d for d in first}
            for d in held:
                xa, xb, ya, yb = T.clip(by_id[d["track_id"]]["bbox"], H, W)
                assert d["bbox"].tolist() == [xa - 3 * age, ya - 3 * age, xb + 3 * age, yb + 3 * age]
    for k in (6, 7):
        live, held, out = frames[k]
        assert not live and not held
        if encode is None:
            assert np.array_equal(out, src)
    live, held, _ = frames[8]                                                # every track was freed: new ids
    assert live and min(d["track_id"] for d in live if d["track_id"] > 0) > max(d["track_id"] for d in first)
    tail = ("track",) + TRACK
    assert any(k[-len(tail):] == tail and "redact" in k for k in engine.cache.keys())


def test_a_short_pass_advances_the_state_by_its_frames(engine, staged, f32_models):
    mapping = f32_models[0].class_mapping
    engine.track_reset()
    kw = dict(redact=REDACT, track=TRACK)
    res = engine.collect_batch(submit(engine, staged, [0, 1, 2], 4, **kw))
    assert len(res) == 3
    state = engine.track_state().cpu().numpy()
    assert state[3] == 3                                                     # frames seen: the padding frame is none
    tracker = T.Tracker(64)
    for (n_rois, dets, out), src in zip(res, staged[0]):
        live, held = check_against_rule(tracker, dets, mapping, H, W)
        assert np.array_equal(out, expected(src, live, held, mapping))
    assert np.array_equal(state, tracker.words())
    engine.track_reset()
    torch.cuda.synchronize()
    assert not engine.track_state().cpu().numpy().any()


def test_without_the_argument_nothing_changes(engine, staged, f32_models):
    before = engine.collect_batch(submit(engine, staged, [0, 1, 2, 3], 4))
    keys_before = set(engine.cache.keys())
    plain_key = [k for k in keys_before if k[-1:] == ("annotate",) and 4 in k]
    assert len(plain_key) == 1 and "track" not in plain_key[0]
    engine.track_reset()
    tracked = engine.collect_batch(submit(engine, staged, [0, 1, 2, 3], 4, track=TRACK))
    after = engine.collect_batch(submit(engine, staged, [0, 1, 2, 3], 4))
    new = set(engine.cache.keys()) - keys_before
    assert new <= {plain_key[0] + ("track",) + TRACK} and plain_key[0] + ("track",) + TRACK in engine.cache.keys()
    mapping = f32_models[0].class_mapping
    tracker = T.Tracker(64)
    for (na, da, fa), (nb, db, fb), (nt, dt, ft), src in zip(before, after, tracked, staged[0]):
        assert na == nb == nt and np.array_equal(fa, fb) and np.array_equal(fa, draw_ref(src, da))
        assert all("track_id" not in d and "held" not in d for d in da + db)
        assert len(da) == len(db) and all(same_det(x, y) for x, y in zip(da, db))
        live, held = check_against_rule(tracker, dt, mapping, H, W)
        assert len(live) == len(da) and all(same_det(dict(x, track_id=0), dict(y, track_id=0)) for x, y in zip(live, da))      # live rows as today
        assert np.array_equal(ft, expected(src, live, held, mapping, redact=None))


def test_submit_batch_refusals(engine, staged):
    from faster_rcnn_amd._lib import FrcnnError
    srcs, resized, ratios, pixels = staged
    captures = engine.cache.captures
    one = lambda **kw: engine.submit_batch(resized[:1], ratios[:1], 0.0, pixels[:1], batch=1, **kw)
    with pytest.raises(FrcnnError) as e:
        one(track=TRACK)
    assert "annotate=True" in str(e.value)
    for bad in ((0, 2, 3), (101, 2, 3), (30, 256, 0), (30, 2, 65), (30, 2), "all", (30.5, 2, 3)):
        with pytest.raises(FrcnnError):
            one(annotate=True, track=bad)
    assert engine.cache.captures == captures


# ----------------------------------------------------------------------------------------------------------- annotate_video
def test_annotate_stream_tracks_and_redacts_a_y4m_stream(engine, f32_models, monkeypatch):
    from faster_rcnn_amd import annotate_video, entry, y4m
    mgr, det, _ = f32_models
    mapping = mgr.class_mapping
    h, w, n = 96, 128, 5                                                     # a pass of four and a one-frame pass
    base = frame_pixels(h, w, 71)
    rgbs = [base] * 3 + [frame_pixels(h, w, 72), base]                       # the scene changes for a frame: tracks are held across it
    records = [Y.encode(f, "444", "full") for f in rgbs]
    data = C.stream(records, h, w, "444", "full", tags="F25:1 Ip A1:1")
    seen = []
    collect = entry.DetectionEntry.collect_batch

    def recording(self, ticket):
        res = collect(self, ticket)
        seen.extend(res)
        return res

    monkeypatch.setattr(entry.DetectionEntry, "collect_batch", recording)
    reader = y4m.Y4mReader(io.BytesIO(data), name="clip.y4m")
    sink = io.BytesIO()
    writer = y4m.Y4mWriter(sink, w, h, "444", "full", reader.plan.tags)
    tracks = io.StringIO()
    quiet(annotate_video.annotate_stream, mgr, det, reader, writer, *RESIZE, redact=REDACT, track=TRACK, tracks_out=tracks)
    assert len(seen) == n
    tracker = T.Tracker(64)
    want_frames, want_lines, any_held = [], [], False
    for k, ((n_rois, dets, _), record) in enumerate(zip(seen, records)):
        src = Y.decode(record, h, w, "444", "full")
        live, held = check_against_rule(tracker, dets, mapping, h, w)
        any_held |= bool(held)
        want_frames.append(Y.encode(expected(src, live, held, mapping), "444", "full"))
        want_lines += T.mot_lines(k + 1, live, mapping)
    assert sink.getvalue() == C.stream(want_frames, h, w, "444", "full", tags="F25:1 Ip A1:1")
    assert want_lines and tracks.getvalue() == "".join(x + "\n" for x in want_lines)
    assert tracker.events["match"] and tracker.frames == n
    # a second run starts a new sequence: the same ids, the same bytes
    del seen[:]
    sink2, tracks2 = io.BytesIO(), io.StringIO()
    reader = y4m.Y4mReader(io.BytesIO(data), name="clip.y4m")
    quiet(annotate_video.annotate_stream, mgr, det, reader, y4m.Y4mWriter(sink2, w, h, "444", "full", reader.plan.tags), *RESIZE, redact=REDACT,
          track=TRACK, tracks_out=tracks2)
    assert sink2.getvalue() == sink.getvalue() and tracks2.getvalue() == tracks.getvalue()
