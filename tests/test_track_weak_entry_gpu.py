"""The weak rule through the detection entry: submit_batch(annotate=True, track=..., track_strong=T) uploads the LOW threshold and runs the
tracker's ``strong=T`` form inside the captured pass.  The packed buffers of each pass are read from its slot's host copy (a pass of
another size does not give the same probability bits); tests/track_weak_ref.py over them, in order, is what ``collect_batch`` must return
-- the kept rows with their ids, then the held ones -- and tests/redact_ref.py and the drawing rule over those rows what the frame must
show, byte for byte.  A pass without the option against tests/track_ref.py and the same drawing chain; a y4m stream with ``track_low``
and ``track_lookback`` against tests/track_lookback_ref.py fed with the weak tracked rows."""
import io

import numpy as np
import pytest

from tests import redact_ref as R
from tests import track_lookback_ref as LB
from tests import track_ref as T
from tests import track_weak_ref as WR
from tests import y4m_cases as C
from tests import y4m_ref as Y
from tests.test_redact_entry_gpu import RESIZE, engine, f32_models, frame_pixels, quiet, staged      # noqa: F401  (the synthetic ResNet-50 pair, 200x330 frames)
from tests.test_track_entry_gpu import REDACT, TRACK, check_against_rule, expected, same_det, split_dets, submit, tracked_classes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

H, W = 200, 330
LOW = 0.0


def class_table(mapping):
    table = np.zeros(max(mapping.values()) + 1, dtype=np.uint8)
    for name, idx in mapping.items():
        table[idx] = name in tracked_classes(mapping)
    return table


def test_a_weak_pass_is_the_reference_chain_over_its_packed_buffers(engine, staged, f32_models):
    from faster_rcnn_amd import ops
    mapping = f32_models[0].class_mapping
    rev = {v: k for k, v in mapping.items()}
    table, srcs = class_table(mapping), staged[0]
    # the scores of frame 0 at the low threshold, to put the thresholds between them
    plain = engine.collect_batch(submit(engine, staged, [0, 0], 2, threshold=LOW))
    probs = sorted(float(d["prob"]) for d in plain[0][1] if d["cls_name"] in tracked_classes(mapping))
    assert len(probs) >= 4 and probs[0] < probs[-1], "the test needs scores to put a threshold between"
    strong = float(np.float32(probs[len(probs) // 2]))
    assert any(p < strong for p in probs)
    everything = 0.0                                                         # every row is strong: all the tracked ones start tracks
    engine.track_reset()
    kw = dict(redact=REDACT, track=TRACK)
    before = set(engine.cache.keys())
    tracker = WR.Tracker(64)
    dropped = 0
    for frames, s in (([0, 0], everything), ([0, 0], strong), ([1, 0], strong), ([2], strong)):      # the last: a short pass
        ticket = submit(engine, staged, frames, 2, threshold=LOW, track_strong=s, **kw)
        res = engine.collect_batch(ticket)
        assert len(res) == len(frames)
        for i, (f, (n_rois, dets, out)) in enumerate(zip(frames, res)):
            packed = ticket.slot.out_pin[i].numpy().copy()                   # the pass's own packed buffer, as collect_batch read it
            want = ops.tracked_dets(tracker.update_packed(packed, table, H, W, *TRACK, strong=s), rev)[2]
            assert len(dets) == len(want) and all(same_det(a, b) for a, b in zip(dets, want)), (f, s)
            live, held = split_dets(dets)
            assert all("track_id" in d for d in live) and len(live) <= int(packed[0])
            dropped += int(packed[0]) - len(live)
            assert np.array_equal(out, expected(srcs[f], live, held, mapping)), (f, s)
    assert tracker.events["weak_match"] > 0 and tracker.events["weak_drop"] > 0 and dropped == tracker.events["weak_drop"]
    assert np.array_equal(engine.track_state().cpu().numpy(), tracker.words()) and tracker.frames == 7
    # the keys: the plain tracking key with the tag behind it
    new = set(engine.cache.keys()) - before
    tail = ("track",) + TRACK
    assert {k[-2:] for k in new} == {("weak", everything), ("weak", strong)}
    assert all(k[-2 - len(tail):-2] == tail for k in new)
    engine.track_reset()
    res = engine.collect_batch(submit(engine, staged, [0, 0], 2, threshold=LOW, **kw))   # without the option: the key it always had
    assert any(k[-len(tail):] == tail for k in set(engine.cache.keys()) - new)
    assert len(split_dets(res[0][1])[0]) == len(plain[0][1])                 # ... every packed row is a det
    parent = T.Tracker(64)                                                   # ... and every det and output byte the Tracking rule's chain
    for n_rois, dets, out in res:
        live, held = check_against_rule(parent, dets, mapping, H, W)
        assert np.array_equal(out, expected(srcs[0], live, held, mapping))
    assert np.array_equal(engine.track_state().cpu().numpy(), parent.words())
    engine.track_reset()
    torch.cuda.synchronize()


def test_the_pass_refuses_by_name(engine, staged):
    from faster_rcnn_amd._lib import FrcnnError
    with pytest.raises(FrcnnError, match="track_strong= tells the tracker"):
        submit(engine, staged, [0], 1, track_strong=0.5)
    with pytest.raises(FrcnnError, match="track_strong: det threshold=1.5"):
        submit(engine, staged, [0], 1, track=TRACK, track_strong=1.5)


# ----------------------------------------------------------------------------------------------------------- with track_lookback
LB_TRACK, LB_RADIUS = (30, 1, 1), 4
LH, LW, LN = 96, 128, 6


def run_stream(mgr, det, data, monkeypatch, **kw):
    """A y4m stream through annotate_stream -> (the stream written, the MOT lines, every result collect_batch returned, in order)."""
    import contextlib
    from faster_rcnn_amd import annotate_video, entry, y4m
    seen, collect = [], entry.DetectionEntry.collect_batch

    def recording(self, ticket):
        res = collect(self, ticket)
        seen.extend(res)
        return res

    monkeypatch.setattr(entry.DetectionEntry, "collect_batch", recording)
    reader = y4m.Y4mReader(io.BytesIO(data), name="clip.y4m")
    sink, tracks = io.BytesIO(), io.StringIO()
    writer = y4m.Y4mWriter(sink, LW, LH, "444", "full", reader.plan.tags)
    with contextlib.redirect_stdout(io.StringIO()):
        annotate_video.annotate_stream(mgr, det, reader, writer, *RESIZE, redact=REDACT, track=LB_TRACK, tracks_out=tracks,
                                       track_motion=LB_RADIUS, **kw)
    monkeypatch.setattr(entry.DetectionEntry, "collect_batch", collect)
    return sink.getvalue(), tracks.getvalue(), seen


def test_a_stream_with_track_low_and_lookback_against_the_restatement(engine, f32_models, monkeypatch):
    """tests/test_track_lookback_entry_gpu.py's clip -- two frames of one noise image, four of another --, with ``track_low``: the weak
    tracked rows of the run WITHOUT look-back (n_live under the packed count), pushed through the look-back restatement, are what the run
    with look-back emits -- the same dets, the back-filled rows, and every byte of the stream."""
    mgr, det, _ = f32_models
    mapping = mgr.class_mapping
    a, b = frame_pixels(LH, LW, 71), frame_pixels(LH, LW, 72)
    frames = [a, a] + [np.ascontiguousarray(np.roll(b, 2 * k, axis=1)) for k in range(LN - 2)]
    records = [Y.encode(f, "444", "full") for f in frames]
    data = C.stream(records, LH, LW, "444", "full", tags="F25:1 Ip A1:1")
    _, _, everything = run_stream(mgr, det, data, monkeypatch)               # every detection: the scores to put the threshold between
    probs = sorted(float(d["prob"]) for _, dets, _ in everything for d in dets if "held" not in d)
    strong = float(np.float32(probs[len(probs) // 2]))
    assert 0.0 < strong and probs[0] < strong
    weak = dict(det_threshold=strong, track_low=0.0)
    plain, plain_lines, plain_seen = run_stream(mgr, det, data, monkeypatch, **weak)
    assert any(k[-2:] == ("weak", strong) for k in engine.cache.keys())
    per_frame = [split_dets(dets) for _, dets, _ in plain_seen]
    assert len(per_frame) == len(everything) == LN
    assert all(len(live) <= len(split_dets(dets)[0]) for (live, _), (_, dets, _) in zip(per_frame, everything))
    assert sum(len(live) for live, _ in per_frame) < sum(len(split_dets(dets)[0]) for _, dets, _ in everything)      # rows were dropped
    assert any(d["track_id"] > 0 and float(d["prob"]) < strong for live, _ in per_frame for d in live)              # ... and weak ones kept
    L = min(4, engine.batch)
    got, lines, seen = run_stream(mgr, det, data, monkeypatch, track_lookback=L, **weak)
    assert any(k[-2:] == ("weak", strong) and "lookback" in k for k in engine.cache.keys())
    assert len(seen) == LN and lines == plain_lines and lines
    srcs = [Y.decode(r, LH, LW, "444", "full") for r in records]
    back = LB.backfill_dets(srcs, per_frame, L, LB_RADIUS, LB_TRACK[2])
    assert sum(len(x) for x in back) > 0, "no track reaches back: the test would show nothing"
    want = []
    for k, (src, (live, held)) in enumerate(zip(srcs, per_frame)):
        n_rois, dets, _ = seen[k]
        assert n_rois == plain_seen[k][0]
        rest = [d for d in dets if not d.get("backfilled")]
        assert len(rest) == len(plain_seen[k][1]) and all(same_det(x, y) for x, y in zip(rest, plain_seen[k][1])), k
        filled = [d for d in dets if d.get("backfilled")]
        assert [(d["bbox"].tolist(), d["cls_name"], d["track_id"], d["backfilled"]) for d in filled] == \
            [(d["bbox"].tolist(), d["cls_name"], d["track_id"], d["backfilled"]) for d in back[k]], k
        out = R.redact_dets(src, live + held + back[k], mapping, *REDACT)
        want.append(Y.encode(T.annotate(out, live), "444", "full"))
    assert got == C.stream(want, LH, LW, "444", "full", tags="F25:1 Ip A1:1")
    assert plain == C.stream([Y.encode(T.annotate(R.redact_dets(s, lv + hd, mapping, *REDACT), lv), "444", "full")
                              for s, (lv, hd) in zip(srcs, per_frame)], LH, LW, "444", "full", tags="F25:1 Ip A1:1")
