"""The look-back rule through the detection entry and annotate_video: submit_batch(annotate=True, track=..., track_lookback=L) runs
ops.track_lookback behind the tracker inside the captured pass and returns the frames of the pass before.  The written frames are held
against the host restatement: the per-frame dets of a tracking run WITHOUT look-back, pushed through tests/track_lookback_ref.py, then
tests/redact_ref.py over the live, held and back-filled rows, then the drawing rule with ids -- byte for byte."""
import io

import numpy as np
import pytest

from tests import redact_ref as R
from tests import track_lookback_ref as LB
from tests import track_ref as T
from tests import y4m_cases as C
from tests import y4m_ref as Y
from tests.test_redact_entry_gpu import RESIZE, engine, f32_models, frame_pixels, quiet      # noqa: F401  (the synthetic ResNet-50 pair)
from tests.test_track_entry_gpu import split_dets

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TRACK = (30, 1, 1)                       # hold 1: noise frames fill the table; the first image's tracks are freed in frame 3, where new ones are born
RADIUS = 4
REDACT = ("all", "pixelate", 5, 1)
H, W, N = 96, 128, 6                     # with passes of four: a full pass and a final group of two, which goes through a padded pass


def clip_stream():
    """Two frames of one noise image, then four of another: the tracks of the second image are born once the first's are freed."""
    a, b = frame_pixels(H, W, 71), frame_pixels(H, W, 72)
    frames = [a, a] + [np.ascontiguousarray(np.roll(b, 2 * k, axis=1)) for k in range(N - 2)]
    records = [Y.encode(f, "444", "full") for f in frames]
    return records, C.stream(records, H, W, "444", "full", tags="F25:1 Ip A1:1")


def run_stream(mgr, det, data, monkeypatch, **kw):
    from faster_rcnn_amd import annotate_video, entry, y4m
    seen, collect = [], entry.DetectionEntry.collect_batch

    def recording(self, ticket):
        res = collect(self, ticket)
        seen.extend(res)
        return res

    monkeypatch.setattr(entry.DetectionEntry, "collect_batch", recording)
    reader = y4m.Y4mReader(io.BytesIO(data), name="clip.y4m")
    sink, tracks, printed = io.BytesIO(), io.StringIO(), io.StringIO()
    writer = y4m.Y4mWriter(sink, W, H, "444", "full", reader.plan.tags)
    import contextlib
    with contextlib.redirect_stdout(printed):
        annotate_video.annotate_stream(mgr, det, reader, writer, *RESIZE, redact=REDACT, track=TRACK, tracks_out=tracks, track_motion=RADIUS, **kw)
    monkeypatch.setattr(entry.DetectionEntry, "collect_batch", collect)
    return sink.getvalue(), tracks.getvalue(), printed.getvalue(), seen


def test_a_y4m_stream_with_lookback_against_the_restatement(engine, f32_models, monkeypatch):
    mgr, det, _ = f32_models
    mapping = mgr.class_mapping
    records, data = clip_stream()
    keys0 = set(engine.cache.keys())
    plain, plain_lines, plain_printed, plain_seen = run_stream(mgr, det, data, monkeypatch)
    keys1 = set(engine.cache.keys())
    assert all("lookback" not in k for k in keys1)                           # without the option: the keys of the parent's path
    L = min(4, engine.batch)
    got, lines, printed, seen = run_stream(mgr, det, data, monkeypatch, track_lookback=L)
    tail = ("motion", RADIUS, "lookback", L)
    new = set(engine.cache.keys()) - keys1
    assert new and all(k[-4:] == tail for k in new)
    assert len(seen) == len(plain_seen) == N                                 # as many frames out as in, after the flush
    assert lines == plain_lines and lines                                    # --tracks_out: identical to the run without look-back
    assert [l for l in printed.splitlines() if l.startswith("processing")] == [l for l in plain_printed.splitlines() if l.startswith("processing")]
    srcs = [Y.decode(r, H, W, "444", "full") for r in records]
    per_frame = [split_dets(dets) for _, dets, _ in plain_seen]
    back = LB.backfill_dets(srcs, per_frame, L, RADIUS, TRACK[2])
    assert sum(len(b) for b in back) > 0 and len(back[1]) > 0                # the second image's tracks reach back into the first's frames
    want = []
    for k, (src, (live, held)) in enumerate(zip(srcs, per_frame)):
        n_rois, dets, _ = seen[k]
        assert n_rois == plain_seen[k][0]
        rest = [d for d in dets if not d.get("backfilled")]
        assert len(rest) == len(plain_seen[k][1])
        for a, b in zip(rest, plain_seen[k][1]):                             # the dets the undelayed pass reported
            assert a["bbox"].tolist() == b["bbox"].tolist() and a["cls_name"] == b["cls_name"] and a["prob"] == b["prob"]
            assert a["track_id"] == b["track_id"] and a.get("held") == b.get("held")
        filled = [d for d in dets if d.get("backfilled")]
        assert [(d["bbox"].tolist(), d["cls_name"], d["track_id"], d["backfilled"]) for d in filled] == \
            [(d["bbox"].tolist(), d["cls_name"], d["track_id"], d["backfilled"]) for d in back[k]], k
        out = R.redact_dets(src, live + held + back[k], mapping, *REDACT)
        want.append(Y.encode(T.annotate(out, live), "444", "full"))
    assert got == C.stream(want, H, W, "444", "full", tags="F25:1 Ip A1:1")
    assert got != plain                                                      # the back-filled boxes hid something
    again = run_stream(mgr, det, data, monkeypatch)
    assert again[0] == plain and again[1] == plain_lines                     # and the path without the option is what it was


def test_submit_batch_refusals_and_reset(engine, f32_models):
    from faster_rcnn_amd import shapes, util
    from faster_rcnn_amd._lib import FrcnnError
    a = frame_pixels(H, W, 71)
    imgs = [shapes.Image(shapes.Metadata("m%d" % i, W, H, [], "none"), a) for i in range(2)]
    resized, ratios = util.resize_imgs(imgs, min_size=RESIZE[0], max_size=RESIZE[1])
    pixels = [engine.host_pixels(r) for r in resized]
    captures = engine.cache.captures
    two = lambda **kw: engine.submit_batch(resized, ratios, 0.0, pixels, batch=2, annotate=True, **kw)
    with pytest.raises(FrcnnError) as e:
        two(track_lookback=2)
    assert "track=" in str(e.value)
    with pytest.raises(FrcnnError) as e:
        two(track=TRACK, track_lookback=3)                                   # L <= B
    assert "2 frames" in str(e.value)
    for bad in (0, 17, -1, True, 2.0, "2"):
        with pytest.raises(FrcnnError):
            two(track=TRACK, track_lookback=bad)
    assert engine.cache.captures == captures
    engine.track_reset()
    with pytest.raises(FrcnnError):
        engine.submit_batch([], [], 0.0, [], batch=2, annotate=True, track=TRACK, track_lookback=2)      # nothing to flush
    first = two(track=TRACK, track_lookback=2)
    assert engine.collect_batch(first) == [] and first.emitted is None
    second = two(track=TRACK, track_lookback=2)
    res = engine.collect_batch(second)
    assert len(res) == 2 and second.emitted["images"] == first.image and res[0][2].shape == a.shape
    flush = engine.submit_batch([], [], 0.0, [], batch=2, annotate=True, track=TRACK, track_lookback=2)
    assert len(engine.collect_batch(flush)) == 2
    two(track=TRACK, track_lookback=2)
    win, _ = engine.track_lookback_window(H, W, 2)
    torch.cuda.synchronize()
    assert int(win[:4].view(torch.int32)[0]) == 2
    engine.track_reset()
    torch.cuda.synchronize()
    assert not win[:32].cpu().numpy().any()
    t = two(track=TRACK, track_lookback=2)
    assert engine.collect_batch(t) == []                                     # a reset window emits nothing
    engine.track_reset()


def test_the_eager_path_and_get_annotated_frame_refuse():
    from faster_rcnn_amd import annotate_video
    with pytest.raises(ValueError, match="at once"):
        annotate_video.get_annotated_frame(None, None, None, None, 600, 1000, track=TRACK, track_lookback=2)
    with pytest.raises(ValueError, match="eager"):
        annotate_video._lookback_frames(2, TRACK, None, None)
    with pytest.raises(ValueError, match="track="):
        annotate_video._lookback_frames(2, None, object(), 4)


# ----------------------------------------------------------------------------------------------------------- annotate_images
@pytest.mark.parametrize("png_encoder", ["host", "device"])
def test_annotate_images_with_lookback_against_the_restatement(engine, f32_models, monkeypatch, tmp_path, png_encoder):
    """A directory of six PNG frames through ``annotate_images`` (passes of four: a full group and a last group of TWO, which both runs
    send through a padded pass of four -- a group under half a pass goes through one-frame passes without look-back, whose other
    kernels may round a probability differently), host and device PNG encoder: every file, under its own name, is the restatement's."""
    from PIL import Image as PilImage
    from faster_rcnn_amd import annotate_video, entry
    mgr, det, _ = f32_models
    mapping = mgr.class_mapping
    track = TRACK
    # this synthetic detector fires by position more than by content, so tracks of one noise image go on matching the next one's
    # detections; a flat frame in between loses some of them (held, hold 1) and the image behind it gives birth to new ones, which
    # reach back across the pass boundary into the first group
    a, b = frame_pixels(H, W, 71), frame_pixels(H, W, 72)
    srcs = [a, a, a, np.full((H, W, 3), 128, dtype=np.uint8), b, b]
    names = ["f_%02d.png" % (7 * k) for k in range(len(srcs))]               # (names that are not their positions)
    d_in = tmp_path / "in"
    d_in.mkdir()
    for name, rgb in zip(names, srcs):
        PilImage.fromarray(rgb).save(str(d_in / name))
    seen, collect = [], entry.DetectionEntry.collect_batch

    def recording(self, ticket):
        res = collect(self, ticket)
        seen.extend(res)
        return res

    monkeypatch.setattr(entry.DetectionEntry, "collect_batch", recording)

    def run(out, **kw):
        del seen[:]
        tracks = io.StringIO()
        _, text = quiet(annotate_video.annotate_images, mgr, det, str(d_in), str(tmp_path / out), names, *RESIZE, png_encoder=png_encoder,
                        redact=REDACT, track=track, tracks_out=tracks, track_motion=RADIUS, **kw)
        files = sorted(p.name for p in (tmp_path / out).iterdir())
        assert files == sorted(names)                                        # as many files out as in, under the right names
        return [np.asarray(PilImage.open(str(tmp_path / out / n)).convert("RGB")) for n in names], tracks.getvalue(), text, list(seen)

    plain, plain_lines, plain_text, plain_seen = run("plain")
    L = min(4, engine.batch)
    got, lines, text, got_seen = run("back", track_lookback=L)
    assert len(got_seen) == len(plain_seen) == len(srcs)
    assert lines == plain_lines and lines
    order = lambda t: [x for x in t.splitlines() if x.startswith("processing")]
    assert order(text) == order(plain_text) == ["processing " + str(d_in / n) for n in names]      # in input order
    per_frame = [split_dets(dets) for _, dets, _ in plain_seen]
    back = LB.backfill_dets(srcs, per_frame, L, RADIUS, track[2])
    assert all(len(x) > 0 for x in back[:4]) and any(held for _, held in per_frame)
    for k, (src, (live, held)) in enumerate(zip(srcs, per_frame)):
        filled = [d for d in got_seen[k][1] if d.get("backfilled")]
        assert [(d["bbox"].tolist(), d["track_id"], d["backfilled"]) for d in filled] == [(d["bbox"].tolist(), d["track_id"], d["backfilled"]) for d in back[k]]
        assert np.array_equal(plain[k], T.annotate(R.redact_dets(src, live + held, mapping, *REDACT), live)), names[k]
        assert np.array_equal(got[k], T.annotate(R.redact_dets(src, live + held + back[k], mapping, *REDACT), live)), names[k]
    # (with ~100 boxes a frame pixelated the back-filled boxes fall on hidden ground here: that they hide something is the y4m case's check)
    with pytest.raises(ValueError, match="pass of"):
        annotate_video.annotate_images(mgr, det, str(d_in), str(tmp_path / "no"), names, *RESIZE, track=track, track_lookback=engine.batch + 1)
