"""The back-track rule through the detection entry and annotate_video: submit_batch(annotate=True, track=..., track_motion=R,
detect_every=K, track_backtrack=L) runs ops.track_backtrack behind ops.track_update_interval inside the captured pass and returns the
frames of the pass before.  The emitted rows are held against the two ops composed by hand on the packed detections the passes read back,
the written pixels against tests/redact_ref.py over every emitted row and the drawing rule with ids -- byte for byte."""
import io

import numpy as np
import pytest

from tests import redact_ref as R
from tests import track_motion_ref as M
from tests import track_ref as T
from tests.test_redact_entry_gpu import RESIZE, engine, f32_models, frame_pixels, quiet      # noqa: F401  (the synthetic ResNet-50 pair)
from tests.test_track_entry_gpu import same_det
from tests.test_track_interval_entry_gpu import clip, submit_every      # noqa: F401
from tests.test_track_motion_entry_gpu import H, RADIUS, REDACT, SHIFT, TRACK, W

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

B, K, L = 2, 2, 3                        # passes of F = 4 source frames
F = B * K
OPTS = dict(redact=REDACT, track=TRACK, track_motion=RADIUS, detect_every=K, track_backtrack=L)
TAIL = ("track",) + TRACK + ("motion", RADIUS, "every", K, "backtrack", L)


def submit_back(engine, clip, frames, **kw):
    return submit_every(engine, clip, frames, **dict(dict(track_backtrack=L), **kw))


def flush(engine, **kw):
    return engine.submit_batch([], [], 0.0, [], batch=B, annotate=True, **dict(OPTS, **kw))


def rows_of(dets, mapping):
    """The dets of a result as rows: (bbox, class index, id, "live" / "propagated" / ("held", age) / ("backfilled", k))."""
    kind = lambda d: ("held", d["held"]) if "held" in d else ("backfilled", d["backfilled"]) if "backfilled" in d else \
        "propagated" if d.get("propagated") else "live"
    return [(d["bbox"].tolist(), mapping[d["cls_name"]], d["track_id"], kind(d)) for d in dets]


def rows_of_buffer(buf, between):
    n_rows, n_live, _, _, bbox, cls, _, ids, age = T.split(buf)
    kind = lambda r: ("propagated" if between else "live") if r < n_live else ("held", int(age[r])) if age[r] > 0 else ("backfilled", -int(age[r]))
    return [(bbox[r].tolist(), int(cls[r]), int(ids[r]), kind(r)) for r in range(n_rows)]


def run_clip(engine, clip):
    """The clip's eight frames in two passes and a flush -> (the eight results, the packed detections of the two passes)."""
    engine.track_reset()
    results, packed = [], []
    for part in ([0, 1, 2, 3], [4, 5, 6, 7]):
        ticket = submit_back(engine, clip, part)
        results += engine.collect_batch(ticket)
        packed.append(ticket.slot.out_pin[:B].numpy().copy())
    assert results[F:] == [] and len(results) == F                           # one pass late
    results += engine.collect_batch(flush(engine))
    return results, packed


def test_a_clip_equals_the_two_ops_composed_by_hand(engine, clip, f32_models):
    from faster_rcnn_amd import ops
    mapping = f32_models[0].class_mapping
    srcs = clip[0]
    results, packed = run_clip(engine, clip)
    assert len(results) == 8 and any(k[-len(TAIL):] == TAIL for k in engine.cache.keys())
    cap = ops.track_capacity(engine.track_state())
    rows = (packed[0].shape[1] - 4) // 7
    back = engine.track_lookback_window(H, W, F)[1]
    state, mstate, table = ops.track_state(cap), ops.track_motion_state(H, W), engine.track_table(REDACT[0])
    window = ops.track_lookback_state(F, H, W, rows, cap, back)
    nf = torch.zeros(1, dtype=torch.int32, device="cuda")
    emitted = []
    for p in range(3):
        at = min(p, 1) * F
        frames = torch.from_numpy(np.stack(srcs[at:at + F])).cuda()
        nf.fill_(F if p < 2 else -1)
        tracked = ops.track_update_interval(state, mstate, frames, 3 * H * W, torch.from_numpy(packed[min(p, 1)]).cuda(), nf, table, H, W, *TRACK,
                                            RADIUS, K)
        _, out_t, count = ops.track_backtrack(window, frames, 3 * H * W, tracked, nf, cap, back, H, W, L, RADIUS, TRACK[2], K)
        emitted += list(out_t[:int(count[0])].cpu().numpy())
    assert len(emitted) == 8
    filled = 0
    for f, ((n_rois, dets, out), buf, src) in enumerate(zip(results, emitted, srcs)):
        assert rows_of(dets, mapping) == rows_of_buffer(buf, f % K), f
        assert (n_rois > 0) == (f % K == 0) and (f % K == 0 or n_rois == 0)
        live = [d for d in dets if "held" not in d and "backfilled" not in d]
        assert np.array_equal(out, T.annotate(R.redact_dets(src, dets, mapping, *REDACT), live)), f      # back-filled rows hidden, never drawn
        filled += sum("backfilled" in d for d in dets)
    # every between frame in front of a key frame carries a row tracked back from it for every track that key frame sees
    for f in (1, 3, 5):
        ids = {d["track_id"] for d in results[f + 1][1] if d["track_id"] > 0 and "held" not in d and "backfilled" not in d}
        assert ids and ids <= {d["track_id"] for d in results[f][1] if d.get("backfilled") == 1}
    assert filled > 0 and not any("backfilled" in d for d in results[7][1])


def test_passes_without_the_option_are_what_they_were(engine, clip):
    engine.track_reset()
    before = engine.collect_batch(submit_every(engine, clip, [0, 1, 2, 3]))
    captures, keys = engine.cache.captures, set(engine.cache.keys())
    run_clip(engine, clip)
    engine.track_reset()
    mid = engine.cache.captures
    after = engine.collect_batch(submit_every(engine, clip, [0, 1, 2, 3]))
    assert engine.cache.captures == mid                                      # the old key, hit
    new = set(engine.cache.keys()) - keys
    assert all(k[-len(TAIL):] == TAIL and k[0] != "canvas" for k in new) and mid - captures == len(new) <= 1
    assert len(before) == len(after) == 4
    for (n_a, dets_a, out_a), (n_b, dets_b, out_b) in zip(before, after):
        assert n_a == n_b and len(dets_a) == len(dets_b) and all(same_det(a, b) for a, b in zip(dets_a, dets_b))
        assert np.array_equal(out_a, out_b)


def test_submit_batch_refusals(engine, clip, f32_models):
    from faster_rcnn_amd import entry, resnet
    from faster_rcnn_amd._lib import FrcnnError
    from faster_rcnn_amd.det_util import DetTrainingManager
    engine.track_reset()
    captures = engine.cache.captures
    srcs, resized, ratios, pixels = clip
    with pytest.raises(FrcnnError, match="track_backtrack= follows the tracks .* pass detect_every=K"):
        engine.submit_batch(resized[:2], ratios[:2], 0.0, pixels[:2], batch=B, annotate=True, redact=REDACT, track=TRACK, track_motion=RADIUS,
                            track_backtrack=L)
    with pytest.raises(FrcnnError, match="track_backtrack= together with track_lookback= is not supported"):
        submit_back(engine, clip, [0, 1, 2, 3], track_lookback=2)
    with pytest.raises(FrcnnError, match="detect_every= together with track_lookback= is not supported"):      # (pinned: as it was)
        submit_every(engine, clip, [0, 1, 2, 3], track_lookback=2)
    for bad in (0, 17, -1, False, 2.0, "2"):
        with pytest.raises(FrcnnError, match="track_backtrack=.*an integer in 1..16"):
            submit_back(engine, clip, [0, 1, 2, 3], track_backtrack=bad)
    with pytest.raises(FrcnnError, match="a frame would be emitted before its rows are in place"):
        submit_back(engine, clip, [0, 1, 2, 3], track_backtrack=F + 1)
    with pytest.raises(FrcnnError, match="frames no detection reaches would stay uncovered"):
        submit_every(engine, clip, [0, 1, 2, 3, 4, 5, 6, 7], every=4, track_backtrack=2)
    with pytest.raises(FrcnnError, match="a flush"):
        flush(engine)                                                        # nothing to flush
    assert engine.cache.captures == captures
    mgr, det, _ = f32_models
    mgr2 = DetTrainingManager(rpn_model=mgr.rpn_model, class_mapping=mgr.class_mapping, preprocess_func=lambda d: resnet.preprocess(d),
                              anchor_dims=mgr.anchor_dims)
    foreign = entry.for_models(mgr2, det, 64, 16, 1)
    assert foreign is not None and not foreign.device_preprocess
    with pytest.raises(FrcnnError, match="detect_every= needs the device-side preprocess"):
        foreign.submit_batch([resized[0], resized[2]], [ratios[0], ratios[2]], 0.0, [foreign.host_pixels(r) for r in resized[:4]], batch=B,
                             annotate=True, **OPTS)
    assert foreign.cache.captures == 0


def test_annotate_images_writes_the_same_files_one_pass_late(engine, clip, f32_models, monkeypatch, tmp_path):
    """A directory of seven PNG frames with detect_every 2 and the value a bare ``--track_backtrack`` gives: a full pass of B * K frames, a
    padded one of the rest and a flush.  The files are those submit_batch's results stand for, under their own names, in input order."""
    from PIL import Image as PilImage
    from faster_rcnn_amd import annotate_video, entry
    mgr, det, _ = f32_models
    mapping = mgr.class_mapping
    per_pass = engine.batch * K
    n = per_pass + 3
    a = frame_pixels(H, W, 71)
    srcs = [np.ascontiguousarray(M.shifted(a, k * SHIFT[0], k * SHIFT[1])) for k in range(n)]
    names = ["f_%02d.png" % (7 * k) for k in range(n)]
    d_in, d_out = tmp_path / "in", tmp_path / "out"
    d_in.mkdir()
    for name, rgb in zip(names, srcs):
        PilImage.fromarray(rgb).save(str(d_in / name))
    seen, sizes, collect = [], [], entry.DetectionEntry.collect_batch

    def recording(self, ticket):
        res = collect(self, ticket)
        sizes.append((ticket.frames, len(res), sorted(p.name for p in d_out.iterdir()) if d_out.exists() else []))
        seen.extend(res)
        return res

    monkeypatch.setattr(entry.DetectionEntry, "collect_batch", recording)
    args = annotate_video.build_parser().parse_args(["a.h5", "b.h5", "frames", "--track", "--track_motion", str(RADIUS), "--detect_every", str(K),
                                                     "--track_backtrack"])
    option = annotate_video.track_backtrack_from_args(args)
    tracks = io.StringIO()
    _, text = quiet(annotate_video.annotate_images, mgr, det, str(d_in), str(d_out), names, *RESIZE, png_encoder="host", redact=REDACT,
                    track=TRACK, tracks_out=tracks, track_motion=RADIUS, detect_every=K, track_backtrack=option)
    assert [(a, b) for a, b, _ in sizes] == [(per_pass, 0), (3, per_pass), (0, 3)]       # every pass returns the one before; the flush the last
    assert sizes[1][2] == []                                                 # nothing was written before the second pass came back
    assert sorted(p.name for p in d_out.iterdir()) == sorted(names) and len(seen) == n
    assert [x for x in text.splitlines() if x.startswith("processing")] == ["processing " + str(d_in / x) for x in names]
    tail = ("every", K, "backtrack", min(16, per_pass))
    assert any(k[-4:] == tail for k in engine.cache.keys())
    want_lines = []
    for k, (src, (_, dets, _)) in enumerate(zip(srcs, seen)):
        live = [d for d in dets if "held" not in d and "backfilled" not in d]
        want_lines += T.mot_lines(k + 1, live, mapping)
        got = np.asarray(PilImage.open(str(d_out / names[k])).convert("RGB"))
        assert np.array_equal(got, T.annotate(R.redact_dets(src, dets, mapping, *REDACT), live)), names[k]
    assert tracks.getvalue() == "".join(x + "\n" for x in want_lines)
    assert sum("backfilled" in d for _, dets, _ in seen for d in dets) > 0
    with pytest.raises(ValueError, match="a frame would be emitted before its rows are in place"):
        annotate_video.annotate_images(mgr, det, str(d_in), str(tmp_path / "no"), names, *RESIZE, track=TRACK, track_motion=RADIUS,
                                       detect_every=2, track_backtrack=2 * engine.batch + 1)
    with pytest.raises(ValueError, match="it needs .*detect_every=K"):
        annotate_video.annotate_images(mgr, det, str(d_in), str(tmp_path / "no"), names, *RESIZE, track=TRACK, track_motion=RADIUS,
                                       track_backtrack=2)
