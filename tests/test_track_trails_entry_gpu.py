"""track_trails through the detection entry and annotate_video: submit_batch(annotate=True, track=..., track_trails=(N, W)) runs one
ops.track_trails_update behind the tracker call (behind the look-back call of a delayed pass, over the emitted buffers) and one
ops.track_trails_draw_u8 per frame between the redaction and the drawing step.  Every frame is held against the restatements applied
to the rows the same pass returned: tests/redact_ref.py over all of them, tests/track_trails_ref.py over the live ones in the order the
frames came out, then the drawing rule with ids -- byte for byte."""
import io

import numpy as np
import pytest

from tests import redact_ref as R
from tests import track_ref as T
from tests import track_trails_ref as TR
from tests.test_redact_entry_gpu import RESIZE, engine, f32_models, quiet      # noqa: F401  (the synthetic ResNet-50 pair)
from tests.test_track_cut_entry_gpu import CUT, NAMES, PCT, annotate, footage      # noqa: F401  (six PNG frames: scene A x 3, scene B x 3)
from tests.test_track_entry_gpu import split_dets
from tests.test_track_motion_entry_gpu import H, RADIUS, REDACT, TRACK, W

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TRAILS = (3, 2)                          # N = 3: the six frames overrun the ring


def live_buffer(live, mapping):
    """The live rows of a frame's returned dets as a tracked buffer (the rows the trail rule reads)."""
    rows = max(len(live), 1)
    b = np.zeros(4 + 8 * rows, dtype=np.int32)
    b[0] = b[1] = len(live)
    for r, d in enumerate(live):
        b[4 + 4 * r:8 + 4 * r] = [int(v) for v in d["bbox"]]
        b[4 + 4 * rows + r] = mapping[d["cls_name"]]
        b[4 + 6 * rows + r] = d.get("track_id", 0)
    return b


def check_frames(engine, srcs, results, mapping, every=1, trails=TRAILS):
    """Every returned frame == redaction, then trails, then boxes, from the frame's own returned rows -> the frames' point lists."""
    n, width = trails
    ref = TR.Trails(H, W, engine.track_trails_capacity(), n, (TRACK[1] + 1) * every)
    lists = []
    for f, (src, res) in enumerate(zip(srcs, results)):
        dets, out = res[1], res[2]
        filled = [d for d in dets if d.get("backfilled")]
        live, held = split_dets([d for d in dets if not d.get("backfilled")])
        plist = ref.frame(live_buffer(live, mapping))
        want = R.redact_dets(src, live + held + filled, mapping, *REDACT)
        want = T.annotate(TR.draw(want, plist, n, width, 1), live)          # (file-backed frames are uploaded R, G, B)
        assert np.array_equal(out, want), (f, np.argwhere(out != want)[:4])
        lists.append(dict(TR.trails_of(plist, n)))
    assert np.array_equal(engine.track_trails_state(n).cpu().numpy(), ref.words()) and ref.dropped == 0
    return lists


def files_match(files, results):
    from PIL import Image as PilImage
    for name, res in zip(NAMES, results):
        assert np.array_equal(np.asarray(PilImage.open(io.BytesIO(files[name])).convert("RGB")), res[2]), name


@pytest.mark.parametrize("every", [1, 2])
def test_frames_are_redaction_then_trails_then_boxes(engine, f32_models, footage, monkeypatch, tmp_path, every):
    """Plain (with track_motion): a pass of frames 0-3 and a padded one of 4-5.  detect_every 2: one pass of six frames, whose between
    frames extend the trails with their propagated rows."""
    mapping = f32_models[0].class_mapping
    kw = {} if every == 1 else {"detect_every": every}
    results, text, lines, files = annotate(f32_models, footage, tmp_path / "out", monkeypatch, track_trails=TRAILS, **kw)
    assert len(results) == 6 and all(len(r) == 3 for r in results)
    lists = check_frames(engine, footage[1], results, mapping, every)
    files_match(files, results)
    # trails grow from frame to frame, the ring is overrun, and the lines are visible
    assert any(len(p) == 1 for p in lists[0].values()) and any(len(p) == 3 for p in lists[5].values())
    assert any(len(set(p)) > 1 for l in lists for p in l.values())
    if every == 2:                                                          # a between frame's rows are points too
        assert any(len(p) >= 2 for p in lists[1].values())
    plain = annotate(f32_models, footage, tmp_path / "plain", monkeypatch, **kw)
    assert plain[1:3] == (text, lines) and any(files[n] != plain[3][n] for n in NAMES)
    tail = ("motion", RADIUS) + (("every", every) if every > 1 else ()) + ("trails",) + TRAILS
    assert any(k[-len(tail):] == tail for k in engine.cache.keys())


def test_no_trail_crosses_a_scene_cut(engine, f32_models, footage, monkeypatch, tmp_path):
    from faster_rcnn_amd import ops
    mapping = f32_models[0].class_mapping
    results, _, _, files = annotate(f32_models, footage, tmp_path / "out", monkeypatch, track_trails=TRAILS, track_scene_cut=PCT)
    assert [r[3] for r in results] == [{"scene_cut": True} if f == CUT else {} for f in range(6)]
    lists = check_frames(engine, footage[1], results, mapping)
    files_match(files, results)
    assert engine.track_trails_capacity() == 2 * ops.track_capacity(engine.track_state())      # (the old scene's trails wait for their expiry)
    assert lists[CUT] and all(len(p) == 1 for p in lists[CUT].values()) and any(len(p) > 1 for p in lists[CUT - 1].values())
    assert not set(lists[CUT]) & set().union(*lists[:CUT])
    assert any(k[-5:] == ("cut", PCT, "trails") + TRAILS for k in engine.cache.keys())


def test_a_delayed_pass_draws_in_emitted_order(engine, f32_models, footage, monkeypatch, tmp_path):
    """track_lookback: the pass of frames 4-5 returns frames 0-3 and the flush the rest; the trail call reads the emitted buffers."""
    mapping = f32_models[0].class_mapping
    results, text, _, files = annotate(f32_models, footage, tmp_path / "out", monkeypatch, track_trails=TRAILS, track_lookback=2)
    assert len(results) == 6
    assert [x for x in text.splitlines() if x.startswith("processing")] == ["processing " + str(footage[0] / n) for n in NAMES]
    lists = check_frames(engine, footage[1], results, mapping)
    files_match(files, results)
    assert any(len(p) == 3 for p in lists[5].values())
    assert any(k[-5:] == ("lookback", 2, "trails") + TRAILS for k in engine.cache.keys())


def mot_trails(lines, frames, capacity):
    """The trail state the MOT lines of a run imply: a frame's lines are its live tracked rows, in row order."""
    ref = TR.Trails(H, W, capacity, TRAILS[0], TRACK[1] + 1)
    rows = [[int(float(v)) for v in x.split(",")[:6]] + [int(x.split(",")[7])] for x in lines.splitlines()]
    for f in range(1, frames + 1):
        live = [r for r in rows if r[0] == f]
        b = np.zeros(4 + 8 * max(len(live), 1), dtype=np.int32)
        b[0] = b[1] = len(live)
        for r, (_, tid, left, top, w, h, cls) in enumerate(live):
            b[4 + 4 * r:8 + 4 * r] = (left, top, left + w, top + h)
            b[4 + 4 * max(len(live), 1) + r], b[4 + 6 * max(len(live), 1) + r] = cls, tid
        ref.frame(b)
    return ref


@pytest.mark.parametrize("fast", [True, False])
def test_get_annotated_frame_frame_by_frame(engine, f32_models, footage, monkeypatch, tmp_path, fast):
    """The one-frame paths over the same six frames: the captured one gives the batched run's frames, and on both the trail state is the
    one the run's own MOT lines imply."""
    from faster_rcnn_amd import annotate_video, entry, ops, shapes, voc_dets
    mgr, det, _ = f32_models
    results, _, want_lines, _ = annotate(f32_models, footage, tmp_path / "out", monkeypatch, track_trails=TRAILS)
    tracks, outs = io.StringIO(), []
    voc_dets.FAST_ENTRY = fast
    try:
        annotate_video.reset_tracks(mgr, det, 1)
        for k, src in enumerate(footage[1]):
            frame = np.ascontiguousarray(src[:, :, ::-1])                    # (the file's R,G,B as the one-frame path takes it: B,G,R)
            img = shapes.InMemoryImage(data=frame, width=W, height=H)
            quiet(annotate_video.get_annotated_frame, mgr, det, frame, img, *RESIZE, redact=REDACT, track=TRACK, tracks_out=tracks,
                  frame_no=k + 1, track_motion=RADIUS, track_trails=TRAILS)
            outs.append(frame)
    finally:
        voc_dets.FAST_ENTRY = True
    torch.cuda.synchronize()
    if fast:
        state, cap = engine.track_trails_state(TRAILS[0]), engine.track_trails_capacity()
        rows = lambda text: [x.split(",")[:6] + x.split(",")[7:] for x in text.splitlines()]
        assert rows(tracks.getvalue()) == rows(want_lines)
        for k, (out, res) in enumerate(zip(outs, results)):
            assert np.array_equal(out[:, :, ::-1], res[2]), k
    else:
        state, cap = annotate_video._eager_trails_state(mgr.class_mapping, TRAILS[0]), min(2 * entry.TRACK_CAPACITY, ops.TRACK_MAX)
        assert any((out != src[:, :, ::-1]).any() for out, src in zip(outs, footage[1]))
    ref = mot_trails(tracks.getvalue(), 6, cap)
    assert ref.entries and any(len(e["pts"]) == 3 for e in ref.entries)
    assert np.array_equal(state.cpu().numpy(), ref.words())


def test_track_reset_starts_trails_afresh(engine, f32_models, footage, monkeypatch, tmp_path):
    first = annotate(f32_models, footage, tmp_path / "a", monkeypatch, track_trails=TRAILS)
    state = engine.track_trails_state(TRAILS[0])
    torch.cuda.synchronize()
    assert state.cpu().numpy().any()
    engine.track_reset()
    torch.cuda.synchronize()
    assert not state.cpu().numpy().any() and engine.track_trails_state(TRAILS[0]) is state
    again = annotate(f32_models, footage, tmp_path / "b", monkeypatch, track_trails=TRAILS)      # (a run resets the tracks itself)
    assert again[1:] == first[1:]


def test_without_the_option_nothing_changes(engine, f32_models, footage, monkeypatch, tmp_path):
    """The run without the option before and after a run with it: the same files, lines and MOT text, and no cache key but the new
    passes' own carries the tag; a spec built without the field has the key the parent's had."""
    from faster_rcnn_amd import entry
    before = annotate(f32_models, footage, tmp_path / "a", monkeypatch)
    keys = set(engine.cache.keys())
    with_trails = annotate(f32_models, footage, tmp_path / "b", monkeypatch, track_trails=TRAILS)
    after = annotate(f32_models, footage, tmp_path / "c", monkeypatch)
    now = set(engine.cache.keys())
    tagged = {k for k in now if "trails" in k}
    assert tagged and now - tagged == keys - tagged
    assert before[1:] == after[1:] and with_trails[1:3] == before[1:3] and with_trails[3] != before[3]
    spec = entry.PassSpec.checked(engine, 4, annotate=True, redact=REDACT, track=TRACK, track_motion=RADIUS)
    assert spec.track_trails is None and any(k[-len(spec.key_tail(4)):] == spec.key_tail(4) for k in keys)
    assert all(k[-3:] == ("trails",) + TRAILS for k in tagged)               # the tag goes behind everything else


def test_submit_batch_refusals(engine, f32_models, footage):
    from faster_rcnn_amd import shapes, util
    from faster_rcnn_amd._lib import FrcnnError
    imgs = [shapes.Image(shapes.Metadata("t%d" % i, W, H, [], "none"), s) for i, s in enumerate(footage[1][:2])]
    resized, ratios = util.resize_imgs(imgs, min_size=RESIZE[0], max_size=RESIZE[1])
    pixels = [engine.host_pixels(r) for r in resized]
    captures = engine.cache.captures
    two = lambda **kw: engine.submit_batch(resized, ratios, 0.0, pixels, batch=2, annotate=True, **kw)
    with pytest.raises(FrcnnError, match=r"track_trails= draws the paths of the tracker's ids: pass track="):
        two(track_trails=TRAILS)
    with pytest.raises(FrcnnError, match=r"track_trails= together with draw=False is not supported"):
        two(track=TRACK, redact=REDACT, draw=False, track_trails=TRAILS)
    for bad in (1, 65, (3, 0), (3, 10), True, 3.0, "3", (3,), (3, 2, 1)):
        with pytest.raises(FrcnnError, match="track_trails="):
            two(track=TRACK, track_trails=bad)
    assert engine.cache.captures == captures
