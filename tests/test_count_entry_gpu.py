"""count through the detection entry and annotate_video: submit_batch(annotate=True, track=..., count=(lines, classes, W)) runs one
ops.count_update behind the tracker call (behind the look-back / back-track call of a delayed pass, over the emitted buffers) and one
ops.count_draw_u8 per frame over the redaction, heat and trails and under the boxes.  Every frame and every list of crossings is held
against tests/count_ref.py applied to the rows the same pass returned, in the order the frames came out -- byte for byte."""
import numpy as np
import pytest

from tests import count_ref as CR
from tests import redact_ref as R
from tests import track_ref as T
from tests.test_redact_entry_gpu import RESIZE, engine, f32_models, quiet      # noqa: F401  (the synthetic ResNet-50 pair)
from tests.test_track_cut_entry_gpu import CUT, NAMES, PCT, annotate, footage      # noqa: F401  (six PNG frames: scene A x 3, scene B x 3)
from tests.test_track_entry_gpu import split_dets
from tests.test_track_motion_entry_gpu import H, RADIUS, REDACT, TRACK, W
from tests.test_track_trails_entry_gpu import files_match, live_buffer

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# a grid over the 200 x 330 frames (the scenes move by (3, 2) a frame), one line beyond the frame, one clipped by it
LINES = ((0, 50, 329, 50), (0, 100, 329, 100), (0, 150, 329, 150), (80, 0, 80, 199), (165, 199, 165, 0), (250, 0, 250, 199), (-40, -20, 400, 260),
         (400, 0, 400, 199))
COUNT = (LINES, "all", 2)


def check_frames(engine, srcs, results, mapping, every=1, count=COUNT, drawn=True, reference=None):
    """Every returned frame == redaction, then lines and labels, then boxes, and every frame's crossings == the rule's, from the frame's
    own returned rows -> the reference counter."""
    lines, classes, width = count
    table = np.ones(max(mapping.values()) + 1, dtype=np.uint8)
    ref = reference or CR.Counter(H, W, lines, table, engine.track_trails_capacity(), (TRACK[1] + 1) * every)
    for f, (src, res) in enumerate(zip(srcs, results)):
        dets, out, marks = res[1], res[2], res[-1]
        filled = [d for d in dets if d.get("backfilled")]
        live, held = split_dets([d for d in dets if not d.get("backfilled")])
        clist = ref.frame(live_buffer(live, mapping))
        assert marks["crossings"] == CR.events_of(clist), f
        want = R.redact_dets(src, live + held + filled, mapping, *REDACT)
        want = T.annotate(CR.draw(want, clist, lines, width, 1) if drawn else want, live) if drawn else want
        assert np.array_equal(out, want), (f, np.argwhere(out != want)[:4])
    return ref


def state_matches(engine, ref):
    torch.cuda.synchronize()
    assert np.array_equal(engine.count_state().cpu().numpy(), ref.words())


@pytest.mark.parametrize("every", [1, 2])
def test_crossings_and_frames_match_the_rule(engine, f32_models, footage, monkeypatch, tmp_path, every):
    """Plain (with track_motion): a pass of frames 0-3 and a short, padded one of 4-5 continuing one state.  detect_every 2: one pass of
    six frames."""
    mapping = f32_models[0].class_mapping
    kw = {} if every == 1 else {"detect_every": every}
    counts = tmp_path / "counts.csv"
    results, text, lines, files = annotate(f32_models, footage, tmp_path / "out", monkeypatch, count=COUNT, counts_out=str(counts), **kw)
    assert len(results) == 6 and all(len(r) == 4 and set(r[3]) == {"crossings"} for r in results)
    ref = check_frames(engine, footage[1], results, mapping, every)
    state_matches(engine, ref)
    files_match(files, results)
    total = sum(map(sum, ref.totals))
    assert total > 0 and ref.dropped == 0
    # the CSV and the printed totals
    names = {v: k for k, v in mapping.items()}
    rows = ["%d,%d,%s,%d,%s" % (f + 1, l, "+" if d else "-", i, names[c]) for f, r in enumerate(results) for l, d, i, c in r[3]["crossings"]]
    assert counts.read_text().splitlines() == ["frame,line,direction,id,cls"] + rows and len(rows) == total
    printed = [x for x in text.splitlines() if x.startswith("line ")]
    assert printed == ["line %d: +%d -%d" % (l, ref.totals[l][1], ref.totals[l][0]) for l in range(8)]
    assert sum(int(x.split("+")[1].split()[0]) + int(x.split("-")[1]) for x in text.splitlines() if x.startswith("crossings of ")) == total
    plain = annotate(f32_models, footage, tmp_path / "plain", monkeypatch, **kw)
    assert plain[2] == lines and any(files[n] != plain[3][n] for n in NAMES)
    assert [x for x in text.splitlines() if not x.startswith(("line ", "crossings of "))] == plain[1].splitlines()
    tail = ("motion", RADIUS) + (("every", every) if every > 1 else ()) + ("count",) + COUNT
    assert any(k[-len(tail):] == tail for k in engine.cache.keys())


def test_with_scene_cut_trails_and_heat_one_dict_carries_both_marks(engine, f32_models, footage, monkeypatch, tmp_path):
    from tests import heat_ref, track_trails_ref as TR
    mapping = f32_models[0].class_mapping
    results, _, _, files = annotate(f32_models, footage, tmp_path / "out", monkeypatch, count=COUNT, track_scene_cut=PCT, track_trails=(3, 2),
                                    heatmap=("all", 160, 0))
    assert [set(r[3]) for r in results] == [{"crossings", "scene_cut"} if f == CUT else {"crossings"} for f in range(6)] and all(len(r) == 4 for r in results)
    # the crossings are the rule's over the returned rows; the ids end at the cut, so no step crosses it
    table = np.ones(max(mapping.values()) + 1, dtype=np.uint8)
    ref = CR.Counter(H, W, LINES, table, engine.track_trails_capacity(), TRACK[1] + 1)
    trails, heat = TR.Trails(H, W, engine.track_trails_capacity(), 3, TRACK[1] + 1), heat_ref.Heat(H, W)
    for f, (src, res) in enumerate(zip(footage[1], results)):
        live, held = split_dets(res[1])
        buf = live_buffer(live, mapping)
        clist, plist = ref.frame(buf), trails.frame(buf)
        assert res[3]["crossings"] == CR.events_of(clist), f
        want = R.redact_dets(src, live + held, mapping, *REDACT)
        heat.update(buf, table, 0, tracked=True)
        want = T.annotate(CR.draw(TR.draw(heat.draw(want, 160, 1), plist, 3, 2, 1), clist, LINES, 2, 1), live)
        assert np.array_equal(res[2], want), (f, np.argwhere(res[2] != want)[:4])
    state_matches(engine, ref)
    assert not results[CUT][3]["crossings"]
    assert any(k[-4:] == ("count",) + COUNT for k in engine.cache.keys())


@pytest.mark.parametrize("delayed", ["track_lookback", "track_backtrack"])
def test_a_delayed_pass_counts_in_emitted_order(engine, f32_models, footage, monkeypatch, tmp_path, delayed):
    """The crossings arrive with the emitted frames and sum to the undelayed run's totals."""
    mapping = f32_models[0].class_mapping
    kw = {"track_lookback": 2} if delayed == "track_lookback" else {"detect_every": 2, "track_backtrack": 2}
    every = kw.get("detect_every", 1)
    results, text, _, files = annotate(f32_models, footage, tmp_path / "out", monkeypatch, count=COUNT, **kw)
    assert len(results) == 6 and all(set(r[-1]) == {"crossings"} for r in results)
    ref = check_frames(engine, footage[1], results, mapping, every)
    state_matches(engine, ref)
    files_match(files, results)
    undelayed, _, _, _ = annotate(f32_models, footage, tmp_path / "plain", monkeypatch, count=COUNT, **({"detect_every": 2} if every == 2 else {}))
    plain = check_frames(engine, footage[1], undelayed, mapping, every)
    assert ref.totals == plain.totals and sum(map(sum, ref.totals)) > 0


def test_no_draw_counts_and_draws_no_line(engine, f32_models, footage, monkeypatch, tmp_path):
    mapping = f32_models[0].class_mapping
    results, _, _, _ = annotate(f32_models, footage, tmp_path / "out", monkeypatch, count=COUNT, draw=False)
    ref = check_frames(engine, footage[1], results, mapping, drawn=False)
    state_matches(engine, ref)
    assert sum(map(sum, ref.totals)) > 0
    bare, _, _, _ = annotate(f32_models, footage, tmp_path / "bare", monkeypatch, draw=False)
    assert all(np.array_equal(a[2], b[2]) for a, b in zip(results, bare))


def test_count_reset_and_track_reset(engine, f32_models, footage, monkeypatch, tmp_path):
    from faster_rcnn_amd import ops
    first = annotate(f32_models, footage, tmp_path / "a", monkeypatch, count=COUNT)
    state = engine.count_state()
    torch.cuda.synchronize()
    before = ops.count_totals(state)
    assert before["entries"] > 0 and sum(map(sum, before["totals"])) > 0
    engine.track_reset()                                                     # the ids end, what was counted stays counted
    torch.cuda.synchronize()
    after = ops.count_totals(state)
    assert after["entries"] == 0 and after["totals"] == before["totals"] and after["frames"] == before["frames"]
    assert not state[ops.COUNT_HEAD:].cpu().numpy().any()
    engine.count_reset()
    torch.cuda.synchronize()
    assert not state.cpu().numpy().any() and engine.count_state() is state
    again = annotate(f32_models, footage, tmp_path / "b", monkeypatch, count=COUNT)          # (a run starts from zero totals itself)
    assert again[1:] == first[1:] and [r[3] for r in again[0]] == [r[3] for r in first[0]]


def test_without_the_option_nothing_changes(engine, f32_models, footage, monkeypatch, tmp_path):
    """The run without the option before and after a run with it: the same files, lines and MOT text, and no cache key but the new
    passes' own carries the tag; a spec built without the field has the key the parent's had."""
    from faster_rcnn_amd import entry
    before = annotate(f32_models, footage, tmp_path / "a", monkeypatch)
    keys = set(engine.cache.keys())
    with_count = annotate(f32_models, footage, tmp_path / "b", monkeypatch, count=COUNT)
    after = annotate(f32_models, footage, tmp_path / "c", monkeypatch)
    now = set(engine.cache.keys())
    tagged = {k for k in now if "count" in k}
    assert tagged and now - tagged == keys - tagged
    assert before[1:] == after[1:] and with_count[2] == before[2] and with_count[3] != before[3]
    assert all(len(r) == 3 for r in before[0]) and all(len(r) == 3 for r in after[0])
    spec = entry.PassSpec.checked(engine, 4, annotate=True, redact=REDACT, track=TRACK, track_motion=RADIUS)
    assert spec.count is None and any(k[-len(spec.key_tail(4)):] == spec.key_tail(4) for k in keys)
    assert all(k[-4:] == ("count",) + COUNT for k in tagged)                 # the tag goes behind everything else


def test_submit_batch_refusals(engine, f32_models, footage):
    from faster_rcnn_amd import shapes, util
    from faster_rcnn_amd._lib import FrcnnError
    imgs = [shapes.Image(shapes.Metadata("t%d" % i, W, H, [], "none"), s) for i, s in enumerate(footage[1][:2])]
    resized, ratios = util.resize_imgs(imgs, min_size=RESIZE[0], max_size=RESIZE[1])
    pixels = [engine.host_pixels(r) for r in resized]
    captures = engine.cache.captures
    two = lambda **kw: engine.submit_batch(resized, ratios, 0.0, pixels, batch=2, annotate=True, **kw)
    with pytest.raises(FrcnnError, match=r"count= counts the tracker's ids as they cross a line: pass track="):
        two(count=COUNT)
    for bad in ((((1, 1, 1, 1),), "all", 2), (LINES + LINES[:1], "all", 2), (LINES, "tram", 2), (LINES, "all", 0), LINES, (((0, 0, 70000, 1),), "all", 2)):
        with pytest.raises(FrcnnError, match="count="):
            two(track=TRACK, count=bad)
    assert engine.cache.captures == captures


def mot_counts(lines, frames, capacity, mapping):
    """The counter and the CSV rows the MOT lines of a run imply: a frame's lines are its live tracked rows, in row order."""
    names = {v: k for k, v in mapping.items()}
    ref = CR.Counter(H, W, LINES, np.ones(max(mapping.values()) + 1, dtype=np.uint8), capacity, TRACK[1] + 1)
    rows = [[int(float(v)) for v in x.split(",")[:6]] + [int(x.split(",")[7])] for x in lines.splitlines()]
    csv = []
    for f in range(1, frames + 1):
        live = [(tid, cls, (left, top, left + w, top + h)) for n, tid, left, top, w, h, cls in rows if n == f]
        clist = ref.frame(CR.make_tracked(live, max(len(live), 1)))
        csv += ["%d,%d,%s,%d,%s" % (f, l, "+" if d else "-", i, names[c]) for l, d, i, c in CR.events_of(clist)]
    return ref, csv


@pytest.mark.parametrize("fast", [True, False])
def test_get_annotated_frame_frame_by_frame(engine, f32_models, footage, monkeypatch, tmp_path, fast):
    """The one-frame paths over the same six frames continue one state: the captured one gives the batched run's frames and crossings, and
    on both the count state and the CSV rows are the ones the run's own MOT lines imply; reset_counts zeroes it, reset_tracks keeps the
    totals."""
    import io
    from faster_rcnn_amd import annotate_video, entry, ops, shapes, voc_dets
    mgr, det, _ = f32_models
    results, _, want_lines, _ = annotate(f32_models, footage, tmp_path / "out", monkeypatch, count=COUNT)
    tracks, counts, outs = io.StringIO(), io.StringIO(), []
    voc_dets.FAST_ENTRY = fast
    try:
        annotate_video.reset_tracks(mgr, det, 1)
        annotate_video.reset_counts(mgr, det, 1)
        for k, src in enumerate(footage[1]):
            frame = np.ascontiguousarray(src[:, :, ::-1])                    # (the file's R,G,B as the one-frame path takes it: B,G,R)
            img = shapes.InMemoryImage(data=frame, width=W, height=H)
            quiet(annotate_video.get_annotated_frame, mgr, det, frame, img, *RESIZE, redact=REDACT, track=TRACK, tracks_out=tracks,
                  frame_no=k + 1, track_motion=RADIUS, count=COUNT, counts_out=counts)
            outs.append(frame)
        torch.cuda.synchronize()
        if fast:
            state, cap = annotate_video._engine(mgr, det, 1).count_state(), annotate_video._engine(mgr, det, 1).track_trails_capacity()
            rows = lambda text: [x.split(",")[:6] + x.split(",")[7:] for x in text.splitlines()]
            assert rows(tracks.getvalue()) == rows(want_lines)
            for k, (out, res) in enumerate(zip(outs, results)):
                assert np.array_equal(out[:, :, ::-1], res[2]), k
        else:
            state, cap = annotate_video._eager_count_state(mgr.class_mapping), min(2 * entry.TRACK_CAPACITY, ops.TRACK_MAX)
            assert any((out != src[:, :, ::-1]).any() for out, src in zip(outs, footage[1]))
        ref, csv = mot_counts(tracks.getvalue(), 6, cap, mgr.class_mapping)
        assert sum(map(sum, ref.totals)) > 0 and csv and counts.getvalue().splitlines() == csv
        assert np.array_equal(state.cpu().numpy(), ref.words())
        before = ops.count_totals(state)
        annotate_video.reset_tracks(mgr, det, 1)
        torch.cuda.synchronize()
        after = ops.count_totals(state)
        assert after["entries"] == 0 and after["totals"] == before["totals"]
        annotate_video.reset_counts(mgr, det, 1)
        torch.cuda.synchronize()
        assert not state.cpu().numpy().any()
    finally:
        voc_dets.FAST_ENTRY = True
    with pytest.raises(ValueError, match="needs track="):
        annotate_video.get_annotated_frame(mgr, det, outs[0], None, *RESIZE, count=COUNT)
    with pytest.raises(ValueError, match="counts_out is where the crossings are written"):
        annotate_video.get_annotated_frame(mgr, det, outs[0], None, *RESIZE, track=TRACK, counts_out=counts)
