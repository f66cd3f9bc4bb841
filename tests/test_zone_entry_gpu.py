"""zone through the detection entry and annotate_video: submit_batch(annotate=True, track=..., zone=(zones, classes, W, anchor)) runs one
ops.zone_update behind the count update (behind the look-back / back-track call of a delayed pass, over the emitted buffers) and one
ops.zone_draw_u8 per frame behind the heat map and under every line.  Every frame, every occupancy and every list of events is held
against tests/zone_ref.py applied to the rows the same pass returned, in the order the frames came out -- byte for byte."""
import numpy as np
import pytest

from tests import count_ref as CR
from tests import redact_ref as R
from tests import track_ref as T
from tests import zone_ref as ZR
from tests.test_count_entry_gpu import COUNT, LINES
from tests.test_redact_entry_gpu import RESIZE, engine, f32_models, quiet      # noqa: F401  (the synthetic ResNet-50 pair)
from tests.test_track_cut_entry_gpu import CUT, NAMES, PCT, annotate, footage      # noqa: F401  (six PNG frames: scene A x 3, scene B x 3)
from tests.test_track_entry_gpu import split_dets
from tests.test_track_motion_entry_gpu import H, RADIUS, REDACT, TRACK, W
from tests.test_track_trails_entry_gpu import files_match, live_buffer

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# over the 200 x 330 frames (the scenes move by (3, 2) a frame): the left half, its neighbour, a triangle, an "L", a band clipped by the
# frame and one zone beyond it
ZONES = (((0, 0), (165, 0), (165, 200), (0, 200)), ((165, 0), (330, 0), (330, 200), (165, 200)), ((20, 190), (160, 10), (310, 190)),
         ((40, 20), (300, 20), (300, 90), (140, 90), (140, 180), (40, 180)), ((-50, 95), (400, 80), (400, 125), (-50, 110)),
         ((400, 0), (500, 0), (450, 199)))
ZONE = (ZONES, "all", 2, 1)


def check_frames(engine, srcs, results, mapping, every=1, zone=ZONE, drawn=True, reference=None):
    """Every returned frame == redaction, then the zones, then boxes, and every frame's occupancy and events == the rule's, from the
    frame's own returned rows -> the reference."""
    zones, classes, width, anchor = zone
    table = np.ones(max(mapping.values()) + 1, dtype=np.uint8)
    ref = reference or ZR.Zones(H, W, zones, table, engine.track_trails_capacity(), (TRACK[1] + 1) * every, anchor)
    for f, (src, res) in enumerate(zip(srcs, results)):
        dets, out, marks = res[1], res[2], res[-1]
        filled = [d for d in dets if d.get("backfilled")]
        live, held = split_dets([d for d in dets if not d.get("backfilled")])
        zlist = ref.frame(live_buffer(live, mapping))
        assert marks["zones"] == {"occupancy": ZR.occupancy_of(zlist, len(zones)), "events": ZR.events_of(zlist)}, f
        want = R.redact_dets(src, live + held + filled, mapping, *REDACT)
        want = T.annotate(ZR.draw(want, zlist, zones, width, 1), live) if drawn else want
        assert np.array_equal(out, want), (f, np.argwhere(out != want)[:4])
    return ref


def state_matches(engine, ref):
    torch.cuda.synchronize()
    assert np.array_equal(engine.zone_state().cpu().numpy(), ref.words())


@pytest.mark.parametrize("every", [1, 2])
def test_events_and_frames_match_the_rule(engine, f32_models, footage, monkeypatch, tmp_path, every):
    from faster_rcnn_amd import ops
    mapping = f32_models[0].class_mapping
    kw = {} if every == 1 else {"detect_every": every}
    csv = tmp_path / "zones.csv"
    results, text, lines, files = annotate(f32_models, footage, tmp_path / "out", monkeypatch, zone=ZONE, zones_out=str(csv), **kw)
    assert len(results) == 6 and all(len(r) == 4 and set(r[3]) == {"zones"} for r in results)
    ref = check_frames(engine, footage[1], results, mapping, every)
    state_matches(engine, ref)
    files_match(files, results)
    assert sum(ref.visitors) > 0 and ref.dropped == 0 and max(ref.peak) > 0
    # the CSV and the printed summary
    names = {v: k for k, v in mapping.items()}
    rows = ["%d,%d,%s,%d,%s,%d" % (f + 1, z, ops.ZONE_KINDS[k], i, names[c], d) for f, r in enumerate(results) for z, k, i, c, d in r[3]["zones"]["events"]]
    assert csv.read_text().splitlines() == ["frame,zone,kind,id,cls,dwell"] + rows and rows
    printed = [x for x in text.splitlines() if x.startswith("zone ")]
    mean = lambda z: "%.1f frames" % (ref.dwell[z] / ref.stays[z]) if ref.stays[z] else "-"
    assert printed == ["zone %d: visitors %d peak %d stays %d mean dwell %s" % (z, ref.visitors[z], ref.peak[z], ref.stays[z], mean(z))
                       for z in range(len(ZONES))]
    plain = annotate(f32_models, footage, tmp_path / "plain", monkeypatch, **kw)
    assert plain[2] == lines and any(files[n] != plain[3][n] for n in NAMES)
    # (the synthetic model's many boxes give some frames more than 64 events: the warning says how many rows the file is short by)
    warned = [x for x in text.splitlines() if x.startswith("warning: ") and "zone events" in x]
    assert warned == (["warning: %d zone events did not fit their frames' lists: the zones file is short by that many rows; the totals are exact"
                       % ref.events_dropped] if ref.events_dropped else [])
    assert [x for x in text.splitlines() if not x.startswith("zone ") and x not in warned] == plain[1].splitlines()
    tail = ("motion", RADIUS) + (("every", every) if every > 1 else ()) + ("zone",) + ZONE
    assert any(k[-len(tail):] == tail for k in engine.cache.keys())


def test_with_scene_cut_trails_heat_and_count_one_dict_carries_all_marks(engine, f32_models, footage, monkeypatch, tmp_path):
    from tests import heat_ref, track_trails_ref as TR
    mapping = f32_models[0].class_mapping
    results, _, _, files = annotate(f32_models, footage, tmp_path / "out", monkeypatch, zone=ZONE, count=COUNT, track_scene_cut=PCT, track_trails=(3, 2),
                                    heatmap=("all", 160, 0))
    assert [set(r[3]) for r in results] == [{"crossings", "zones", "scene_cut"} if f == CUT else {"crossings", "zones"} for f in range(6)]
    assert all(len(r) == 4 for r in results)
    table = np.ones(max(mapping.values()) + 1, dtype=np.uint8)
    cap, exp = engine.track_trails_capacity(), TRACK[1] + 1
    ref, counter = ZR.Zones(H, W, ZONES, table, cap, exp, 1), CR.Counter(H, W, LINES, table, cap, exp)
    trails, heat = TR.Trails(H, W, cap, 3, exp), heat_ref.Heat(H, W)
    for f, (src, res) in enumerate(zip(footage[1], results)):
        live, held = split_dets(res[1])
        buf = live_buffer(live, mapping)
        zlist, clist, plist = ref.frame(buf), counter.frame(buf), trails.frame(buf)
        assert res[3]["zones"] == {"occupancy": ZR.occupancy_of(zlist, len(ZONES)), "events": ZR.events_of(zlist)}, f
        assert res[3]["crossings"] == CR.events_of(clist), f
        want = R.redact_dets(src, live + held, mapping, *REDACT)
        heat.update(buf, table, 0, tracked=True)
        # the order: heat, zones, trails, lines, boxes
        want = T.annotate(CR.draw(TR.draw(ZR.draw(heat.draw(want, 160, 1), zlist, ZONES, 2, 1), plist, 3, 2, 1), clist, LINES, 2, 1), live)
        assert np.array_equal(res[2], want), (f, np.argwhere(res[2] != want)[:4])
    state_matches(engine, ref)
    tail = ("count",) + COUNT + ("zone",) + ZONE
    assert any(k[-len(tail):] == tail for k in engine.cache.keys())


@pytest.mark.parametrize("delayed", ["track_lookback", "track_backtrack"])
def test_a_delayed_pass_counts_in_emitted_order(engine, f32_models, footage, monkeypatch, tmp_path, delayed):
    mapping = f32_models[0].class_mapping
    kw = {"track_lookback": 2} if delayed == "track_lookback" else {"detect_every": 2, "track_backtrack": 2}
    every = kw.get("detect_every", 1)
    results, text, _, files = annotate(f32_models, footage, tmp_path / "out", monkeypatch, zone=ZONE, **kw)
    assert len(results) == 6 and all(set(r[-1]) == {"zones"} for r in results)
    ref = check_frames(engine, footage[1], results, mapping, every)
    state_matches(engine, ref)
    files_match(files, results)
    assert ref.frames == 6 and sum(ref.visitors) > 0


def test_no_draw_counts_and_draws_nothing(engine, f32_models, footage, monkeypatch, tmp_path):
    mapping = f32_models[0].class_mapping
    results, _, _, _ = annotate(f32_models, footage, tmp_path / "out", monkeypatch, zone=ZONE, draw=False)
    ref = check_frames(engine, footage[1], results, mapping, drawn=False)
    state_matches(engine, ref)
    assert sum(ref.visitors) > 0
    bare, _, _, _ = annotate(f32_models, footage, tmp_path / "bare", monkeypatch, draw=False)
    assert all(np.array_equal(a[2], b[2]) for a, b in zip(results, bare))


def test_zone_reset_and_track_reset(engine, f32_models, footage, monkeypatch, tmp_path):
    from faster_rcnn_amd import ops
    first = annotate(f32_models, footage, tmp_path / "a", monkeypatch, zone=ZONE)
    state = engine.zone_state()
    torch.cuda.synchronize()
    before = ops.zone_totals(state)
    assert before["entries"] > 0 and sum(before["visitors"]) > 0
    engine.track_reset()                                                     # the ids end without events; the totals stay
    torch.cuda.synchronize()
    assert ops.zone_totals(state) == dict(before, entries=0) and not state[ops.ZONE_HEAD:].cpu().numpy().any()
    engine.zone_reset()
    torch.cuda.synchronize()
    assert not state.cpu().numpy().any() and engine.zone_state() is state
    again = annotate(f32_models, footage, tmp_path / "b", monkeypatch, zone=ZONE)            # (a run starts from an empty state itself)
    assert again[1:] == first[1:] and [r[3] for r in again[0]] == [r[3] for r in first[0]]


def test_without_the_option_nothing_changes(engine, f32_models, footage, monkeypatch, tmp_path):
    from faster_rcnn_amd import entry
    before = annotate(f32_models, footage, tmp_path / "a", monkeypatch)
    keys = set(engine.cache.keys())
    with_zone = annotate(f32_models, footage, tmp_path / "b", monkeypatch, zone=ZONE)
    after = annotate(f32_models, footage, tmp_path / "c", monkeypatch)
    now = set(engine.cache.keys())
    tagged = {k for k in now if "zone" in k}
    assert tagged and now - tagged == keys - tagged
    assert before[1:] == after[1:] and with_zone[2] == before[2] and with_zone[3] != before[3]
    assert all(len(r) == 3 for r in before[0]) and all(len(r) == 3 for r in after[0])
    spec = entry.PassSpec.checked(engine, 4, annotate=True, redact=REDACT, track=TRACK, track_motion=RADIUS)
    assert spec.zone is None and any(k[-len(spec.key_tail(4)):] == spec.key_tail(4) for k in keys)
    assert all(k[-5:] == ("zone",) + ZONE for k in tagged)                   # the tag goes behind everything else


def test_submit_batch_refusals(engine, f32_models, footage):
    from faster_rcnn_amd import shapes, util
    from faster_rcnn_amd._lib import FrcnnError
    imgs = [shapes.Image(shapes.Metadata("t%d" % i, W, H, [], "none"), s) for i, s in enumerate(footage[1][:2])]
    resized, ratios = util.resize_imgs(imgs, min_size=RESIZE[0], max_size=RESIZE[1])
    pixels = [engine.host_pixels(r) for r in resized]
    captures = engine.cache.captures
    two = lambda **kw: engine.submit_batch(resized, ratios, 0.0, pixels, batch=2, annotate=True, **kw)
    with pytest.raises(FrcnnError, match=r"zone= tests the tracker's ids against the zones: pass track="):
        two(zone=ZONE)
    tri = ((1, 1), (9, 1), (5, 9))
    for bad in (((tri[:2],), "all", 2, 0), ((tri,) * 9, "all", 2, 0), ((tri,), "tram", 2, 0), ((tri,), "all", 0, 0), ((tri,), "all", 2, "top"), (tri,),
                ((((1, 1), (1, 1), (5, 9)),), "all", 2, 0), ((((0, 0), (70000, 1), (5, 9)),), "all", 2, 0)):
        with pytest.raises(FrcnnError, match="zone="):
            two(track=TRACK, zone=bad)
    assert engine.cache.captures == captures


def mot_zones(lines, frames, capacity, mapping):
    """The reference and the CSV rows the MOT lines of a run imply: a frame's lines are its live tracked rows, in row order."""
    from faster_rcnn_amd import ops
    names = {v: k for k, v in mapping.items()}
    ref = ZR.Zones(H, W, ZONES, np.ones(max(mapping.values()) + 1, dtype=np.uint8), capacity, TRACK[1] + 1, 1)
    rows = [[int(float(v)) for v in x.split(",")[:6]] + [int(x.split(",")[7])] for x in lines.splitlines()]
    csv = []
    for f in range(1, frames + 1):
        live = [(tid, cls, (left, top, left + w, top + h)) for n, tid, left, top, w, h, cls in rows if n == f]
        zlist = ref.frame(ZR.make_tracked(live, max(len(live), 1)))
        csv += ["%d,%d,%s,%d,%s,%d" % (f, z, ops.ZONE_KINDS[k], i, names[c], d) for z, k, i, c, d in ZR.events_of(zlist)]
    return ref, csv


@pytest.mark.parametrize("fast", [True, False])
def test_get_annotated_frame_frame_by_frame(engine, f32_models, footage, monkeypatch, tmp_path, fast):
    import io
    from faster_rcnn_amd import annotate_video, entry, ops, shapes, voc_dets
    mgr, det, _ = f32_models
    results, _, want_lines, _ = annotate(f32_models, footage, tmp_path / "out", monkeypatch, zone=ZONE)
    tracks, zones_csv, outs = io.StringIO(), io.StringIO(), []
    voc_dets.FAST_ENTRY = fast
    try:
        annotate_video.reset_tracks(mgr, det, 1)
        annotate_video.reset_zones(mgr, det, 1)
        for k, src in enumerate(footage[1]):
            frame = np.ascontiguousarray(src[:, :, ::-1])                    # (the file's R,G,B as the one-frame path takes it: B,G,R)
            img = shapes.InMemoryImage(data=frame, width=W, height=H)
            quiet(annotate_video.get_annotated_frame, mgr, det, frame, img, *RESIZE, redact=REDACT, track=TRACK, tracks_out=tracks,
                  frame_no=k + 1, track_motion=RADIUS, zone=ZONE, zones_out=zones_csv)
            outs.append(frame)
        torch.cuda.synchronize()
        if fast:
            state, cap = annotate_video._engine(mgr, det, 1).zone_state(), annotate_video._engine(mgr, det, 1).track_trails_capacity()
            rows = lambda text: [x.split(",")[:6] + x.split(",")[7:] for x in text.splitlines()]
            assert rows(tracks.getvalue()) == rows(want_lines)
            for k, (out, res) in enumerate(zip(outs, results)):
                assert np.array_equal(out[:, :, ::-1], res[2]), k
        else:
            state, cap = annotate_video._eager_states(mgr.class_mapping).zone_state(), min(2 * entry.TRACK_CAPACITY, ops.TRACK_MAX)
            assert any((out != src[:, :, ::-1]).any() for out, src in zip(outs, footage[1]))
        ref, csv = mot_zones(tracks.getvalue(), 6, cap, mgr.class_mapping)
        assert sum(ref.visitors) > 0 and csv and zones_csv.getvalue().splitlines() == csv
        assert np.array_equal(state.cpu().numpy(), ref.words())
        before = ops.zone_totals(state)
        annotate_video.reset_tracks(mgr, det, 1)
        torch.cuda.synchronize()
        assert ops.zone_totals(state) == dict(before, entries=0)
        annotate_video.reset_zones(mgr, det, 1)
        torch.cuda.synchronize()
        assert not state.cpu().numpy().any()
    finally:
        voc_dets.FAST_ENTRY = True
    with pytest.raises(ValueError, match="needs track="):
        annotate_video.get_annotated_frame(mgr, det, outs[0], None, *RESIZE, zone=ZONE)
    with pytest.raises(ValueError, match="zones_out is where the zone events are written"):
        annotate_video.get_annotated_frame(mgr, det, outs[0], None, *RESIZE, track=TRACK, zones_out=zones_csv)
