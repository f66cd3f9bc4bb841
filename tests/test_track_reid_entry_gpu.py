"""track_reid through the detection entry and annotate_video: submit_batch(annotate=True, track=..., track_reid=(pct, keep)) runs one
ops.track_reid_update behind the tracker call, and everything the host gets back -- the dets' "track_id", the MOT lines, the "reid" list of
the trailing dict, the CSV, the printed lines, the engine's state -- is held against tests/track_reid_ref.py applied to the rows that the
SAME run without the option returned (the tracker does not know about the stage: its ids are the same in both runs)."""
import io

import numpy as np
import pytest

from tests import track_reid_ref as ref
from tests.test_redact_entry_gpu import RESIZE, engine, f32_models, quiet      # noqa: F401  (the synthetic ResNet-50 pair)
from tests.test_annotate_gpu import frame_pixels
from tests.test_track_entry_gpu import split_dets
from tests.test_track_motion_entry_gpu import H, RADIUS, REDACT, TRACK, W

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

REID = (30, 50)
# scene A stands still for two frames, scene B for hold + 2 -- every track of A is freed --, then A is back for hold + 3: its objects return,
# at once where the tracker has a free slot, else when B's held tracks have left (this detector fills the tracker's 64 slots)
SCENES = [0, 0] + [1] * (TRACK[1] + 2) + [0] * (TRACK[1] + 3)
NAMES = ["r_%02d.png" % (3 * k) for k in range(len(SCENES))]
BACK = 2 + TRACK[1] + 2                                   # the first frame of A's return


@pytest.fixture(scope="module")
def footage(tmp_path_factory):
    from PIL import Image as PilImage
    # (dark against bright noise: no bin is shared, so no object of one scene is taken for one of the other)
    scenes = [frame_pixels(H, W, 81) // 2, 128 + frame_pixels(H, W, 82) // 2]
    srcs = [scenes[k] for k in SCENES]
    d_in = tmp_path_factory.mktemp("reid") / "in"
    d_in.mkdir()
    for name, rgb in zip(NAMES, srcs):
        PilImage.fromarray(rgb).save(str(d_in / name))
    return d_in, srcs


def annotate(f32_models, footage, d_out, monkeypatch, **kw):
    """``annotate_images`` over the footage -> (the results its passes returned, the printed text, the MOT text)."""
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
    return seen, text, tracks.getvalue()


def rule_over(plain, srcs, mapping, capacity, reid=REID, rgb=True):
    """The rule over the rows a run WITHOUT the option returned -> (per frame: the ids of its dets in order, its events; the state)."""
    table = np.array([name != "bg" for name, _ in sorted(mapping.items(), key=lambda kv: kv[1])], dtype=np.uint8)
    state, ids, events = ref.new_state(capacity), [], []
    for src, res in zip(srcs, plain):
        live, held = split_dets(res[1])
        row = lambda d: ([int(v) for v in d["bbox"]], mapping[d["cls_name"]], d.get("track_id", 0))
        R = max(len(live) + len(held), 1)
        cut = len(res) > 3 and bool(res[3].get("scene_cut"))
        state, out, lists, _ = ref.update(state, capacity, src[None], ref.pack(R, [row(d) for d in live], [row(d) for d in held])[None], 1, table,
                                          *reid, rgb, np.array([int(cut)], dtype=np.int32))
        ids.append(out[0, 4 + 6 * R:4 + 6 * R + len(live) + len(held)].tolist())
        events.append(ref.events(lists[0]))
    return ids, events, state


def ids_of(results):
    return [[d.get("track_id", 0) for d in r[1]] for r in results]


@pytest.mark.parametrize("kw", [{}, {"detect_every": 2}, {"track_scene_cut": 40}], ids=["plain", "every2", "cut"])
def test_ids_events_and_state_match_the_rule(engine, f32_models, footage, monkeypatch, tmp_path, kw):
    mapping = f32_models[0].class_mapping
    plain, _, plain_mot = annotate(f32_models, footage, tmp_path / "a", monkeypatch, **kw)
    csv = tmp_path / "reid.csv"
    got, text, mot = annotate(f32_models, footage, tmp_path / "b", monkeypatch, track_reid=REID, reid_out=str(csv), **kw)
    torch.cuda.synchronize()
    capacity = (engine.reid_state().numel() - 4) // ref.ENTRY_WORDS
    want_ids, want_events, want_state = rule_over(plain, footage[1], mapping, capacity)
    assert len(got) == len(SCENES) and all("reid" in r[-1] for r in got)
    assert [r[-1]["reid"] for r in got] == want_events
    assert ids_of(got) == want_ids
    assert np.array_equal(engine.reid_state().cpu().numpy(), want_state)
    n = sum(len(e) for e in want_events)
    if "track_scene_cut" not in kw:                       # scene A returns: its objects take their ids back (a cut forgets them)
        assert n > 0 and not any(want_events[:BACK]) and ids_of(got) != ids_of(plain) and mot != plain_mot
        # an older id every time.  (Which one is the reference's to say: this detector fills the tracker, rows it left out in frames 1-2
        # have no entry of their own, and dark noise looks alike, so a row may take a neighbour's.)
        assert all(p < t and d * 100 <= REID[0] * 8192 for evs in want_events for p, t, c, d, g in evs)
    else:
        assert any(r[-1].get("scene_cut") for r in got)
    # the CSV, the printed lines and the key tag
    names = {v: k for k, v in mapping.items()}
    rows = ["%d,%d,%d,%s,%d,%d" % (f + 1, p, t, names[c], d, g) for f, evs in enumerate(want_events) for p, t, c, d, g in evs]
    assert csv.read_text().splitlines() == ["frame,id,tracker_id,cls,distance,gap"] + rows
    lines = text.splitlines()
    printed = [x for x in lines if x.startswith("re-identified: ")]
    path = lambda f: str(footage[0] / NAMES[f])
    assert printed == ["re-identified: %s id %d" % (path(f), ev[0]) for f, evs in enumerate(want_events) for ev in evs] + ["re-identified: %d" % n]
    for f, evs in enumerate(want_events):
        if evs:                                           # in front of that frame's lines
            assert lines.index("re-identified: %s id %d" % (path(f), evs[0][0])) < lines.index("processing " + path(f))
    assert any(k[-3:] == ("track_reid",) + REID for k in engine.cache.keys())


def test_main_writes_the_csv_and_prints_the_lines(f32_models, footage, monkeypatch, tmp_path):
    from faster_rcnn_amd import annotate_video, resnet
    mgr, det, _ = f32_models
    loaded = []
    monkeypatch.setattr(resnet, "rpn_from_h5", lambda path, **kw: loaded.append(path) or mgr.rpn_model)
    monkeypatch.setattr(resnet, "det_from_h5", lambda path, **kw: loaded.append(path) or det)
    common = ["rpn.h5", "det.h5", str(footage[0]), "--out_dir", str(tmp_path / "out"), "--resize_dims", "%d,%d" % RESIZE, "--png_encoder", "host"]
    for argv, why in ((["--reid_keep", "5"], "needs --track_reid"), (["--reid_out", "x.csv"], "needs --track_reid"),
                      (["--track_reid"], "needs --track"), (["--track", "--track_reid", "101"], "pct"),
                      (["--track", "--track_reid", "--reid_keep", "4096"], "keep"),
                      (["--track", "--track_reid", "--track_lookback", "2"], "not supported")):
        with pytest.raises(ValueError, match=why):
            annotate_video.main(common + argv)
    assert not loaded
    (tmp_path / "out").mkdir()
    csv, mot = tmp_path / "reid.csv", tmp_path / "mot.txt"
    thr, hold, grow = TRACK
    _, text = quiet(annotate_video.main, common + ["--track", "--track_iou", str(thr), "--track_hold", str(hold), "--track_grow", str(grow),
                                                   "--tracks_out", str(mot), "--track_reid", "--reid_keep", "50", "--reid_out", str(csv)])
    assert loaded == ["rpn.h5", "det.h5"]
    rows = csv.read_text().splitlines()
    assert rows[0] == "frame,id,tracker_id,cls,distance,gap" and len(rows) > 1
    back = [r.split(",") for r in rows[1:]]
    assert all(int(r[0]) > BACK and int(r[1]) < int(r[2]) for r in back)
    printed = [x for x in text.splitlines() if x.startswith("re-identified: ")]
    assert printed[-1] == "re-identified: %d" % (len(rows) - 1) and len(printed) == len(rows)
    # the MOT file carries the ids the CSV names, not the tracker's
    last = max(int(r[0]) for r in back)
    mot_ids = {int(x.split(",")[1]) for x in mot.read_text().splitlines() if int(x.split(",")[0]) == last}
    assert {int(r[1]) for r in back if int(r[0]) == last} <= mot_ids and not ({int(r[2]) for r in back} & mot_ids)


@pytest.mark.parametrize("fast", [True, False])
def test_get_annotated_frame_frame_by_frame(engine, f32_models, footage, monkeypatch, tmp_path, fast):
    from faster_rcnn_amd import annotate_video, ops, shapes, voc_dets
    mgr, det, _ = f32_models
    tracks, reid_csv, plain_tracks = io.StringIO(), io.StringIO(), io.StringIO()
    voc_dets.FAST_ENTRY = fast
    try:
        texts = []
        for kw, mot in (({}, plain_tracks), ({"track_reid": REID, "reid_out": reid_csv}, tracks)):
            annotate_video.reset_tracks(mgr, det, 1)
            for k, src in enumerate(footage[1]):
                frame = np.ascontiguousarray(src[:, :, ::-1])                # (the one-frame path takes B, G, R)
                img = shapes.InMemoryImage(data=frame, width=W, height=H)
                texts.append(quiet(annotate_video.get_annotated_frame, mgr, det, frame, img, *RESIZE, redact=REDACT, track=TRACK, tracks_out=mot,
                                   frame_no=k + 1, track_motion=RADIUS, **kw)[1])
        torch.cuda.synchronize()
        states = annotate_video._engine(mgr, det, 1).edit_states if fast else annotate_video._eager_states(mgr.class_mapping)
        totals = ops.track_reid_totals(states.reid_state())
        rows = reid_csv.getvalue().splitlines()
        assert totals["frames"] == len(SCENES) and totals["reidentified"] == len(rows) > 0
        back = [r.split(",") for r in rows]
        assert all(int(r[0]) > BACK and int(r[1]) < int(r[2]) for r in back)
        ids_at = lambda text, f: [int(x.split(",")[1]) for x in text.splitlines() if int(x.split(",")[0]) == f]
        want = {int(r[2]): int(r[1]) for r in back}     # every id the tracker issued anew, and whose it is
        for f in range(1, len(SCENES) + 1):
            assert [want.get(t, t) for t in ids_at(plain_tracks.getvalue(), f)] == ids_at(tracks.getvalue(), f), f
        assert "re-identified: %s id %s" % (back[0][0], back[0][1]) in texts[len(SCENES) + int(back[0][0]) - 1].splitlines()
        annotate_video.reset_tracks(mgr, det, 1)
        torch.cuda.synchronize()
        assert not states.reid_state().cpu().numpy().any()
    finally:
        voc_dets.FAST_ENTRY = True
    with pytest.raises(ValueError, match="needs track="):
        annotate_video.get_annotated_frame(mgr, det, footage[1][0], None, *RESIZE, track_reid=REID)
    with pytest.raises(ValueError, match="reid_out is where"):
        annotate_video.get_annotated_frame(mgr, det, footage[1][0], None, *RESIZE, track=TRACK, reid_out=reid_csv)


def test_refusals_the_key_and_the_resets(engine, f32_models, footage, monkeypatch, tmp_path):
    from faster_rcnn_amd import entry, ops, shapes, util
    from faster_rcnn_amd._lib import FrcnnError
    imgs = [shapes.Image(shapes.Metadata("t%d" % i, W, H, [], "none"), s) for i, s in enumerate(footage[1][:2])]
    resized, ratios = util.resize_imgs(imgs, min_size=RESIZE[0], max_size=RESIZE[1])
    pixels = [engine.host_pixels(r) for r in resized]
    captures = engine.cache.captures
    two = lambda **kw: engine.submit_batch(resized, ratios, 0.0, pixels, batch=2, annotate=True, **kw)
    with pytest.raises(FrcnnError, match=r"track_reid= gives the tracker's ids back: pass track="):
        two(track_reid=REID)
    with pytest.raises(FrcnnError, match="track_reid= together with track_lookback= is not supported"):
        two(track=TRACK, track_lookback=2, track_reid=REID)
    with pytest.raises(FrcnnError, match="track_reid= together with track_backtrack= is not supported"):
        two(track=TRACK, track_motion=RADIUS, detect_every=2, track_backtrack=2, track_reid=REID)
    for bad in ((0, 50), (101, 50), (30, 0), (30, 4096), (30.0, 50), 30, (30,)):
        with pytest.raises(FrcnnError, match="track_reid="):
            two(track=TRACK, track_reid=bad)
    assert engine.cache.captures == captures
    spec = entry.PassSpec.checked(engine, 4, annotate=True, redact=REDACT, track=TRACK, track_motion=RADIUS, remove=("all", 2, 3, 4),
                                  track_reid=(None, None))
    assert spec.track_reid == (25, 250) and spec.key_tail(4)[-3:] == ("track_reid", 25, 250) and spec.key_tail(4)[-8:-3][0] == "remove"
    plain = entry.PassSpec.checked(engine, 4, annotate=True, redact=REDACT, track=TRACK, track_motion=RADIUS)
    assert plain.track_reid is None and "track_reid" not in plain.key_tail(4)
    # the resets: reid_reset forgets the looks and leaves the tracker; track_reset empties both
    annotate(f32_models, footage, tmp_path / "a", monkeypatch, track_reid=REID)
    torch.cuda.synchronize()
    state = engine.reid_state()
    assert ops.track_reid_totals(state)["entries"] > 0 and engine.edit_states.tracker()[1] > 0
    engine.reid_reset()
    torch.cuda.synchronize()
    assert not state.cpu().numpy().any() and engine.reid_state() is state and engine.edit_states.tracker()[1] > 0
    state[0] = 1
    engine.track_reset()
    torch.cuda.synchronize()
    assert not state.cpu().numpy().any() and not engine.edit_states.tracker().cpu().numpy().any()
