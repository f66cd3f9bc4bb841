"""remove= through the detection entry and annotate_video: submit_batch(annotate=True, remove=(classes, S, T, M)) runs one
ops.plate_update on every untouched frame and one ops.plate_fill_u8 behind its redaction, inside the captured pass.  Every returned frame
and the engine's plate state are held against tests/plate_ref.py applied to the source frames and the rows the passes returned -- byte
for byte.  The frames are noise: T = 255 lets every run go on, so the plate settles after S frames wherever no box lies."""
import io

import numpy as np
import pytest

from tests import plate_ref as P
from tests import redact_ref as R
from tests import track_ref as T
from tests.test_redact_entry_gpu import REDACT as NAMED_REDACT, RESIZE, engine, f32_models, frame_pixels, quiet, staged, submit      # noqa: F401
from tests.test_track_cut_entry_gpu import CUT, NAMES, PCT, annotate, footage      # noqa: F401  (six PNG frames of two scenes)
from tests.test_track_entry_gpu import split_dets
from tests.test_track_motion_entry_gpu import H, REDACT, TRACK, W

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

REMOVE = ("all", 2, 255, 1)
BLUR_ALL = ("all", "blur", 3, 2)


def table_of(mapping, classes):
    t = np.zeros(max(mapping.values()) + 1, dtype=np.uint8)
    for name, idx in mapping.items():
        t[idx] = (name != "bg") if classes == "all" else (name in classes)
    return t


def buffer_of(dets, mapping, tracked):
    """The returned rows of a frame -- live, held and back-filled alike -- as the buffer the plate rule reads (their order does not matter)."""
    rows = max(len(dets), 1)
    items = [tuple(int(v) for v in d["bbox"]) + (mapping[d["cls_name"]],) for d in dets]
    return (P.tracked if tracked else P.packed)(rows, items), rows


def plate_step(ref, src, dets, mapping, remove, redact=None, tracked=False, cut=None):
    """One frame through the rule: the update from ``src``, the redaction, the fill -> (the frame, filled from the plate, left unknown)."""
    classes, S, Tol, M = remove
    buf, rows = buffer_of(dets, mapping, tracked)
    P.update(ref, src, buf, rows, S, Tol, M, cut=cut)
    out = src.copy() if redact is None else np.array(R.redact_dets(src, dets, mapping, *redact))
    names = lambda c: {n for n in mapping if n != "bg"} if c == "all" else set(c)
    keep = redact is not None and names(classes) <= names(redact[0])        # the redaction shows where its classes cover the remove classes
    return P.fill(out, ref, buf, rows, table_of(mapping, classes), M, keep)


def same_dets(a, b):
    return len(a) == len(b) and all(x["cls_name"] == y["cls_name"] and np.array_equal(x["bbox"], y["bbox"]) and x["prob"] == y["prob"]
                                    for x, y in zip(a, b))


def engine_state(engine, h, w, rgb):
    torch.cuda.synchronize()
    return engine.plate_state(h, w, rgb).cpu().numpy()[:4 + 2 * h * w]


NAMED_REMOVE = (("car", "person", "dog", "motorbike"), 2, 255, 1)         # names NAMED_REDACT holds


@pytest.mark.parametrize("leg", ["alone", "track", "redact covers", "redact does not cover", "names within the redacted names",
                                 "all within every name", "names the redaction lacks"])
def test_a_remove_pass_is_the_rule_over_the_returned_rows(engine, staged, f32_models, leg):
    """draw=False: the returned frame is the redaction and the fill alone.  Three submits of four frames each -- the same four frames
    again, so the plate of the first pass is what the second fills from --, then a padded one of one frame.  The redaction shows under
    unknown pixels exactly when its classes are a superset of the remove classes, however either is spelt."""
    mapping = f32_models[0].class_mapping
    srcs = staged[0]
    h, w = srcs[0].shape[:2]
    every = (tuple(n for n in mapping if n != "bg"),) + NAMED_REDACT[1:]
    lacking = (tuple(n for n in NAMED_REDACT[0] if n != "person"),) + NAMED_REDACT[1:]
    kw = {"track": dict(track=TRACK), "redact covers": dict(redact=BLUR_ALL), "redact does not cover": dict(redact=NAMED_REDACT),
          "names within the redacted names": dict(redact=NAMED_REDACT), "all within every name": dict(redact=every),
          "names the redaction lacks": dict(redact=lacking)}.get(leg, {})
    remove = NAMED_REMOVE if leg.startswith("names") else REMOVE
    keeps = leg in ("redact covers", "names within the redacted names", "all within every name")
    redact, tracked = kw.get("redact"), "track" in kw
    engine.plate_reset()
    engine.track_reset()
    ref, filled, unknown = P.empty(h, w), 0, 0
    for k, B in enumerate((4, 4, 1)):
        got = submit(engine, staged, B, draw=False, remove=remove, **kw)
        assert len(got) == B
        for f, (n_rois, dets, out) in enumerate(got):
            want, from_plate, left = plate_step(ref, srcs[f], dets, mapping, remove, redact, tracked)
            assert np.array_equal(out, want), (k, f, np.argwhere(out != want)[:4])
            filled, unknown = filled + int(from_plate.sum()), unknown + int(left.sum())
            if keeps and left.any():                                        # unknown pixels show the redaction, not black
                assert np.array_equal(out[left], np.array(R.redact_dets(srcs[f], dets, mapping, *redact))[left])
            if redact is not None and not keeps and left.any():
                assert not out[left].any()
        assert np.array_equal(engine_state(engine, h, w, False), ref), k
    print("%s: %d frames, %d known of %d, %d filled, %d unknown" % (leg, ref[0], ref[1], h * w, filled, unknown))
    assert ref[0] == 9 and ref[1] > 0 and filled > 0 and unknown > 0           # (a padding frame does not count; no leg is vacuous)
    tail = ("remove",) + remove
    assert any(k[-5:] == tail and "nodraw" in k and ("track" in k) == tracked for k in engine.cache.keys())


def check_footage(engine, srcs, results, mapping, cuts=False):
    """Every returned frame == redaction, fill, boxes from the frame's own returned rows, in the order the frames came out."""
    ref, stats = P.empty(H, W), []
    for f, (src, res) in enumerate(zip(srcs, results)):
        dets = res[1]
        live, _ = split_dets([d for d in dets if not d.get("backfilled")])
        cut = int(bool(res[3].get("scene_cut"))) if cuts else None
        out, from_plate, left = plate_step(ref, src, dets, mapping, REMOVE, REDACT, True, cut)
        want = T.annotate(out, live)
        assert np.array_equal(res[2], want), (f, np.argwhere(res[2] != want)[:4])
        stats.append((int(ref[1]), int(from_plate.sum()), int(left.sum())))
    assert np.array_equal(engine_state(engine, H, W, True), ref)              # (file-backed frames: R, G, B, a state of their own)
    return ref, stats


@pytest.mark.parametrize("kw", [dict(track_lookback=2), dict(track_scene_cut=PCT)], ids=["lookback", "cut"])
def test_delayed_and_cut_passes_through_annotate_images(engine, f32_models, footage, monkeypatch, tmp_path, kw):
    """annotate_images over six file-backed frames with --redact all --track --track_motion: with the look-back the pass of frames 4-5
    returns frames 0-3 and the flush the rest; with the cut rule the plate is empty after the
    cut frame.  --plate_out and the printed line."""
    from PIL import Image as PilImage
    from faster_rcnn_amd import ops
    mapping = f32_models[0].class_mapping
    out_png = tmp_path / "plate.png"
    results, text, lines, files = annotate(f32_models, footage, tmp_path / "out", monkeypatch, remove=REMOVE, plate_out=str(out_png), **kw)
    assert len(results) == 6
    cuts = "track_scene_cut" in kw
    ref, stats = check_footage(engine, footage[1], results, mapping, cuts)
    print(kw, stats)
    assert ref[0] == 6 and ref[1] > 0 and any(s[1] for s in stats) and any(s[2] for s in stats)
    if cuts:
        assert [bool(r[3].get("scene_cut")) for r in results] == [f == CUT for f in range(6)]
        assert stats[CUT - 1][0] > 0 and stats[CUT][0] == 0 and stats[CUT][1] == 0      # S = 2: nothing is known on the cut frame
    # (what back-filled rows do to the plate is tests/test_frame_edit_plate_gpu.py's: this footage's tracks are born on covered ground)
    for name, res in zip(NAMES, results):
        assert np.array_equal(np.asarray(PilImage.open(io.BytesIO(files[name])).convert("RGB")), res[2]), name
    _, known, plate, _ = ops.plate_image(ref, H, W)
    with PilImage.open(str(out_png)) as im:
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), plate)
    assert "plate %dx%d: 6 frames, %.1f %% known\n" % (W, H, 100.0 * known / (H * W)) in text
    plain = annotate(f32_models, footage, tmp_path / "plain", monkeypatch, **kw)
    assert plain[2] == lines and plain[1] == text.replace([x for x in text.splitlines(True) if x.startswith("plate ")][0], "")
    if not cuts:                                                            # (the cut leg's few filled pixels, thin strips a box grew by since the frame
        assert any(files[n] != plain[3][n] for n in NAMES)                  # before, lie under the drawn outlines: ``stats`` is what shows them)


def test_without_the_option_nothing_changes_and_the_resets(engine, staged, f32_models):
    """The pass without the option before and after a pass with it: the same bytes, and no cache key but the new passes' own carries
    the tag, which goes behind everything else.  track_reset() leaves the plate, plate_reset() empties it, the tensor stays."""
    from faster_rcnn_amd import entry
    h, w = staged[0][0].shape[:2]
    before = submit(engine, staged, 4, redact=NAMED_REDACT)
    keys = set(engine.cache.keys())
    engine.plate_reset()
    with_remove = submit(engine, staged, 4, redact=NAMED_REDACT, remove=REMOVE)
    after = submit(engine, staged, 4, redact=NAMED_REDACT)
    now = set(engine.cache.keys())
    tagged = {k for k in now if "remove" in k}
    assert tagged and now - tagged == keys - tagged and all(k[-5] == "remove" for k in tagged) and any(k[-5:] == ("remove",) + REMOVE for k in tagged - keys)
    for a, b, c in zip(before, after, with_remove):
        assert np.array_equal(a[2], b[2]) and same_dets(a[1], b[1]) and len(a[1]) == len(c[1])
    assert any((a[2] != c[2]).any() for a, c in zip(before, with_remove))
    spec = entry.PassSpec.checked(engine, 4, annotate=True, redact=NAMED_REDACT)
    assert spec.remove is None and any(k[-len(spec.key_tail(4)):] == spec.key_tail(4) for k in keys)
    state = engine.plate_state(h, w, False)                                 # (this engine has met the size in both channel orders)
    engine.track_reset()
    torch.cuda.synchronize()
    assert int(state[0]) == 4
    engine.plate_reset()
    torch.cuda.synchronize()
    assert not state.cpu().numpy().any() and engine.plate_state(h, w, False) is state
    from faster_rcnn_amd._lib import FrcnnError
    if (h, w, True) in engine.edit_states.plate:
        with pytest.raises(FrcnnError, match="met in both channel orders"):
            engine.plate_state(h, w)


def test_submit_batch_refusals(engine, staged):
    from faster_rcnn_amd._lib import FrcnnError
    srcs, resized, ratios, pixels = staged
    captures = engine.cache.captures
    two = lambda **kw: engine.submit_batch(resized[:2], ratios[:2], 0.0, pixels[:2], batch=2, **kw)
    with pytest.raises(FrcnnError, match=r"remove= paints the objects out of the frame an ANNOTATING pass returns: pass annotate=True"):
        two(remove=REMOVE)
    for bad in (("all", 0, 0, 0), ("all", 256, 0, 0), ("all", 8, 256, 0), ("all", 8, -1, 0), ("all", 8, 10, 65), (("tram",), 8, 10, 8),
                ((), 8, 10, 8), "all", ("all", 8, 10), ("all", True, 0, 0), ("all", 8.0, 0, 0)):
        with pytest.raises(FrcnnError, match="submit_batch: remove="):
            two(annotate=True, remove=bad)
    assert engine.cache.captures == captures


def test_the_eager_path_continues_the_plate_one_frame_at_a_time():
    """draw_eager (foreign models): one-frame calls on a state of its own per class mapping, frame size and channel order."""
    from faster_rcnn_amd import annotate_video as av
    from faster_rcnn_amd.data.voc_data_helpers import VOC_CLASS_MAPPING as mapping
    h, w = 37, 90
    states = av._eager_states(mapping)
    state = states.plate_state(h, w, False)
    states.reset_plate()
    ref = P.empty(h, w)
    det = lambda box, name: {"bbox": np.array(box, dtype=np.int64), "cls_name": name, "prob": np.float32(0.9)}
    frames_dets = [[det([5, 3, 40, 20], "person")], [], [det([15, 3, 50, 22], "person"), det([60, 10, 120, 30], "car")], [det([0, 0, 30, 36], "car")]]
    src = np.random.RandomState(40).randint(0, 256, (h, w, 3)).astype(np.uint8)
    remove = (("person",), 2, 0, 1)
    seen = []
    for f, dets in enumerate(frames_dets):
        frame = src.copy()
        av.draw_eager(frame, list(dets), mapping, draw=False, remove=remove)
        want, from_plate, left = plate_step(ref, src, dets, mapping, remove)
        assert np.array_equal(frame, want), f
        seen.append((int(from_plate.sum()), int(left.sum())))
    assert np.array_equal(state.cpu().numpy()[:4 + 2 * h * w], ref) and ref[0] == 4 and seen[0] == (0, 38 * 20) and seen[2][0] > 0 and seen[3] == (0, 0)
    assert states.plate_state(h, w, False) is state and states.plate_state(h, w, True) is not state


# ----------------------------------------------------------------------------------------------------------- the command line
LATE = dict(H=96, W=128, track=(30, 1, 1), radius=4, redact=("all", "pixelate", 5, 1))      # tests/test_track_lookback_entry_gpu.py's clip


def two_image_footage(d_in):
    """Two frames of one noise image, then four of another, each moved on by two pixels, as PNG files."""
    from PIL import Image as PilImage
    a, b = frame_pixels(LATE["H"], LATE["W"], 71), frame_pixels(LATE["H"], LATE["W"], 72)
    srcs = [a, a] + [np.ascontiguousarray(np.roll(b, 2 * k, axis=1)) for k in range(4)]
    names = ["f_%02d.png" % (7 * k) for k in range(len(srcs))]
    d_in.mkdir()
    for name, rgb in zip(names, srcs):
        PilImage.fromarray(rgb).save(str(d_in / name))
    return names, srcs


def test_main_with_remove_and_plate_out(f32_models, monkeypatch, tmp_path):
    """``annotate_video.main`` itself, its model files replaced by the synthetic pair: --remove all --plate_out with --redact all --track
    --track_motion --track_lookback over six PNG files.  The files are the rule's over the rows the passes returned, the plate file and
    the printed line are the reference's, and the satellite options without --remove are refused before any model is loaded.  (This
    detector's tracks are born where other rows already lie: what BACK-FILLED rows do is tests/test_frame_edit_plate_gpu.py's.)"""
    from PIL import Image as PilImage
    from faster_rcnn_amd import annotate_video, entry, ops, resnet
    mgr, det, _ = f32_models
    mapping = mgr.class_mapping
    loaded = []
    monkeypatch.setattr(resnet, "rpn_from_h5", lambda path, **kw: loaded.append(path) or mgr.rpn_model)
    monkeypatch.setattr(resnet, "det_from_h5", lambda path, **kw: loaded.append(path) or det)
    names, srcs = two_image_footage(tmp_path / "in")
    H, W = LATE["H"], LATE["W"]
    common = ["rpn.h5", "det.h5", str(tmp_path / "in"), "--out_dir", str(tmp_path / "out"), "--resize_dims", "%d,%d" % RESIZE, "--png_encoder", "host"]
    for argv in (["--plate_out", str(tmp_path / "no.png")], ["--remove_settle", "2"], ["--remove", "all", "--remove_margin", "65"]):
        with pytest.raises(ValueError, match="remov"):
            annotate_video.main(common + argv)
    assert not loaded and not (tmp_path / "no.png").exists()
    seen, collect = [], entry.DetectionEntry.collect_batch

    def recording(self, ticket):
        res = collect(self, ticket)
        seen.extend(res)
        return res

    monkeypatch.setattr(entry.DetectionEntry, "collect_batch", recording)
    (tmp_path / "out").mkdir()
    plate_png = tmp_path / "plate.png"
    cls, mode, size, margin = LATE["redact"]
    thr, hold, grow = LATE["track"]
    remove = ("all", 2, 255, 1)
    _, text = quiet(annotate_video.main, common + [
        "--redact", cls, "--redact_mode", mode, "--redact_size", str(size), "--redact_margin", str(margin), "--track", "--track_iou", str(thr),
        "--track_hold", str(hold), "--track_grow", str(grow), "--track_motion", str(LATE["radius"]), "--track_lookback", "4",
        "--remove", "all", "--remove_settle", "2", "--remove_tol", "255", "--remove_margin", "1", "--plate_out", str(plate_png)])
    monkeypatch.setattr(entry.DetectionEntry, "collect_batch", collect)
    assert loaded == ["rpn.h5", "det.h5"] and len(seen) == len(srcs)
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == sorted(names)
    ref = P.empty(H, W)
    for k, (src, (_, dets, _)) in enumerate(zip(srcs, seen)):
        live, _ = split_dets([d for d in dets if not d.get("backfilled")])
        out, from_plate, left = plate_step(ref, src, dets, mapping, remove, LATE["redact"], True)
        got = np.asarray(PilImage.open(str(tmp_path / "out" / names[k])).convert("RGB"))
        assert np.array_equal(got, T.annotate(out, live)), (names[k], np.argwhere(got != T.annotate(out, live))[:4])
    frames, known, plate, _ = ops.plate_image(ref, H, W)
    assert frames == len(srcs) and 0 < known < H * W
    with PilImage.open(str(plate_png)) as im:
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), plate)
    assert "plate %dx%d: %d frames, %.1f %% known\n" % (W, H, frames, 100.0 * known / (H * W)) in text
    assert [x for x in text.splitlines() if x.startswith("processing")] == ["processing " + str(tmp_path / "in" / n) for n in names]


def test_get_annotated_frame_continues_the_engines_plate_and_reset_plate(f32_models, footage, monkeypatch):
    """The captured one-frame path: every call is a one-frame submit that continues the plate of the calls before it on the engine of one
    pass in flight; ``reset_plate`` empties that engine's states."""
    from faster_rcnn_amd import annotate_video, entry, shapes
    mgr, det, _ = f32_models
    mapping = mgr.class_mapping
    seen, collect = [], entry.DetectionEntry.collect_batch

    def recording(self, ticket):
        res = collect(self, ticket)
        seen.extend(res)
        return res

    monkeypatch.setattr(entry.DetectionEntry, "collect_batch", recording)
    annotate_video.reset_plate(mgr, det, 1)
    ref, filled = P.empty(H, W), 0
    for k, src in enumerate(footage[1]):
        bgr = np.ascontiguousarray(src[:, :, ::-1])                         # (the one-frame path takes B, G, R)
        frame = bgr.copy()
        img = shapes.InMemoryImage(data=frame, width=W, height=H)
        quiet(annotate_video.get_annotated_frame, mgr, det, frame, img, *RESIZE, draw=False, remove=REMOVE, frame_no=k + 1)
        assert len(seen) == k + 1
        want, from_plate, _ = plate_step(ref, bgr, seen[k][1], mapping, REMOVE)
        assert np.array_equal(frame, want), k
        filled += int(from_plate.sum())
    monkeypatch.setattr(entry.DetectionEntry, "collect_batch", collect)
    eng = annotate_video._engine(mgr, det, 1)
    assert np.array_equal(engine_state(eng, H, W, False), ref) and ref[0] == 6 and ref[1] > 0 and filled > 0
    state = eng.plate_state(H, W, False)
    annotate_video.reset_plate(mgr, det, 1)
    torch.cuda.synchronize()
    assert not state.cpu().numpy().any() and eng.plate_state(H, W, False) is state
    with pytest.raises(ValueError, match="remove settle=0"):
        annotate_video.get_annotated_frame(mgr, det, frame, None, *RESIZE, remove=("all", 0, 0, 0))
