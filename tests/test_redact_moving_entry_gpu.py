"""redact_moving= through the detection entry and the editing chain: submit_batch(annotate=True, redact_moving=...) runs the plate update,
ops.redact_moving_build and the region extension's prepare and apply inside the captured pass.  Every returned frame, the trailing dict and
the engine's moving state are held against the reference chain -- tests/plate_ref.py, then tests/redact_moving_ref.py -- applied to the
source frames and the rows the passes returned, byte for byte.  The sequence is generated: one noise frame that stands still, and blocks
that differ from it in frames 2 and 3; a pass without the option, next to it on the same engine, is what it was: bytes and key."""
import numpy as np
import pytest

from tests import plate_ref as P
from tests import redact_moving_ref as M
from tests.test_plate_entry_gpu import buffer_of, plate_step, table_of
from tests.test_redact_entry_gpu import RESIZE, engine, f32_models, frame_pixels, quiet      # noqa: F401  (the synthetic ResNet-50 pair)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

H, W = 200, 330
THRESHOLD = 0.9                                                             # few rows: every row blocks the plate
MOVING = dict(tol=24, vote=8, hold=1, grow=8, feather=4, mode="pixelate", size=8, settle=2, plate_tol=10, margin=1)
TRACK = (30, 2, 3)


@pytest.fixture(scope="module")
def sequence(engine):
    """Eight frames: the background three times, blocks in frames 3 and 4 (moved by 4 pixels), the background three times."""
    from faster_rcnn_amd import shapes, util
    back = frame_pixels(H, W, 300)
    rs = np.random.RandomState(5)
    srcs = []
    for f in range(8):
        a = back.copy()
        if f in (3, 4):
            for y, x in ((10, 20), (60, 250), (120, 100), (170, 290), (150, 8)):
                x += 4 * (f - 3)
                a[y:y + 24, x:x + 24] = rs.randint(0, 256, (24, 24, 3))
        srcs.append(a)
    imgs = [shapes.Image(shapes.Metadata("s%d" % i, W, H, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=RESIZE[0], max_size=RESIZE[1])
    return srcs, resized, ratios, [engine.host_pixels(r) for r in resized]


def submit(engine, seq, frames, B, **kw):
    srcs, resized, ratios, pixels = seq
    return engine.collect_batch(engine.submit_batch([resized[i] for i in frames], [ratios[i] for i in frames], THRESHOLD,
                                                    [pixels[i] for i in frames], batch=B, annotate=True, **kw))


def reference_step(plate, state, src, dets, mapping, option, remove=None, tracked=False):
    """One frame through the reference chain -> (the frame, the moving stats)."""
    D, K, Hd, G, F, unknown, classes, mode, size, S, T, Mg = option
    buf, rows = buffer_of(dets, mapping, tracked)
    if remove is None:
        P.update(plate, src, buf, rows, S, T, Mg)
        current = src.copy()
    else:
        current, _, _ = plate_step(plate, src, dets, mapping, remove, None, tracked)
    table = np.zeros(max(mapping.values()) + 1, dtype=np.uint8) if classes == () else table_of(mapping, classes)
    out = M.build(state, src, plate, buf, rows, table, Mg, D, K, Hd, G, F, ("show", "hide").index(unknown))
    return M.apply(current, src, out["W"], mode, size), out["stats"]


@pytest.mark.parametrize("leg", ["alone", "remove", "track"])
def test_a_captured_pass_is_the_reference_chain(engine, sequence, f32_models, leg):
    from faster_rcnn_amd import ops
    mapping = f32_models[0].class_mapping
    srcs = sequence[0]
    remove = ("all", 2, 10, 1) if leg == "remove" else None
    kw = {"remove": dict(remove=remove), "track": dict(track=TRACK)}.get(leg, {})
    option = engine.redact_moving_option(MOVING, remove)
    engine.plate_reset(), engine.moving_reset(), engine.track_reset()
    plate, state, hidden = P.empty(H, W), M.empty(H, W), 0
    for frames in ([0, 1, 2, 3], [4, 5, 6, 7], [7]):                        # (the last one padded: the padding is no frame)
        got = submit(engine, sequence, frames, 4, draw=False, redact_moving=MOVING, **kw)
        assert len(got) == len(frames)
        for f, (n_rois, dets, out, marks) in zip(frames, got):
            want, stats = reference_step(plate, state, srcs[f], dets, mapping, option, remove, leg == "track")
            assert np.array_equal(out, want), (leg, f, np.argwhere(out != want)[:4])
            assert marks["moving"] == {"cells": stats[1], "covered": stats[2]}, (leg, f)
            hidden += stats[2]
    torch.cuda.synchronize()
    frames_seen, cells_now, left = ops.redact_moving_left(engine.moving_state(H, W, False), H, W)
    assert (frames_seen, cells_now) == (9, state[1]) and np.array_equal(left, state[2])
    assert hidden > 0                                                       # (the net hid something: the leg is not vacuous)
    tail = ("moving",) + option
    assert any(k[-len(tail):] == tail and "nodraw" in k for k in engine.cache.keys())
    engine.track_reset()


def test_the_pass_without_the_option_is_untouched(engine, sequence):
    before = submit(engine, sequence, [0, 1, 2, 3], 4)
    keys_before = set(engine.cache.keys())
    captures = engine.cache.captures
    submit(engine, sequence, [0, 1, 2, 3], 4, redact_moving=True)
    new = set(engine.cache.keys()) - keys_before
    assert engine.cache.captures == captures + 1 and len(new) == 1
    key = new.pop()
    assert key[-13:-12] == ("moving",) and key[:-13] in keys_before and key[:-13][-1:] == ("annotate",)
    assert key[-12:] == (24, 8, 4, 8, 0, "show", (), "pixelate", 16, 8, 10, 8)
    captures = engine.cache.captures
    after = submit(engine, sequence, [0, 1, 2, 3], 4)
    assert engine.cache.captures == captures and set(engine.cache.keys()) == keys_before | {key}
    for a, b in zip(before, after):
        assert len(a) == len(b) == 3 and a[0] == b[0] and len(a[1]) == len(b[1]) and np.array_equal(a[2], b[2])


def test_submit_batch_refusals(engine, sequence):
    from faster_rcnn_amd._lib import FrcnnError
    srcs, resized, ratios, pixels = sequence
    captures = engine.cache.captures
    one = lambda **kw: engine.submit_batch(resized[:1], ratios[:1], 0.0, pixels[:1], batch=1, **kw)
    with pytest.raises(FrcnnError) as e:
        one(redact_moving=True)
    assert "annotate=True" in str(e.value)
    for bad in (dict(tol=300), dict(vote=0), dict(hold=-1), dict(grow=33), dict(feather=40), dict(unknown="perhaps"), dict(mode="smear"),
                dict(except_classes=("unicorn",)), dict(nonsense=1), (1, 2, 3), 5):
        with pytest.raises(FrcnnError) as e:
            one(annotate=True, redact_moving=bad)
        assert "redact_moving" in str(e.value)
    assert engine.cache.captures == captures


# ----------------------------------------------------------------------------------------------------------- annotate_video's entry points
NAMES = ["s%02d.png" % i for i in range(8)]


@pytest.fixture(scope="module")
def footage(sequence, tmp_path_factory):
    """The sequence as a directory of PNG files: file-backed frames are uploaded as the decoder delivers them (R, G, B)."""
    from PIL import Image as PilImage
    d_in = tmp_path_factory.mktemp("moving") / "in"
    d_in.mkdir()
    for name, rgb in zip(NAMES, sequence[0]):
        PilImage.fromarray(rgb).save(str(d_in / name))
    return d_in, sequence[0]


def annotate(f32_models, footage, d_out, monkeypatch, **kw):
    """``annotate_images`` over the footage -> (the results its passes returned, the printed text)."""
    from faster_rcnn_amd import annotate_video, entry
    mgr, det, _ = f32_models
    seen, collect = [], entry.DetectionEntry.collect_batch

    def recording(self, ticket):
        res = collect(self, ticket)
        seen.extend(res)
        return res

    monkeypatch.setattr(entry.DetectionEntry, "collect_batch", recording)
    try:
        _, text = quiet(annotate_video.annotate_images, mgr, det, str(footage[0]), str(d_out), NAMES, *RESIZE, png_encoder="host", draw=False,
                        det_threshold=THRESHOLD, **kw)
    finally:
        monkeypatch.setattr(entry.DetectionEntry, "collect_batch", collect)
    return seen, text


@pytest.mark.parametrize("kw", [dict(), dict(track=TRACK, track_lookback=2)], ids=["plain", "delayed"])
def test_annotate_images_csv_and_line_and_a_delayed_pass(engine, f32_models, footage, monkeypatch, tmp_path, kw):
    """annotate_images over the eight file-backed frames: the list starts from an empty state; with the look-back every pass returns the
    frames of the pass before it and the flush the rest, and the net ran on the frames as they were emitted: bytes, the trailing dict, the
    CSV and the printed line are the reference chain's."""
    from PIL import Image as PilImage
    mapping = f32_models[0].class_mapping
    srcs = footage[1]
    csv = tmp_path / "moving.csv"
    results, text = annotate(f32_models, footage, tmp_path / "out", monkeypatch, redact_moving=MOVING, moving_out=str(csv), **kw)
    assert len(results) == 8
    option = engine.redact_moving_option(MOVING)
    plate, state, rows, covered = P.empty(H, W), M.empty(H, W), ["frame,cells,covered"], []
    for f, (src, res) in enumerate(zip(srcs, results)):
        want, stats = reference_step(plate, state, src, res[1], mapping, option, None, "track" in kw)
        assert np.array_equal(res[2], want), (f, np.argwhere(res[2] != want)[:4])
        assert res[3]["moving"] == {"cells": stats[1], "covered": stats[2]}, f
        rows.append("%d,%d,%d" % (f + 1, stats[1], stats[2]))
        covered.append(stats[2])
        got = np.asarray(PilImage.open(str(tmp_path / "out" / NAMES[f])).convert("RGB"))
        assert np.array_equal(got, want), f
    assert sum(covered) > 0 and csv.read_text() == "\n".join(rows) + "\n"
    assert M.summary_line(W, H, covered) in text.splitlines()


def test_the_eager_path_gives_the_captured_bytes_and_continues_the_state(engine, sequence, f32_models):
    """draw_eager frame by frame on the dets the captured passes returned: the same bytes and the same counts, the state going on from
    call to call; get_annotated_frame continues its engine's state and reset_moving empties it."""
    from faster_rcnn_amd import annotate_video, ops, shapes
    mgr, det, _ = f32_models
    mapping = mgr.class_mapping
    srcs = sequence[0]
    engine.plate_reset(), engine.moving_reset()
    eager = annotate_video._eager_states(mapping)
    eager.reset_plate(), eager.reset_moving()
    hidden = 0
    for f in range(6):
        n_rois, dets, out, marks = submit(engine, sequence, [f], 1, draw=False, redact_moving=MOVING)[0]
        frame, info = srcs[f].copy(), {}
        plain = [{k: d[k] for k in ("bbox", "cls_name", "prob")} for d in dets]
        ret = annotate_video.draw_eager(frame, plain, mapping, draw=False, redact_moving=MOVING, info=info)
        assert ret is frame and np.array_equal(frame, out), f
        assert info["moving"] == marks["moving"], f
        hidden += marks["moving"]["covered"]
    assert hidden > 0
    # get_annotated_frame (its engine holds one pass in flight) continues that engine's state from call to call; reset_moving empties it
    eng1 = annotate_video._engine(mgr, det, 1)
    annotate_video.reset_moving(mgr, det)
    annotate_video.reset_plate(mgr, det)
    log = annotate_video.MovingLog(None)
    for k in (1, 2):
        frame = srcs[5 + k].copy()
        quiet(annotate_video.get_annotated_frame, mgr, det, frame, shapes.InMemoryImage(data=frame, width=W, height=H), *RESIZE, draw=False,
              redact_moving=MOVING, moving_out=log, det_threshold=THRESHOLD, frame_no=k)
        torch.cuda.synchronize()
        assert ops.redact_moving_left(eng1.moving_state(H, W, False), H, W)[0] == k
    assert list(log.per_size) == [(H, W)] and len(log.per_size[(H, W)]) == 2
    annotate_video.reset_moving(mgr, det)
    torch.cuda.synchronize()
    assert ops.redact_moving_left(eng1.moving_state(H, W, False), H, W)[0] == 0


def test_the_eager_list_writes_the_same_files_csv_and_line(engine, f32_models, footage, monkeypatch, tmp_path):
    """annotate_images on the eager path (no engine: one get_annotated_frame per frame, the log handed down) against the captured run of
    the same list: the same frames, the same CSV, the same line."""
    from faster_rcnn_amd import annotate_video, voc_dets
    runs = {}
    for fast in (True, False):
        csv, d_out = tmp_path / ("moving_%d.csv" % fast), tmp_path / ("out_%d" % fast)
        monkeypatch.setattr(voc_dets, "FAST_ENTRY", fast)
        try:
            _, text = annotate(f32_models, footage, d_out, monkeypatch, redact_moving=MOVING, moving_out=str(csv))
        finally:
            monkeypatch.setattr(voc_dets, "FAST_ENTRY", True)
        runs[fast] = (csv.read_text(), [l for l in text.splitlines() if l.startswith("moving net")], {n: (d_out / n).read_bytes() for n in NAMES})
    assert runs[True][0] == runs[False][0] and runs[True][0].count("\n") == 9
    assert runs[True][1] == runs[False][1] and len(runs[True][1]) == 1
    assert runs[True][2] == runs[False][2]
    assert any(int(row.split(",")[2]) > 0 for row in runs[True][0].splitlines()[1:])
