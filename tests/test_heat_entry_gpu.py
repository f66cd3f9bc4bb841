"""heat= through the detection entry and annotate_video: submit_batch(annotate=True, heat=(classes, A, S)) runs one ops.heat_update and
one ops.heat_draw_u8 per frame between the redaction and the trail draw, on the engine's heat state of the frame size.  Plain passes are
held against the same frames of a pass WITHOUT the option put through the two ops one by one; tracking passes against the restatements
applied to the rows the pass itself returned (tests/redact_ref.py, tests/heat_ref.py over the live rows in the order the frames came
out, then the drawing rule) -- byte for byte."""
import io

import numpy as np
import pytest

from tests import heat_ref as HR
from tests import redact_ref as R
from tests import track_ref as T
from tests.test_redact_entry_gpu import REDACT as PLAIN_REDACT, RESIZE, engine, f32_models, quiet, staged, submit      # noqa: F401
from tests.test_track_cut_entry_gpu import NAMES, annotate, footage      # noqa: F401  (six PNG frames of two scenes)
from tests.test_track_entry_gpu import split_dets
from tests.test_track_motion_entry_gpu import H, REDACT, W

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HEAT = (PLAIN_REDACT[0], 200, 2)             # every VOC class but one by name: a table that filters; a decay that rounds
ALL = ("all", 160, 0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def packed_of(dets, mapping):
    """The returned dets of a frame as a packed buffer (the heat rule does not depend on the order of the rows)."""
    return HR.make_packed(max(len(dets), 1), [[int(v) for v in d["bbox"]] for d in dets], cls=[mapping[d["cls_name"]] for d in dets])


def table_of(mapping, classes):
    t = np.zeros(max(mapping.values()) + 1, dtype=np.uint8)
    for name, idx in mapping.items():
        t[idx] = (name != "bg") if classes == "all" else (name in classes)
    return t


def through_the_ops(state, base, mapping, heat):
    """The frames of a pass without the option, heated one by one on ``state`` -> the frames."""
    from faster_rcnn_amd import ops
    classes, A, S = heat
    table, outs = dev(table_of(mapping, classes)), []
    for _, dets, out in base:
        h, w = out.shape[:2]
        ops.heat_update(state, h, w, dev(packed_of(dets, mapping)), table, S)
        outs.append(ops.heat_draw_u8(dev(out), state, A, rgb=False).cpu().numpy())      # (in-memory frames are uploaded B, G, R)
    return outs


def same_dets(a, b):
    return len(a) == len(b) and all(x["cls_name"] == y["cls_name"] and np.array_equal(x["bbox"], y["bbox"]) and x["prob"] == y["prob"]
                                    for x, y in zip(a, b))


def test_a_heat_pass_is_the_plain_pass_put_through_the_ops(engine, staged, f32_models):
    """draw=False, so the plain pass returns the very frame the heat is blended into.  Two submits of two frames, then a padded one of one
    frame: the state continues across them and a padding frame does not count; heat_reset() starts anew; track_reset() does not."""
    from PIL import Image as PilImage
    from faster_rcnn_amd import ops
    mapping = f32_models[0].class_mapping
    srcs, resized, ratios, pixels = staged
    h, w = srcs[0].shape[:2]
    groups = [(0, 2), (2, 4), (1, 2)]
    two = lambda lo, hi, **kw: engine.collect_batch(engine.submit_batch(resized[lo:hi], ratios[lo:hi], 0.0, pixels[lo:hi], batch=2, annotate=True,
                                                                        redact=PLAIN_REDACT, draw=False, **kw))
    base = [two(lo, hi) for lo, hi in groups]
    engine.heat_reset()
    state = ops.heat_state(h, w)
    for k, (lo, hi) in enumerate(groups):
        got = two(lo, hi, heat=HEAT)
        want = through_the_ops(state, base[k], mapping, HEAT)
        assert len(got) == hi - lo
        for f, ((n_rois, dets, out), (b_rois, b_dets, _)) in enumerate(zip(got, base[k])):
            assert n_rois == b_rois and same_dets(dets, b_dets)
            assert np.array_equal(out, want[f]), (k, f)
        torch.cuda.synchronize()
        assert np.array_equal(engine.heat_state(h, w).cpu().numpy()[:4 + h * w], state.cpu().numpy()[:4 + h * w]), k
    frames, peak, _, heat_map = ops.heat_map(state.cpu().numpy(), h, w)
    assert frames == 5 and peak > 256 and (heat_map > 0).any() and (want[0] != base[2][0][2]).any()
    # one encoder: the same frames as PNG files of the device encoder
    engine.heat_reset()
    state.zero_()
    got = two(0, 2, heat=HEAT, encode="png")
    want = through_the_ops(state, base[0], mapping, HEAT)
    for f, (_, _, data) in enumerate(got):
        assert np.array_equal(np.asarray(PilImage.open(io.BytesIO(data)).convert("RGB"))[:, :, ::-1], want[f]), f
    # track_reset() leaves the map, heat_reset() cools it, and the state is the same tensor
    engine.track_reset()
    torch.cuda.synchronize()
    assert int(engine.heat_state(h, w)[0]) == 2
    engine.heat_reset()
    torch.cuda.synchronize()
    assert not engine.heat_state(h, w).cpu().numpy().any()
    again = two(0, 2, heat=HEAT)
    state.zero_()
    for f, out in enumerate(through_the_ops(state, base[0], mapping, HEAT)):
        assert np.array_equal(again[f][2], out), f
    assert any(k[-4:] == ("heat",) + HEAT and "nodraw" in k for k in engine.cache.keys())


def test_in_flight_four_equals_in_flight_one(engine, staged, f32_models):
    """The map depends on the order of the frames: heat passes replay in submit order on one stream whatever ``in_flight`` is.  Four
    submits of one frame each are in flight at once on the engine of four; an engine of one gives the same bytes."""
    from faster_rcnn_amd import entry
    mgr, det, _ = f32_models
    srcs, resized, ratios, pixels = staged
    one = entry.for_models(mgr, det, 64, 16, in_flight=1)
    assert engine.in_flight == 4 and one.in_flight == 1 and one is not engine
    outs = []
    for eng in (engine, one):
        eng.heat_reset()
        px = [eng.host_pixels(r) for r in resized]
        tickets = [eng.submit_batch([resized[i]], [ratios[i]], 0.0, [px[i]], batch=1, annotate=True, heat=ALL) for i in range(4)]
        outs.append([eng.collect_batch(t)[0] for t in tickets])
        torch.cuda.synchronize()
        assert int(eng.heat_state(*srcs[0].shape[:2])[0]) == 4
    for f, (a, b) in enumerate(zip(*outs)):
        assert same_dets(a[1], b[1]) and np.array_equal(a[2], b[2]), f
    assert any((a[2] != s).any() for a, s in zip(outs[0], srcs))
    assert np.array_equal(engine.heat_state(*srcs[0].shape[:2]).cpu().numpy(), one.heat_state(*srcs[0].shape[:2]).cpu().numpy())


def live_buffer(live, mapping):
    """The live rows of a frame's returned dets as a tracked buffer (the rows the heat rule reads)."""
    rows = max(len(live), 1)
    return HR.make_tracked(rows, len(live), [[int(v) for v in d["bbox"]] for d in live], cls=[mapping[d["cls_name"]] for d in live])


def check_tracked_frames(engine, srcs, results, mapping, heat):
    """Every returned frame == redaction, then heat, then boxes, from the frame's own returned rows, in the order the frames came out."""
    classes, A, S = heat
    ref, table = HR.Heat(H, W), table_of(mapping, classes)
    for f, (src, res) in enumerate(zip(srcs, results)):
        dets, out = res[1], res[2]
        filled = [d for d in dets if d.get("backfilled")]
        live, held = split_dets([d for d in dets if not d.get("backfilled")])
        ref.update(live_buffer(live, mapping), table, S, tracked=True)      # (held and back-filled rows are guesses: they do not count)
        want = T.annotate(ref.draw(R.redact_dets(src, live + held + filled, mapping, *REDACT), A, rgb=True), live)      # (file-backed frames: R, G, B)
        assert np.array_equal(out, want), (f, np.argwhere(out != want)[:4])
    torch.cuda.synchronize()
    assert np.array_equal(engine.heat_state(H, W).cpu().numpy()[:4 + H * W], ref.words())
    return ref


@pytest.mark.parametrize("kw", [dict(), dict(track_lookback=2), dict(detect_every=2)], ids=["track", "lookback", "every"])
def test_tracking_passes_heat_the_live_rows_in_emitted_order(engine, f32_models, footage, monkeypatch, tmp_path, kw):
    """annotate_images over six file-backed frames (a pass of four and a padded one of two; with the look-back the pass of frames 4-5
    returns frames 0-3 and the flush the rest; with detect_every 2 the between frames' propagated rows count) and --heatmap_out."""
    from PIL import Image as PilImage
    mapping = f32_models[0].class_mapping
    out_png = tmp_path / "heat.png"
    results, text, lines, files = annotate(f32_models, footage, tmp_path / "out", monkeypatch, heatmap=ALL, heatmap_out=str(out_png), **kw)
    assert len(results) == 6
    ref = check_tracked_frames(engine, footage[1], results, mapping, ALL)
    assert ref.frames == 6 and ref.peak > 256
    for name, res in zip(NAMES, results):
        assert np.array_equal(np.asarray(PilImage.open(io.BytesIO(files[name])).convert("RGB")), res[2]), name
    with PilImage.open(str(out_png)) as im:
        assert im.mode == "L" and np.array_equal(np.asarray(im), ref.levels().astype(np.uint8))
    plain = annotate(f32_models, footage, tmp_path / "plain", monkeypatch, **kw)
    assert plain[1:3] == (text, lines) and any(files[n] != plain[3][n] for n in NAMES)
    assert any(k[-4:] == ("heat",) + ALL and "track" in k for k in engine.cache.keys())


def test_without_the_option_nothing_changes(engine, staged, f32_models):
    """The pass without the option before and after a pass with it: the same bytes, and no cache key but the new passes' own carries
    the tag, which goes behind everything else."""
    from faster_rcnn_amd import entry
    before = submit(engine, staged, 4, redact=PLAIN_REDACT)
    keys = set(engine.cache.keys())
    with_heat = submit(engine, staged, 4, redact=PLAIN_REDACT, heat=ALL)
    after = submit(engine, staged, 4, redact=PLAIN_REDACT)
    now = set(engine.cache.keys())
    tagged = {k for k in now if "heat" in k}
    assert tagged and now - tagged == keys - tagged and all(k[-4:] == ("heat",) + ALL for k in tagged if k not in keys)
    for a, b, c in zip(before, after, with_heat):
        assert np.array_equal(a[2], b[2]) and same_dets(a[1], b[1]) and same_dets(a[1], c[1])
    assert any((a[2] != c[2]).any() for a, c in zip(before, with_heat))
    spec = entry.PassSpec.checked(engine, 4, annotate=True, redact=PLAIN_REDACT)
    assert spec.heat is None and any(k[-len(spec.key_tail(4)):] == spec.key_tail(4) for k in keys)


def test_submit_batch_refusals(engine, staged):
    from faster_rcnn_amd._lib import FrcnnError
    srcs, resized, ratios, pixels = staged
    captures = engine.cache.captures
    two = lambda **kw: engine.submit_batch(resized[:2], ratios[:2], 0.0, pixels[:2], batch=2, **kw)
    with pytest.raises(FrcnnError, match=r"heat= blends the heat map into the frame an ANNOTATING pass returns: pass annotate=True"):
        two(heat=ALL)
    for bad in (("all", 0, 0), ("all", 256, 0), ("all", 160, 16), ("all", 160, -1), (("tram",), 160, 0), ((), 160, 0), "all", ("all", 160),
                ("all", True, 0), ("all", 160.0, 0)):
        with pytest.raises(FrcnnError, match="submit_batch: heat="):
            two(annotate=True, heat=bad)
    device = engine.device_preprocess
    engine.device_preprocess = False
    try:
        with pytest.raises(FrcnnError, match=r"heat= needs the device-side preprocess"):
            two(annotate=True, heat=ALL)
    finally:
        engine.device_preprocess = device
    assert engine.cache.captures == captures


def test_the_eager_path_heats_one_frame_at_a_time():
    """draw_eager (foreign models): one-frame calls on a state of its own per class mapping and frame size; a frame without detections
    is blended too, and with draw=False the frame is the restatement's."""
    from faster_rcnn_amd import annotate_video as av, ops
    from faster_rcnn_amd.data.voc_data_helpers import VOC_CLASS_MAPPING as mapping
    h, w = 37, 90
    state = ops.heat_reset(av._eager_heat_state(mapping, h, w))
    ref, table = HR.Heat(h, w), table_of(mapping, HEAT[0])
    det = lambda box, name: {"bbox": np.array(box, dtype=np.int64), "cls_name": name, "prob": np.float32(0.9)}
    frames_dets = [[det([5, 3, 40, 20], "person")], [det([15, 3, 50, 22], "person"), det([60, 10, 120, 30], "car"), det([0, 0, 89, 36], "aeroplane")], []]
    for f, dets in enumerate(frames_dets):
        src = np.random.RandomState(40 + f).randint(0, 256, (h, w, 3)).astype(np.uint8)
        frame = src.copy()
        av.draw_eager(frame, list(dets), mapping, draw=False, heatmap=HEAT)
        ref.update(packed_of(dets, mapping), table, HEAT[2])
        assert np.array_equal(frame, ref.draw(src, HEAT[1], rgb=False)), f
        assert (frame != src).any()
    assert np.array_equal(state.cpu().numpy()[:4 + h * w], ref.words()) and ref.frames == 3
    assert av._eager_heat_state(mapping, h, w) is state and av._eager_heat_state(mapping, h, w + 1) is not state
