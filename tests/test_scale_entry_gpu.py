"""out_size= through the detection entry and annotate_video: submit_batch(annotate=True, out_size=("size", W, H) | ("scale", N)) scales
every edited frame down inside the captured pass, behind the whole editing chain and in front of every encoder.  Every result is held
against tests/scale_ref.py applied to the bytes the SAME pass returns without the option -- byte for byte --, and the dets, the printed
lines and the tracks file are what they are without it."""
import io

import numpy as np
import pytest

from tests import scale_ref as S
from tests import y4m_cases as C
from tests import y4m_ref as Y
from tests.test_redact_entry_gpu import REDACT, RESIZE, engine, f32_models, frame_pixels, quiet, staged, submit      # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

H, W = 200, 330                                                              # ``staged``'s frames
TRACK = (30, 1, 1)
OPTIONS = [("scale", 2), ("size", 111, 67)]                                  # 100 x 165; a ragged ratio on both axes


def same_dets(a, b):
    return len(a) == len(b) and all(x["cls_name"] == y["cls_name"] and np.array_equal(x["bbox"], y["bbox"]) and x["prob"] == y["prob"]
                                    and x.get("track_id") == y.get("track_id") for x, y in zip(a, b))


@pytest.mark.parametrize("B", [1, 4])
def test_a_pass_returns_the_rule_applied_to_what_it_returns_without(engine, staged, B):
    plain = submit(engine, staged, B, redact=REDACT)
    assert any((out != src).any() for (_, _, out), src in zip(plain, staged[0]))      # the models fire: there is something to shrink
    for option in OPTIONS:
        h2, w2 = S.target(option, H, W)
        res = submit(engine, staged, B, redact=REDACT, out_size=option)
        assert len(res) == B
        for (n_rois, dets, out), (p_rois, p_dets, p_out) in zip(res, plain):
            assert out.shape == (h2, w2, 3) and out.dtype == np.uint8
            assert np.array_equal(out, S.downscale(p_out, h2, w2)), option
            assert n_rois == p_rois and same_dets(dets, p_dets)             # SOURCE coordinates, the same rows
        tail = ("scale",) + option
        assert any(k[-len(tail):] == tail and "annotate" in k for k in engine.cache.keys())


def test_device_encoders_take_the_scaled_frame(engine, staged):
    from PIL import Image as PilImage
    option = OPTIONS[1]
    h2, w2 = S.target(option, H, W)
    raw = submit(engine, staged, 4, out_size=option)
    for kw in (dict(encode="png"), dict(encode="png-huffman"), dict(encode="jpeg", quality=90),
               dict(encode="jpeg", quality=90, subsampling=420, huffman="optimized")):
        res = submit(engine, staged, 4, out_size=option, **kw)
        for (_, dets, data), (_, r_dets, r_out) in zip(res, raw):
            im = PilImage.open(io.BytesIO(data))
            assert im.size == (w2, h2), kw
            assert same_dets(dets, r_dets)
            if kw["encode"].startswith("png"):                              # (in-memory frames are uploaded BGR; the file is RGB)
                assert np.array_equal(np.asarray(im.convert("RGB"))[:, :, ::-1], r_out), kw
    for mode in (("444", "full"), ("420jpeg", "limited")):
        res = submit(engine, staged, 4, out_size=option, encode="y4m", y4m=mode)
        for (_, _, record), (_, _, r_out) in zip(res, raw):
            assert record == Y.encode(r_out, *mode, bgr=True), mode


def test_without_the_option_the_key_is_todays(engine, staged, f32_models):
    from faster_rcnn_amd import entry
    assert entry.PassSpec.checked(engine, 4, annotate=True).key_tail(4) == (4, "annotate")
    assert entry.PassSpec.checked(engine, 1, annotate=True, encode="png").key_tail(1) == ("annotate", "png")
    assert entry.PassSpec.checked(engine, 4, annotate=True, redact=REDACT).key_tail(4) == (4, "annotate", "redact") + REDACT
    assert entry.PassSpec.checked(engine, 4, annotate=True, redact=REDACT, out_size=("scale", 2)).key_tail(4) == \
        (4, "annotate", "redact") + REDACT + ("scale", "scale", 2)
    before = set(engine.cache.keys())
    submit(engine, staged, 1)
    geometry = engine.geometry_of(staged[3][0])
    assert geometry + ("annotate",) in engine.cache.keys()
    assert not any("scale" in k for k in set(engine.cache.keys()) - before)


def test_refusals_fire_before_any_capture(engine, staged):
    from faster_rcnn_amd._lib import FrcnnError
    srcs, resized, ratios, pixels = staged
    captures = engine.cache.captures
    one = lambda **kw: engine.submit_batch(resized[:1], ratios[:1], 0.0, pixels[:1], batch=1, **kw)
    with pytest.raises(FrcnnError, match="out_size= scales the frame an ANNOTATING pass returns: pass annotate=True"):
        one(out_size=("scale", 2))
    for bad, why in ((("size", W + 1, H), "larger than the 330x200 frame"), (("size", W, H + 1), "larger than the 330x200 frame"),
                     (("size", 20, H), "less than 1/16"), (("size", W, 12), "less than 1/16"), (("size", 0, 10), "at least 1"),
                     (("scale", 1), "2..16"), (("scale", 17), "2..16"), (("scale", 2.0), "out_size="), ("half", "out_size="),
                     (("size", 10), "out_size=")):
        with pytest.raises(FrcnnError, match=why):
            one(annotate=True, out_size=bad)
        with pytest.raises(FrcnnError, match=why):
            one(annotate=True, encode="png", out_size=bad)
    assert engine.cache.captures == captures


def test_a_lookback_pass_scales_what_it_emits(engine, staged):
    srcs, resized, ratios, pixels = staged
    option = OPTIONS[0]
    h2, w2 = S.target(option, H, W)

    def sequence(**kw):
        engine.track_reset()
        out = []
        two = lambda lo: engine.submit_batch(resized[lo:lo + 2], ratios[lo:lo + 2], 0.0, pixels[lo:lo + 2], batch=2, annotate=True, redact=REDACT,
                                             track=TRACK, track_lookback=2, **kw)
        out += engine.collect_batch(two(0))
        out += engine.collect_batch(two(2))
        out += engine.collect_batch(engine.submit_batch([], [], 0.0, [], batch=2, annotate=True, track=TRACK, track_lookback=2, **kw))
        engine.track_reset()
        return out
    plain, small = sequence(), sequence(out_size=option)
    assert len(plain) == len(small) == 4
    for (n_rois, dets, out), (p_rois, p_dets, p_out) in zip(small, plain):
        assert out.shape == (h2, w2, 3) and np.array_equal(out, S.downscale(p_out, h2, w2))
        assert n_rois == p_rois and same_dets(dets, p_dets)


def test_annotate_stream_writes_the_scaled_stream_and_the_same_lines(engine, f32_models):
    from faster_rcnn_amd import annotate_video, y4m
    mgr, det, _ = f32_models
    h, w, n = 96, 128, 5                                                     # a pass of four and a one-frame pass
    rgbs = [frame_pixels(h, w, 71)] * 3 + [frame_pixels(h, w, 72), frame_pixels(h, w, 71)]
    data = C.stream([Y.encode(f, "444", "full") for f in rgbs], h, w, "444", "full", tags="F25:1 Ip A1:1")

    def run(size, **kw):
        reader = y4m.Y4mReader(io.BytesIO(data), name="clip.y4m")
        sink, tracks = io.BytesIO(), io.StringIO()
        writer = y4m.Y4mWriter(sink, size[1], size[0], "444", "full", reader.plan.tags)
        _, printed = quiet(annotate_video.annotate_stream, mgr, det, reader, writer, *RESIZE, redact=REDACT, track=TRACK, tracks_out=tracks, **kw)
        return sink.getvalue(), tracks.getvalue(), printed

    plain, plain_tracks, plain_printed = run((h, w))
    option = ("scale", 2)
    small, small_tracks, small_printed = run((h // 2, w // 2), out_size=option)
    assert plain_tracks and small_tracks == plain_tracks and small_printed == plain_printed
    # the header carries the scaled size, and n records of it follow, each behind its "FRAME\n" (their bytes: the test above)
    head = C.stream([], h // 2, w // 2, "444", "full", tags="F25:1 Ip A1:1")
    record = 3 * (h // 2) * (w // 2)
    assert head.startswith(b"YUV4MPEG2 W64 H48 ") and small.startswith(head) and len(small) == len(head) + n * (6 + record)
    assert all(small[len(head) + k * (6 + record):][:6] == b"FRAME\n" for k in range(n))
    assert len(plain) == len(C.stream([], h, w, "444", "full", tags="F25:1 Ip A1:1")) + n * (6 + 3 * h * w)
    # a writer of the source size no longer fits, and a frame smaller than --out_size is named
    with pytest.raises(ValueError, match=r"clip.y4m.*scaled: 64x48.*128x96"):
        run((h, w), out_size=option)
    with pytest.raises(ValueError, match=r"clip.y4m.*\(128x96\).*larger than the 128x96 frame"):
        run((h, w), out_size=("size", 129, 96))
