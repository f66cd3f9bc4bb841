"""YUV4MPEG2 streams through the detection entry (annotate_video.annotate_stream; entry.Y4mFile items, submit_batch(encode="y4m")):
the device converts exactly as tests/y4m_ref.py states, so a stream must come out as the SAME frames the existing file path gives when
it is fed the restatement's conversion of the input and its output is converted by the restatement's encoder -- byte for byte, with the
same printed lines."""
import io
import os

import numpy as np
import pytest

from tests import png_dec_cases as P
from tests import y4m_cases as C
from tests import y4m_ref as R
from tests.test_png_entry_gpu import f32_models, quiet      # noqa: F401  (the small f32 models)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
PilImage = pytest.importorskip("PIL.Image")

H, W, N = 96, 128, 5                                          # five frames at four per pass: one full pass and a short group
RESIZE = (320, 540)


@pytest.fixture(scope="module")
def clip():
    """The input stream (4:2:0, limited range) and the restatement's view of its frames (RGB)."""
    frames = [R.encode(np.ascontiguousarray(P.photo()[3 * k:3 * k + H, 2 * k:2 * k + W]), "420jpeg", "limited") for k in range(N)]
    return C.stream(frames, H, W, tags="F30:1 Ip A1:1"), [R.decode(f, H, W, "420jpeg", "limited") for f in frames]


@pytest.fixture(scope="module")
def by_files(f32_models, clip, tmp_path_factory):
    """The reference run: the restatement's frames saved as PNGs through the existing ``annotate_images`` with host codecs -> (the input
    directory, its file names, the printed lines, the annotated frames as RGB arrays)."""
    from faster_rcnn_amd import annotate_video
    mgr, det, _ = f32_models
    root = tmp_path_factory.mktemp("y4m_by_files")
    d_in, d_out = root / "in", root / "out"
    d_in.mkdir()
    names = ["%06d.png" % k for k in range(N)]
    for name, rgb in zip(names, clip[1]):
        PilImage.fromarray(rgb).save(str(d_in / name))
    _, text = quiet(annotate_video.annotate_images, mgr, det, str(d_in), str(d_out), names, *RESIZE)
    return str(d_in), names, text, [np.asarray(PilImage.open(str(d_out / name)).convert("RGB")) for name in names]


def _lines(text, labels):
    """The printed lines with each "processing <label>" checked and taken out: what is left must be equal between two runs."""
    lines = text.splitlines()
    assert [x for x in lines if x.startswith("processing ")] == ["processing " + x for x in labels]
    return [x for x in lines if not x.startswith("processing ")]


def _run_stream(models, data, chroma="420jpeg", name="clip.y4m"):
    from faster_rcnn_amd import annotate_video, y4m
    mgr, det, _ = models
    reader = y4m.Y4mReader(io.BytesIO(data), name=name)
    out = io.BytesIO()
    writer = y4m.Y4mWriter(out, reader.plan.w, reader.plan.h, chroma, reader.plan.range_name, reader.plan.tags)
    _, text = quiet(annotate_video.annotate_stream, mgr, det, reader, writer, *RESIZE)
    return out.getvalue(), text


def _expected(frames_rgb, chroma="420jpeg", range_="limited", tags="F30:1 Ip A1:1"):
    return C.stream([R.encode(f, chroma, range_) for f in frames_rgb], H, W, chroma, range_, tags=tags)


def test_stream_to_stream_equals_the_file_path(f32_models, clip, by_files):
    from faster_rcnn_amd import entry
    d_in, names, text, annotated = by_files
    got, said = _run_stream(f32_models, clip[0])
    assert got == _expected(annotated)
    assert any((a != b).any() for a, b in zip(annotated, clip[1])), "nothing was drawn: the comparison would show nothing"
    labels = ["clip.y4m#%d" % k for k in range(N)]
    assert _lines(said, labels) == _lines(text, [os.path.join(d_in, n) for n in names]) and "{'bbox'" in said
    mgr, det, _ = f32_models
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight("f32"))
    slots = [sl for v in eng.cache._slots.values() for sl in v if sl.y4m_items is not None and len(sl.y4m_items)]
    assert slots and all(sl.encode == "y4m" and sl.y4m_mode == ("420jpeg", "limited") for sl in slots)
    assert {len(sl.y4m_items) for sl in slots} == {4, 1}                        # the pass of four, the one-frame pass of the short group
    assert any(k[-4:] == ("annotate", "y4m", "420jpeg", "limited") for k in eng.cache.keys())
    # a captured replay: the same stream again, the same bytes, nothing captured anew
    captures = eng.cache.captures
    again, _ = _run_stream(f32_models, clip[0])
    assert again == got and eng.cache.captures == captures
    # 4:4:4 output: a pass of its own
    got444, _ = _run_stream(f32_models, clip[0], chroma="444")
    assert got444 == _expected(annotated, chroma="444")


def test_stream_to_png_files_on_the_device(f32_models, clip, by_files, tmp_path):
    """y4m in, frame files out through the device PNG encoder: the files ``annotate_images --png_encoder device`` writes for the PNG
    frames, byte for byte, under the names frame_%06d.png."""
    from faster_rcnn_amd import annotate_video, y4m
    mgr, det, _ = f32_models
    d_in, names, _, _ = by_files
    quiet(annotate_video.annotate_images, mgr, det, d_in, str(tmp_path / "files"), names, *RESIZE, png_encoder="device")
    reader = y4m.Y4mReader(io.BytesIO(clip[0]), name="clip.y4m")
    quiet(annotate_video.annotate_stream, mgr, det, reader, str(tmp_path / "stream"), *RESIZE, png_encoder="device")
    assert sorted(os.listdir(str(tmp_path / "stream"))) == ["frame_%06d.png" % k for k in range(N)]
    for k, name in enumerate(names):
        with open(str(tmp_path / "files" / name), "rb") as a, open(str(tmp_path / "stream" / ("frame_%06d.png" % k)), "rb") as b:
            assert a.read() == b.read(), k


def test_png_directory_to_stream(f32_models, clip, by_files, tmp_path):
    """A PNG directory of one size in, a stream out: the same stream; a frame of another size fails and says why."""
    from faster_rcnn_amd import annotate_video, y4m
    mgr, det, _ = f32_models
    d_in, names, text, annotated = by_files
    out = io.BytesIO()
    writer = y4m.Y4mWriter(out, W, H, "420jpeg", "limited", {"F": "25:1"})
    _, said = quiet(annotate_video.annotate_stream, mgr, det, annotate_video.directory_frames(d_in, names), writer, *RESIZE)
    assert out.getvalue() == _expected(annotated, tags="F25:1 Ip A0:0")
    assert said == text
    odd = tmp_path / "odd"
    odd.mkdir()
    PilImage.fromarray(clip[1][0]).save(str(odd / "a.png"))
    PilImage.fromarray(clip[1][0][:, :100]).save(str(odd / "b.png"))
    writer = y4m.Y4mWriter(io.BytesIO(), W, H)
    with pytest.raises(ValueError, match="b.png is 100x96, the output stream's frames are 128x96"):
        quiet(annotate_video.annotate_stream, mgr, det, annotate_video.directory_frames(str(odd), ["a.png", "b.png"]), writer, *RESIZE)


def test_one_frame_stream_and_other_input_modes(f32_models, clip, by_files):
    """A stream of one frame; and a full-range 4:4:4 input stream, whose frames the pass must convert as the restatement does: its
    detections are those of the restatement's pixels."""
    from faster_rcnn_amd import annotate_video, y4m
    mgr, det, _ = f32_models
    _, _, _, annotated = by_files
    one = C.stream([clip[0].split(b"FRAME\n")[1]], H, W, tags="F30:1 Ip A1:1")
    got, _ = _run_stream(f32_models, one)
    assert got == _expected(annotated[:1])
    # full range, 4:4:4: against the file path fed the restatement's pixels
    src = R.encode(clip[1][1], "444", "full")
    rgb = R.decode(src, H, W, "444", "full")
    got, said = _run_stream(f32_models, C.stream([src], H, W, "444", "full"), chroma="444", name="full.y4m")
    frame = annotate_video._Frame(rgb)
    resized, ratio = frame.resize_within_bounds(*RESIZE)
    from faster_rcnn_amd import entry
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight("f32"))
    (_, _, drawn), = eng.collect_batch(eng.submit_batch([resized], [ratio], 0.0, [eng.host_pixels(resized)], batch=1, annotate=True))
    assert got == C.stream([R.encode(drawn, "444", "full")], H, W, "444", "full")


def test_submit_batch_checks_the_y4m_arguments(f32_models, clip):
    from faster_rcnn_amd import annotate_video, entry
    from faster_rcnn_amd._lib import FrcnnError
    mgr, det, _ = f32_models
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight("f32"))
    resized, ratio = annotate_video._Frame(clip[1][0]).resize_within_bounds(*RESIZE)
    pixels = [eng.host_pixels(resized)]
    captures = eng.cache.captures
    for kw in (dict(encode="y4m"), dict(annotate=True, encode="y4m", y4m=("422", "limited")), dict(annotate=True, encode="y4m", y4m=("444", "tv")),
               dict(annotate=True, encode="png", y4m=("444", "full")), dict(annotate=True, encode="y4m", quality=90)):
        with pytest.raises(FrcnnError):
            eng.submit_batch([resized], [ratio], 0.0, pixels, batch=1, **kw)
    assert eng.cache.captures == captures
