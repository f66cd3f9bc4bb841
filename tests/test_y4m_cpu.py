"""YUV4MPEG2 on the host: the header and its refusals, the reader (a pipe, FRAME tags, a cut frame) and the writer, the product's
numpy conversion against the contract (tests/y4m_ref.py), the contract's colour matrices against float64 BT.601 and against Pillow over
all 2^24 triples, and the command line's argument checks and stdout discipline."""
import contextlib
import io
import os
import threading

import numpy as np
import pytest

from tests import y4m_cases as C
from tests import y4m_ref as R


def test_header_round_trip_and_tags():
    from faster_rcnn_amd import ops, y4m
    for chroma in R.CHROMAS:
        for range_ in R.RANGES:
            line = y4m.header_line(33, 17, chroma, range_, {"F": "30000:1001", "A": "1:1"})
            plan = ops.y4m_parse_header(line + b"FRAME\n")
            assert (plan.w, plan.h, plan.chroma_name, plan.range_name) == (33, 17, chroma, range_)
            assert plan.frame_bytes == R.frame_bytes(17, 33, chroma) == ops.y4m_frame_bytes(17, 33, chroma)
            assert plan.tags == {"F": "30000:1001", "A": "1:1", "I": "p"} and plan.header_len == len(line)
    bare = ops.y4m_parse_header(b"YUV4MPEG2 W4 H2 C420\n")
    assert bare.chroma_name == "420jpeg" and bare.range_name == "limited" and bare.tags == {"F": "25:1", "A": "0:0", "I": "p"}
    assert ops.y4m_parse_header(b"YUV4MPEG2 W4 H2\n").chroma_name == "420jpeg"              # no C tag: the format's default
    assert ops.y4m_parse_header(b"YUV4MPEG2 H2 W4 XYSCSS=420JPEG XCOLORRANGE=FULL Ip\n").range_name == "full"


@pytest.mark.parametrize("header, reason", [
    (b"YUV4MPEG2 W4 H4 C420p10\n", "10 bits"), (b"YUV4MPEG2 W4 H4 C422p12\n", "12 bits"), (b"YUV4MPEG2 W4 H4 C444p16\n", "16 bits"),
    (b"YUV4MPEG2 W4 H4 It\n", "interlaced"), (b"YUV4MPEG2 W4 H4 Ib\n", "interlaced"), (b"YUV4MPEG2 W4 H4 Im\n", "interlaced"),
    (b"YUV4MPEG2 W4 H4 C420paldv\n", "C420paldv"), (b"YUV4MPEG2 W4 H4 C411\n", "C411"), (b"YUV4MPEG2 W4 H4 C444alpha\n", "C444alpha")])
def test_refusals_name_their_reason(header, reason):
    from faster_rcnn_amd import ops
    from faster_rcnn_amd._lib import FrcnnError
    assert issubclass(ops.Y4mUnsupported, FrcnnError)
    with pytest.raises(ops.Y4mUnsupported, match=reason):
        ops.y4m_parse_header(header)


@pytest.mark.parametrize("header", [b"", b"YUV4MPEG W4 H4\n", b"YUV4MPEG2 W4 H4", b"YUV4MPEG2 W4\n", b"YUV4MPEG2 W0 H4\n", b"YUV4MPEG2 Wx H4\n",
                                    b"YUV4MPEG2 W4 H4 F25\n", b"YUV4MPEG2 W4 H4 W5\n", b"YUV4MPEG2 W4 H4 Iq\n", b"YUV4MPEG2 W99999 H4\n"])
def test_broken_headers(header):
    from faster_rcnn_amd import ops
    from faster_rcnn_amd._lib import FrcnnError
    with pytest.raises(FrcnnError) as e:
        ops.y4m_parse_header(header)
    assert not isinstance(e.value, ops.Y4mUnsupported)


def test_reader_skips_frame_tags_and_names_a_short_frame():
    from faster_rcnn_amd import y4m
    from faster_rcnn_amd._lib import FrcnnError
    frames = [C.frame(5, 7, "420jpeg", seed=k) for k in range(3)]
    reader = y4m.Y4mReader(io.BytesIO(C.stream(frames, 5, 7, frame_tags=" Ip XNOTE=1")), name="clip.y4m")
    assert (reader.plan.h, reader.plan.w, reader.name) == (5, 7, "clip.y4m") and list(reader) == frames
    cut = C.stream(frames, 5, 7)[:-4]
    reader = y4m.Y4mReader(io.BytesIO(cut), name="clip.y4m")
    assert next(reader) == frames[0] and next(reader) == frames[1]
    with pytest.raises(FrcnnError, match="clip.y4m: frame 2 is cut short"):
        next(reader)
    with pytest.raises(FrcnnError, match="frame 0: no FRAME line"):
        next(y4m.Y4mReader(io.BytesIO(C.stream([], 5, 7) + b"JUNK\n")))


def test_reader_on_a_pipe_and_writer_round_trip():
    """A non-seekable pipe fed in small pieces by another thread: short reads are put together; what the writer wrote reads back."""
    from faster_rcnn_amd import y4m
    frames = [C.frame(48, 64, "444", seed=k) for k in range(4)]
    buf = io.BytesIO()
    w = y4m.Y4mWriter(buf, 64, 48, "444", "full", {"F": "30:1", "A": "1:1"})
    for f in frames:
        w.write(f)
    assert w.frames == 4
    with pytest.raises(Exception, match="frame 4 has 5 bytes"):
        w.write(b"short")
    data = buf.getvalue()
    rd, wr = os.pipe()

    def feed():
        with os.fdopen(wr, "wb", buffering=0) as f:
            for k in range(0, len(data), 1000):
                f.write(data[k:k + 1000])
    t = threading.Thread(target=feed)
    t.start()
    with os.fdopen(rd, "rb") as f:
        assert not f.seekable()
        reader = y4m.Y4mReader(f)
        got = list(reader)
    t.join()
    assert got == frames and reader.plan.range_name == "full" and reader.plan.tags["F"] == "30:1"


def test_host_conversion_equals_the_contract():
    """faster_rcnn_amd/y4m.py (whole-plane shifts) against tests/y4m_ref.py (index arrays), every mode, range and size; the sweep too."""
    from faster_rcnn_amd import y4m
    assert R.coefficients_from_reals() == ((R.DEC_Y, R.DEC_RV, R.DEC_GU, R.DEC_GV, R.DEC_BU), R.ENC_Y, R.ENC_CB, R.ENC_CR)
    for chroma in R.CHROMAS:
        for range_ in R.RANGES:
            for h, w in C.SIZES:
                data = C.frame(h, w, chroma)
                plan = y4m.make_plan(h, w, chroma, range_)
                for bgr in (False, True):
                    assert np.array_equal(y4m.decode_host(data, plan, bgr), R.decode(data, h, w, chroma, range_, bgr)), (chroma, range_, h, w)
    for range_ in R.RANGES:
        for y in C.SWEEP_Y:
            data = C.sweep_444(y)
            assert np.array_equal(y4m.decode_host(data, y4m.make_plan(256, 256, "444", range_)), R.decode(data, 256, 256, "444", range_))


def _triples(lo, hi):
    v = np.arange(256, dtype=np.int64)
    return np.meshgrid(np.arange(lo, hi, dtype=np.int64), v, v, indexing="ij")


def test_limited_range_against_float64_bt601():
    """All 2^24 (Y, Cb, Cr) triples through the decoder's matrix and all 2^24 (R, G, B) triples through the encoder's, against BT.601
    evaluated in float64 and rounded to nearest (clamped to 0..255).  The bound, 1 level, is derived: a fixed-point result is the
    rounding of (the real value + an error of at most 3 coefficients x 2^-17 x 255 < 0.003), so it can differ from the rounded real
    value only where the real value lies that close to a half, and then by one.
    Measured: maximum difference 1 on every channel; share of differing triples: decode R 0.005 %, G 0.038 %, B 0.009 %; encode Y
    0.054 %, Cb 0.194 %, Cr 0.055 %."""
    worst, differing = {}, {}
    for lo in range(0, 256, 32):
        a, b, c = _triples(lo, lo + 32)
        y, cb, cr = (a - 16) * (255 / 219), (b - 128) * (255 / 224), (c - 128) * (255 / 224)
        real = {"R": y + 2 * (1 - R.KR) * cr, "G": y - 2 * (1 - R.KB) * R.KB / R.KG * cb - 2 * (1 - R.KR) * R.KR / R.KG * cr,
                "B": y + 2 * (1 - R.KB) * cb}
        got = dict(zip("RGB", R.ycc_to_rgb(a, b, c, "limited")))
        luma = R.KR * a + R.KG * b + R.KB * c
        real.update({"Y": 16 + luma * (219 / 255), "Cb": 128 + (c - luma) / (2 * (1 - R.KB)) * (224 / 255),
                     "Cr": 128 + (a - luma) / (2 * (1 - R.KR)) * (224 / 255)})
        got.update(dict(zip(("Y", "Cb", "Cr"), R.rgb_to_ycc(a, b, c, "limited"))))
        for k in real:
            d = np.abs(got[k] - np.clip(np.floor(real[k] + 0.5), 0, 255).astype(np.int64))
            worst[k] = max(worst.get(k, 0), int(d.max()))
            differing[k] = differing.get(k, 0) + int((d > 0).sum())
    print("limited range against float64: max", worst, "differing share", {k: v / 2.0 ** 24 for k, v in differing.items()})
    assert max(worst.values()) <= 1, worst


def test_full_range_against_pillow():
    """The JFIF matrices (16 fractional bits) against Pillow's YCbCr <-> RGB (tables with 6 fractional bits, truncated) over all 2^24
    triples, both directions.  Ours is the rounding of the real value to within 0.003; Pillow's tables are each rounded to 1/64 and its
    sum is cut, not rounded, so its result lies within 1 of the real value on either side of ours: two integers within 0.51 and within
    1 of one real number differ by at most 1.  Measured: maximum difference 1 in both directions (70 % of the triples differ in some
    channel on decode, 85 % on encode)."""
    PilImage = pytest.importorskip("PIL.Image")
    worst = {}
    for lo in range(0, 256, 64):
        a, b, c = _triples(lo, lo + 64)
        packed = np.stack([a, b, c], axis=-1).astype(np.uint8).reshape(-1, 256, 3)
        size = (packed.shape[1], packed.shape[0])
        pil = np.asarray(PilImage.frombytes("YCbCr", size, packed.tobytes()).convert("RGB")).astype(np.int64)
        ours = np.stack(R.ycc_to_rgb(a, b, c, "full"), axis=-1).reshape(pil.shape)
        worst["decode"] = max(worst.get("decode", 0), int(np.abs(pil - ours).max()))
        pil = np.frombuffer(PilImage.frombytes("RGB", size, packed.tobytes()).convert("YCbCr").tobytes(), dtype=np.uint8)
        ours = np.stack(R.rgb_to_ycc(a, b, c, "full"), axis=-1).reshape(-1)
        worst["encode"] = max(worst.get("encode", 0), int(np.abs(pil.astype(np.int64) - ours).max()))
    print("full range against Pillow: max", worst)
    assert worst["decode"] <= 1 and worst["encode"] <= 1, worst


# ---------------------------------------------------------------------------------------------------------------- command line
def _args(*extra):
    from faster_rcnn_amd import annotate_video
    return annotate_video.build_parser().parse_args(["rpn.h5", "det.h5"] + list(extra))


def test_cli_argument_validation():
    from faster_rcnn_amd import annotate_video as av
    assert av.video_options(_args("frames")) == (False, None, "420jpeg")
    assert av.video_options(_args("clip.y4m")) == (True, None, "420jpeg")
    assert av.video_options(_args("-", "--out_video", "-", "--video_chroma", "444")) == (True, "-", "444")
    assert av.video_options(_args("frames", "--out_video", "out.y4m")) == (False, "out.y4m", "420jpeg")
    with pytest.raises(ValueError, match="needs --out_video"):
        av.video_options(_args("clip.y4m", "--video_chroma", "444"))
    for extra in (("--frame_format", "jpg"), ("--png_encoder", "device"), ("--frame_format", "jpg", "--jpeg_quality", "80")):
        with pytest.raises(ValueError, match="do not go with it"):
            av.video_options(_args("clip.y4m", "--out_video", "-", *extra))
    with pytest.raises(SystemExit):
        with contextlib.redirect_stderr(io.StringIO()):
            _args("clip.y4m", "--video_chroma", "422")


def test_cli_stdout_carries_only_the_stream(monkeypatch, capfdbinary):
    """``--out_video -`` through ``main`` with the models and the engine stubbed: stdout holds the y4m stream and nothing else, every
    printed line is on stderr; a frame of another size fails with a message that says so."""
    from faster_rcnn_amd import annotate_video as av
    from faster_rcnn_amd import resnet, y4m
    frames = [C.frame(6, 8, "420jpeg", seed=k) for k in range(3)]
    seen = {}

    def fake_stream(manager, detector, reader, sink, resize_min, resize_max, **kw):
        seen["sink"] = (sink.w, sink.h, sink.chroma, sink.range)
        for label, frame in av.stream_frames(reader):
            print("processing {}".format(label))
            print("num rois: 0")
            sink.write(frame.data)
        sink.flush()
    monkeypatch.setattr(av, "annotate_stream", fake_stream)
    for name in ("rpn_from_h5", "det_from_h5"):
        monkeypatch.setattr(resnet, name, lambda *a, **k: type("Stub", (), {"output": (0, 0, 0)})())
    src = C.stream(frames, 6, 8, tags="F30:1 Ip A4:3")
    rd, wr = os.pipe()
    os.write(wr, src)
    os.close(wr)
    import sys
    monkeypatch.setattr(sys, "stdin", io.TextIOWrapper(os.fdopen(rd, "rb")))
    av.main(["rpn.h5", "det.h5", "-", "--out_video", "-"])
    sys.stdout.flush()
    out, err = capfdbinary.readouterr()
    assert seen["sink"] == (8, 6, "420jpeg", "limited")
    assert out == y4m.header_line(8, 6, "420jpeg", "limited", {"F": "30:1", "A": "4:3"}) + b"".join(b"FRAME\n" + f for f in frames)
    assert err.decode().splitlines() == [line for k in range(3) for line in ("processing <stdin>#%d" % k, "num rois: 0")]


def test_one_stream_one_frame_size():
    """annotate_stream's size check (the part in front of any device work): a frame that is not the writer's size."""
    from faster_rcnn_amd import annotate_video as av
    from faster_rcnn_amd import y4m
    frame = av._Y4mFrame(C.frame(6, 8, "420jpeg"), y4m.make_plan(6, 8), "clip#0")
    assert frame.raw_size() == (6, 8) and frame.raw_rgb.shape == (6, 8, 3) and np.array_equal(frame.raw, frame.raw_rgb[:, :, ::-1])
    half, ratio = frame.resize_within_bounds(3, 4)
    assert (half.height, half.width, ratio) == (3, 4, 0.5) and half.raw_file() is frame.data and half.y4m_plan is frame.y4m_plan
