"""The device JPEG encoder inside the detection entry's annotating passes (entry.DetectionEntry.submit_batch(annotate=True, encode="jpeg",
quality=q)) and behind ``annotate_video --frame_format jpg``: the files are ops.jpeg_bytes of the frames the raw annotating pass returns,
a file longer than the first read-back comes back whole, every quality is a pass of its own beside the PNG passes, and the command line
writes <stem>.jpg files and prints what the PNG run prints."""
import io
import os

import numpy as np
import pytest

from tests import jpeg_ref as R
from tests.test_jpeg_cpu import PSNR_DEFICIT_MARGIN_DB, PSNR_SURPLUS_MARGIN_DB, psnr
from tests.test_png_entry_gpu import B, _named, f32_models, frame_pixels, quiet, same_dets      # noqa: F401  (the small f32 models)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
PilImage = pytest.importorskip("PIL.Image")


def _engine(f32_models):
    from faster_rcnn_amd import entry
    mgr, det, _ = f32_models
    return entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight("f32"))


@pytest.mark.parametrize("count", [1, 3])
def test_jpeg_encoding_passes(f32_models, tmp_path, monkeypatch, count):
    """200x330 frames in memory (BGR) and as files (uploaded RGB), one frame in a one-frame pass and three in a padded pass of four: the
    JPEG pass returns the dets of the raw annotating pass and, per frame, ops.jpeg_bytes of the frame that pass returns."""
    from faster_rcnn_amd import ops, util, voc_dets
    monkeypatch.setattr(voc_dets, "CAPTURE_MIN", 1)
    eng = _engine(f32_models)
    assert eng.batch == B
    take, quality = (1 if count == 1 else B), 90
    srcs = [frame_pixels(200, 330, 300 + i) for i in range(count)]
    mem = [_named("m%d" % i, pixels=s) for i, s in enumerate(srcs)]
    files = []
    for i, s in enumerate(srcs):
        p = str(tmp_path / ("f%d.png" % i))
        PilImage.fromarray(s[:, :, ::-1]).save(p)
        files.append(_named("f%d" % i, path=p, size=s.shape[:2]))
    for kind, imgs in (("mem", mem), ("file", files)):
        resized, ratios = util.resize_imgs(imgs, min_size=320, max_size=540)
        pixels = [eng.host_pixels(r) for r in resized]
        raw = eng.collect_batch(eng.submit_batch(resized, ratios, 0.0, pixels, batch=take, annotate=True))
        jpg = eng.collect_batch(eng.submit_batch(resized, ratios, 0.0, pixels, batch=take, annotate=True, encode="jpeg", quality=quality))
        again = eng.collect_batch(eng.submit_batch(resized, ratios, 0.0, pixels, batch=take, annotate=True, encode="jpeg", quality=quality))
        assert len(raw) == len(jpg) == count and all(len(r) == 3 for r in jpg)
        for (n0, d0, frame), (n1, d1, data), (_, _, data2) in zip(raw, jpg, again):
            assert n0 == n1
            same_dets(d1, d0, tol=0.0)
            assert isinstance(data, bytes) and 0 < len(data) <= ops.jpeg_bound(*frame.shape[:2]) and data == data2
            assert data == ops.jpeg_bytes(torch.from_numpy(frame).cuda(), quality=quality, bgr=kind == "mem")
            assert data == R.encode(frame, quality, bgr=kind == "mem")
            img = PilImage.open(io.BytesIO(data))
            assert img.mode == "RGB" and img.size == (frame.shape[1], frame.shape[0])


def test_long_file_comes_back_through_the_second_copy(f32_models, monkeypatch):
    """A 64x136 noise frame, annotated, at quality 100 encodes to more bytes than the first read-back holds: collect_batch fetches the
    rest, and the file is whole."""
    from faster_rcnn_amd import ops, util, voc_dets
    monkeypatch.setattr(voc_dets, "CAPTURE_MIN", 1)
    eng = _engine(f32_models)
    src = frame_pixels(64, 136, 7)
    resized, ratios = util.resize_imgs([_named("n", pixels=src)], min_size=320, max_size=700)      # (the pass encodes the SOURCE frame)
    pixels = [eng.host_pixels(resized[0])]
    (_, _, frame), = eng.collect_batch(eng.submit_batch(resized, ratios, 0.0, pixels, batch=1, annotate=True))
    ticket = eng.submit_batch(resized, ratios, 0.0, pixels, batch=1, annotate=True, encode="jpeg", quality=100)
    first_copy = ticket.slot.first_copy
    (_, _, data), = eng.collect_batch(ticket)
    assert first_copy == 16 + ops.jpeg_header_bytes() + src.nbytes // 4
    # (the frame that is encoded carries the drawn boxes and labels, flat patches over the noise: its file is shorter than bare noise's
    # 36 361 bytes, and still far past the first copy)
    assert 16 + len(data) > first_copy, (len(data), first_copy)
    assert (frame != src).any()
    assert data == ops.jpeg_bytes(torch.from_numpy(frame).cuda(), quality=100, bgr=True) == R.encode(frame, 100, bgr=True)
    (_, _, small), = eng.collect_batch(eng.submit_batch(resized, ratios, 0.0, pixels, batch=1, annotate=True, encode="jpeg", quality=10))
    assert 16 + len(small) <= first_copy and small == R.encode(frame, 10, bgr=True)


def test_cache_keys_and_refused_arguments(f32_models, monkeypatch):
    """Two qualities are two passes; the PNG passes keep their keys; encode="jpeg" without annotate, a quality with another encode, and a
    quality outside 1..100 raise before anything is captured."""
    from faster_rcnn_amd import util, voc_dets
    from faster_rcnn_amd._lib import FrcnnError
    monkeypatch.setattr(voc_dets, "CAPTURE_MIN", 1)
    eng = _engine(f32_models)
    resized, ratios = util.resize_imgs([_named("x", pixels=frame_pixels(180, 300, 1))], min_size=320, max_size=540)
    pixels = [eng.host_pixels(resized[0])]
    run = lambda **kw: eng.collect_batch(eng.submit_batch(resized, ratios, 0.0, pixels, batch=1, annotate=True, **kw))[0][2]
    geometry = eng.geometry_of(pixels[0])
    png = run(encode="png")
    keys_before = set(eng.cache.keys())
    assert geometry + ("annotate", "png") in keys_before
    captures = eng.cache.captures
    a, b = run(encode="jpeg", quality=90), run(encode="jpeg", quality=60)
    assert eng.cache.captures == captures + 2 and len(b) < len(a)
    assert run(encode="jpeg", quality=90) == a and run(encode="png") == png and eng.cache.captures == captures + 2
    keys = set(eng.cache.keys())
    assert keys - keys_before == {geometry + ("annotate", "jpeg", 90), geometry + ("annotate", "jpeg", 60)} and keys_before <= keys
    for kw in (dict(encode="jpeg", quality=90), dict(annotate=True, encode="png", quality=90), dict(annotate=True, quality=90),
               dict(annotate=True, encode="png-huffman", quality=90), dict(annotate=True, encode="jpeg", quality=0),
               dict(annotate=True, encode="jpeg", quality=101), dict(annotate=True, encode="jpeg")):
        with pytest.raises(FrcnnError):
            eng.submit_batch(resized, ratios, 0.0, pixels, batch=1, **kw)
    assert eng.cache.captures == captures + 2


def test_main_frame_format_jpg(f32_models, tmp_path):
    """``annotate_video --frame_format jpg`` with both encoders against the PNG run on three small PNG files: the same printed lines,
    <stem>.jpg names; the device files are ops.jpeg_bytes of the PNG run's frames, the host files decode as close to those frames."""
    from faster_rcnn_amd import annotate_video, ops
    from faster_rcnn_amd.weights import save_npz
    _, _, w = f32_models
    npz = str(tmp_path / "w.npz")
    save_npz(npz, w)
    d_in = tmp_path / "frames"
    d_in.mkdir()
    names = ["%06d.png" % i for i in range(3)]
    y, x = np.mgrid[0:180, 0:260]
    for i, name in enumerate(names):                                        # smooth frames with a little noise
        f = np.stack([x // 2 + y // 3 + 9 * i, 200 - y + x // 5, (x + 2 * y) // 3], -1) + frame_pixels(180, 260, 40 + i) % 5
        PilImage.fromarray((f % 256).astype(np.uint8)).save(str(d_in / name))
    text, flags = {}, {"png": [], "host": ["--frame_format", "jpg", "--jpeg_quality", "85"],
                       "device": ["--frame_format", "jpg", "--jpeg_encoder", "device", "--jpeg_quality", "85"]}
    for leg, extra in flags.items():
        argv = [npz, npz, str(d_in), "--resize_dims", "320,540", "--out_dir", str(tmp_path / leg)] + extra
        _, text[leg] = quiet(annotate_video.main, argv)
        assert sorted(os.listdir(str(tmp_path / leg))) == (names if leg == "png" else [n[:-4] + ".jpg" for n in names])
    assert text["png"] == text["host"] == text["device"] and "{'bbox'" in text["png"]
    for name in names:
        frame = np.asarray(PilImage.open(str(tmp_path / "png" / name)).convert("RGB"))        # the annotated frame, lossless
        data = open(str(tmp_path / "device" / (name[:-4] + ".jpg")), "rb").read()
        assert data == ops.jpeg_bytes(torch.from_numpy(frame).cuda(), quality=85) == R.encode(frame, 85)
        dev = PilImage.open(io.BytesIO(data))
        host = PilImage.open(str(tmp_path / "host" / (name[:-4] + ".jpg")))
        assert dev.mode == host.mode == "RGB" and dev.size == host.size == (260, 180)
        p_dev, p_host = psnr(np.asarray(dev), frame), psnr(np.asarray(host), frame)
        assert -PSNR_SURPLUS_MARGIN_DB <= p_host - p_dev <= PSNR_DEFICIT_MARGIN_DB, (name, p_dev, p_host)
    # the eager path of annotate_images (no captured entry): the same files
    import faster_rcnn_amd.voc_dets as voc_dets
    old = voc_dets.FAST_ENTRY
    voc_dets.FAST_ENTRY = False
    try:
        argv = [npz, npz, str(d_in), "--resize_dims", "320,540", "--out_dir", str(tmp_path / "eager"), "--frame_format", "jpg",
                "--jpeg_encoder", "device", "--jpeg_quality", "85"]
        quiet(annotate_video.main, argv)
    finally:
        voc_dets.FAST_ENTRY = old
    for name in names:
        jpg = name[:-4] + ".jpg"
        img = PilImage.open(str(tmp_path / "eager" / jpg))
        assert img.mode == "RGB" and img.size == (260, 180)
