"""The device PNG decoder behind the entry points (entry.set_png_decoder / FRCNN_ENTRY_PNG_DECODER, annotate_images(png_decoder=...)): the
pixels are Pillow's, so detections, printed lines and output files must be IDENTICAL to the host decoder's; a file outside the supported
set rides in the same passes host-decoded; a pass may mix .jpg and .png files; a damaged file raises FrcnnError naming it."""
import os

import numpy as np
import pytest

from tests import png_dec_cases as C
from tests.test_jpeg_dec_entry_gpu import _image, _same
from tests.test_png_entry_gpu import _by_image, f32_models, quiet      # noqa: F401  (the small f32 models)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
PilImage = pytest.importorskip("PIL.Image")


def _crop(k, h, w):
    return np.ascontiguousarray(C.photo()[2 * k:2 * k + h, k:k + w])


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return path


def _engine(f32_models):
    from faster_rcnn_amd import entry
    mgr, det, _ = f32_models
    return entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight("f32"))


def _decoded_png_slots(eng):
    return [sl for slots in eng.cache._slots.values() for sl in slots if sl.png_items is not None and len(sl.png_items)]


def test_annotate_images_device_decoder_equals_host(f32_models, tmp_path):
    """Six small frames: two sizes, one RGBA, one palette file (the planner refuses it: PIL, inside the same run).  The same printed
    lines, byte-identical output files, and the device leg really decoded (its passes hold PNG items)."""
    from faster_rcnn_amd import annotate_video, entry
    mgr, det, _ = f32_models
    d_in = tmp_path / "frames"
    d_in.mkdir()
    names = ["%06d.png" % i for i in range(6)]
    for i, name in enumerate(names):
        frame = _crop(i, 180, 260) if i < 4 else _crop(i, 200, 300)
        if i == 1:
            frame = np.dstack([frame, np.full(frame.shape[:2], 128 + i, np.uint8)])
        if i == 2:
            PilImage.fromarray(frame).convert("P", palette=PilImage.ADAPTIVE).save(str(d_in / name))
        else:
            _write(str(d_in / name), C.pil_file(frame, compress_level=6))
    text = {}
    try:
        for decoder in ("host", "device"):
            _, text[decoder] = quiet(annotate_video.annotate_images, mgr, det, str(d_in), str(tmp_path / decoder), names, 320, 540,
                                     png_decoder=decoder)
            assert sorted(os.listdir(str(tmp_path / decoder))) == names
            assert bool(_decoded_png_slots(_engine(f32_models))) == (decoder == "device")
    finally:
        entry.set_png_decoder(None)
    assert text["host"] == text["device"] and "{'bbox'" in text["host"]
    for name in names:
        with open(str(tmp_path / "host" / name), "rb") as a, open(str(tmp_path / "device" / name), "rb") as b:
            assert a.read() == b.read(), name


def _dets(f32_models, images, png, jpeg, monkeypatch):
    from faster_rcnn_amd import entry, util, voc_dets
    monkeypatch.setattr(voc_dets, "CAPTURE_MIN", 1)
    mgr, det, _ = f32_models
    resized, ratios = util.resize_imgs(images, min_size=320, max_size=540)
    entry.set_png_decoder(png)
    entry.set_jpeg_decoder(jpeg)
    try:
        by_cls, _ = quiet(voc_dets.get_dets_by_cls, mgr, det, ratios, resized, det_threshold=0.1)
    finally:
        entry.set_png_decoder(None)
        entry.set_jpeg_decoder(None)
    return _by_image(by_cls)


SIZES = ((200, 330), (204, 330), (200, 326), (208, 334), (196, 322), (204, 326), (200, 330))


def _png_list(tmp_path, extra=()):
    images = []
    for k, (h, w) in enumerate(SIZES):
        frame = _crop(k, h, w)
        data = C.pil_file(np.dstack([frame, frame[:, :, 0]]) if k == 2 else frame, compress_level=1 if k % 2 else 6)
        images.append(_image("crop%d" % k, _write(str(tmp_path / ("crop%d.png" % k)), data)))
    for name, data in extra:
        images.append(_image(name.split(".")[0], _write(str(tmp_path / name), data)))
    return images


def test_canvas_passes_with_mixed_sizes(f32_models, tmp_path, monkeypatch):
    """More sizes than CANVAS_MIN_GEOMETRIES: canvas passes form, their slots hold PNG items with ``device``, the detections are equal."""
    from faster_rcnn_amd import entry
    images = _png_list(tmp_path)
    assert len(set(SIZES)) > entry.CANVAS_MIN_GEOMETRIES
    host = _dets(f32_models, images, "host", "host", monkeypatch)
    dev = _dets(f32_models, images, "device", "host", monkeypatch)
    _same(dev, host)
    eng = _engine(f32_models)
    assert eng.canvas and any(sl.canvas for sl in _decoded_png_slots(eng))
    entry.set_png_decoder("device")
    try:
        assert isinstance(eng.host_pixels(images[0])[0], entry.PngFile)
    finally:
        entry.set_png_decoder(None)
    assert isinstance(eng.host_pixels(images[0])[0], np.ndarray)          # every option unset: today's path


def test_a_pass_mixing_jpg_and_png(f32_models, tmp_path, monkeypatch):
    """One geometry, .jpg and .png files alternating: a batched pass decodes both kinds, each with its own call; equal detections."""
    images = []
    for k in range(4):
        frame = _crop(3 * k, 200, 330)
        if k % 2:
            path = str(tmp_path / ("f%d.jpg" % k))
            PilImage.fromarray(frame).save(path, "JPEG", quality=90)
        else:
            path = _write(str(tmp_path / ("f%d.png" % k)), C.pil_file(frame, compress_level=6))
        images.append(_image("f%d" % k, path))
    host = _dets(f32_models, images, "host", "host", monkeypatch)
    dev = _dets(f32_models, images, "device", "device", monkeypatch)
    _same(dev, host)
    eng = _engine(f32_models)
    assert any(sl.jpg_count and len(sl.png_items) for sl in _decoded_png_slots(eng))


def test_zz_damaged_png_raises_naming_it(f32_models, tmp_path, monkeypatch):
    from faster_rcnn_amd._lib import FrcnnError
    path = _write(str(tmp_path / "damaged_frame.png"), C.damaged()[2])
    with pytest.raises(FrcnnError, match="device PNG decoder: .*damaged_frame.png"):
        _dets(f32_models, [_image("damaged", path)], "device", "host", monkeypatch)
