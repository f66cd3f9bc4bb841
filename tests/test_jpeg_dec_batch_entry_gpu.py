"""The batched device JPEG decoder behind entry.DetectionEntry: canvas passes take files (a list of many sizes, the VOC case), a pass
decodes all its files in one call (FRCNN_ENTRY_JPEG_BATCH=0 keeps the per-file loop), a pass may mix files with host-decoded frames, and a
damaged file in a canvas pass raises FrcnnError naming it.  The pixels are Pillow's either way, so detections are EQUAL, not close."""
import shutil

import numpy as np
import pytest

from tests import jpeg_dec_cases as C
from tests.test_jpeg_dec_entry_gpu import _dets, _image, _same
from tests.test_png_entry_gpu import f32_models      # noqa: F401  (the small f32 models)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
PilImage = pytest.importorskip("PIL.Image")

# (height, width, Pillow subsampling) of the crops: more sizes than CANVAS_MIN_GEOMETRIES, close enough to share canvas classes
CROPS = ((200, 330, 2), (204, 330, 1), (200, 326, 0), (208, 334, 2), (196, 322, 1), (204, 326, 2), (200, 330, 0))


def _engine(f32_models):
    from faster_rcnn_amd import entry
    mgr, det, _ = f32_models
    return entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight("f32"))


def _mixed_list(tmp_path, extra=()):
    """Crops of the golden image saved as baseline JPEG at mixed subsampling, one progressive file among them."""
    images = []
    with PilImage.open(C.GOLDEN) as im:
        im = im.convert("RGB")
        for k, (h, w, ss) in enumerate(CROPS):
            path = str(tmp_path / ("crop%d.jpg" % k))
            im.crop((k, 2 * k, k + w, 2 * k + h)).save(path, "JPEG", quality=90, subsampling=ss)
            images.append(_image("crop%d" % k, path))
        prog = str(tmp_path / "progressive.jpg")
        im.crop((5, 5, 5 + 326, 5 + 204)).save(prog, "JPEG", quality=90, progressive=True)
    images.insert(3, _image("prog", prog))
    for name, data in extra:
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(data)
        images.append(_image(name.split(".")[0], path))
    return images


def test_canvas_list_device_decoder_equals_host(f32_models, tmp_path, monkeypatch):
    """A list of more sizes than CANVAS_MIN_GEOMETRIES: canvas passes form, with ``device`` their slots hold a file area (on the parent
    commit canvas slots never did), the detections equal the host decoder's, the progressive file rides in the same passes host-decoded,
    and the header's geometry is the decoded frame's."""
    from faster_rcnn_amd import entry
    images = _mixed_list(tmp_path)
    assert len({(h, w) for h, w, _ in CROPS}) > entry.CANVAS_MIN_GEOMETRIES
    host = _dets(f32_models, images, "host", monkeypatch)
    eng = _engine(f32_models)
    canvas_keys = [k for k in eng.cache.keys() if k[0] == "canvas"]
    assert eng.canvas and canvas_keys
    assert not any(sl.jpg_dev is not None for slots in eng.cache._slots.values() for sl in slots)
    monkeypatch.setenv("FRCNN_ENTRY_JPEG_BATCH", "1")
    dev = _dets(f32_models, images, "device", monkeypatch)
    _same(dev, host)
    assert [k for k in eng.cache.keys() if k[0] == "canvas"] == canvas_keys          # the same passes: the key does not know who decodes
    assert any(sl.canvas and sl.jpg_dev is not None for k in canvas_keys for sl in eng.cache._slots[k])
    entry.set_jpeg_decoder("device")
    try:
        from faster_rcnn_amd import util
        resized, _ = util.resize_imgs(images, min_size=320, max_size=540)
        assert eng.canvas
        kinds = [type(eng.host_pixels(r)[0]) for r in resized]
        assert kinds.count(np.ndarray) == 1 and kinds[3] is np.ndarray and kinds.count(entry.JpegFile) == len(CROPS)
        for r in resized:
            px = eng.host_pixels(r)
            assert eng.probe_geometry(r) == eng.geometry(px) and eng.geometry(px)[0] == "canvas"
    finally:
        entry.set_jpeg_decoder(None)
    # the per-file loop through the same canvas passes
    monkeypatch.setenv("FRCNN_ENTRY_JPEG_BATCH", "0")
    _same(_dets(f32_models, images, "device", monkeypatch), host)


def test_batch_switch_exact_geometry(f32_models, tmp_path, monkeypatch):
    """The golden image and a copy (one geometry: a batched per-geometry pass, padded with its first frame): equal detections from the
    host decoder, the batched decode and the per-file loop."""
    copy = str(tmp_path / "copy.jpg")
    shutil.copy(C.GOLDEN, copy)
    images = [_image("000005", C.GOLDEN), _image("copy", copy)]
    host = _dets(f32_models, images, "host", monkeypatch)
    eng = _engine(f32_models)
    assert not eng.canvas
    monkeypatch.setenv("FRCNN_ENTRY_JPEG_BATCH", "1")
    batched = _dets(f32_models, images, "device", monkeypatch)
    monkeypatch.setenv("FRCNN_ENTRY_JPEG_BATCH", "0")
    per_file = _dets(f32_models, images, "device", monkeypatch)
    _same(batched, host)
    _same(per_file, batched)
    assert any(not sl.canvas and sl.jpg_dev is not None and sl.batch > 1 for slots in eng.cache._slots.values() for sl in slots)


def test_annotating_pass_over_files(f32_models, tmp_path):
    """An annotating pass over two .jpg frames (never a canvas pass): the same detections and the same drawn frames from either decoder."""
    from faster_rcnn_amd import entry, util
    eng = _engine(f32_models)
    copy = str(tmp_path / "copy.jpg")
    shutil.copy(C.GOLDEN, copy)
    images = [_image("000005", C.GOLDEN), _image("copy", copy)]
    resized, ratios = util.resize_imgs(images, min_size=320, max_size=540)
    got = {}
    for decoder in ("host", "device"):
        entry.set_jpeg_decoder(decoder)
        try:
            pixels = [eng.host_pixels(r) for r in resized]
            assert isinstance(pixels[0][0], entry.JpegFile) == (decoder == "device")
            got[decoder] = eng.collect_batch(eng.submit_batch(resized, ratios, 0.1, pixels, batch=eng.batch, annotate=True))
        finally:
            entry.set_jpeg_decoder(None)
    assert len(got["host"]) == len(got["device"]) == 2
    for (n0, d0, f0), (n1, d1, f1) in zip(got["host"], got["device"]):
        assert n0 == n1 and len(d0) == len(d1) and f0.shape == f1.shape and f0.ndim == 3
        assert np.array_equal(f0, f1)
        for x, y in zip(d0, d1):
            assert x["cls_name"] == y["cls_name"] and np.array_equal(x["bbox"], y["bbox"]) and float(x["prob"]) == float(y["prob"])


def test_damaged_file_in_a_canvas_pass_raises_naming_it(f32_models, tmp_path, monkeypatch):
    from faster_rcnn_amd._lib import FrcnnError
    images = _mixed_list(tmp_path, extra=[("damaged_canvas_frame.jpg", C.damaged())])       # (33x65: any canvas holds it)
    eng = _engine(f32_models)
    with pytest.raises(FrcnnError, match="damaged_canvas_frame.jpg"):
        _dets(f32_models, images, "device", monkeypatch)
    assert eng.canvas
