"""The device JPEG decoder behind the entry points (FRCNN_ENTRY_JPEG_DECODER / entry.set_jpeg_decoder, FRCNN_FEED_JPEG_DECODER): the pixels
are Pillow's, so detections and the fed tensor must be IDENTICAL to the host decoder's; a file outside the supported set takes the host
path; a damaged file raises FrcnnError naming it."""
import os
import shutil

import numpy as np
import pytest

from tests import jpeg_dec_cases as C
from tests.test_png_entry_gpu import _by_image, _named, f32_models, quiet      # noqa: F401  (the small f32 models)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
PilImage = pytest.importorskip("PIL.Image")


def _image(name, path):
    with PilImage.open(path) as im:
        w, h = im.size
    return _named(name, path=path, size=(h, w))


def _dets(f32_models, images, decoder, monkeypatch):
    from faster_rcnn_amd import entry, util, voc_dets
    monkeypatch.setattr(voc_dets, "CAPTURE_MIN", 1)
    mgr, det, _ = f32_models
    resized, ratios = util.resize_imgs(images, min_size=320, max_size=540)
    entry.set_jpeg_decoder(decoder)
    try:
        by_cls, _ = quiet(voc_dets.get_dets_by_cls, mgr, det, ratios, resized, det_threshold=0.1)
    finally:
        entry.set_jpeg_decoder(None)
    return _by_image(by_cls)


def _same(a, b):
    assert a.keys() == b.keys() and len(a) > 0
    for k in a:
        assert len(a[k]) == len(b[k])
        for x, y in zip(a[k], b[k]):                              # equal, not close: the pixels are identical
            assert x["cls_name"] == y["cls_name"] and np.array_equal(x["bbox"], y["bbox"]) and float(x["prob"]) == float(y["prob"]), (k, x, y)


def test_get_dets_by_cls_device_decoder_equals_host(f32_models, tmp_path, monkeypatch):
    """The golden VOC image (and a copy, so that a batched pass forms) and a progressive file of another size: equal arrays either way,
    and the device path really decoded the baseline files (the engine's slots hold a file area)."""
    from faster_rcnn_amd import entry
    prog = str(tmp_path / "progressive.jpg")
    with PilImage.open(C.GOLDEN) as im:
        im.crop((0, 0, 330, 200)).save(prog, "JPEG", quality=90, progressive=True)
    copy = str(tmp_path / "copy.jpg")
    shutil.copy(C.GOLDEN, copy)
    images = [_image("000005", C.GOLDEN), _image("copy", copy), _image("prog", prog)]
    host = _dets(f32_models, images, "host", monkeypatch)
    dev = _dets(f32_models, images, "device", monkeypatch)
    _same(dev, host)
    mgr, det, _ = f32_models
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight("f32"))
    assert any(sl.jpg_dev is not None for slots in eng.cache._slots.values() for sl in slots)
    entry.set_jpeg_decoder("device")
    try:
        assert isinstance(eng.host_pixels(images[0])[0], entry.JpegFile)
        assert isinstance(eng.host_pixels(images[2])[0], np.ndarray)          # progressive: today's path
    finally:
        entry.set_jpeg_decoder(None)


def test_damaged_file_raises_naming_it(f32_models, tmp_path, monkeypatch):
    from faster_rcnn_amd._lib import FrcnnError
    path = str(tmp_path / "damaged_frame.jpg")
    with open(path, "wb") as f:
        f.write(C.damaged())
    host = _dets(f32_models, [_image("damaged", path)], "host", monkeypatch)     # (PIL decodes what it can: no error on the host path)
    assert isinstance(host, dict)
    with pytest.raises(FrcnnError, match="damaged_frame.jpg"):
        _dets(f32_models, [_image("damaged", path)], "device", monkeypatch)


def test_feed_device_image_same_bits(tmp_path, monkeypatch):
    """feed.device_image: the same float32 tensor from the device decoder as from PIL, flipped and resized too; the status word is looked
    at by check_decodes without a wait of its own; a progressive file goes the host way; a damaged one raises naming the file."""
    from faster_rcnn_amd import feed, resnet, shapes
    from faster_rcnn_amd._lib import FrcnnError
    prog = str(tmp_path / "progressive.jpg")
    with PilImage.open(C.GOLDEN) as im:
        im.save(prog, "JPEG", quality=90, progressive=True)
    bad = str(tmp_path / "damaged_feed.jpg")
    with open(bad, "wb") as f:
        f.write(C.damaged())

    def img(path, size, flipped=False):
        return shapes.Image(shapes.Metadata("x", size[1], size[0], [], path, flipped=flipped))

    for path, size, flipped in ((C.GOLDEN, (375, 500), False), (C.GOLDEN, (600, 800), True), (prog, (375, 500), False)):
        monkeypatch.setenv("FRCNN_FEED_JPEG_DECODER", "host")
        want = feed.device_image(img(path, size, flipped), resnet.preprocess)
        monkeypatch.setenv("FRCNN_FEED_JPEG_DECODER", "device")
        image = img(path, size, flipped)
        planned = feed.plan_file(image)
        assert (planned is None) == (path == prog)
        feed.decode_ahead(image)
        got = feed.device_image(image, resnet.preprocess)
        torch.cuda.synchronize()
        feed.check_decodes()
        assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)
    assert not feed._DECODE_STATUS
    feed.device_image(img(bad, (33, 65)), resnet.preprocess)
    torch.cuda.synchronize()
    with pytest.raises(FrcnnError, match="damaged_feed.jpg"):
        feed.check_decodes()
    assert not feed._DECODE_STATUS
