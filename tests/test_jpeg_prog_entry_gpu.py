"""The device decoder for progressive JPEG files behind the entry points, under the JPEG decoder setting "device_full"
(FRCNN_ENTRY_JPEG_DECODER / entry.set_jpeg_decoder, FRCNN_FEED_JPEG_DECODER): baseline files keep the baseline decoder, progressive ones
take the new one, in the same pass; the pixels are Pillow's, so detections and the fed tensor are IDENTICAL to the host decoder's; a
damaged progressive file raises FrcnnError naming it."""
import shutil

import numpy as np
import pytest

from tests import jpeg_dec_cases as C
from tests import jpeg_prog_cases as P
from tests.test_jpeg_dec_entry_gpu import _dets, _image, _same
from tests.test_png_entry_gpu import f32_models      # noqa: F401  (the small f32 models)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
torch = pytest.importorskip("torch")
PilImage = pytest.importorskip("PIL.Image")


def _progressive(path, box, **kw):
    with PilImage.open(C.GOLDEN) as im:
        (im.crop(box) if box else im).save(path, "JPEG", quality=90, progressive=True, **kw)
    return path


def test_get_dets_by_cls_device_full_equals_host(f32_models, tmp_path, monkeypatch):
    """The golden VOC image, a copy of it and a progressive crop: every file is planned (the progressive one is an ndarray under
    "device"), the detections are the host decoder's."""
    from faster_rcnn_amd import _lib, entry
    prog = _progressive(str(tmp_path / "progressive.jpg"), (0, 0, 330, 200))
    copy = str(tmp_path / "copy.jpg")
    shutil.copy(C.GOLDEN, copy)
    images = [_image("000005", C.GOLDEN), _image("copy", copy), _image("prog", prog)]
    host = _dets(f32_models, images, "host", monkeypatch)
    dev = _dets(f32_models, images, "device_full", monkeypatch)
    _same(dev, host)
    mgr, det, _ = f32_models
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight("f32"))
    assert any(sl.full_items is not None and len(sl.full_items) for slots in eng.cache._slots.values() for sl in slots)
    entry.set_jpeg_decoder("device_full")
    try:
        kinds = [type(eng.host_pixels(im)[0].plan) for im in images]
        assert kinds == [_lib.JpegDecPlan, _lib.JpegDecPlan, _lib.JpegDecFullPlan]
        entry.set_jpeg_decoder("device")
        assert isinstance(eng.host_pixels(images[2])[0], np.ndarray)
    finally:
        entry.set_jpeg_decoder(None)


def test_canvas_pass_of_mixed_sizes(f32_models, tmp_path, monkeypatch):
    """More sizes than CANVAS_MIN_GEOMETRIES: canvas passes; one progressive file among baseline ones."""
    boxes = [(0, 0, 330, 200), (0, 0, 300, 220), (10, 10, 350, 260), (0, 0, 280, 240), (20, 0, 340, 230), (0, 0, 310, 250)]
    images = []
    for k, box in enumerate(boxes):
        path = str(tmp_path / ("frame%d.jpg" % k))
        if k == 2:
            _progressive(path, box, subsampling=1)
        else:
            with PilImage.open(C.GOLDEN) as im:
                im.crop(box).save(path, "JPEG", quality=90)
        images.append(_image("frame%d" % k, path))
    host = _dets(f32_models, images, "host", monkeypatch)
    dev = _dets(f32_models, images, "device_full", monkeypatch)
    _same(dev, host)


def test_damaged_progressive_file_raises_naming_it(f32_models, tmp_path, monkeypatch):
    from faster_rcnn_amd._lib import FrcnnError
    path = str(tmp_path / "damaged_progressive.jpg")
    with open(path, "wb") as f:
        f.write(P.damaged()["dc_first"])
    with pytest.raises(FrcnnError, match="damaged_progressive.jpg"):
        _dets(f32_models, [_image("damaged", path)], "device_full", monkeypatch)


def test_feed_device_image_same_bits(tmp_path, monkeypatch):
    """feed.device_image under FRCNN_FEED_JPEG_DECODER=device_full: the same float32 tensor as from PIL for a baseline and for a
    progressive file, flipped and resized too; a damaged progressive file raises naming the file."""
    from faster_rcnn_amd import _lib, feed, resnet, shapes
    prog = _progressive(str(tmp_path / "progressive.jpg"), None)
    bad = str(tmp_path / "damaged_feed.jpg")
    with open(bad, "wb") as f:
        f.write(P.damaged()["ac_refinement"])

    def img(path, size, flipped=False):
        return shapes.Image(shapes.Metadata("x", size[1], size[0], [], path, flipped=flipped))

    for path, size, flipped in ((C.GOLDEN, (375, 500), False), (prog, (375, 500), False), (prog, (600, 800), True)):
        monkeypatch.setenv("FRCNN_FEED_JPEG_DECODER", "host")
        want = feed.device_image(img(path, size, flipped), resnet.preprocess)
        monkeypatch.setenv("FRCNN_FEED_JPEG_DECODER", "device_full")
        image = img(path, size, flipped)
        assert isinstance(feed.plan_file(image)[1], _lib.JpegDecFullPlan if path == prog else _lib.JpegDecPlan)
        feed.decode_ahead(image)
        got = feed.device_image(image, resnet.preprocess)
        torch.cuda.synchronize()
        feed.check_decodes()
        assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)
    assert not feed._DECODE_STATUS
    feed.device_image(img(bad, (64, 136)), resnet.preprocess)
    torch.cuda.synchronize()
    with pytest.raises(_lib.FrcnnError, match="damaged_feed.jpg"):
        feed.check_decodes()
    assert not feed._DECODE_STATUS
