"""The full-format device PNG decoder behind the entry points (png_decoder "device_full": entry.set_png_decoder / FRCNN_ENTRY_PNG_DECODER,
annotate_images(png_decoder=...), FRCNN_FEED_PNG_DECODER): the pixels are Pillow's, so detections, printed lines, output files and fed
tensors must be IDENTICAL to the host decoder's; a file the full planner refuses (16-bit grey) rides in the same passes host-decoded;
"device" still sends a palette file to PIL; a damaged file raises FrcnnError naming it."""
import os

import numpy as np
import pytest

from tests import png_dec_cases as C
from tests import png_full_cases as F
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


def _palette_file(frame, interlace=0):
    """The frame as a palette file (Pillow's ADAPTIVE palette) from the cases' writer, so that it can be interlaced."""
    pimg = PilImage.fromarray(frame).convert("P", palette=PilImage.ADAPTIVE)
    return F.written(np.asarray(pimg).astype(np.int64)[:, :, None], 3, 8, interlace, F.mixed, bytes(pimg.getpalette()[:768]))


def _engine(f32_models):
    from faster_rcnn_amd import entry
    mgr, det, _ = f32_models
    return entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight("f32"))


def _slots(eng):
    return [sl for slots in eng.cache._slots.values() for sl in slots if sl.png_items is not None and len(sl.png_items)]


def _full_items(eng):
    from faster_rcnn_amd import _lib
    return sum(len(sl.png_items) for sl in _slots(eng) if sl.png_items._type_ is _lib.PngDecFullBatchItem)


def test_annotate_images_device_full_equals_host(f32_models, tmp_path):
    """Six small frames of two sizes: RGB, palette, Adam7 RGB, 16-bit grey (refused: PIL, inside the same run), an Adam7 palette file and
    an RGBA file.  The same printed lines and byte-identical output files under host and device_full; the device_full leg really decoded
    (its passes hold full-format PNG items); under "device" the palette file still goes to PIL."""
    from faster_rcnn_amd import _lib, annotate_video, entry, feed, shapes
    mgr, det, _ = f32_models
    d_in = tmp_path / "frames"
    d_in.mkdir()
    names = ["%06d.png" % i for i in range(6)]
    for i, name in enumerate(names):
        frame = _crop(i, 180, 260) if i < 4 else _crop(i, 200, 300)
        if i == 0:
            data = C.pil_file(frame, compress_level=6)
        elif i == 1:
            data = _palette_file(frame)
        elif i == 2:
            data = F.written(frame.astype(np.int64), 2, 8, 1, F.mixed)
        elif i == 3:
            data = F.written(frame[:, :, :1].astype(np.int64) * 257, 0, 16)
        elif i == 4:
            data = _palette_file(frame, 1)
        else:
            data = C.pil_file(np.dstack([frame, np.full(frame.shape[:2], 133, np.uint8)]), compress_level=6)
        _write(str(d_in / name), data)
    text = {}
    try:
        for decoder in ("host", "device", "device_full"):
            _, text[decoder] = quiet(annotate_video.annotate_images, mgr, det, str(d_in), str(tmp_path / decoder), names, 320, 540,
                                     png_decoder=decoder)
            assert sorted(os.listdir(str(tmp_path / decoder))) == names
            kinds = {sl.png_items._type_ for sl in _slots(_engine(f32_models))}
            if decoder == "device":                                          # revision 1's items: nothing changed under "device"
                assert _lib.PngDecBatchItem in kinds and _full_items(_engine(f32_models)) == 0
            if decoder == "device_full":
                assert _full_items(_engine(f32_models)) > 0
    finally:
        entry.set_png_decoder(None)
    assert text["host"] == text["device_full"] == text["device"] and "{'bbox'" in text["host"]
    for name in names:
        with open(str(tmp_path / "host" / name), "rb") as a, open(str(tmp_path / "device_full" / name), "rb") as b:
            assert a.read() == b.read(), name

    def img(name, h, w):
        return shapes.Image(shapes.Metadata("x", w, h, [], str(d_in / name)))
    assert feed.plan_entry_file(img(names[1], 180, 260), png=True) is None                 # "device": the palette file is PIL's
    assert isinstance(feed.plan_entry_file(img(names[1], 180, 260), png="full")[1], _lib.PngDecFullPlan)
    assert feed.plan_entry_file(img(names[3], 180, 260), png="full") is None               # 16-bit grey: PIL's under either


def _dets(f32_models, images, png, monkeypatch):
    from faster_rcnn_amd import entry, util, voc_dets
    monkeypatch.setattr(voc_dets, "CAPTURE_MIN", 1)
    mgr, det, _ = f32_models
    resized, ratios = util.resize_imgs(images, min_size=320, max_size=540)
    entry.set_png_decoder(png)
    try:
        by_cls, _ = quiet(voc_dets.get_dets_by_cls, mgr, det, ratios, resized, det_threshold=0.1)
    finally:
        entry.set_png_decoder(None)
    return _by_image(by_cls)


SIZES = ((200, 330), (204, 330), (200, 326), (208, 334), (196, 322), (204, 326), (200, 330))


def test_canvas_passes_with_mixed_sizes(f32_models, tmp_path, monkeypatch):
    """More sizes than CANVAS_MIN_GEOMETRIES: canvas passes form, their slots hold full-format PNG items, the detections are equal."""
    from faster_rcnn_amd import _lib, entry
    images = []
    for k, (h, w) in enumerate(SIZES):
        frame = _crop(k, h, w)
        data = (_palette_file(frame, k & 1), F.written(frame.astype(np.int64), 2, 8, 1, F.mixed), C.pil_file(frame, compress_level=6))[k % 3]
        images.append(_image("crop%d" % k, _write(str(tmp_path / ("crop%d.png" % k)), data)))
    assert len(set(SIZES)) > entry.CANVAS_MIN_GEOMETRIES
    host = _dets(f32_models, images, "host", monkeypatch)
    dev = _dets(f32_models, images, "device_full", monkeypatch)
    _same(dev, host)
    eng = _engine(f32_models)
    assert eng.canvas and any(sl.canvas and sl.png_items._type_ is _lib.PngDecFullBatchItem for sl in _slots(eng))
    entry.set_png_decoder("device_full")
    try:
        got = eng.host_pixels(images[0])[0]
        assert isinstance(got, entry.PngFile) and isinstance(got.plan, _lib.PngDecFullPlan)
    finally:
        entry.set_png_decoder(None)
    assert isinstance(eng.host_pixels(images[0])[0], np.ndarray)          # every option unset: today's path


def test_feed_device_image_same_bits(tmp_path, monkeypatch):
    """feed.device_image under FRCNN_FEED_PNG_DECODER=device_full: the same float32 tensor as from PIL for a palette file and for an RGB
    file, flipped and resized too, planned ahead or not; a 16-bit grey file goes the host way; feed.plan_file never takes a .png."""
    from faster_rcnn_amd import _lib, feed, resnet, shapes
    frame = _crop(3, 120, 170)
    files = {"palette.png": _palette_file(frame, 1), "rgb.png": C.pil_file(frame, compress_level=6),
             "grey16.png": F.written(frame[:, :, :1].astype(np.int64) * 257, 0, 16)}
    for name, data in files.items():
        _write(str(tmp_path / name), data)

    def img(name, size, flipped=False):
        return shapes.Image(shapes.Metadata("x", size[1], size[0], [], str(tmp_path / name), flipped=flipped))
    monkeypatch.delenv("FRCNN_FEED_JPEG_DECODER", raising=False)
    for name in files:
        for size, flipped, ahead in (((120, 170), False, False), ((200, 280), True, True)):
            monkeypatch.setenv("FRCNN_FEED_PNG_DECODER", "host")
            assert feed.plan_feed_file(img(name, size)) is None
            want = feed.device_image(img(name, size, flipped), resnet.preprocess)
            monkeypatch.setenv("FRCNN_FEED_PNG_DECODER", "device_full")
            image = img(name, size, flipped)
            planned = feed.plan_feed_file(image)
            assert feed.plan_file(image) is None
            assert (planned is None) == (name == "grey16.png")
            assert planned is None or isinstance(planned[1], _lib.PngDecFullPlan)
            if ahead:
                feed.decode_ahead(image)
            got = feed.device_image(image, resnet.preprocess)
            torch.cuda.synchronize()
            feed.check_decodes()
            assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), (name, size)
    monkeypatch.setenv("FRCNN_FEED_PNG_DECODER", "device")                  # revision 1 through the same door
    got = feed.device_image(img("rgb.png", (120, 170)), resnet.preprocess)
    assert isinstance(feed.plan_feed_file(img("rgb.png", (120, 170)))[1], _lib.PngDecPlan) and feed.plan_feed_file(img("palette.png", (120, 170))) is None
    monkeypatch.setenv("FRCNN_FEED_PNG_DECODER", "host")
    torch.cuda.synchronize()
    feed.check_decodes()
    assert torch.equal(got, feed.device_image(img("rgb.png", (120, 170)), resnet.preprocess))
    assert not feed._DECODE_STATUS


def test_zz_damaged_files_raise_naming_them(f32_models, tmp_path, monkeypatch):
    """Last: a file whose payload is damaged, through the entry (collect_batch) and through the feed (check_decodes)."""
    from faster_rcnn_amd import feed, resnet, shapes
    from faster_rcnn_amd._lib import FrcnnError
    path = _write(str(tmp_path / "damaged_frame.png"), F.damaged()["payload"])
    with pytest.raises(FrcnnError, match="device PNG decoder: .*damaged_frame.png"):
        _dets(f32_models, [_image("damaged", path)], "device_full", monkeypatch)
    monkeypatch.setenv("FRCNN_FEED_PNG_DECODER", "device_full")
    feed.device_image(shapes.Image(shapes.Metadata("x", 65, 33, [], path)), resnet.preprocess)
    torch.cuda.synchronize()
    with pytest.raises(FrcnnError, match="device PNG decoder: .*damaged_frame.png"):
        feed.check_decodes()
    assert not feed._DECODE_STATUS
