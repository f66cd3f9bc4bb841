"""The device JPEG encoder's 4:2:0 / optimised-Huffman modes inside the detection entry's annotating passes
(entry.DetectionEntry.submit_batch(annotate=True, encode="jpeg", quality=q, subsampling=..., huffman=...)): the files are ops.jpeg_bytes
of the annotated frame in that mode, the detections are the detection-only pass's, a file longer than the first read-back comes back whole,
and a pass keyed (444, "standard") is the existing JPEG pass -- the same cache key, the same bytes."""
import io

import pytest

from tests import jpeg_opt_ref as O
from tests.test_png_entry_gpu import B, _named, f32_models, frame_pixels, same_dets      # noqa: F401  (the small f32 models)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
PilImage = pytest.importorskip("PIL.Image")

MODE = dict(subsampling=420, huffman="optimized")


def _engine(f32_models):
    from faster_rcnn_amd import entry
    mgr, det, _ = f32_models
    return entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight("f32"))


@pytest.mark.parametrize("count", [1, 3])
def test_optimized_420_passes(f32_models, monkeypatch, count):
    """150x250 frames, one in a one-frame pass and three in a padded pass of four: the pass returns the detections of the detection-only
    pass and, per frame, ops.jpeg_bytes (= the restatement's file) of the frame the raw annotating pass returns."""
    from faster_rcnn_amd import ops, util, voc_dets
    monkeypatch.setattr(voc_dets, "CAPTURE_MIN", 1)
    eng = _engine(f32_models)
    take, quality = (1 if count == 1 else B), 90
    imgs = [_named("m%d" % i, pixels=frame_pixels(150, 250, 500 + i)) for i in range(count)]
    resized, ratios = util.resize_imgs(imgs, min_size=320, max_size=540)
    pixels = [eng.host_pixels(r) for r in resized]
    dets = eng.collect_batch(eng.submit_batch(resized, ratios, 0.0, pixels, batch=take))
    raw = eng.collect_batch(eng.submit_batch(resized, ratios, 0.0, pixels, batch=take, annotate=True))
    jpg = eng.collect_batch(eng.submit_batch(resized, ratios, 0.0, pixels, batch=take, annotate=True, encode="jpeg", quality=quality, **MODE))
    again = eng.collect_batch(eng.submit_batch(resized, ratios, 0.0, pixels, batch=take, annotate=True, encode="jpeg", quality=quality, **MODE))
    assert len(dets) == len(raw) == len(jpg) == count and all(len(r) == 3 for r in jpg)
    for (n0, d0), (_, _, frame), (n1, d1, data), (_, _, data2) in zip(dets, raw, jpg, again):
        assert n0 == n1
        same_dets(d1, d0, tol=0.0)
        assert isinstance(data, bytes) and 0 < len(data) <= ops.jpeg_bound(frame.shape[0], frame.shape[1], **MODE) and data == data2
        assert data == ops.jpeg_bytes(torch.from_numpy(frame).cuda(), quality=quality, bgr=True, **MODE)
        assert data == O.encode(frame, quality, 420, "optimized", bgr=True)
        img = PilImage.open(io.BytesIO(data))
        assert img.mode == "RGB" and img.size == (frame.shape[1], frame.shape[0])


def test_long_file_and_cache_keys(f32_models, monkeypatch):
    """A 64x136 noise frame at quality 100 encodes, optimised at 4:2:0 too, to more bytes than the first read-back holds: collect_batch
    fetches the rest.  Every mode pair but the default is a pass of its own, tagged with the pair; (444, "standard") is the pass
    without the keywords: no new capture, the same key, the same bytes.  Unknown modes, and modes without encode="jpeg", are refused
    before anything is captured."""
    from faster_rcnn_amd import ops, util, voc_dets
    from faster_rcnn_amd._lib import FrcnnError
    monkeypatch.setattr(voc_dets, "CAPTURE_MIN", 1)
    eng = _engine(f32_models)
    src = frame_pixels(64, 136, 7)
    resized, ratios = util.resize_imgs([_named("n", pixels=src)], min_size=320, max_size=700)      # (the pass encodes the SOURCE frame)
    pixels = [eng.host_pixels(resized[0])]
    submit = lambda **kw: eng.submit_batch(resized, ratios, 0.0, pixels, batch=1, annotate=True, **kw)
    (_, _, frame), = eng.collect_batch(submit())
    dev = torch.from_numpy(frame).cuda()
    ticket = submit(encode="jpeg", quality=100, **MODE)
    first_copy = ticket.slot.first_copy
    (_, _, data), = eng.collect_batch(ticket)
    assert first_copy == 16 + ops.jpeg_header_bytes() + src.nbytes // 4
    assert 16 + len(data) > first_copy, (len(data), first_copy)
    assert data == ops.jpeg_bytes(dev, quality=100, bgr=True, **MODE) == O.encode(frame, 100, 420, "optimized", bgr=True)
    geometry = eng.geometry_of(pixels[0])
    assert geometry + ("annotate", "jpeg", 100, 420, "optimized") in set(eng.cache.keys())
    # the default pair: the existing pass
    (_, _, old), = eng.collect_batch(submit(encode="jpeg", quality=100))
    keys, captures = set(eng.cache.keys()), eng.cache.captures
    assert geometry + ("annotate", "jpeg", 100) in keys
    (_, _, same), = eng.collect_batch(submit(encode="jpeg", quality=100, subsampling=444, huffman="standard"))
    assert same == old == ops.jpeg_bytes(dev, quality=100, bgr=True) and set(eng.cache.keys()) == keys and eng.cache.captures == captures
    (_, _, opt444), = eng.collect_batch(submit(encode="jpeg", quality=100, huffman="optimized"))
    assert set(eng.cache.keys()) - keys == {geometry + ("annotate", "jpeg", 100, 444, "optimized")} and eng.cache.captures == captures + 1
    assert opt444 == ops.jpeg_bytes(dev, quality=100, bgr=True, huffman="optimized") and len(data) < len(opt444) < len(old)
    for kw in (dict(encode="jpeg", quality=90, subsampling=422), dict(encode="jpeg", quality=90, huffman="best"), dict(encode="png", subsampling=420),
               dict(huffman="optimized"), dict(encode="png-huffman", huffman="optimized"), dict(encode="jpeg", quality=90, subsampling="420")):
        with pytest.raises(FrcnnError):
            submit(**kw)
    assert eng.cache.captures == captures + 1


def test_main_with_both_options(f32_models, tmp_path):
    """``annotate_video --frame_format jpg --jpeg_subsampling 420 --jpeg_huffman optimized`` with both encoders on two small PNG files:
    the same printed lines as the PNG run; the device files are ops.jpeg_bytes of the PNG run's frames in that mode; the host files are
    PIL's with ``subsampling=2, optimize=True``."""
    import os

    import numpy as np

    from faster_rcnn_amd import annotate_video, ops
    from faster_rcnn_amd.weights import save_npz
    from tests import jpeg_dec_ref as D
    from tests import jpeg_ref as R
    from tests.test_png_entry_gpu import quiet
    _, _, w = f32_models
    npz = str(tmp_path / "w.npz")
    save_npz(npz, w)
    d_in = tmp_path / "frames"
    d_in.mkdir()
    names = ["%06d.png" % i for i in range(2)]
    y, x = np.mgrid[0:150, 0:250]
    for i, name in enumerate(names):
        f = np.stack([x // 2 + y // 3 + 9 * i, 200 - y + x // 5, (x + 2 * y) // 3], -1) + frame_pixels(150, 250, 60 + i) % 5
        PilImage.fromarray((f % 256).astype(np.uint8)).save(str(d_in / name))
    both = ["--frame_format", "jpg", "--jpeg_quality", "85", "--jpeg_subsampling", "420", "--jpeg_huffman", "optimized"]
    text, flags = {}, {"png": [], "host": both, "device": both + ["--jpeg_encoder", "device"]}
    for leg, extra in flags.items():
        argv = [npz, npz, str(d_in), "--resize_dims", "320,540", "--out_dir", str(tmp_path / leg)] + extra
        _, text[leg] = quiet(annotate_video.main, argv)
        assert sorted(os.listdir(str(tmp_path / leg))) == (names if leg == "png" else [n[:-4] + ".jpg" for n in names])
    assert text["png"] == text["host"] == text["device"] and "{'bbox'" in text["png"]
    standard = [(list(b), list(v)) for b, v in R.HUFFMAN]
    for name in names:
        frame = np.asarray(PilImage.open(str(tmp_path / "png" / name)).convert("RGB"))        # the annotated frame, lossless
        data = open(str(tmp_path / "device" / (name[:-4] + ".jpg")), "rb").read()
        assert data == ops.jpeg_bytes(torch.from_numpy(frame.copy()).cuda(), quality=85, **MODE) == O.encode(frame, 85, 420, "optimized")
        host = open(str(tmp_path / "host" / (name[:-4] + ".jpg")), "rb").read()
        buf = io.BytesIO()
        PilImage.fromarray(frame).save(buf, format="JPEG", quality=85, subsampling=2, optimize=True)
        assert host == buf.getvalue()
        for f in (data, host):                                              # both: Y at 2x2, tables of their own
            p = D.plan(f)
            assert (p.hs, p.vs) == (2, 2)
            tables = [(list(f[p.dht_off[tc][th]:p.dht_off[tc][th] + 16]), list(f[p.dht_off[tc][th] + 16:p.dht_off[tc][th] + 16 + p.dht_n[tc][th]]))
                      for tc, th in ((0, 0), (1, 0), (0, 1), (1, 1))]
            assert all(sum(b) == len(v) for b, v in tables) and all(len(t[1]) < len(s[1]) for t, s in zip(tables[1::2], standard[1::2]))
