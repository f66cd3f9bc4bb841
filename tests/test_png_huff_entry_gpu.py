"""The huffman mode of the device PNG encoder inside the detection entry's annotating passes
(entry.DetectionEntry.submit_batch(annotate=True, encode="png-huffman")) and behind ``annotate_video --png_encoder device --png_compress
huffman``: the same detections as the raw annotating pass, files that decode to its frames and equal the CPU restatement's, passes of
their own beside the "png" passes."""
import io
import os

import numpy as np
import pytest

from tests import png_huff_ref as R
from tests.test_png_entry_gpu import B, _named, f32_models, frame_pixels, quiet, same_dets      # noqa: F401  (the small f32 models)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
PilImage = pytest.importorskip("PIL.Image")


def test_huffman_encoding_passes(f32_models, tmp_path, monkeypatch):
    """Four 200x330 frames per pass, in memory (BGR) and as files (uploaded RGB): the huffman pass returns the dets of the raw annotating
    pass and files that decode to its frames in RGB order -- the restatement's files of those frames, byte for byte; the "png" passes
    stay cached beside it under keys of their own."""
    from faster_rcnn_amd import entry, ops, util, voc_dets
    monkeypatch.setattr(voc_dets, "CAPTURE_MIN", 1)
    mgr, det, _ = f32_models
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight("f32"))
    assert eng.batch == B
    srcs = [frame_pixels(200, 330, 300 + i) for i in range(B)]
    mem = [_named("m%d" % i, pixels=s) for i, s in enumerate(srcs)]
    files = []
    for i, s in enumerate(srcs):
        p = str(tmp_path / ("f%d.png" % i))
        PilImage.fromarray(s[:, :, ::-1]).save(p)
        files.append(_named("f%d" % i, path=p, size=s.shape[:2]))
    for kind, imgs in (("mem", mem), ("file", files)):
        resized, ratios = util.resize_imgs(imgs, min_size=320, max_size=540)
        pixels = [eng.host_pixels(r) for r in resized]
        raw = eng.collect_batch(eng.submit_batch(resized, ratios, 0.0, pixels, batch=B, annotate=True))
        runs = eng.collect_batch(eng.submit_batch(resized, ratios, 0.0, pixels, batch=B, annotate=True, encode="png"))
        captures = eng.cache.captures
        huff = eng.collect_batch(eng.submit_batch(resized, ratios, 0.0, pixels, batch=B, annotate=True, encode="png-huffman"))
        assert eng.cache.captures == captures + 1                           # a pass of its own
        again = eng.collect_batch(eng.submit_batch(resized, ratios, 0.0, pixels, batch=B, annotate=True, encode="png-huffman"))
        runs2 = eng.collect_batch(eng.submit_batch(resized, ratios, 0.0, pixels, batch=B, annotate=True, encode="png"))
        assert eng.cache.captures == captures + 1                           # ... and both kinds replay from the cache
        assert len(raw) == len(huff) == B and all(len(r) == 3 for r in huff)
        drawn_any = False
        for (n0, d0, frame), (n1, d1, png), (_, _, png2), (_, _, png_runs), (_, _, png_runs2), src in zip(raw, huff, again, runs, runs2, srcs):
            assert n0 == n1
            same_dets(d1, d0, tol=0.0)
            assert isinstance(png, bytes) and 0 < len(png) <= ops.png_bound(*frame.shape[:2], compress="huffman") and png == png2
            assert png_runs == png_runs2 and png_runs != png
            img = PilImage.open(io.BytesIO(png))
            assert img.mode == "RGB" and img.size == (frame.shape[1], frame.shape[0])
            assert np.array_equal(np.asarray(img), frame[:, :, ::-1] if kind == "mem" else frame), kind
            assert png == R.encode(frame, bgr=kind == "mem")
            drawn_any |= bool((frame != (src if kind == "mem" else src[:, :, ::-1])).any())
        assert drawn_any
    keys = eng.cache.keys()
    assert sum(k[-1:] == ("annotate",) for k in keys) == 2 and sum(k[-2:] == ("annotate", "png") for k in keys) == 2
    assert sum(k[-2:] == ("annotate", "png-huffman") for k in keys) == 2


def test_huffman_encode_needs_annotate(f32_models):
    from faster_rcnn_amd import entry, util
    from faster_rcnn_amd._lib import FrcnnError
    mgr, det, _ = f32_models
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight("f32"))
    resized, ratios = util.resize_imgs([_named("x", pixels=frame_pixels(200, 330, 1))], min_size=320, max_size=540)
    pixels = [eng.host_pixels(resized[0])]
    captures = eng.cache.captures
    with pytest.raises(FrcnnError):
        eng.submit_batch(resized, ratios, 0.0, pixels, batch=1, encode="png-huffman")
    with pytest.raises(FrcnnError):
        eng.submit_batch(resized, ratios, 0.0, pixels, batch=1, annotate=True, encode="png-lz77")
    assert eng.cache.captures == captures


def test_main_png_compress_huffman(f32_models, tmp_path):
    """``annotate_video --png_encoder device --png_compress huffman`` against ``--png_encoder host`` on three small PNG files: the same
    printed lines, the same file names, the same pixels, and smaller files than the runs mode's."""
    from faster_rcnn_amd import annotate_video
    from faster_rcnn_amd.weights import save_npz
    _, _, w = f32_models
    npz = str(tmp_path / "w.npz")
    save_npz(npz, w)
    d_in = tmp_path / "frames"
    d_in.mkdir()
    names = ["%06d.png" % i for i in range(3)]
    y, x = np.mgrid[0:180, 0:260]
    for i, name in enumerate(names):                                        # smooth frames with a little noise: something to compress
        f = np.stack([x // 2 + y // 3 + 9 * i, 200 - y + x // 5, (x + 2 * y) // 3], -1) + frame_pixels(180, 260, 40 + i) % 5
        PilImage.fromarray((f % 256).astype(np.uint8)).save(str(d_in / name))
    text, flags = {}, {"host": ["--png_encoder", "host"], "runs": ["--png_encoder", "device"],
                       "huffman": ["--png_encoder", "device", "--png_compress", "huffman"]}
    for leg, extra in flags.items():
        argv = [npz, npz, str(d_in), "--resize_dims", "320,540", "--out_dir", str(tmp_path / leg)] + extra
        _, text[leg] = quiet(annotate_video.main, argv)
        assert sorted(os.listdir(str(tmp_path / leg))) == names
    assert text["host"] == text["huffman"] == text["runs"]
    for name in names:
        host, dev = PilImage.open(str(tmp_path / "host" / name)), PilImage.open(str(tmp_path / "huffman" / name))
        assert dev.mode == "RGB" and np.array_equal(np.asarray(host.convert("RGB")), np.asarray(dev)), name
        data = open(str(tmp_path / "huffman" / name), "rb").read()
        assert data == R.encode(np.asarray(dev))
        assert len(data) < os.path.getsize(str(tmp_path / "runs" / name))
