"""Frames/s of the annotating passes (annotate_video.py) against detection alone, on two model / frame-size pairs:

  kitti_r101_bf16: ResNet-101, bf16, KITTI classes, 375x1242 frames at --resize_dims 600,1500 (BASELINE configs[3])
  voc_r50_f32:     ResNet-50, fp32, VOC classes, 375x500 frames at 600,1000

per pair (a) voc_dets.get_dets_by_cls over N in-memory frames, (b) the same frames through annotating passes (detections + the
frame drawn and read back), (c) annotate_video.annotate_images from PNG files to PNG files, with the host's PNG decode and encode
per frame timed on their own (one thread).  Synthetic weights, dense_class calibrated so that many classes fire.  Prints one
JSON line.  ``--png_encoder device`` (or ``both``) adds leg (c) with the frames encoded inside the pass (ops.png_encode_u8) and the
writer threads only writing bytes, plus the bytes written per frame by either encoder.  ``--png_encoder all`` runs three legs (c) --
host, device with --png_compress runs, device with --png_compress huffman -- ALTERNATING inside every repetition, so that drift of the
machine falls on all three alike.  ``--content photo`` fills the frames with the VOC fixture photograph (tiled to the frame size, shifted
per frame) instead of uniform noise: noise does not compress, so bytes per frame mean something only on the photograph.
``--legs`` names the legs (c) outright, alternating in the same way: besides the three PNG legs, ``jpeg_host`` and ``jpeg_device`` write
``--frame_format jpg`` at quality 90 with PIL on the writer threads and with the device encoder (ops.jpeg_encode_u8) inside the pass.
``jpeg_host_420_opt`` and ``jpeg_device_420_opt`` are the same two with ``jpeg_subsampling=420, jpeg_huffman="optimized"`` (PIL's
``subsampling=2, optimize=True``; the device encoder's csrc/jpeg_opt.hip); every leg reports its bytes per frame.

``--y4m`` runs three file-to-file legs instead (``run_y4m``): a YUV4MPEG2 stream to a YUV4MPEG2 stream, the stream to PNG files (device
encoder) and PNG files to PNG files (host codecs), alternating in one session.

``--redact`` runs the redaction's cost instead (``run_redact``): the same frames with and without ``--redact all --redact_mode blur``
(radius 12, the default), alternating in one session -- through in-memory annotating passes and through annotate_images from PNG files
to PNG files with the device encoder -- and reports the frames/s of both and their ratio.

``--track`` runs the tracker's cost instead (``run_track``): the ``--redact`` leg's frames and redaction without and with ``--track``
(IoU 30 %, hold 8, grow 0, the defaults), alternating in one session through in-memory annotating passes; ``--track_motion`` likewise
(``run_track_motion``) the ``--track`` leg without and with ``--track_motion 8``, and the tracker part of one pass alone; tracking passes replay on one
stream of the engine, so the figure includes what that ordering costs.  ``--detect_every`` (``run_detect_every``) runs the ``--track --track_motion 8`` leg
without and with ``--detect_every 4``.  ``--track_backtrack`` (``run_track_backtrack``) runs the ``--detect_every 4`` leg without and with
``--track_backtrack`` at its default, and times the back-track call of one pass alone.  ``--track_lookback`` (``run_track_lookback``) runs the
``--track --track_motion 8`` leg without and with ``--track_lookback`` at its default (as many frames as a pass holds, at most 8), and the
look-back call of one pass alone.  ``--track_scene_cut`` (``run_track_scene_cut``) runs the ``--track --track_motion 8`` leg without and with
``--track_scene_cut`` at its default.  ``--track_trails`` (``run_track_trails``) runs the same leg without and with ``--track_trails`` at its
defaults.  ``--count_line`` (``run_count_line``) runs the same leg without and with two counting lines.  ``--zone`` (``run_zone``) runs the same leg without and with two rectangular zones of a quarter of the frame each.  ``--heatmap`` (``run_heatmap``) runs the same leg without and with ``--heatmap all`` at its defaults.  ``--remove`` (``run_remove``) runs the same leg without and with ``--remove all`` at its (provisional) defaults.  ``--track_reid`` (``run_track_reid``; ``--track --track_reid`` says the same) runs the same leg without and with ``--track_reid`` at its (provisional) defaults.  ``--out_scale`` (``run_out_scale``) runs in-memory annotating passes, the PNG-file to PNG-file leg (device encoder, huffman) and y4m to y4m, each without and with ``--out_scale 2``.  ``--post`` (``run_post``) runs in-memory annotating passes without and with ``--nms soft_gaussian --box_vote`` (the post-process option, an engine of its own).  ``--redact_shape`` (``run_redact_shape``) runs the ``--redact all --redact_mode blur`` passes without and with ``--redact_shape ellipse --redact_feather 8``.  ``--track_low`` (``run_track_low``) runs the ``--det_threshold 0.5 --track --track_motion 8`` leg without and with ``--track_low 0.1``.  ``--redact_region`` (``run_redact_region``) runs in-memory annotating passes without and with two ``--redact_region`` polygons of a tenth of the frame each, ``--region_mode blur --region_feather 8``.  ``--redact_moving`` (``run_redact_moving``) runs in-memory annotating passes plain, with ``--redact_moving`` (S = 8) and with ``--remove all`` on a generated sequence -- a noise background with a 64 x 64 block that moves 4 pixels a frame.

    python scripts/bench_annotate.py [--frames 256] [--reps 3] [--pairs kitti_r101_bf16,voc_r50_f32] [--png_encoder host|device|both|all]
                                     [--legs host,device_huffman,jpeg_host,jpeg_device,jpeg_host_420_opt,jpeg_device_420_opt,pngdec_host,pngdec_device,pngdec_device_full] [--content noise|photo]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")          # as voc_dets.main / annotate_video.main (read when the runtime starts)

PAIRS = {
    "kitti_r101_bf16": dict(depth=101, dtype="bf16", kitti=True, anchors=(16, 32, 64, 128, 256, 512), hw=(375, 1242), resize=(600, 1500)),
    "voc_r50_f32": dict(depth=50, dtype="f32", kitti=False, anchors=(128, 256, 512), hw=(375, 500), resize=(600, 1000)),
}


def build(cfg):
    import numpy as np
    import torch
    from faster_rcnn_amd import resnet, util
    from faster_rcnn_amd.data.voc_data_helpers import KITTI_CLASS_MAPPING, VOC_CLASS_MAPPING
    from faster_rcnn_amd.det_util import DetTrainingManager
    from faster_rcnn_amd.pipeline import InferencePipeline
    from faster_rcnn_amd.weights import calibrate_classifier, synthetic_resnet
    mapping = KITTI_CLASS_MAPPING if cfg["kitti"] else VOC_CLASS_MAPPING
    C = len(mapping)
    anchors = util.get_anchors(list(cfg["anchors"]))
    dtype = cfg["dtype"] if cfg["dtype"] == "bf16" else None
    kw = {"dtype": dtype} if dtype else {}
    w = synthetic_resnet(cfg["depth"], anchors_per_loc=len(anchors), num_classes=C, seed=1)
    base = (resnet.resnet50_base if cfg["depth"] == 50 else resnet.resnet101_base)(weights=w, **kw)
    rpn = (resnet.resnet50_rpn if cfg["depth"] == 50 else resnet.resnet101_rpn)(base, include_conv=True, anchors_per_loc=len(anchors))
    det = (resnet.resnet50_classifier if cfg["depth"] == 50 else resnet.resnet101_classifier)(64, C, weights=w, **kw)
    x = resnet.preprocess(np.random.RandomState(99).randint(0, 256, (320, 480, 3)).astype(np.uint8))[None].astype(np.float32)
    out = InferencePipeline(rpn, det, anchors).forward_dev(torch.from_numpy(x).cuda())
    n = int(out["n_rois"].item())
    det.get_layer("dense_class_%d" % C).set_weights(calibrate_classifier(w, C, out["cls"][:n].float().cpu().numpy()))
    mgr = DetTrainingManager(rpn_model=rpn, class_mapping=mapping, preprocess_func=resnet.preprocess, anchor_dims=anchors)
    return mgr, det


def annotate_in_memory(eng, resized, ratios, **kwargs):
    """(b): the frames through annotating passes, eng.batch per pass, eng.in_flight passes in flight (annotate_images' loop
    without the files).  ``kwargs``: further arguments of submit_batch (``redact``).  With ``track_lookback`` a flush submit ends the
    list: the passes return the frames of the pass before.  With ``detect_every`` = K a pass takes eng.batch * K frames and every K-th
    of them is one of its images.  ``det_threshold`` (0.0): the score threshold every pass uploads."""
    B, window, frames = eng.batch, [], []
    thr = kwargs.pop("det_threshold", 0.0)
    K = kwargs.get("detect_every") or 1
    for i in range(0, len(resized), B * K):
        part = resized[i:i + B * K]
        window.append(eng.submit_batch(part[::K], ratios[i:i + B * K:K], thr, [eng.host_pixels(r) for r in part], batch=B, annotate=True, **kwargs))
        if len(window) >= eng.in_flight:
            frames += [r[2] for r in eng.collect_batch(window.pop(0))]
    if kwargs.get("track_lookback") is not None or kwargs.get("track_backtrack") is not None:
        window.append(eng.submit_batch([], [], thr, [], batch=B, annotate=True, **kwargs))
    while window:
        frames += [r[2] for r in eng.collect_batch(window.pop(0))]
    assert len(frames) == len(resized)
    return frames


# leg -> annotate_images' options
LEGS = {"host": dict(png_encoder="host", png_compress="runs"), "device": dict(png_encoder="device", png_compress="runs"),
        "device_huffman": dict(png_encoder="device", png_compress="huffman"),
        "jpeg_host": dict(png_encoder="host", png_compress="runs", frame_format="jpg", jpeg_encoder="host", jpeg_quality=90),
        "jpeg_device": dict(png_encoder="host", png_compress="runs", frame_format="jpg", jpeg_encoder="device", jpeg_quality=90),
        "jpeg_host_420_opt": dict(png_encoder="host", png_compress="runs", frame_format="jpg", jpeg_encoder="host", jpeg_quality=90,
                                  jpeg_subsampling=420, jpeg_huffman="optimized"),
        "jpeg_device_420_opt": dict(png_encoder="host", png_compress="runs", frame_format="jpg", jpeg_encoder="device", jpeg_quality=90,
                                    jpeg_subsampling=420, jpeg_huffman="optimized"),
        # who decodes the .png INPUT frames, under the device_huffman output leg: PIL on the decode threads, or csrc/png_dec.hip inside the pass
        "pngdec_host": dict(png_encoder="device", png_compress="huffman", png_decoder="host"),
        "pngdec_device": dict(png_encoder="device", png_compress="huffman", png_decoder="device"),
        # ... or csrc/png_dec_full.hip (the same files here: the leg measures what the third launch and the wider planner cost on them)
        "pngdec_device_full": dict(png_encoder="device", png_compress="huffman", png_decoder="device_full")}


def photo_frames(h, w, n):
    """The VOC fixture photograph tiled to (h, w), shifted by a few pixels per frame (BGR, as cv2 would have read it)."""
    import numpy as np
    from PIL import Image as PilImage
    rgb = np.asarray(PilImage.open(os.path.join(ROOT, "tests", "golden", "VOC_test", "JPEGImages", "000005.jpg")).convert("RGB"))
    big = np.tile(rgb, (-(-h // rgb.shape[0]) + 1, -(-w // rgb.shape[1]) + 1, 1))
    return [np.ascontiguousarray(big[i % 97:i % 97 + h, 3 * i % 211:3 * i % 211 + w, ::-1]) for i in range(n)]


def run_pair(name, cfg, n_frames, reps, encoders=("host",), content="noise"):
    import numpy as np
    from PIL import Image as PilImage
    from faster_rcnn_amd import annotate_video, entry, shapes, util, voc_dets
    mgr, det = build(cfg)
    h, w = cfg["hw"]
    rs = np.random.RandomState(5)
    srcs = photo_frames(h, w, n_frames) if content == "photo" else [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n_frames)]
    imgs = [shapes.Image(shapes.Metadata("f%04d" % i, w, h, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=cfg["resize"][0], max_size=cfg["resize"][1])
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight(cfg["dtype"]))

    def timed(fn):
        with contextlib.redirect_stdout(io.StringIO()):
            fn()                                                    # warm-up: captures
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
        return statistics.median(ts), ts

    ta, tas = timed(lambda: voc_dets.get_dets_by_cls(mgr, det, ratios, resized, det_threshold=0.0))
    tb, tbs = timed(lambda: annotate_in_memory(eng, resized, ratios))
    res = {"frames": n_frames, "frame_hw": [h, w], "resize_dims": list(cfg["resize"]), "dtype": cfg["dtype"], "depth": cfg["depth"],
           "images_per_pass": eng.batch, "in_flight": eng.in_flight,
           "a_get_dets_by_cls_fps": round(n_frames / ta, 1), "b_annotate_fps": round(n_frames / tb, 1),
           "b_over_a": round(ta / tb, 3), "a_runs_s": [round(t, 4) for t in tas], "b_runs_s": [round(t, 4) for t in tbs]}
    with tempfile.TemporaryDirectory() as tmp:
        d_in, d_out = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        os.makedirs(d_in)
        names = ["%06d.png" % i for i in range(n_frames)]
        for nm, s in zip(names, srcs):
            PilImage.fromarray(s[:, :, ::-1]).save(os.path.join(d_in, nm), compress_level=1)
        legs, times, sizes = {}, {enc: [] for enc in encoders}, {}

        def leg(enc):
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                try:
                    annotate_video.annotate_images(mgr, det, d_in, d_out, names, cfg["resize"][0], cfg["resize"][1], **LEGS[enc])
                finally:
                    entry.set_png_decoder(None)                 # (the option is process-wide: the next leg starts from the default)
            return time.perf_counter() - t0

        for enc in encoders:                                        # warm-up: captures
            leg(enc)
        for _ in range(reps):                                       # the legs alternate inside every repetition
            for enc in encoders:
                times[enc].append(leg(enc))
                ext = ".jpg" if LEGS[enc].get("frame_format") == "jpg" else ".png"
                sizes[enc] = sum(os.path.getsize(os.path.join(d_out, nm[:-4] + ext)) for nm in names) // n_frames
        for enc in encoders:
            tag = "c_" if enc == "host" else "c_%s_" % enc
            legs.update({tag + "annotate_images_fps": round(n_frames / statistics.median(times[enc]), 1),
                         tag + "runs_s": [round(t, 4) for t in times[enc]], tag + "bytes_per_frame": sizes[enc]})
        k = min(32, n_frames)
        t0 = time.perf_counter()
        decoded = [annotate_video._read_rgb(os.path.join(d_in, nm)) for nm in names[:k]]
        t_dec = (time.perf_counter() - t0) / k
        t0 = time.perf_counter()
        for nm, f in zip(names[:k], decoded):
            annotate_video._write_png(os.path.join(tmp, "enc_" + nm), f)
        t_enc = (time.perf_counter() - t0) / k
    res.update(legs)
    res.update({"raw_bytes_per_frame": h * w * 3, "content": content, "c_png_decode_ms_per_frame_1thread": round(t_dec * 1e3, 2), "c_png_encode_ms_per_frame_1thread": round(t_enc * 1e3, 2),
                "c_decode_threads": annotate_video.DECODE_THREADS, "c_write_threads": annotate_video.WRITE_THREADS})
    return res


def run_y4m(name, cfg, n_frames, reps, content="noise"):
    """``--y4m``: three file-to-file legs in ONE session, alternating inside every repetition: a YUV4MPEG2 stream to a YUV4MPEG2 stream
    (annotate_stream: the frames converted on the device at both ends of their pass), the same stream to PNG files through the device PNG
    encoder, and the PNG-file to PNG-file leg (c) with the host's codecs, as ``run_pair`` times it.  The input stream is the PNG
    frames' content converted by ops.y4m_encode_u8 (4:2:0, limited range)."""
    import numpy as np
    import torch
    from PIL import Image as PilImage
    from faster_rcnn_amd import annotate_video, ops, y4m
    mgr, det = build(cfg)
    h, w = cfg["hw"]
    rs = np.random.RandomState(5)
    srcs = photo_frames(h, w, n_frames) if content == "photo" else [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n_frames)]
    with tempfile.TemporaryDirectory() as tmp:
        d_in, d_out, clip, clip_out = (os.path.join(tmp, x) for x in ("in", "out", "in.y4m", "out.y4m"))
        os.makedirs(d_in)
        names = ["%06d.png" % i for i in range(n_frames)]
        with open(clip, "wb") as f:
            writer = y4m.Y4mWriter(f, w, h, "420jpeg", "limited", {"F": "25:1"})
            for nm, s in zip(names, srcs):
                PilImage.fromarray(s[:, :, ::-1]).save(os.path.join(d_in, nm), compress_level=1)
                writer.write(ops.y4m_encode_u8(torch.from_numpy(s).cuda(), "420jpeg", "limited", bgr=True).cpu().numpy().tobytes())

        def y4m_to_y4m():
            with open(clip, "rb") as fin, open(clip_out, "wb") as fout:
                reader = y4m.Y4mReader(fin, name=clip)
                sink = y4m.Y4mWriter(fout, w, h, "420jpeg", reader.plan.range_name, reader.plan.tags)
                annotate_video.annotate_stream(mgr, det, reader, sink, *cfg["resize"])

        def y4m_to_png():
            with open(clip, "rb") as fin:
                annotate_video.annotate_stream(mgr, det, y4m.Y4mReader(fin, name=clip), d_out, *cfg["resize"], png_encoder="device")

        def png_to_png():
            annotate_video.annotate_images(mgr, det, d_in, d_out, names, *cfg["resize"], png_encoder="host", png_compress="runs")

        legs = {"y4m_to_y4m": y4m_to_y4m, "y4m_to_png_device": y4m_to_png, "png_to_png_host": png_to_png}
        times = {k: [] for k in legs}
        with contextlib.redirect_stdout(io.StringIO()):
            for fn in legs.values():                                # warm-up: captures
                fn()
            for _ in range(reps):
                for k, fn in legs.items():
                    t0 = time.perf_counter()
                    fn()
                    times[k].append(time.perf_counter() - t0)
    res = {"frames": n_frames, "frame_hw": [h, w], "resize_dims": list(cfg["resize"]), "dtype": cfg["dtype"], "depth": cfg["depth"], "content": content,
           "y4m_bytes_per_frame": y4m.frame_bytes(h, w, "420jpeg")}
    for k, ts in times.items():
        res[k + "_fps"] = round(n_frames / statistics.median(ts), 1)
        res[k + "_runs_s"] = [round(t, 4) for t in ts]
    return res


OUT_SCALE_LEG = ("scale", 2)                             # --out_scale 2


def run_out_scale(name, cfg, n_frames, reps, content="noise"):
    """``--out_scale``: what the scale step (DESIGN §8 "Scale rule") costs and saves.  Three pairs of legs in ONE session, each leg without
    and with ``out_size=("scale", 2)``, all six alternating inside every repetition: (a) annotating passes in memory (``run_pair``'s leg
    (b): with the option the kernel is added and a quarter of the bytes is copied back), (b) PNG files to PNG files through the device
    encoder's huffman mode, (c) a YUV4MPEG2 stream to a YUV4MPEG2 stream.  The kernel alone is not separated from the smaller read-back."""
    import numpy as np
    import torch
    from PIL import Image as PilImage
    from faster_rcnn_amd import annotate_video, entry, ops, shapes, util, y4m
    mgr, det = build(cfg)
    h, w = cfg["hw"]
    h2, w2 = ops.scale_option(OUT_SCALE_LEG, (h, w))
    rs = np.random.RandomState(5)
    srcs = photo_frames(h, w, n_frames) if content == "photo" else [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n_frames)]
    imgs = [shapes.Image(shapes.Metadata("f%04d" % i, w, h, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=cfg["resize"][0], max_size=cfg["resize"][1])
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight(cfg["dtype"]))
    with tempfile.TemporaryDirectory() as tmp:
        d_in, d_out, clip, clip_out = (os.path.join(tmp, x) for x in ("in", "out", "in.y4m", "out.y4m"))
        os.makedirs(d_in)
        names = ["%06d.png" % i for i in range(n_frames)]
        with open(clip, "wb") as f:
            writer = y4m.Y4mWriter(f, w, h, "420jpeg", "limited", {"F": "25:1"})
            for nm, s in zip(names, srcs):
                PilImage.fromarray(s[:, :, ::-1]).save(os.path.join(d_in, nm), compress_level=1)
                writer.write(ops.y4m_encode_u8(torch.from_numpy(s).cuda(), "420jpeg", "limited", bgr=True).cpu().numpy().tobytes())

        def y4m_to_y4m(size, **kw):
            def run():
                with open(clip, "rb") as fin, open(clip_out, "wb") as fout:
                    reader = y4m.Y4mReader(fin, name=clip)
                    sink = y4m.Y4mWriter(fout, size[1], size[0], "420jpeg", reader.plan.range_name, reader.plan.tags)
                    annotate_video.annotate_stream(mgr, det, reader, sink, *cfg["resize"], **kw)
            return run

        png = lambda **kw: lambda: annotate_video.annotate_images(mgr, det, d_in, d_out, names, *cfg["resize"], png_encoder="device",
                                                                  png_compress="huffman", **kw)
        legs = {"a_in_memory": lambda: annotate_in_memory(eng, resized, ratios),
                "a_in_memory_scaled": lambda: annotate_in_memory(eng, resized, ratios, out_size=OUT_SCALE_LEG),
                "b_png_to_png_device_huffman": png(), "b_png_to_png_device_huffman_scaled": png(out_size=OUT_SCALE_LEG),
                "c_y4m_to_y4m": y4m_to_y4m((h, w)), "c_y4m_to_y4m_scaled": y4m_to_y4m((h2, w2), out_size=OUT_SCALE_LEG)}
        times, sizes = {k: [] for k in legs}, {}
        with contextlib.redirect_stdout(io.StringIO()):
            for fn in legs.values():                                # warm-up: captures
                fn()
            for _ in range(reps):
                for k, fn in legs.items():
                    t0 = time.perf_counter()
                    fn()
                    times[k].append(time.perf_counter() - t0)
                    if k.startswith("b_"):
                        sizes[k] = sum(os.path.getsize(os.path.join(d_out, nm)) for nm in names) // n_frames
    res = {"frames": n_frames, "frame_hw": [h, w], "scaled_hw": [h2, w2], "out_size": list(OUT_SCALE_LEG), "resize_dims": list(cfg["resize"]),
           "dtype": cfg["dtype"], "depth": cfg["depth"], "content": content, "images_per_pass": eng.batch, "in_flight": eng.in_flight}
    for k, ts in times.items():
        res[k + "_fps"] = round(n_frames / statistics.median(ts), 1)
        res[k + "_runs_s"] = [round(t, 4) for t in ts]
    for k, v in sizes.items():
        res[k + "_bytes_per_frame"] = v
    for pair in ("a_in_memory", "b_png_to_png_device_huffman", "c_y4m_to_y4m"):
        res[pair + "_scaled_over_plain"] = round(statistics.median(times[pair]) / statistics.median(times[pair + "_scaled"]), 3)
    return res


REDACT_LEG = ("all", "blur", None, 0)                    # --redact all --redact_mode blur


def run_redact(name, cfg, n_frames, reps, content="noise"):
    """``--redact``: what hiding every detected object costs.  Two pairs of legs in ONE session, each pair alternating inside every
    repetition: the frames through in-memory annotating passes (leg (b) of ``run_pair``) without and with ``redact=REDACT_LEG``, and
    annotate_images from PNG files to PNG files (device encoder) without and with it.  Reports frames/s of each and with / without."""
    import numpy as np
    from PIL import Image as PilImage
    from faster_rcnn_amd import annotate_video, entry, shapes, util
    mgr, det = build(cfg)
    h, w = cfg["hw"]
    rs = np.random.RandomState(5)
    srcs = photo_frames(h, w, n_frames) if content == "photo" else [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n_frames)]
    imgs = [shapes.Image(shapes.Metadata("f%04d" % i, w, h, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=cfg["resize"][0], max_size=cfg["resize"][1])
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight(cfg["dtype"]))
    with tempfile.TemporaryDirectory() as tmp:
        d_in, d_out = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        os.makedirs(d_in)
        names = ["%06d.png" % i for i in range(n_frames)]
        for nm, s in zip(names, srcs):
            PilImage.fromarray(s[:, :, ::-1]).save(os.path.join(d_in, nm), compress_level=1)
        files = lambda **kw: annotate_video.annotate_images(mgr, det, d_in, d_out, names, *cfg["resize"], png_encoder="device", **kw)
        legs = {"passes": lambda: annotate_in_memory(eng, resized, ratios),
                "passes_redact": lambda: annotate_in_memory(eng, resized, ratios, redact=REDACT_LEG),
                "files": files, "files_redact": lambda: files(redact=REDACT_LEG)}
        times = {k: [] for k in legs}
        with contextlib.redirect_stdout(io.StringIO()):
            for fn in legs.values():                                # warm-up: captures
                fn()
            for _ in range(reps):
                for k, fn in legs.items():
                    t0 = time.perf_counter()
                    fn()
                    times[k].append(time.perf_counter() - t0)
        hidden = annotate_in_memory(eng, resized[:eng.batch], ratios[:eng.batch], redact=REDACT_LEG)
        share = float(np.mean([(a != b).any(axis=2).mean() for a, b in zip(hidden, annotate_in_memory(eng, resized[:eng.batch], ratios[:eng.batch]))]))
    res = {"frames": n_frames, "frame_hw": [h, w], "resize_dims": list(cfg["resize"]), "dtype": cfg["dtype"], "depth": cfg["depth"], "content": content,
           "redact": ["all", "blur", 12, 0], "images_per_pass": eng.batch, "in_flight": eng.in_flight, "pixels_changed_share": round(share, 3)}
    for k, ts in times.items():
        res[k + "_fps"] = round(n_frames / statistics.median(ts), 1)
        res[k + "_runs_s"] = [round(t, 4) for t in ts]
    for k in ("passes", "files"):
        res[k + "_redact_over_plain"] = round(statistics.median(times[k]) / statistics.median(times[k + "_redact"]), 3)
    return res


REDACT_SHAPE_LEG = ("ellipse", 8)                        # --redact_shape ellipse --redact_feather 8


def run_redact_shape(name, cfg, n_frames, reps, content="noise"):
    """``--redact_shape``: what the shaped, soft-edged redaction (DESIGN §8 "Shape rule") costs against the plain one.  One pair of legs in
    ONE session, alternating inside every repetition: the ``--redact`` leg's frames through in-memory annotating passes with
    ``redact=REDACT_LEG``, without and with ``redact_shape=REDACT_SHAPE_LEG``.  Reports frames/s of both, their ratio and the share of
    the pixels each changes.  Not separated: the phase-two kernel alone, and photo content (on noise frames the detector fires all over
    the frame, so most tiles meet a box or a ring)."""
    import numpy as np
    from faster_rcnn_amd import entry, shapes, util
    mgr, det = build(cfg)
    h, w = cfg["hw"]
    rs = np.random.RandomState(5)
    srcs = photo_frames(h, w, n_frames) if content == "photo" else [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n_frames)]
    imgs = [shapes.Image(shapes.Metadata("f%04d" % i, w, h, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=cfg["resize"][0], max_size=cfg["resize"][1])
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight(cfg["dtype"]))
    legs = {"redact": lambda: annotate_in_memory(eng, resized, ratios, redact=REDACT_LEG),
            "redact_shape": lambda: annotate_in_memory(eng, resized, ratios, redact=REDACT_LEG, redact_shape=REDACT_SHAPE_LEG)}
    times = {k: [] for k in legs}
    for fn in legs.values():                                        # warm-up: captures
        fn()
    for _ in range(reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    few = slice(0, eng.batch)
    plain = annotate_in_memory(eng, resized[few], ratios[few])
    share = {k: float(np.mean([(a != b).any(axis=2).mean() for a, b in zip(annotate_in_memory(eng, resized[few], ratios[few], redact=REDACT_LEG, **kw), plain)]))
             for k, kw in (("redact", {}), ("redact_shape", {"redact_shape": REDACT_SHAPE_LEG}))}
    res = {"frames": n_frames, "frame_hw": [h, w], "resize_dims": list(cfg["resize"]), "dtype": cfg["dtype"], "depth": cfg["depth"], "content": content,
           "redact": ["all", "blur", 12, 0], "redact_shape": list(REDACT_SHAPE_LEG), "images_per_pass": eng.batch, "in_flight": eng.in_flight,
           "pixels_changed_share": {k: round(v, 3) for k, v in share.items()}}
    for k, ts in times.items():
        res[k + "_fps"] = round(n_frames / statistics.median(ts), 1)
        res[k + "_runs_s"] = [round(t, 4) for t in ts]
    res["shape_over_redact"] = round(statistics.median(times["redact"]) / statistics.median(times["redact_shape"]), 3)
    return res


def region_leg(h, w):
    """Two polygons of about a tenth of the frame each -- a band along the bottom (a bonnet) and a triangle in the top right corner (a
    house window seen at an angle) --, ``--region_mode blur --region_feather 8``."""
    band = ((0, h - h // 10), (w, h - h // 10), (w, h), (0, h))
    side = int((0.2 * h * w) ** 0.5)                     # a right triangle of legs ``side``: a tenth of the frame
    corner = ((w - side, 0), (w, 0), (w, side))
    return (band, corner), None, "blur", None, 8


def run_redact_region(name, cfg, n_frames, reps, content="noise"):
    """``--redact_region``: what hiding static areas (DESIGN §8 "Region rule") costs.  One pair of legs in ONE session, alternating inside
    every repetition: in-memory annotating passes without and with ``redact_region=region_leg(h, w)``.  Reports frames/s of both, their
    ratio and the share of the pixels the option changes.  Not separated: the apply kernel alone, and photo content."""
    import numpy as np
    from faster_rcnn_amd import entry, shapes, util
    mgr, det = build(cfg)
    h, w = cfg["hw"]
    rs = np.random.RandomState(5)
    srcs = photo_frames(h, w, n_frames) if content == "photo" else [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n_frames)]
    imgs = [shapes.Image(shapes.Metadata("f%04d" % i, w, h, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=cfg["resize"][0], max_size=cfg["resize"][1])
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight(cfg["dtype"]))
    leg = region_leg(h, w)
    legs = {"plain": lambda: annotate_in_memory(eng, resized, ratios),
            "redact_region": lambda: annotate_in_memory(eng, resized, ratios, redact_region=leg)}
    times = {k: [] for k in legs}
    for fn in legs.values():                                        # warm-up: captures, and the plane
        fn()
    for _ in range(reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    few = slice(0, eng.batch)
    plain = annotate_in_memory(eng, resized[few], ratios[few])
    share = float(np.mean([(a != b).any(axis=2).mean() for a, b in zip(annotate_in_memory(eng, resized[few], ratios[few], redact_region=leg), plain)]))
    res = {"frames": n_frames, "frame_hw": [h, w], "resize_dims": list(cfg["resize"]), "dtype": cfg["dtype"], "depth": cfg["depth"], "content": content,
           "redact_region": {"regions": [list(map(list, p)) for p in leg[0]], "mode": "blur", "size": 12, "feather": 8},
           "images_per_pass": eng.batch, "in_flight": eng.in_flight, "pixels_changed_share": round(share, 3)}
    for k, ts in times.items():
        res[k + "_fps"] = round(n_frames / statistics.median(ts), 1)
        res[k + "_runs_s"] = [round(t, 4) for t in ts]
    res["region_over_plain"] = round(statistics.median(times["plain"]) / statistics.median(times["redact_region"]), 3)
    return res


def moving_frames(h, w, n):
    """A generated fixed-camera sequence: one noise background, and a 64 x 64 block of other noise that moves 4 pixels a frame along a
    row in the middle (wrapping), so that the plate settles and the net really hides something."""
    import numpy as np
    rs = np.random.RandomState(5)
    back, block = rs.randint(0, 256, (h, w, 3)).astype(np.uint8), rs.randint(0, 256, (64, 64, 3)).astype(np.uint8)
    y, out = max((h - 64) // 2, 0), []
    for i in range(n):
        a, x = back.copy(), (4 * i) % max(w - 64, 1)
        a[y:y + 64, x:x + 64] = block[:min(64, h - y), :min(64, w - x)]
        out.append(a)
    return out


def run_redact_moving(name, cfg, n_frames, reps, content="generated"):
    """``--redact_moving``: what the moving net (DESIGN §8 "Moving rule") costs.  Three legs in ONE session, alternating inside every
    repetition, on ``moving_frames`` (noise frames never settle a plate): in-memory annotating passes plain, with ``redact_moving`` at its
    defaults and S = 8, and with ``remove=("all", 8, 10, 8)`` on the same frames; plate and moving state are reset in front of every run.
    Reports frames/s of each, the ratios and the mean share of the frame the net hid.  Not separated: the three build kernels alone, the
    plate update a pass without ``remove`` now runs, and real content."""
    import numpy as np
    from faster_rcnn_amd import entry, ops, shapes, util
    mgr, det = build(cfg)
    h, w = cfg["hw"]
    srcs = moving_frames(h, w, n_frames)
    imgs = [shapes.Image(shapes.Metadata("f%04d" % i, w, h, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=cfg["resize"][0], max_size=cfg["resize"][1])
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight(cfg["dtype"]))
    moving = ops.redact_moving_option(settle=8)

    def leg(**kw):
        def run():
            eng.plate_reset()
            eng.moving_reset()
            return annotate_in_memory(eng, resized, ratios, **kw)
        return run

    legs = {"plain": leg(), "redact_moving": leg(redact_moving=moving), "remove": leg(remove=ops.plate_option("all"))}
    times = {k: [] for k in legs}
    for fn in legs.values():                                        # warm-up: captures
        fn()
    for _ in range(reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    hidden = [float((a != b).any(axis=2).mean()) for a, b in zip(legs["redact_moving"](), legs["plain"]())]      # (both draw the same boxes)
    res = {"frames": n_frames, "frame_hw": [h, w], "resize_dims": list(cfg["resize"]), "dtype": cfg["dtype"], "depth": cfg["depth"],
           "content": "generated: noise background, a 64x64 block moving 4 px a frame", "redact_moving": list(moving),
           "images_per_pass": eng.batch, "in_flight": eng.in_flight, "pixels_changed_share_mean": round(float(np.mean(hidden)), 4),
           "pixels_changed_share_peak": round(max(hidden), 4)}
    for k, ts in times.items():
        res[k + "_fps"] = round(n_frames / statistics.median(ts), 1)
        res[k + "_runs_s"] = [round(t, 4) for t in ts]
    res["moving_over_plain"] = round(statistics.median(times["plain"]) / statistics.median(times["redact_moving"]), 3)
    res["moving_over_remove"] = round(statistics.median(times["remove"]) / statistics.median(times["redact_moving"]), 3)
    return res


TRACK_LEG = (30, 8, 0)                                   # --track with its defaults


def run_track(name, cfg, n_frames, reps, content="noise"):
    """``--track``: what tracking costs on top of the redaction.  One pair of legs in ONE session, alternating inside every repetition:
    the ``--redact`` leg's frames through in-memory annotating passes with ``redact=REDACT_LEG``, without and with ``track=TRACK_LEG``
    (the tracker is reset in front of every tracked run).  Reports frames/s of both, with / without, and what the tracker saw."""
    import numpy as np
    from faster_rcnn_amd import entry, shapes, util
    mgr, det = build(cfg)
    h, w = cfg["hw"]
    rs = np.random.RandomState(5)
    srcs = photo_frames(h, w, n_frames) if content == "photo" else [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n_frames)]
    imgs = [shapes.Image(shapes.Metadata("f%04d" % i, w, h, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=cfg["resize"][0], max_size=cfg["resize"][1])
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight(cfg["dtype"]))

    def tracked():
        eng.track_reset()
        return annotate_in_memory(eng, resized, ratios, redact=REDACT_LEG, track=TRACK_LEG)

    legs = {"redact": lambda: annotate_in_memory(eng, resized, ratios, redact=REDACT_LEG), "redact_track": tracked}
    times = {k: [] for k in legs}
    for fn in legs.values():                                        # warm-up: captures
        fn()
    for _ in range(reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    import torch
    torch.cuda.synchronize()
    state = eng.track_state().cpu().numpy()
    res = {"frames": n_frames, "frame_hw": [h, w], "resize_dims": list(cfg["resize"]), "dtype": cfg["dtype"], "depth": cfg["depth"], "content": content,
           "redact": ["all", "blur", 12, 0], "track": list(TRACK_LEG), "images_per_pass": eng.batch, "in_flight": eng.in_flight,
           "tracker": {"live_slots": int(state[0]), "ids_issued": int(state[1]), "overflow": int(state[2]), "frames": int(state[3])}}
    for k, ts in times.items():
        res[k + "_fps"] = round(n_frames / statistics.median(ts), 1)
        res[k + "_runs_s"] = [round(t, 4) for t in ts]
    res["track_over_plain"] = round(statistics.median(times["redact"]) / statistics.median(times["redact_track"]), 3)
    return res


MOTION_LEG = 8                                           # --track_motion with its default radius


def tracker_part_us(eng, h, w, radius, iters=20):
    """HIP-event time of the tracker part of ONE pass of eng.batch frames, outside a graph: a copy of the engine's tracker state as the
    run left it, every live slot detected again where it is (so the slots stay), noise frames; ``radius`` None: ops.track_update (one
    launch), else ops.track_update_motion (2 B + 1 launches, the kept frame primed by a first call).  -> the median in microseconds."""
    import numpy as np
    import torch
    from faster_rcnn_amd import ops
    B, rows = eng.batch, 300
    words = eng.track_state().cpu().numpy()
    cap, n = (words.size - 4) // 8, int(words[0])
    packed = np.zeros(4 + 7 * rows, dtype=np.int32)
    packed[0] = n
    packed[4:4 + 4 * n] = words[4 + 2 * cap:4 + 2 * cap + 4 * n]
    packed[4 + 4 * rows:4 + 4 * rows + n] = words[4 + cap:4 + cap + n]
    packed[4 + 5 * rows:4 + 5 * rows + n] = words[4 + 6 * cap:4 + 6 * cap + n]
    dets = torch.from_numpy(np.stack([packed] * B)).cuda()
    frames = torch.from_numpy(np.random.RandomState(9).randint(0, 256, (B, h * w * 3)).astype(np.uint8)).cuda()
    nf = torch.tensor([B], dtype=torch.int32, device="cuda")
    table, mstate = eng.track_table("all"), ops.track_motion_state(h, w)
    out = torch.zeros((B, 4 + 8 * (rows + cap)), dtype=torch.int32, device="cuda")
    start = torch.from_numpy(words).cuda()

    def once(state):
        if radius is None:
            ops.track_update(state, dets, nf, table, h, w, *TRACK_LEG, out=out)
        else:
            ops.track_update_motion(state, mstate, frames, h * w * 3, dets, nf, table, h, w, *TRACK_LEG, radius, out=out)

    state = start.clone()
    once(state)                                                     # (primes the kept frame; the state's frame count and the header agree)
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        once(state)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1000.0)
    return round(statistics.median(times), 1), n


def run_track_motion(name, cfg, n_frames, reps, content="noise"):
    """``--track_motion``: what the motion step costs on top of tracking.  One pair of legs in ONE session, alternating inside every
    repetition: ``run_track``'s frames through in-memory annotating passes with ``redact=REDACT_LEG, track=TRACK_LEG``, without and with
    ``track_motion=MOTION_LEG`` (the tracker is reset in front of every run).  Reports frames/s of both and their ratio, the tracker's
    state at the end, and the HIP-event time of the tracker part of one pass both ways (``tracker_part_us``)."""
    import numpy as np
    from faster_rcnn_amd import entry, shapes, util
    mgr, det = build(cfg)
    h, w = cfg["hw"]
    rs = np.random.RandomState(5)
    srcs = photo_frames(h, w, n_frames) if content == "photo" else [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n_frames)]
    imgs = [shapes.Image(shapes.Metadata("f%04d" % i, w, h, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=cfg["resize"][0], max_size=cfg["resize"][1])
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight(cfg["dtype"]))

    def leg(**kw):
        def run():
            eng.track_reset()
            return annotate_in_memory(eng, resized, ratios, redact=REDACT_LEG, track=TRACK_LEG, **kw)
        return run

    legs = {"track": leg(), "track_motion": leg(track_motion=MOTION_LEG)}
    times = {k: [] for k in legs}
    for fn in legs.values():                                        # warm-up: captures
        fn()
    for _ in range(reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    import torch
    torch.cuda.synchronize()
    state = eng.track_state().cpu().numpy()
    res = {"frames": n_frames, "frame_hw": [h, w], "resize_dims": list(cfg["resize"]), "dtype": cfg["dtype"], "depth": cfg["depth"], "content": content,
           "redact": ["all", "blur", 12, 0], "track": list(TRACK_LEG), "track_motion": MOTION_LEG, "images_per_pass": eng.batch,
           "in_flight": eng.in_flight,
           "tracker": {"live_slots": int(state[0]), "ids_issued": int(state[1]), "overflow": int(state[2]), "frames": int(state[3])}}
    for k, ts in times.items():
        res[k + "_fps"] = round(n_frames / statistics.median(ts), 1)
        res[k + "_runs_s"] = [round(t, 4) for t in ts]
    res["motion_over_track"] = round(statistics.median(times["track"]) / statistics.median(times["track_motion"]), 3)
    res["tracker_part_us"] = {"track_update": tracker_part_us(eng, h, w, None)[0]}
    res["tracker_part_us"]["track_update_motion"], res["tracker_part_us"]["live_slots"] = tracker_part_us(eng, h, w, MOTION_LEG)
    return res


def run_track_scene_cut(name, cfg, n_frames, reps, content="noise"):
    """``--track_scene_cut``: what the cut rule costs on top of ``--track --track_motion 8``.  One pair of legs in ONE session, alternating
    inside every repetition: ``run_track_motion``'s ``track_motion`` leg without and with ``track_scene_cut`` at its default (the tracker
    is reset in front of every run).  Reports frames/s of both, their ratio, the tracker's state at the end and the cuts the last run
    with the option saw (independent noise frames of this size differ by a small share of the largest distance: none is expected)."""
    import numpy as np
    from faster_rcnn_amd import entry, ops, shapes, util
    mgr, det = build(cfg)
    h, w = cfg["hw"]
    rs = np.random.RandomState(5)
    srcs = photo_frames(h, w, n_frames) if content == "photo" else [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n_frames)]
    imgs = [shapes.Image(shapes.Metadata("f%04d" % i, w, h, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=cfg["resize"][0], max_size=cfg["resize"][1])
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight(cfg["dtype"]))
    pct = ops.track_cut_option()
    cuts = [0]
    collect = eng.collect_batch

    def counting(ticket):                                           # (the marks ride behind every frame's payload)
        res = collect(ticket)
        cuts[0] += sum(1 for r in res if len(r) > 3 and r[3].get("scene_cut"))
        return res

    eng.collect_batch = counting

    def leg(**kw):
        def run():
            eng.track_reset()
            cuts[0] = 0
            return annotate_in_memory(eng, resized, ratios, redact=REDACT_LEG, track=TRACK_LEG, track_motion=MOTION_LEG, **kw)
        return run

    legs = {"track_motion": leg(), "track_scene_cut": leg(track_scene_cut=pct)}
    times = {k: [] for k in legs}
    for fn in legs.values():                                        # warm-up: captures
        fn()
    for _ in range(reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    import torch
    torch.cuda.synchronize()
    state = eng.track_state().cpu().numpy()
    res = {"frames": n_frames, "frame_hw": [h, w], "resize_dims": list(cfg["resize"]), "dtype": cfg["dtype"], "depth": cfg["depth"], "content": content,
           "redact": ["all", "blur", 12, 0], "track": list(TRACK_LEG), "track_motion": MOTION_LEG, "track_scene_cut": pct,
           "images_per_pass": eng.batch, "in_flight": eng.in_flight, "cuts_seen": cuts[0],
           "tracker": {"live_slots": int(state[0]), "ids_issued": int(state[1]), "overflow": int(state[2]), "frames": int(state[3])}}
    for k, ts in times.items():
        res[k + "_fps"] = round(n_frames / statistics.median(ts), 1)
        res[k + "_runs_s"] = [round(t, 4) for t in ts]
    res["cut_over_motion"] = round(statistics.median(times["track_motion"]) / statistics.median(times["track_scene_cut"]), 3)
    return res


def run_track_trails(name, cfg, n_frames, reps, content="noise"):
    """``--track_trails``: what the trails cost on top of ``--track --track_motion 8``.  One pair of legs in ONE session, alternating inside
    every repetition: ``run_track_motion``'s ``track_motion`` leg without and with ``track_trails`` at its defaults (the tracker, and with
    it the trail state, is reset in front of every run).  Reports frames/s of both, their ratio and the trail state at the end.  Not
    separated: the draw kernel alone, and photo content (independent noise frames keep few ids for long, so few trails grow long)."""
    import numpy as np
    from faster_rcnn_amd import entry, ops, shapes, util
    mgr, det = build(cfg)
    h, w = cfg["hw"]
    rs = np.random.RandomState(5)
    srcs = photo_frames(h, w, n_frames) if content == "photo" else [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n_frames)]
    imgs = [shapes.Image(shapes.Metadata("f%04d" % i, w, h, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=cfg["resize"][0], max_size=cfg["resize"][1])
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight(cfg["dtype"]))
    trails = ops.track_trails_option()

    def leg(**kw):
        def run():
            eng.track_reset()
            return annotate_in_memory(eng, resized, ratios, redact=REDACT_LEG, track=TRACK_LEG, track_motion=MOTION_LEG, **kw)
        return run

    legs = {"track_motion": leg(), "track_trails": leg(track_trails=trails)}
    times = {k: [] for k in legs}
    for fn in legs.values():                                        # warm-up: captures
        fn()
    for _ in range(reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    import torch
    torch.cuda.synchronize()
    state = eng.track_trails_state(trails[0]).cpu().numpy()
    ew = 4 + 2 * trails[0]
    res = {"frames": n_frames, "frame_hw": [h, w], "resize_dims": list(cfg["resize"]), "dtype": cfg["dtype"], "depth": cfg["depth"], "content": content,
           "redact": ["all", "blur", 12, 0], "track": list(TRACK_LEG), "track_motion": MOTION_LEG, "track_trails": list(trails),
           "images_per_pass": eng.batch, "in_flight": eng.in_flight,
           "trails": {"entries": int(state[0]), "frames": int(state[1]), "dropped": int(state[2]),
                      "longest": int(max([state[4 + k * ew + 3] for k in range(int(state[0]))], default=0))}}
    for k, ts in times.items():
        res[k + "_fps"] = round(n_frames / statistics.median(ts), 1)
        res[k + "_runs_s"] = [round(t, 4) for t in ts]
    res["trails_over_motion"] = round(statistics.median(times["track_motion"]) / statistics.median(times["track_trails"]), 3)
    return res


WEAK_LEG = (0.5, 0.1)                                     # --det_threshold T --track_low L


def run_track_low(name, cfg, n_frames, reps, content="noise"):
    """``--track_low``: what the weak rule costs on top of ``--det_threshold 0.5 --track --track_motion 8 --redact all --redact_mode blur``.
    One pair of legs in ONE session, alternating inside every repetition: the passes at det_threshold 0.5, and the passes at det_threshold
    0.1 with ``track_strong=0.5`` (the tracker is reset in front of every run).  Reports frames/s of both, their ratio, and the rows the
    last weak run emitted.  The second leg's post-process emits MORE rows (everything down to 0.1), so the figure is the cost of the
    option as a user meets it, not of the kernel's stage B alone.  Not measured: real footage (missed frames, id switches)."""
    import numpy as np
    from faster_rcnn_amd import entry, shapes, util
    mgr, det = build(cfg)
    h, w = cfg["hw"]
    rs = np.random.RandomState(5)
    srcs = photo_frames(h, w, n_frames) if content == "photo" else [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n_frames)]
    imgs = [shapes.Image(shapes.Metadata("f%04d" % i, w, h, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=cfg["resize"][0], max_size=cfg["resize"][1])
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight(cfg["dtype"]))
    T, L = WEAK_LEG

    def leg(**kw):
        def run():
            eng.track_reset()
            return annotate_in_memory(eng, resized, ratios, redact=REDACT_LEG, track=TRACK_LEG, track_motion=MOTION_LEG, **kw)
        return run

    legs = {"det_threshold": leg(det_threshold=T), "track_low": leg(det_threshold=L, track_strong=T)}
    times = {k: [] for k in legs}
    for fn in legs.values():                                        # warm-up: captures
        fn()
    for _ in range(reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    import torch
    torch.cuda.synchronize()
    state = eng.track_state().cpu().numpy()
    res = {"frames": n_frames, "frame_hw": [h, w], "resize_dims": list(cfg["resize"]), "dtype": cfg["dtype"], "depth": cfg["depth"], "content": content,
           "redact": ["all", "blur", 12, 0], "track": list(TRACK_LEG), "track_motion": MOTION_LEG, "det_threshold": T, "track_low": L,
           "images_per_pass": eng.batch, "in_flight": eng.in_flight,
           "tracker_after_track_low": {"slots": int(state[0]), "ids_issued": int(state[1]), "overflow": int(state[2]), "frames": int(state[3])}}
    for k, ts in times.items():
        res[k + "_fps"] = round(n_frames / statistics.median(ts), 1)
        res[k + "_runs_s"] = [round(t, 4) for t in ts]
    res["track_low_over_det_threshold"] = round(statistics.median(times["det_threshold"]) / statistics.median(times["track_low"]), 3)
    return res


def run_heatmap(name, cfg, n_frames, reps, content="noise"):
    """``--heatmap``: what the heat map costs on top of ``--track --track_motion 8``.  One pair of legs in ONE session, alternating inside
    every repetition: ``run_track_motion``'s ``track_motion`` leg without and with ``heat=("all", 160, 0)`` (the tracker and the map are
    reset in front of every run).  Reports frames/s of both, their ratio and the state at the end.  Not separated: the update kernel
    alone, and photo content (noise frames give a full table of tracks all over the frame: every tile of the map meets boxes)."""
    import numpy as np
    from faster_rcnn_amd import entry, ops, shapes, util
    mgr, det = build(cfg)
    h, w = cfg["hw"]
    rs = np.random.RandomState(5)
    srcs = photo_frames(h, w, n_frames) if content == "photo" else [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n_frames)]
    imgs = [shapes.Image(shapes.Metadata("f%04d" % i, w, h, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=cfg["resize"][0], max_size=cfg["resize"][1])
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight(cfg["dtype"]))
    heat = ops.heat_option("all")

    def leg(**kw):
        def run():
            eng.track_reset()
            eng.heat_reset()
            return annotate_in_memory(eng, resized, ratios, redact=REDACT_LEG, track=TRACK_LEG, track_motion=MOTION_LEG, **kw)
        return run

    legs = {"track_motion": leg(), "heatmap": leg(heat=heat)}
    times = {k: [] for k in legs}
    for fn in legs.values():                                        # warm-up: captures
        fn()
    for _ in range(reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    import torch
    torch.cuda.synchronize()
    frames, peak, saturated, heat_map = ops.heat_map(eng.heat_state(h, w).cpu().numpy(), h, w)
    res = {"frames": n_frames, "frame_hw": [h, w], "resize_dims": list(cfg["resize"]), "dtype": cfg["dtype"], "depth": cfg["depth"], "content": content,
           "redact": ["all", "blur", 12, 0], "track": list(TRACK_LEG), "track_motion": MOTION_LEG, "heat": list(heat),
           "images_per_pass": eng.batch, "in_flight": eng.in_flight,
           "map": {"frames": frames, "peak": peak, "saturated": saturated, "warm_pixels": int((heat_map > 0).sum()), "pixels": h * w}}
    for k, ts in times.items():
        res[k + "_fps"] = round(n_frames / statistics.median(ts), 1)
        res[k + "_runs_s"] = [round(t, 4) for t in ts]
    res["heatmap_over_motion"] = round(statistics.median(times["track_motion"]) / statistics.median(times["heatmap"]), 3)
    return res


def run_remove(name, cfg, n_frames, reps, content="noise"):
    """``--remove``: what the background plate costs on top of ``--track --track_motion 8``.  One pair of legs in ONE session, alternating
    inside every repetition: ``run_track_motion``'s ``track_motion`` leg without and with ``remove=("all", 8, 10, 8)`` (the tracker and
    the plate are reset in front of every run).  Reports frames/s of both, their ratio and the state at the end.  Not separated: the
    update kernel alone, and real content -- noise frames never settle at T = 10, so ``known`` stays 0 and the leg measures the
    streaming cost of the update (8 B of state in and out and 3 B of frame per pixel) and of the box staging, not the fill."""
    import numpy as np
    from faster_rcnn_amd import entry, ops, shapes, util
    mgr, det = build(cfg)
    h, w = cfg["hw"]
    rs = np.random.RandomState(5)
    srcs = photo_frames(h, w, n_frames) if content == "photo" else [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n_frames)]
    imgs = [shapes.Image(shapes.Metadata("f%04d" % i, w, h, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=cfg["resize"][0], max_size=cfg["resize"][1])
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight(cfg["dtype"]))
    remove = ops.plate_option("all")

    def leg(**kw):
        def run():
            eng.track_reset()
            eng.plate_reset()
            return annotate_in_memory(eng, resized, ratios, redact=REDACT_LEG, track=TRACK_LEG, track_motion=MOTION_LEG, **kw)
        return run

    legs = {"track_motion": leg(), "remove": leg(remove=remove)}
    times = {k: [] for k in legs}
    for fn in legs.values():                                        # warm-up: captures
        fn()
    for _ in range(reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    import torch
    torch.cuda.synchronize()
    frames, known, _, _ = ops.plate_image(eng.plate_state(h, w), h, w)
    res = {"frames": n_frames, "frame_hw": [h, w], "resize_dims": list(cfg["resize"]), "dtype": cfg["dtype"], "depth": cfg["depth"], "content": content,
           "redact": ["all", "blur", 12, 0], "track": list(TRACK_LEG), "track_motion": MOTION_LEG, "remove": list(remove),
           "images_per_pass": eng.batch, "in_flight": eng.in_flight, "plate": {"frames": frames, "known": known, "pixels": h * w}}
    for k, ts in times.items():
        res[k + "_fps"] = round(n_frames / statistics.median(ts), 1)
        res[k + "_runs_s"] = [round(t, 4) for t in ts]
    res["remove_over_motion"] = round(statistics.median(times["track_motion"]) / statistics.median(times["remove"]), 3)
    return res


def run_track_reid(name, cfg, n_frames, reps, content="noise"):
    """``--track_reid``: what the re-identify stage costs on top of ``--track --track_motion 8``.  One pair of legs in ONE session,
    alternating inside every repetition: ``run_track_motion``'s ``track_motion`` leg without and with ``track_reid=(25, 250)`` (the
    tracker, and with it the re-identify state, is reset in front of every run).  Reports frames/s of both, their ratio and the state's
    sums at the end.  Noise frames are the dear case for the step kernel: tracks are born in every frame, and each birth takes a turn of
    its one workgroup; what real footage costs is not measured."""
    import numpy as np
    from faster_rcnn_amd import entry, ops, shapes, util
    mgr, det = build(cfg)
    h, w = cfg["hw"]
    rs = np.random.RandomState(5)
    srcs = photo_frames(h, w, n_frames) if content == "photo" else [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n_frames)]
    imgs = [shapes.Image(shapes.Metadata("f%04d" % i, w, h, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=cfg["resize"][0], max_size=cfg["resize"][1])
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight(cfg["dtype"]))
    reid = ops.track_reid_option()

    def leg(**kw):
        def run():
            eng.track_reset()
            return annotate_in_memory(eng, resized, ratios, redact=REDACT_LEG, track=TRACK_LEG, track_motion=MOTION_LEG, **kw)
        return run

    legs = {"track_motion": leg(), "track_reid": leg(track_reid=reid)}
    times = {k: [] for k in legs}
    for fn in legs.values():                                        # warm-up: captures
        fn()
    for _ in range(reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    import torch
    torch.cuda.synchronize()
    res = {"frames": n_frames, "frame_hw": [h, w], "resize_dims": list(cfg["resize"]), "dtype": cfg["dtype"], "depth": cfg["depth"], "content": content,
           "redact": ["all", "blur", 12, 0], "track": list(TRACK_LEG), "track_motion": MOTION_LEG, "track_reid": list(reid),
           "images_per_pass": eng.batch, "in_flight": eng.in_flight, "reid": ops.track_reid_totals(eng.reid_state())}
    for k, ts in times.items():
        res[k + "_fps"] = round(n_frames / statistics.median(ts), 1)
        res[k + "_runs_s"] = [round(t, 4) for t in ts]
    res["track_reid_over_motion"] = round(statistics.median(times["track_motion"]) / statistics.median(times["track_reid"]), 3)
    return res


POST_LEG = ("soft_gaussian", None, None, None, 0.5)        # --nms soft_gaussian --box_vote, everything else at its (provisional) default


def run_post(name, cfg, n_frames, reps, content="noise"):
    """``--post``: what soft-NMS and box voting cost inside the passes.  One pair of legs in ONE session, alternating inside every
    repetition: the frames through in-memory annotating passes (leg (b) of ``run_pair``) on the engine without the option and on the
    engine with ``post=POST_LEG`` (an engine of its own: DESIGN §8 "Post-process rule").  Noise frames give about 300 detections a frame,
    the worst case for the pick loop.  Reports frames/s of each (medians), without / with, and the detections a frame of each leg has."""
    import numpy as np
    from faster_rcnn_amd import entry, ops, shapes, util
    mgr, det = build(cfg)
    h, w = cfg["hw"]
    rs = np.random.RandomState(5)
    srcs = photo_frames(h, w, n_frames) if content == "photo" else [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n_frames)]
    imgs = [shapes.Image(shapes.Metadata("f%04d" % i, w, h, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=cfg["resize"][0], max_size=cfg["resize"][1])
    in_flight = entry.default_in_flight(cfg["dtype"])
    engs = {"plain": entry.for_models(mgr, det, 64, 16, in_flight=in_flight), "post": entry.for_models(mgr, det, 64, 16, in_flight=in_flight, post=POST_LEG)}
    assert engs["plain"] is not engs["post"] and engs["plain"].post is None
    legs = {k: (lambda e=e: annotate_in_memory(e, resized, ratios)) for k, e in engs.items()}
    times = {k: [] for k in legs}
    with contextlib.redirect_stdout(io.StringIO()):
        for fn in legs.values():                                    # warm-up: captures
            fn()
        for _ in range(reps):
            for k, fn in legs.items():
                t0 = time.perf_counter()
                fn()
                times[k].append(time.perf_counter() - t0)
    B = engs["plain"].batch
    dets = {k: [len(r[1]) for r in e.collect_batch(e.submit_batch(resized[:B], ratios[:B], 0.0, [e.host_pixels(r) for r in resized[:B]], batch=B,
                                                                  annotate=True))] for k, e in engs.items()}
    res = {"frames": n_frames, "frame_hw": [h, w], "resize_dims": list(cfg["resize"]), "dtype": cfg["dtype"], "depth": cfg["depth"], "content": content,
           "post": dict(zip(ops.DET_POST_FIELDS, engs["post"].post)), "images_per_pass": B, "in_flight": in_flight,
           "detections_per_frame": {k: round(float(np.mean(v)), 1) for k, v in dets.items()}}
    for k, ts in times.items():
        res[k + "_fps"] = round(n_frames / statistics.median(ts), 1)
        res[k + "_runs_s"] = [round(t, 4) for t in ts]
    res["post_over_plain"] = round(statistics.median(times["plain"]) / statistics.median(times["post"]), 3)
    res["ms_per_frame_added"] = round(1e3 * (statistics.median(times["post"]) - statistics.median(times["plain"])) / n_frames, 4)
    return res


def run_count_line(name, cfg, n_frames, reps, content="noise"):
    """``--count_line``: what counting costs on top of ``--track --track_motion 8``.  One pair of legs in ONE session, alternating inside
    every repetition: ``run_track_motion``'s ``track_motion`` leg without and with ``count`` = two lines (a horizontal and a vertical one
    through the middle of the frame, every class, width 3); the tracker is reset in front of every run and the count state zeroed.
    Reports frames/s of both, their ratio and the count state at the end.  Not separated: the draw kernel alone, and photo content."""
    import numpy as np
    from faster_rcnn_amd import entry, ops, shapes, util
    mgr, det = build(cfg)
    h, w = cfg["hw"]
    rs = np.random.RandomState(5)
    srcs = photo_frames(h, w, n_frames) if content == "photo" else [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n_frames)]
    imgs = [shapes.Image(shapes.Metadata("f%04d" % i, w, h, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=cfg["resize"][0], max_size=cfg["resize"][1])
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight(cfg["dtype"]))
    count = ops.count_option([(0, h // 2, w - 1, h // 2), (w // 2, 0, w // 2, h - 1)])

    def leg(**kw):
        def run():
            eng.track_reset()
            eng.count_reset()
            return annotate_in_memory(eng, resized, ratios, redact=REDACT_LEG, track=TRACK_LEG, track_motion=MOTION_LEG, **kw)
        return run

    legs = {"track_motion": leg(), "count_line": leg(count=count)}
    times = {k: [] for k in legs}
    for fn in legs.values():                                        # warm-up: captures
        fn()
    for _ in range(reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    import torch
    torch.cuda.synchronize()
    state = ops.count_totals(eng.count_state())
    res = {"frames": n_frames, "frame_hw": [h, w], "resize_dims": list(cfg["resize"]), "dtype": cfg["dtype"], "depth": cfg["depth"], "content": content,
           "redact": ["all", "blur", 12, 0], "track": list(TRACK_LEG), "track_motion": MOTION_LEG, "count": [list(map(list, count[0])), count[1], count[2]],
           "images_per_pass": eng.batch, "in_flight": eng.in_flight,
           "counts": {"entries": state["entries"], "frames": state["frames"], "dropped": state["dropped"], "events_dropped": state["events_dropped"],
                      "totals": [list(t) for t in state["totals"][:len(count[0])]]}}
    for k, ts in times.items():
        res[k + "_fps"] = round(n_frames / statistics.median(ts), 1)
        res[k + "_runs_s"] = [round(t, 4) for t in ts]
    res["count_over_motion"] = round(statistics.median(times["track_motion"]) / statistics.median(times["count_line"]), 3)
    return res


def run_zone(name, cfg, n_frames, reps, content="noise"):
    """``--zone``: what the zones cost on top of ``--track --track_motion 8``.  One pair of legs in ONE session, alternating inside every
    repetition: ``run_track_motion``'s ``track_motion`` leg without and with ``zone`` = two rectangles that each cover a quarter of the
    frame (top left and bottom right; every class, width 3, centre anchor); the tracker is reset in front of every run and the zone state
    zeroed.  Reports frames/s of both, their ratio and the zone state at the end.  Not separated: either kernel alone, and photo content."""
    import numpy as np
    from faster_rcnn_amd import entry, ops, shapes, util
    mgr, det = build(cfg)
    h, w = cfg["hw"]
    rs = np.random.RandomState(5)
    srcs = photo_frames(h, w, n_frames) if content == "photo" else [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n_frames)]
    imgs = [shapes.Image(shapes.Metadata("f%04d" % i, w, h, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=cfg["resize"][0], max_size=cfg["resize"][1])
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight(cfg["dtype"]))
    zone = ops.zone_option([[(0, 0), (w // 2, 0), (w // 2, h // 2), (0, h // 2)], [(w // 2, h // 2), (w, h // 2), (w, h), (w // 2, h)]])

    def leg(**kw):
        def run():
            eng.track_reset()
            eng.zone_reset()
            return annotate_in_memory(eng, resized, ratios, redact=REDACT_LEG, track=TRACK_LEG, track_motion=MOTION_LEG, **kw)
        return run

    legs = {"track_motion": leg(), "zone": leg(zone=zone)}
    times = {k: [] for k in legs}
    for fn in legs.values():                                        # warm-up: captures
        fn()
    for _ in range(reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    import torch
    torch.cuda.synchronize()
    state = ops.zone_totals(eng.zone_state())
    n = len(zone[0])
    res = {"frames": n_frames, "frame_hw": [h, w], "resize_dims": list(cfg["resize"]), "dtype": cfg["dtype"], "depth": cfg["depth"], "content": content,
           "redact": ["all", "blur", 12, 0], "track": list(TRACK_LEG), "track_motion": MOTION_LEG,
           "zone": [[list(map(list, zn)) for zn in zone[0]], zone[1], zone[2], zone[3]], "images_per_pass": eng.batch, "in_flight": eng.in_flight,
           "zones": {k: (v[:n] if isinstance(v, list) else v) for k, v in state.items()}}
    for k, ts in times.items():
        res[k + "_fps"] = round(n_frames / statistics.median(ts), 1)
        res[k + "_runs_s"] = [round(t, 4) for t in ts]
    res["zone_over_motion"] = round(statistics.median(times["track_motion"]) / statistics.median(times["zone"]), 3)
    return res


LOOKBACK_BIRTHS = 8                                      # births per frame of ``lookback_part_us``'s synthetic pass


def lookback_part_us(eng, h, w, lookback, radius, iters=20):
    """HIP-event time of ops.track_lookback for ONE pass of eng.batch noise frames, outside a graph, on a window of its own: every frame
    of the pass brings LOOKBACK_BIRTHS new tracks (random boxes of 40..120 pixels a side), so every call chains B x LOOKBACK_BIRTHS births
    back over ``lookback`` frames, into the frames of the call before too.  -> the median in microseconds."""
    import numpy as np
    import torch
    from faster_rcnn_amd import ops
    B, rows, cap = eng.batch, 300, ops.track_capacity(eng.track_state())
    R, back = rows + cap, min(cap, 512 - rows - cap)
    rs = np.random.RandomState(11)
    frames = torch.from_numpy(rs.randint(0, 256, (B, h, w, 3)).astype(np.uint8)).cuda()
    tracked = np.zeros((B, 4 + 8 * R), dtype=np.int32)
    tracked[:, 4:4 + 5 * R] = -1
    n = LOOKBACK_BIRTHS
    window = ops.track_lookback_state(B, h, w, rows, cap, back)
    nf = torch.tensor([B], dtype=torch.int32, device="cuda")
    out, times, next_id = None, [], 1
    for it in range(iters + 1):
        for f in range(B):                                          # ids go on rising from call to call: every row is a birth
            x, y = rs.randint(0, w - 120, n), rs.randint(0, h - 120, n)
            side = rs.randint(40, 121, n)
            tracked[f, 4:4 + 4 * n] = np.stack([x, y, x + side, y + side], axis=1).reshape(-1)
            tracked[f, 4 + 4 * R:4 + 4 * R + n] = 1
            tracked[f, 4 + 6 * R:4 + 6 * R + n] = np.arange(next_id, next_id + n)
            next_id += n
            tracked[f, :4] = (n, n, next_id, 0)
        dev = torch.from_numpy(tracked).cuda()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = ops.track_lookback(window, frames, h * w * 3, dev, nf, cap, back, h, w, lookback, radius, TRACK_LEG[2], out=out)
        b.record()
        b.synchronize()
        if it:                                                      # (the first call has no window in front of it)
            times.append(a.elapsed_time(b) * 1000.0)
    return round(statistics.median(times), 1)


def run_track_lookback(name, cfg, n_frames, reps, content="noise"):
    """``--track_lookback``: what the look-back costs on top of tracking with the motion step.  One pair of legs in ONE session,
    alternating inside every repetition: ``run_track``'s frames through in-memory annotating passes with ``redact=REDACT_LEG,
    track=TRACK_LEG, track_motion=MOTION_LEG``, without and with ``track_lookback`` = min(8, frames per pass), the command line's
    default (the tracker is reset in front of every run; the look-back run ends with its flush submit).  Reports frames/s of both and
    their ratio, the tracker's state and the windows' back_overflow at the end, and the HIP-event time of the look-back call of one pass
    alone (``lookback_part_us``)."""
    import numpy as np
    from faster_rcnn_amd import entry, ops, shapes, util
    mgr, det = build(cfg)
    h, w = cfg["hw"]
    rs = np.random.RandomState(5)
    srcs = photo_frames(h, w, n_frames) if content == "photo" else [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n_frames)]
    imgs = [shapes.Image(shapes.Metadata("f%04d" % i, w, h, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=cfg["resize"][0], max_size=cfg["resize"][1])
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight(cfg["dtype"]))
    lookback = min(ops.TRACK_LOOKBACK[2], eng.batch)
    overflow = []

    def leg(**kw):
        def run():
            eng.track_reset()
            out = annotate_in_memory(eng, resized, ratios, redact=REDACT_LEG, track=TRACK_LEG, track_motion=MOTION_LEG, **kw)
            if kw:                                                  # (read in front of the next reset)
                overflow.append([int(win[:12].view(torch.int32)[2]) for win, _ in eng.edit_states.lookback.values()])
            return out
        return run

    import torch
    legs = {"track_motion": leg(), "track_lookback": leg(track_lookback=lookback)}
    times = {k: [] for k in legs}
    for fn in legs.values():                                        # warm-up: captures
        fn()
    for _ in range(reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    state = eng.track_state().cpu().numpy()
    res = {"frames": n_frames, "frame_hw": [h, w], "resize_dims": list(cfg["resize"]), "dtype": cfg["dtype"], "depth": cfg["depth"], "content": content,
           "redact": ["all", "blur", 12, 0], "track": list(TRACK_LEG), "track_motion": MOTION_LEG, "track_lookback": lookback,
           "images_per_pass": eng.batch, "in_flight": eng.in_flight,
           "tracker": {"live_slots": int(state[0]), "ids_issued": int(state[1]), "overflow": int(state[2]), "frames": int(state[3])},
           "back_overflow": overflow[-1]}
    for k, ts in times.items():
        res[k + "_fps"] = round(n_frames / statistics.median(ts), 1)
        res[k + "_runs_s"] = [round(t, 4) for t in ts]
    res["lookback_over_motion"] = round(statistics.median(times["track_motion"]) / statistics.median(times["track_lookback"]), 3)
    res["lookback_part_us"] = {"births_per_frame": LOOKBACK_BIRTHS, "track_lookback": lookback_part_us(eng, h, w, lookback, MOTION_LEG),
                               "track_lookback_radius_0": lookback_part_us(eng, h, w, lookback, 0)}
    return res


EVERY_LEG = 4                                            # --detect_every 4


def run_detect_every(name, cfg, n_frames, reps, content="noise"):
    """``--detect_every``: what the frame rate gains when the detector runs on every fourth frame only.  One pair of legs in ONE session,
    alternating inside every repetition: ``run_track``'s frames through in-memory annotating passes with ``redact=REDACT_LEG,
    track=TRACK_LEG, track_motion=MOTION_LEG``, without and with ``detect_every=EVERY_LEG`` (the tracker is reset in front of every
    run).  Reports frames/s of both, their ratio and the tracker's state at the end of the last run."""
    import numpy as np
    import torch
    from faster_rcnn_amd import entry, shapes, util
    mgr, det = build(cfg)
    h, w = cfg["hw"]
    rs = np.random.RandomState(5)
    srcs = photo_frames(h, w, n_frames) if content == "photo" else [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n_frames)]
    imgs = [shapes.Image(shapes.Metadata("f%04d" % i, w, h, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=cfg["resize"][0], max_size=cfg["resize"][1])
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight(cfg["dtype"]))

    def leg(**kw):
        def run():
            eng.track_reset()
            return annotate_in_memory(eng, resized, ratios, redact=REDACT_LEG, track=TRACK_LEG, track_motion=MOTION_LEG, **kw)
        return run

    legs = {"track_motion": leg(), "detect_every": leg(detect_every=EVERY_LEG)}
    times = {k: [] for k in legs}
    for fn in legs.values():                                        # warm-up: captures
        fn()
    for _ in range(reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    state = eng.track_state().cpu().numpy()
    res = {"frames": n_frames, "frame_hw": [h, w], "resize_dims": list(cfg["resize"]), "dtype": cfg["dtype"], "depth": cfg["depth"], "content": content,
           "redact": ["all", "blur", 12, 0], "track": list(TRACK_LEG), "track_motion": MOTION_LEG, "detect_every": EVERY_LEG,
           "images_per_pass": eng.batch, "frames_per_pass": eng.batch * EVERY_LEG, "in_flight": eng.in_flight,
           "tracker": {"live_slots": int(state[0]), "ids_issued": int(state[1]), "overflow": int(state[2]), "frames": int(state[3])}}
    for k, ts in times.items():
        res[k + "_fps"] = round(n_frames / statistics.median(ts), 1)
        res[k + "_runs_s"] = [round(t, 4) for t in ts]
    res["every_over_motion"] = round(statistics.median(times["track_motion"]) / statistics.median(times["detect_every"]), 3)
    return res


def backtrack_part_us(eng, h, w, lookback, radius, interval, iters=20):
    """``lookback_part_us`` for ops.track_backtrack: ONE pass of eng.batch * ``interval`` noise frames on a window of its own.  Every KEY
    frame of the pass sees LOOKBACK_BIRTHS tracks it continues (corrections: they walk the ``interval`` - 1 frames in front of it) and
    LOOKBACK_BIRTHS new ones (births: they walk ``lookback`` frames); a between frame shows the continued tracks.  -> the median in
    microseconds."""
    import numpy as np
    import torch
    from faster_rcnn_amd import ops
    F, rows, cap = eng.batch * interval, 300, ops.track_capacity(eng.track_state())
    R, back = rows + cap, min(cap, 512 - rows - cap)
    rs = np.random.RandomState(11)
    frames = torch.from_numpy(rs.randint(0, 256, (F, h, w, 3)).astype(np.uint8)).cuda()
    tracked = np.zeros((F, 4 + 8 * R), dtype=np.int32)
    tracked[:, 4:4 + 5 * R] = -1
    n = LOOKBACK_BIRTHS
    window = ops.track_lookback_state(F, h, w, rows, cap, back)
    nf = torch.tensor([F], dtype=torch.int32, device="cuda")
    out, times, next_id = None, [], n + 1                            # ids 1..n: the continued tracks
    for it in range(iters + 1):
        for f in range(F):
            key = f % interval == 0
            m = 2 * n if key else n
            x, y = rs.randint(0, w - 120, m), rs.randint(0, h - 120, m)
            side = rs.randint(40, 121, m)
            tracked[f, 4:4 + 5 * R] = -1
            tracked[f, 4 + 6 * R:4 + 7 * R] = 0
            tracked[f, 4:4 + 4 * m] = np.stack([x, y, x + side, y + side], axis=1).reshape(-1)
            tracked[f, 4 + 4 * R:4 + 4 * R + m] = 1
            tracked[f, 4 + 6 * R:4 + 6 * R + n] = np.arange(1, n + 1)
            if key:
                tracked[f, 4 + 6 * R + n:4 + 6 * R + m] = np.arange(next_id, next_id + n)
                next_id += n
            tracked[f, :4] = (m, m, next_id, 0)
        dev = torch.from_numpy(tracked).cuda()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = ops.track_backtrack(window, frames, h * w * 3, dev, nf, cap, back, h, w, lookback, radius, TRACK_LEG[2], interval, out=out)
        b.record()
        b.synchronize()
        if it:                                                      # (the first call has no window in front of it)
            times.append(a.elapsed_time(b) * 1000.0)
    return round(statistics.median(times), 1)


def run_track_backtrack(name, cfg, n_frames, reps, content="noise"):
    """``--track_backtrack``: what the back-track rule costs on top of ``--detect_every 4``.  One pair of legs in ONE session, alternating
    inside every repetition: ``run_detect_every``'s ``detect_every`` leg without and with ``track_backtrack`` at the command line's default,
    min(16, frames per pass) (the tracker is reset in front of every run; the back-track run ends with its flush submit).  Reports
    frames/s of both and their ratio, the tracker's state and the windows' back_overflow at the end, and the HIP-event time of the
    back-track call of one pass alone (``backtrack_part_us``) at radius 8 and at radius 0."""
    import numpy as np
    import torch
    from faster_rcnn_amd import entry, ops, shapes, util
    mgr, det = build(cfg)
    h, w = cfg["hw"]
    rs = np.random.RandomState(5)
    srcs = photo_frames(h, w, n_frames) if content == "photo" else [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n_frames)]
    imgs = [shapes.Image(shapes.Metadata("f%04d" % i, w, h, [], "none"), s) for i, s in enumerate(srcs)]
    resized, ratios = util.resize_imgs(imgs, min_size=cfg["resize"][0], max_size=cfg["resize"][1])
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight(cfg["dtype"]))
    lookback = ops.track_backtrack_option(None, EVERY_LEG, eng.batch * EVERY_LEG)
    overflow = []

    def leg(**kw):
        def run():
            eng.track_reset()
            out = annotate_in_memory(eng, resized, ratios, redact=REDACT_LEG, track=TRACK_LEG, track_motion=MOTION_LEG, detect_every=EVERY_LEG, **kw)
            if kw:                                                  # (read in front of the next reset)
                overflow.append([int(win[:12].view(torch.int32)[2]) for win, _ in eng.edit_states.lookback.values()])
            return out
        return run

    legs = {"detect_every": leg(), "track_backtrack": leg(track_backtrack=lookback)}
    times = {k: [] for k in legs}
    for fn in legs.values():                                        # warm-up: captures
        fn()
    for _ in range(reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    state = eng.track_state().cpu().numpy()
    res = {"frames": n_frames, "frame_hw": [h, w], "resize_dims": list(cfg["resize"]), "dtype": cfg["dtype"], "depth": cfg["depth"], "content": content,
           "redact": ["all", "blur", 12, 0], "track": list(TRACK_LEG), "track_motion": MOTION_LEG, "detect_every": EVERY_LEG,
           "track_backtrack": lookback, "images_per_pass": eng.batch, "frames_per_pass": eng.batch * EVERY_LEG, "in_flight": eng.in_flight,
           "tracker": {"live_slots": int(state[0]), "ids_issued": int(state[1]), "overflow": int(state[2]), "frames": int(state[3])},
           "back_overflow": overflow[-1]}
    for k, ts in times.items():
        res[k + "_fps"] = round(n_frames / statistics.median(ts), 1)
        res[k + "_runs_s"] = [round(t, 4) for t in ts]
    res["backtrack_over_every"] = round(statistics.median(times["detect_every"]) / statistics.median(times["track_backtrack"]), 3)
    res["backtrack_part_us"] = {"corrections_and_births_per_key_frame": [LOOKBACK_BIRTHS, LOOKBACK_BIRTHS],
                                "track_backtrack": backtrack_part_us(eng, h, w, lookback, MOTION_LEG, EVERY_LEG),
                                "track_backtrack_radius_0": backtrack_part_us(eng, h, w, lookback, 0, EVERY_LEG)}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", default=",".join(PAIRS))
    ap.add_argument("--png_encoder", choices=("host", "device", "both", "all"), default="host",
                    help="who encodes leg (c)'s output files; all = host, device (runs) and device (huffman), alternating")
    ap.add_argument("--legs", default=None, help="the legs (c) by name, comma-separated (%s); overrides --png_encoder" % ", ".join(LEGS))
    ap.add_argument("--content", choices=("noise", "photo"), default="noise", help="what the frames hold (see the module docstring)")
    ap.add_argument("--y4m", action="store_true", help="instead of the legs above: y4m to y4m, y4m to PNG files (device encoder) and PNG files "
                                                       "to PNG files (host codecs), alternating in one session")
    ap.add_argument("--redact", action="store_true", help="instead of the legs above: the same frames with and without --redact all "
                                                          "--redact_mode blur, alternating in one session (passes in memory, and files to files)")
    ap.add_argument("--track", action="store_true", help="instead of the legs above: the --redact leg's frames and redaction without and with "
                                                         "--track (IoU 30, hold 8), alternating in one session (passes in memory)")
    ap.add_argument("--track_motion", action="store_true", help="instead of the legs above: the --track leg's frames, redaction and tracking "
                                                                "without and with --track_motion 8, alternating in one session")
    ap.add_argument("--track_lookback", action="store_true", help="instead of the legs above: the --track --track_motion 8 leg without and "
                                                                  "with --track_lookback at its default, alternating in one session")
    ap.add_argument("--detect_every", action="store_true", help="instead of the legs above: the --track --track_motion 8 leg without and "
                                                                "with --detect_every 4, alternating in one session")
    ap.add_argument("--track_backtrack", action="store_true", help="instead of the legs above: the --detect_every 4 leg without and with "
                                                                   "--track_backtrack at its default, alternating in one session")
    ap.add_argument("--track_scene_cut", action="store_true", help="instead of the legs above: the --track --track_motion 8 leg without and "
                                                                   "with --track_scene_cut at its default, alternating in one session")
    ap.add_argument("--track_trails", action="store_true", help="instead of the legs above: the --track --track_motion 8 leg without and "
                                                                "with --track_trails at its defaults, alternating in one session")
    ap.add_argument("--heatmap", action="store_true", help="instead of the legs above: the --track --track_motion 8 leg without and with "
                                                           "--heatmap all at its defaults, alternating in one session")
    ap.add_argument("--remove", action="store_true", help="instead of the legs above: the --track --track_motion 8 leg without and with "
                                                          "--remove all at its defaults, alternating in one session")
    ap.add_argument("--count_line", action="store_true", help="instead of the legs above: the --track --track_motion 8 leg without and "
                                                              "with two --count_line lines, alternating in one session")
    ap.add_argument("--zone", action="store_true", help="instead of the legs above: the --track --track_motion 8 leg without and with two "
                                                        "--zone rectangles of a quarter of the frame each, alternating in one session")
    ap.add_argument("--track_reid", action="store_true", help="instead of the legs above: the --track --track_motion 8 leg without and "
                                                              "with --track_reid at its defaults, alternating in one session (also as "
                                                              "--track --track_reid)")
    ap.add_argument("--post", action="store_true", help="instead of the legs above: in-memory annotating passes without and with --nms "
                                                        "soft_gaussian --box_vote (the post-process option), alternating in one session")
    ap.add_argument("--out_scale", action="store_true", help="instead of the legs above: in-memory annotating passes, PNG files to PNG files "
                                                             "(device encoder, huffman) and y4m to y4m, each without and with --out_scale 2, "
                                                             "alternating in one session")
    ap.add_argument("--redact_shape", action="store_true", help="instead of the legs above: the --redact all --redact_mode blur leg without and "
                                                                "with --redact_shape ellipse --redact_feather 8, alternating in one session")
    ap.add_argument("--track_low", action="store_true", help="instead of the legs above: the --det_threshold 0.5 --track --track_motion 8 "
                                                             "leg without and with --track_low 0.1, alternating in one session")
    ap.add_argument("--redact_region", action="store_true", help="instead of the legs above: in-memory annotating passes without and with two "
                                                                 "--redact_region polygons of a tenth of the frame each, --region_mode blur "
                                                                 "--region_feather 8, alternating in one session")
    ap.add_argument("--redact_moving", action="store_true", help="instead of the legs above: in-memory annotating passes plain, with "
                                                                 "--redact_moving (S = 8) and with --remove all, on a generated sequence "
                                                                 "with a moving block, alternating in one session")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_annotate.py needs a GPU")
    out = {"metric": "annotate_frames_per_s", "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES")}
    for name in args.pairs.split(","):
        if args.y4m:
            out[name] = run_y4m(name, PAIRS[name], args.frames, args.reps, args.content)
            continue
        if args.redact_moving:
            out[name] = run_redact_moving(name, PAIRS[name], args.frames, args.reps)
            continue
        if args.redact_region:
            out[name] = run_redact_region(name, PAIRS[name], args.frames, args.reps, args.content)
            continue
        if args.track_low:
            out[name] = run_track_low(name, PAIRS[name], args.frames, args.reps, args.content)
            continue
        if args.redact_shape:
            out[name] = run_redact_shape(name, PAIRS[name], args.frames, args.reps, args.content)
            continue
        if args.out_scale:
            out[name] = run_out_scale(name, PAIRS[name], args.frames, args.reps, args.content)
            continue
        if args.post:
            out[name] = run_post(name, PAIRS[name], args.frames, args.reps, args.content)
            continue
        if args.track_reid:
            out[name] = run_track_reid(name, PAIRS[name], args.frames, args.reps, args.content)
            continue
        if args.heatmap:
            out[name] = run_heatmap(name, PAIRS[name], args.frames, args.reps, args.content)
            continue
        if args.remove:
            out[name] = run_remove(name, PAIRS[name], args.frames, args.reps, args.content)
            continue
        if args.zone:
            out[name] = run_zone(name, PAIRS[name], args.frames, args.reps, args.content)
            continue
        if args.count_line:
            out[name] = run_count_line(name, PAIRS[name], args.frames, args.reps, args.content)
            continue
        if args.track_trails:
            out[name] = run_track_trails(name, PAIRS[name], args.frames, args.reps, args.content)
            continue
        if args.track_scene_cut:
            out[name] = run_track_scene_cut(name, PAIRS[name], args.frames, args.reps, args.content)
            continue
        if args.track_backtrack:
            out[name] = run_track_backtrack(name, PAIRS[name], args.frames, args.reps, args.content)
            continue
        if args.detect_every:
            out[name] = run_detect_every(name, PAIRS[name], args.frames, args.reps, args.content)
            continue
        if args.track_lookback:
            out[name] = run_track_lookback(name, PAIRS[name], args.frames, args.reps, args.content)
            continue
        if args.track_motion:
            out[name] = run_track_motion(name, PAIRS[name], args.frames, args.reps, args.content)
            continue
        if args.track:
            out[name] = run_track(name, PAIRS[name], args.frames, args.reps, args.content)
            continue
        if args.redact:
            out[name] = run_redact(name, PAIRS[name], args.frames, args.reps, args.content)
            continue
        encoders = {"both": ("host", "device"), "all": ("host", "device", "device_huffman")}.get(args.png_encoder, (args.png_encoder,))
        if args.legs:
            encoders = tuple(args.legs.split(","))
            if any(e not in LEGS for e in encoders):
                raise SystemExit("--legs: one or more of %s" % ", ".join(LEGS))
        out[name] = run_pair(name, PAIRS[name], args.frames, args.reps, encoders, args.content)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
