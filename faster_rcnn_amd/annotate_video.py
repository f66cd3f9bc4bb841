"""Mirror of the reference's annotate_video.py (annotate_video.py:15-82): detections drawn on a directory of frames.

``get_annotated_frame(training_manager, detector, frame, img, resize_min, resize_max)`` draws into ``frame`` in place and
returns it; ``annotate_images(...)`` walks ``image_filenames`` of ``input_dir`` and writes each annotated frame to ``out_dir``
under its own name, printing what the reference prints ("processing <path>", "num rois: N", every drawn det).

What is drawn (annotate_video.py:32-41): every det except classes 'DontCare' / 'Misc' and boxes with x1 < 0, x2 > width,
y1 < 0 or y2 > height of the ORIGINAL frame; a 3-pixel (0,255,0) box and the label "{} {:6.2f}".format(cls_name, prob) at
(x1, y2 + 16).  The pixels are this project's rule (ops.annotate_u8): square box corners and a 5x7 bitmap font
at scale 2 instead of cv2's Hershey strokes -- the same primitives in the same places, not cv2's pixels.

On the captured path the drawing is part of the detection pass: the frame is already on the device, the draw runs after the
post-process inside the same hipGraph, and the annotated frame comes back with the detections.  ``annotate_images`` decodes
PNGs ahead on threads, uploads them in the decoder's RGB order (green is (0,255,0) in either order), groups frames of one
geometry into ``entry.default_batch`` passes with ``entry.default_in_flight`` of them in flight, and writes PNGs on a few
threads (PIL, compress_level=1) in list order.  PNGs that are not 8-bit RGB (grey, palette, 16-bit, alpha) are read through
PIL's ``convert("RGB")``; cv2.imread's colour conversion may differ from it for 16-bit files.

``png_encoder="device"`` (``--png_encoder device``, or FRCNN_ANNOTATE_PNG_ENCODER=device as the default) moves the encode into the pass
as well: ops.png_encode_u8 turns the drawn frame into the bytes of a .png file on the device (csrc/png.hip), the file comes back instead
of the raw frame and the writer threads only write it out.  The files decode to the same pixels as the host encoder's; their bytes
differ (and are larger: fixed Huffman codes with run matches).  The default stays "host".

``png_compress="huffman"`` (``--png_compress huffman``, or FRCNN_ANNOTATE_PNG_COMPRESS=huffman as the default) selects the device
encoder's second mode: adaptive row filters and a dynamic Huffman code per band of eight rows, files about the size of the host
encoder's.  It is a mode of the DEVICE encoder: with the host encoder it raises ValueError.  The default stays "runs".

``frame_format="jpg"`` (``--frame_format jpg``, or FRCNN_ANNOTATE_FRAME_FORMAT=jpg as the default) writes every annotated frame as
``<stem>.jpg`` instead: a baseline JPEG at ``jpeg_quality`` (``--jpeg_quality``, 1..100, default 90) without chroma subsampling (the boxes
are 3 pixels wide).  ``jpeg_encoder="host"`` (the default; FRCNN_ANNOTATE_JPEG_ENCODER) is PIL on the writer threads,
``jpeg_encoder="device"`` encodes inside the pass (ops.jpeg_encode_u8, csrc/jpeg.hip): the file comes back instead of the raw frame.  Both
use the Annex K tables at the same IJG quality; their bytes differ in the rounding of colour transform and DCT.  The JPEG
options with ``png`` frames, and the device PNG options with ``jpg`` frames, raise ValueError.  The default stays "png".

``jpeg_subsampling=420`` (``--jpeg_subsampling 420``, FRCNN_ANNOTATE_JPEG_SUBSAMPLING) halves the chroma planes both ways and
``jpeg_huffman="optimized"`` (``--jpeg_huffman optimized``, FRCNN_ANNOTATE_JPEG_HUFFMAN) writes Huffman tables built from each frame's own
symbol counts: the two options every JPEG writer has, honoured by both encoders (PIL: ``subsampling=2``, ``optimize=True``; device:
csrc/jpeg_opt.hip).  Both need ``jpg`` frames; the defaults stay 444 / "standard" (sizes: DESIGN §8).

A video STREAM goes through ``annotate_stream``: the command line's ``input_dir`` may be a YUV4MPEG2 file (``.y4m``) or ``-`` (stdin), and
``--out_video PATH|-`` writes one y4m stream (``--video_chroma`` 420jpeg or 444; range and the F / A tags are the input's, limited / F25:1
for a frame directory, whose frames must then share one size) instead of frame files -- with ``-`` every printed line goes to stderr.  The
frames' chroma upsampling and colour matrix, and the inverse on the way out, run inside the passes (csrc/y4m.hip); a frame's
"path" in the printed lines is ``<name>#<frame index>``.

What is DONE to the frames on the way -- hiding objects (``redact``, ``redact_shape``, ``remove``), hiding places (``redact_region``) and
whatever moves (``redact_moving``), tracking (``track`` and its ``track_*`` forms, ``detect_every``), the heat map, count lines and
zones, the thresholds, the post-process and the output size -- is one value, ``AnnotateOptions``: its docstring describes every option
once, every entry point takes its fields as keywords, and ``build_parser``'s help texts state the flag of each (``--redact CLASSES``,
``--track``, ``--count_line X1,Y1,X2,Y2``, ...) with its range and default.  All of it runs inside the passes, in front of every encoder
and for every input format, in the order ``frame_edit.EditChain``'s docstring states; without an option no pass, key, printed line or
output byte is another.
"""
import collections
import dataclasses
import os
import pathlib
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib, entry, ops, shapes, voc_dets, y4m
from .frame_edit import EditChain, EditStates
from .util import resize_imgs

STRIDE = 16                                       # get_dets' default: annotate_video.py:29 passes none
DET_THRESHOLD = 0.0                               # annotate_video.py:30
DECODE_THREADS = int(os.environ.get("FRCNN_ANNOTATE_DECODE_THREADS", "4"))
# PNG writers: PIL releases the interpreter lock while it encodes; KITTI frames (44 ms each on one thread) run at 78 frames/s on four
# writers and 125 on eight (scripts/bench_annotate.py)
WRITE_THREADS = int(os.environ.get("FRCNN_ANNOTATE_WRITE_THREADS", "8"))
PNG_COMPRESS_LEVEL = 1
PNG_ENCODERS = ("host", "device")
PNG_COMPRESS = ("runs", "huffman")                # modes of the device encoder (ops.PNG_COMPRESS)
FRAME_FORMATS = ("png", "jpg")
JPEG_ENCODERS = ("host", "device")
JPEG_QUALITY = 90
JPEG_SUBSAMPLINGS = (444, 420)
JPEG_HUFFMANS = ("standard", "optimized")


def default_png_encoder():
    """FRCNN_ANNOTATE_PNG_ENCODER, else "host" (PIL on the writer threads)."""
    enc = os.environ.get("FRCNN_ANNOTATE_PNG_ENCODER", "host")
    if enc not in PNG_ENCODERS:
        raise ValueError("FRCNN_ANNOTATE_PNG_ENCODER=%r: one of %s" % (enc, ", ".join(PNG_ENCODERS)))
    return enc


def default_png_compress():
    """FRCNN_ANNOTATE_PNG_COMPRESS, else "runs"."""
    mode = os.environ.get("FRCNN_ANNOTATE_PNG_COMPRESS", "runs")
    if mode not in PNG_COMPRESS:
        raise ValueError("FRCNN_ANNOTATE_PNG_COMPRESS=%r: one of %s" % (mode, ", ".join(PNG_COMPRESS)))
    return mode


def png_options(png_encoder=None, png_compress=None):
    """-> (encoder, compress) with None replaced by the defaults; ValueError for an unknown name and for "huffman" with the host encoder."""
    png_encoder = default_png_encoder() if png_encoder is None else png_encoder
    png_compress = default_png_compress() if png_compress is None else png_compress
    if png_encoder not in PNG_ENCODERS:
        raise ValueError("png_encoder=%r: one of %s" % (png_encoder, ", ".join(PNG_ENCODERS)))
    if png_compress not in PNG_COMPRESS:
        raise ValueError("png_compress=%r: one of %s" % (png_compress, ", ".join(PNG_COMPRESS)))
    if png_compress != "runs" and png_encoder != "device":
        raise ValueError("png_compress=%r is a mode of the device encoder: it needs png_encoder=\"device\" (--png_encoder device)"
                         % (png_compress,))
    return png_encoder, png_compress


def default_frame_format():
    """FRCNN_ANNOTATE_FRAME_FORMAT, else "png"."""
    fmt = os.environ.get("FRCNN_ANNOTATE_FRAME_FORMAT", "png")
    if fmt not in FRAME_FORMATS:
        raise ValueError("FRCNN_ANNOTATE_FRAME_FORMAT=%r: one of %s" % (fmt, ", ".join(FRAME_FORMATS)))
    return fmt


def default_jpeg_encoder():
    """FRCNN_ANNOTATE_JPEG_ENCODER, else "host" (PIL on the writer threads)."""
    enc = os.environ.get("FRCNN_ANNOTATE_JPEG_ENCODER", "host")
    if enc not in JPEG_ENCODERS:
        raise ValueError("FRCNN_ANNOTATE_JPEG_ENCODER=%r: one of %s" % (enc, ", ".join(JPEG_ENCODERS)))
    return enc


def default_jpeg_subsampling():
    """FRCNN_ANNOTATE_JPEG_SUBSAMPLING (444 or 420), else 444."""
    value = os.environ.get("FRCNN_ANNOTATE_JPEG_SUBSAMPLING", "444")
    if value not in [str(s) for s in JPEG_SUBSAMPLINGS]:
        raise ValueError("FRCNN_ANNOTATE_JPEG_SUBSAMPLING=%r: one of %s" % (value, ", ".join(str(s) for s in JPEG_SUBSAMPLINGS)))
    return int(value)


def default_jpeg_huffman():
    """FRCNN_ANNOTATE_JPEG_HUFFMAN, else "standard" (the tables of Annex K.3)."""
    value = os.environ.get("FRCNN_ANNOTATE_JPEG_HUFFMAN", "standard")
    if value not in JPEG_HUFFMANS:
        raise ValueError("FRCNN_ANNOTATE_JPEG_HUFFMAN=%r: one of %s" % (value, ", ".join(JPEG_HUFFMANS)))
    return value


def jpeg_size_options(frame_format, jpeg_subsampling=None, jpeg_huffman=None):
    """-> (jpeg_subsampling, jpeg_huffman) with None replaced by the defaults.  ``frame_format``: what ``jpeg_options`` returned.
    ValueError for an unknown value, and for 420 or "optimized" with "png" frames: both are settings of JPEG frames, of either encoder."""
    jpeg_subsampling = default_jpeg_subsampling() if jpeg_subsampling is None else jpeg_subsampling
    jpeg_huffman = default_jpeg_huffman() if jpeg_huffman is None else jpeg_huffman
    if isinstance(jpeg_subsampling, bool) or jpeg_subsampling not in JPEG_SUBSAMPLINGS:
        raise ValueError("jpeg_subsampling=%r: one of %s" % (jpeg_subsampling, ", ".join(str(s) for s in JPEG_SUBSAMPLINGS)))
    if not isinstance(jpeg_huffman, str) or jpeg_huffman not in JPEG_HUFFMANS:
        raise ValueError("jpeg_huffman=%r: one of %s" % (jpeg_huffman, ", ".join(JPEG_HUFFMANS)))
    if frame_format != "jpg":
        if jpeg_subsampling != 444:
            raise ValueError("jpeg_subsampling=%r is a setting of JPEG frames: it needs frame_format=\"jpg\" (--frame_format jpg)" % (jpeg_subsampling,))
        if jpeg_huffman != "standard":
            raise ValueError("jpeg_huffman=%r is a setting of JPEG frames: it needs frame_format=\"jpg\" (--frame_format jpg)" % (jpeg_huffman,))
    return int(jpeg_subsampling), jpeg_huffman


def jpeg_options(frame_format=None, jpeg_encoder=None, jpeg_quality=None, png_encoder="host", png_compress="runs"):
    """-> (frame_format, jpeg_encoder, jpeg_quality) with None replaced by the defaults (quality: JPEG_QUALITY).  ``png_encoder`` /
    ``png_compress``: what ``png_options`` returned.  ValueError for an unknown name, a quality outside 1..100, the device JPEG encoder
    or a quality with "png" frames, and the device PNG encoder or its huffman mode with "jpg" frames."""
    frame_format = default_frame_format() if frame_format is None else frame_format
    jpeg_encoder = default_jpeg_encoder() if jpeg_encoder is None else jpeg_encoder
    if frame_format not in FRAME_FORMATS:
        raise ValueError("frame_format=%r: one of %s" % (frame_format, ", ".join(FRAME_FORMATS)))
    if jpeg_encoder not in JPEG_ENCODERS:
        raise ValueError("jpeg_encoder=%r: one of %s" % (jpeg_encoder, ", ".join(JPEG_ENCODERS)))
    if jpeg_quality is not None and (isinstance(jpeg_quality, bool) or not isinstance(jpeg_quality, (int, np.integer))
                                     or not 1 <= int(jpeg_quality) <= 100):
        raise ValueError("jpeg_quality=%r: an integer in 1..100" % (jpeg_quality,))
    if frame_format == "png":
        if jpeg_encoder != "host":
            raise ValueError("jpeg_encoder=%r encodes JPEG frames: it needs frame_format=\"jpg\" (--frame_format jpg)" % (jpeg_encoder,))
        if jpeg_quality is not None:
            raise ValueError("jpeg_quality=%r is a setting of JPEG frames: it needs frame_format=\"jpg\" (--frame_format jpg)" % (jpeg_quality,))
    elif png_encoder != "host" or png_compress != "runs":
        raise ValueError("png_encoder=%r / png_compress=%r are settings of PNG frames: not with frame_format=\"jpg\"" % (png_encoder, png_compress))
    return frame_format, jpeg_encoder, JPEG_QUALITY if jpeg_quality is None else int(jpeg_quality)


def drawn(det, width, height):
    """The reference's filter (annotate_video.py:33-38): is this det drawn on a frame of (width, height)?"""
    if det["cls_name"] in ops.ANNOTATE_SKIP:
        return False
    x1, y1, x2, y2 = det["bbox"]
    return not (x1 < 0 or x2 > width or y1 < 0 or y2 > height)


def png_filenames(input_dir):
    """annotate_video.py:69: the ``*.png`` names of ``input_dir``, sorted."""
    return sorted(f for f in os.listdir(input_dir) if f.endswith(".png"))


def _engine(training_manager, detector, in_flight, post=None):
    """``post``: the post-process option (ops.det_post_option); an engine with it is one of its own, with its own editing states."""
    if not voc_dets.FAST_ENTRY:
        return None
    eng = entry.for_models(training_manager, detector, 64, STRIDE, in_flight=in_flight, post=post)
    return eng if eng is not None and eng.device_preprocess else None


def _pack_dets(dets, class_mapping):
    """Host dets -> the post-process's packed layout (ops.split_detections), for an eager draw."""
    rows = max(1, len(dets))
    packed = np.zeros(4 + 7 * rows, dtype=np.int32)
    packed[0] = len(dets)
    for k, d in enumerate(dets):
        packed[4 + 4 * k:8 + 4 * k] = np.asarray(d["bbox"], dtype=np.int64).astype(np.int32)
        packed[4 + 4 * rows + k] = class_mapping[d["cls_name"]]
        packed[4 + 5 * rows + k] = np.float32(d["prob"]).view(np.int32)
    return packed


_EAGER_STATES = {}                                        # class mapping -> the eager path's EditStates


def _names_by_index(class_mapping):
    rev = {v: k for k, v in class_mapping.items()}
    return [rev.get(i, "") for i in range(max(rev) + 1)]


def _eager_states(class_mapping):
    """The eager path's editing states (frame_edit.EditStates) of this class mapping, made on first use: a tracker of
    entry.TRACK_CAPACITY slots, trail and count states of twice as many entries."""
    key = tuple(sorted(class_mapping.items()))
    states = _EAGER_STATES.get(key)
    if states is None:
        states = _EAGER_STATES[key] = EditStates(_names_by_index(class_mapping), entry.TRACK_CAPACITY,
                                                 min(2 * entry.TRACK_CAPACITY, ops.TRACK_MAX))
    return states


def _eager_count_state(class_mapping):
    return _eager_states(class_mapping).count_state()


def _eager_trails_state(class_mapping, length):
    return _eager_states(class_mapping).trails_state(length)


def _eager_heat_state(class_mapping, h, w):
    return _eager_states(class_mapping).heat_state(h, w)


def draw_eager(frame, dets, class_mapping, redact=None, draw=True, track=None, info=None, rgb=False, **options):
    """The editing chain over ONE frame and its host dets (the eager path, foreign models): ``frame`` (h, w, 3) uint8 is edited in
    place, by a one-frame ``frame_edit.EditChain`` -- its docstring states the calls and their order -- on this class mapping's eager
    states, which go on from the call before (``reset_tracks``, ``reset_heat``, ``reset_counts``, ``reset_zones``, ``reset_plate`` and
    ``reset_moving`` empty them); ``rgb``: the frame's channel order (False: B, G, R).  ``redact``, ``draw``, ``track`` and ``options``:
    the options of ``AnnotateOptions`` that edit a frame -- no ``track_lookback`` / ``detect_every`` / ``track_backtrack``, no ``post``
    and no output.  A frame without detections still teaches the heat map, the plate and the moving net.
    With ``track``, ``dets`` is edited in place as ``collect_batch`` returns it: "track_id" on every det, the held rows appended with
    "held".  ``info``, a dict, receives the frame's marks as a pass's result carries them: "scene_cut": True when the frame is a cut,
    "crossings": [(line, dir, id, cls)], "zones": {"occupancy", "events"}, "reid": [(pid, tid, cls, distance, gap)] and "moving":
    {"cells", "covered"}, each with its option.  With ``out_size`` the edited frame scaled down on the device is what is returned, a new
    (H, W, 3) array; ``frame`` is edited in place as without it."""
    return _edit_eager(frame, dets, class_mapping, AnnotateOptions.checked(class_mapping, "draw", frame, redact=redact, draw=draw, track=track,
                                                                           **options), info, rgb)


def _edit_eager(frame, dets, class_mapping, o, info=None, rgb=False):
    """``draw_eager`` with its options checked: ``o``, an ``AnnotateOptions``."""
    import torch
    scaled_hw = None if o.out_size is None else ops.scale_option(o.out_size, frame.shape[:2])
    if dets and (o.draw or o.redact is not None) or any(v is not None for v in (o.track, o.heatmap, o.remove, o.redact_region, o.redact_moving)):
        dev = torch.from_numpy(np.ascontiguousarray(frame)).cuda()      # (else the frame stays as it is)
        packed = torch.from_numpy(_pack_dets(dets, class_mapping)).cuda()
        states = _eager_states(class_mapping)
        chain = EditChain(states, entry.PassSpec(**o.edit_keywords()), 1, 1, frame.shape[:2], rgb)
        chain.update(dev.view(-1), 0, packed, states.one_frame())         # (in front of the edits: ``dev`` is still the frame as it came)
        chain.edit(0, dev)
        if o.track is not None:
            _, ids, held = ops.tracked_dets(chain.host_tracked[0].cpu().numpy(), _names_by_index(class_mapping), start=len(dets))
            for k, d in enumerate(dets):
                d["track_id"] = int(ids[k])
            dets += held
        if info is not None and o.track_scene_cut is not None and int(chain.cuts[0]):
            info["scene_cut"] = True
        if info is not None and o.count is not None:
            info["crossings"] = ops.count_events(chain.count_lists[0].cpu().numpy())
        if info is not None and o.zone is not None:
            zlist = chain.zone_lists[0].cpu().numpy()
            info["zones"] = {"occupancy": ops.zone_occupancy(zlist, len(o.zone[0])), "events": ops.zone_events(zlist)}
        if info is not None and o.track_reid is not None:
            info["reid"] = ops.track_reid_events(chain.reid_lists[0].cpu().numpy())
        if info is not None and o.redact_moving is not None:
            stats = ops.redact_moving_stats(chain.moving_stats[0])
            info["moving"] = {"cells": stats["cells"], "covered": stats["covered"]}
        frame[...] = dev.cpu().numpy()
    if scaled_hw is not None:
        return ops.downscale_u8(torch.from_numpy(np.ascontiguousarray(frame)).cuda(), *scaled_hw).cpu().numpy()
    return frame


REDACT_MODES = ("pixelate", "blur", "fill")


def redact_from_args(args, class_mapping):
    """(host only) The redaction the command line asks for -> (classes, mode, size, margin) as ``submit_batch(redact=...)`` takes it, or
    None without ``--redact``.  classes: "all", or the tuple of names (of ``class_mapping``, the active one) in the order given; size:
    the mode's default when not stated.  ValueError, with the reason, for an unknown class name, for ``--redact_mode`` /
    ``--redact_size`` / ``--redact_margin`` without ``--redact``, for a size out of the mode's range and for a negative margin."""
    if args.redact is None:
        for flag, value in (("--redact_mode", args.redact_mode), ("--redact_size", args.redact_size), ("--redact_margin", args.redact_margin)):
            if value is not None:
                raise ValueError("%s=%s is a setting of the redaction: it needs --redact CLASSES" % (flag, value))
        return None
    names = [n.strip() for n in args.redact.split(",") if n.strip()]
    if not names:
        raise ValueError("--redact takes comma-separated class names, or all")
    classes = "all" if names == ["all"] else ops.redact_class_list(_names_by_index(class_mapping), names)
    mode = "pixelate" if args.redact_mode is None else args.redact_mode
    size = ops.redact_size(mode, args.redact_size)
    margin = 0 if args.redact_margin is None else int(args.redact_margin)
    if margin < 0:
        raise ValueError("--redact_margin=%d: an integer >= 0" % margin)
    return classes, mode, size, margin


def _redact_shape(redact_shape, redact):
    """``annotate_images`` / ``annotate_stream`` / ``get_annotated_frame`` / ``draw_eager``'s ``redact_shape`` checked against ``redact``
    -> (shape, feather), or None: without it and for ("box", 0), which is the plain redaction."""
    if redact_shape is None:
        return None
    if redact is None:
        raise ValueError("redact_shape=%r shapes the redaction: it needs redact=(classes, mode, size, margin)" % (redact_shape,))
    try:
        shape, feather = redact_shape
    except (TypeError, ValueError):
        raise ValueError("redact_shape=%r: (shape, feather)" % (redact_shape,)) from None
    option = ops.redact_shape_option(shape, feather)
    return None if option == ("box", 0) else option


def _redact_region(redact_region):
    """``annotate_images`` / ``annotate_stream`` / ``get_annotated_frame`` / ``draw_eager``'s ``redact_region`` checked -> (regions, mask,
    mode, size, feather) in ops.redact_region_option's form, or None.  ValueError with the reason."""
    if redact_region is None:
        return None
    try:
        regions, mask, mode, size, feather = redact_region
    except (TypeError, ValueError):
        raise ValueError("redact_region=%r: (regions, mask, mode, size, feather)" % (redact_region,)) from None
    return ops.redact_region_option(regions, mask, mode, size, feather)


def _redact_moving(redact_moving, remove, owner):
    """``annotate_images`` / ``annotate_stream`` / ``get_annotated_frame`` / ``draw_eager``'s ``redact_moving`` checked against the
    normalised ``remove`` -> ops.redact_moving_option's form, or None (ops.redact_moving_form).  ``owner``: the class mapping, or the
    training manager that holds it (read only when there is an option to check).  ValueError with the reason."""
    if redact_moving is None or redact_moving is False:
        return None
    mapping = owner if isinstance(owner, dict) else owner.class_mapping
    return ops.redact_moving_form(redact_moving, remove, _names_by_index(mapping))


MOVING_SATELLITES = ("moving_tol", "moving_min", "moving_hold", "moving_grow", "moving_feather", "moving_unknown", "moving_except",
                     "moving_mode", "moving_size", "moving_out")


def redact_moving_from_args(args, class_mapping, remove=None):
    """(host only) The moving net the command line asks for -> (the option in ops.redact_moving_option's form as
    ``submit_batch(redact_moving=...)`` takes it, the path of ``--moving_out`` or None), or (None, None) without ``--redact_moving``.
    ``remove``: what ``remove_from_args`` returned -- with it the plate's settle, tolerance and margin are its own; without it they are
    ``--remove_settle`` / ``--remove_tol`` / ``--remove_margin``, which go with either flag.  ValueError, with the reason, for any
    ``--moving_*`` flag without ``--redact_moving`` (by its name), an unknown class name and a value out of range."""
    if not getattr(args, "redact_moving", False):
        for name in MOVING_SATELLITES:
            value = getattr(args, name, None)
            if value is not None:
                raise ValueError("--%s=%s is a setting of the moving net: it needs --redact_moving" % (name, value))
        return None, None
    classes = None
    if args.moving_except is not None:
        classes = tuple(n.strip() for n in args.moving_except.split(",") if n.strip())
        if not classes:
            raise ValueError("--moving_except takes comma-separated class names, or all")
    kw = dict(tol=args.moving_tol, vote=args.moving_min, hold=args.moving_hold, grow=args.moving_grow, feather=args.moving_feather,
              unknown=args.moving_unknown, except_classes=classes, mode=args.moving_mode, size=args.moving_size)
    if remove is None:
        kw.update(settle=args.remove_settle, plate_tol=args.remove_tol, margin=args.remove_margin)
    try:
        option = ops.redact_moving_form(kw, remove, _names_by_index(class_mapping))
    except ValueError as e:
        raise ValueError("--redact_moving / --moving_* / --remove_settle / --remove_tol / --remove_margin: %s" % e) from None
    return option, _moving_out(args.moving_out, option)


def _moving_out(moving_out, redact_moving):
    """``moving_out`` checked against ``redact_moving`` -> the path, or None."""
    if moving_out is None:
        return None
    if redact_moving is None:
        raise ValueError("moving_out=%r is where the moving net's counts are written: it needs redact_moving=" % (moving_out,))
    return moving_out


def moving_line(w, h, covered):
    """The line printed at the end for the frame size (w, h): ``moving net 1242x375: 128 frames, mean 3.2 % hidden, peak 17.0 %`` --
    ``covered``: the pixels with W > 0 of every frame of that size, in order."""
    pct = [100.0 * c / (w * h) for c in covered]
    return "moving net %dx%d: %d frames, mean %.1f %% hidden, peak %.1f %%" % (w, h, len(pct), sum(pct) / max(len(pct), 1), max(pct + [0.0]))


class MovingLog:
    """Where the moving net's counts of a sequence go: the ``--moving_out`` CSV ``frame,cells,covered`` (``path`` None: none) and the
    covered pixels per frame size, for the lines at the end.  A sequence report (``_reports``)."""
    output = "moving_out"

    def __init__(self, path):
        self.file = open(path, "w") if path is not None else None
        if self.file is not None:
            self.file.write("frame,cells,covered\n")
        self.per_size = collections.OrderedDict()         # (h, w) -> [covered of every frame of that size]

    def add(self, frame_no, h, w, moving):
        self.per_size.setdefault((int(h), int(w)), []).append(int(moving["covered"]))
        if self.file is not None:
            self.file.write("%d,%d,%d\n" % (frame_no, moving["cells"], moving["covered"]))

    def lines(self):
        return [moving_line(w, h, covered) for (h, w), covered in sorted(self.per_size.items())]

    def frame(self, pos, label, frame, dets, marks):
        self.add(pos + 1, frame.height, frame.width, marks["moving"])

    def end(self):                                        # (host only: what the passes returned; ``close`` closes the file)
        for line in self.lines():
            print(line)

    def close(self):
        if self.file is not None:
            self.file.close()
            self.file = None


def redact_region_from_args(args):
    """(host only) The static areas the command line asks for -> (regions, mask, mode, size, feather) as
    ``submit_batch(redact_region=...)`` takes it, or None without ``--redact_region`` / ``--redact_mask``.  Every ``--redact_region``
    takes ``--zone``'s grammar; ``--redact_mask`` is read through PIL, ``convert("L")``.  ValueError, with the reason, for
    ``--region_mode`` / ``--region_size`` / ``--region_feather`` without either, for a polygon the rule refuses, a file PIL cannot open
    and a value out of range."""
    specs, path = args.redact_region or [], args.redact_mask
    if not specs and path is None:
        for flag, value in (("--region_mode", args.region_mode), ("--region_size", args.region_size), ("--region_feather", args.region_feather)):
            if value is not None:
                raise ValueError("%s=%s is a setting of the static areas: it needs --redact_region X1,Y1,X2,Y2,X3,Y3[,...] or --redact_mask "
                                 "PATH" % (flag, value))
        return None
    regions = []
    for spec in specs:
        parts = [v.strip() for v in spec.split(",")]
        if len(parts) < 6 or len(parts) % 2 or not all(re.fullmatch(r"[+-]?\d+", v) for v in parts):
            raise ValueError("--redact_region=%s: X1,Y1,X2,Y2,X3,Y3[,...], an even number of integers, six at least" % spec)
        v = [int(x) for x in parts]
        regions.append(tuple(zip(v[0::2], v[1::2])))
    mask = None
    if path is not None:
        from PIL import Image
        try:
            with Image.open(path) as im:
                mask = np.asarray(im.convert("L"), dtype=np.uint8)
        except (OSError, ValueError) as e:
            raise ValueError("--redact_mask=%s: %s" % (path, e)) from None
    try:
        return ops.redact_region_option(tuple(regions), mask, args.region_mode, args.region_size, args.region_feather)
    except ValueError as e:
        raise ValueError("--redact_region / --redact_mask: %s" % e) from None


def region_line(w, h, option, stats):
    """The line printed at the end for the frame size (w, h): ``redact regions 1242x375: 2 regions + mask, 12.3 % of the frame hidden``
    -- ``stats``: ops.redact_region_stats of the size's plane; hidden counts every pixel with W > 0."""
    regions, mask = option[0], option[1]
    what = []
    if regions:
        what.append("%d region%s" % (len(regions), "" if len(regions) == 1 else "s"))
    if mask is not None:
        what.append("mask")
    return "redact regions %dx%d: %s, %.1f %% of the frame hidden" % (w, h, " + ".join(what), 100.0 * stats["covered"] / (w * h))


def blacken_plate(image, weights):
    """(host only) ``image``, an (h, w, 3) plate picture, with every pixel whose region weight in ``weights`` ((h, w), W of the plane) is
    > 0 written black -> a new array: the plate picture never shows a static area in clear."""
    out = np.array(image, copy=True)
    out[np.asarray(weights) > 0] = 0
    return out


def redact_shape_from_args(args):
    """(host only) The shape of the redaction the command line asks for -> (shape, feather) as ``submit_batch(redact_shape=...)`` takes
    it, or None without ``--redact_shape`` / ``--redact_feather`` and for "box" with feather 0, which is the plain redaction.  ValueError,
    with the reason, for either flag without ``--redact`` and for a feather outside 0..32."""
    if args.redact_shape is None and args.redact_feather is None:
        return None
    if args.redact is None:
        for flag, value in (("--redact_shape", args.redact_shape), ("--redact_feather", args.redact_feather)):
            if value is not None:
                raise ValueError("%s=%s is a setting of the redaction: it needs --redact CLASSES" % (flag, value))
    try:
        option = ops.redact_shape_option(args.redact_shape, args.redact_feather)
    except ValueError as e:
        raise ValueError("--redact_shape / --redact_feather: %s" % e) from None
    return None if option == ("box", 0) else option


def track_from_args(args):
    """(host only) The tracking the command line asks for -> (thr, hold, grow) as ``submit_batch(track=...)`` takes it, or None without
    ``--track``.  ValueError, with the reason, for ``--track_iou`` / ``--track_hold`` / ``--track_grow`` / ``--tracks_out`` without
    ``--track`` and for a value out of range (1..100, 0..255, 0..64)."""
    if not args.track:
        for flag, value in (("--track_iou", args.track_iou), ("--track_hold", args.track_hold), ("--track_grow", args.track_grow),
                            ("--tracks_out", args.tracks_out)):
            if value is not None:
                raise ValueError("%s=%s is a setting of the tracker: it needs --track" % (flag, value))
        return None
    try:
        return ops.track_option(args.track_iou, args.track_hold, args.track_grow)
    except ValueError as e:
        raise ValueError("--track_iou / --track_hold / --track_grow: %s" % e) from None


def track_motion_from_args(args):
    """(host only) The motion step the command line asks for -> the search radius as ``submit_batch(track_motion=...)`` takes it (8 for
    a bare ``--track_motion``), or None without the flag.  ValueError, with the reason, for ``--track_motion`` without ``--track`` and for
    a radius outside 1..16."""
    if args.track_motion is None:
        return None
    if not args.track:
        raise ValueError("--track_motion=%s is a setting of the tracker: it needs --track" % args.track_motion)
    try:
        return ops.track_motion_radius(args.track_motion)
    except ValueError as e:
        raise ValueError("--track_motion: %s" % e) from None


TRACK_LOOKBACK_AUTO = 0        # a bare --track_lookback: as far back as one pass holds, at most ops.TRACK_LOOKBACK[2] = 8 frames


def track_lookback_from_args(args):
    """(host only) The look-back the command line asks for -> the frames as ``annotate_images(track_lookback=...)`` takes them
    (TRACK_LOOKBACK_AUTO for a bare ``--track_lookback``), or None without the flag.  ValueError, with the reason, for
    ``--track_lookback`` without ``--track`` and for a value outside 1..16."""
    if args.track_lookback is None:
        return None
    if not args.track:
        raise ValueError("--track_lookback=%s is a setting of the tracker: it needs --track" % args.track_lookback)
    if args.track_lookback == TRACK_LOOKBACK_AUTO and not isinstance(args.track_lookback, bool):
        return TRACK_LOOKBACK_AUTO
    try:
        return ops.track_lookback_option(args.track_lookback)
    except ValueError as e:
        raise ValueError("--track_lookback: %s" % e) from None


def detect_every_from_args(args):
    """(host only) The detection interval the command line asks for -> K as ``annotate_images(detect_every=...)`` takes it, or None without
    the flag.  ValueError, with the reason, for ``--detect_every`` without ``--track --track_motion``, together with ``--track_lookback``
    and for a value outside 2..16."""
    if args.detect_every is None:
        return None
    if not args.track or args.track_motion is None:
        raise ValueError("--detect_every=%s follows the tracks by block matching between two detected frames: it needs --track --track_motion"
                         % args.detect_every)
    if args.track_lookback is not None:
        raise ValueError("--detect_every together with --track_lookback is not supported: the look-back window keeps one tracked buffer per "
                         "detected frame")
    try:
        return ops.track_interval_option(args.detect_every)
    except ValueError as e:
        raise ValueError("--detect_every: %s" % e) from None


def _detect_every(detect_every, track, track_motion, track_lookback, eng, B):
    """``annotate_images`` / ``annotate_stream``'s ``detect_every`` checked -> the K of their passes, or None."""
    if detect_every is None:
        return None
    if track is None or track_motion is None:
        raise ValueError("detect_every=%r follows the tracks by block matching between two detected frames: it needs track=(thr, hold, grow) "
                         "and track_motion=R" % (detect_every,))
    if track_lookback is not None:
        raise ValueError("detect_every=%r together with track_lookback=%r is not supported: the look-back window keeps one tracked buffer per "
                         "detected frame" % (detect_every, track_lookback))
    if eng is None:
        raise ValueError("detect_every=%r runs the detector once per pass of several frames: the eager path (a foreign model) detects one "
                         "frame at a time and cannot" % (detect_every,))
    k = ops.track_interval_option(detect_every)
    if B * k > _lib.TRACK_MAX_FRAMES:                     # (what submit_batch would refuse at the first pass)
        raise ValueError("detect_every=%d with passes of %d images is %d frames per pass: at most %d here" % (k, B, B * k, _lib.TRACK_MAX_FRAMES // B))
    return k


TRACK_BACKTRACK_AUTO = 0       # a bare --track_backtrack: as far back as one pass of B * K frames holds, at most 16 frames


def track_backtrack_from_args(args):
    """(host only) The back-track look-back the command line asks for -> the frames as ``annotate_images(track_backtrack=...)`` takes them
    (TRACK_BACKTRACK_AUTO for a bare ``--track_backtrack``), or None without the flag.  ValueError, with the reason, for
    ``--track_backtrack`` without ``--track --track_motion --detect_every K``, together with ``--track_lookback``, for a value outside
    1..16 and for one under K - 1."""
    if args.track_backtrack is None:
        return None
    if not args.track or args.track_motion is None or args.detect_every is None:
        raise ValueError("--track_backtrack=%s follows the tracks of a detected frame back over the frames between two detections: it needs "
                         "--track --track_motion --detect_every K" % args.track_backtrack)
    if args.track_lookback is not None:
        raise ValueError("--track_backtrack together with --track_lookback is not supported: the back-track rule hides a new track in the "
                         "earlier frames itself")
    if args.track_backtrack == TRACK_BACKTRACK_AUTO and not isinstance(args.track_backtrack, bool):
        return TRACK_BACKTRACK_AUTO
    try:
        k = ops.track_interval_option(args.detect_every)
        return ops.track_backtrack_option(args.track_backtrack, k, max(ops.TRACK_LOOKBACK[1], k))      # (the pass's frames: known with the engine)
    except ValueError as e:
        raise ValueError("--track_backtrack: %s" % e) from None


def _backtrack_frames(track_backtrack, every, track_lookback, eng, B):
    """``annotate_images`` / ``annotate_stream``'s ``track_backtrack`` checked against the K of their passes (``_detect_every``'s result)
    -> the look-back of their passes, or None."""
    if track_backtrack is None:
        return None
    if track_lookback is not None:
        raise ValueError("track_backtrack=%r together with track_lookback=%r is not supported: the back-track rule hides a new track in the "
                         "earlier frames itself" % (track_backtrack, track_lookback))
    if every is None:
        raise ValueError("track_backtrack=%r follows the tracks of a detected frame back over the frames between two detections: it needs "
                         "track=(thr, hold, grow), track_motion=R and detect_every=K" % (track_backtrack,))
    if eng is None:
        raise ValueError("track_backtrack=%r delays the output by one pass: the eager path (a foreign model) returns every frame at once and "
                         "cannot" % (track_backtrack,))
    auto = track_backtrack == TRACK_BACKTRACK_AUTO and not isinstance(track_backtrack, bool)
    return ops.track_backtrack_option(None if auto else track_backtrack, every, B * every)


def _every_parts(group, B, every):
    """The passes of a ``detect_every`` group of <= B * K frames of one geometry -> [(frames, images of the pass)]: one pass of B (padded)
    when its key frames fill at least half of it, else one-image passes of K frames."""
    keys = -(-len(group) // every)
    if B > 1 and keys >= max(2, B // 2):
        return [(group, B)]
    return [(group[i:i + every], 1) for i in range(0, len(group), every)]


def track_scene_cut_from_args(args):
    """(host only) The scene-cut threshold the command line asks for -> the percentage as ``submit_batch(track_scene_cut=...)`` takes it
    (ops.TRACK_CUT_PCT[2] = 40 for a bare ``--track_scene_cut``), or None without the flag.  ValueError, with the reason, for
    ``--track_scene_cut`` without ``--track --track_motion``, together with ``--track_lookback`` or ``--track_backtrack`` and for a value
    outside 1..100."""
    if args.track_scene_cut is None:
        return None
    if not args.track or args.track_motion is None:
        raise ValueError("--track_scene_cut=%s compares every frame with the frame the block match keeps: it needs --track --track_motion"
                         % args.track_scene_cut)
    for flag, value in (("--track_lookback", args.track_lookback), ("--track_backtrack", args.track_backtrack)):
        if value is not None:
            raise ValueError("--track_scene_cut together with %s is not supported: a backward chain would have to stop at a cut" % flag)
    try:
        return ops.track_cut_option(args.track_scene_cut)
    except ValueError as e:
        raise ValueError("--track_scene_cut: %s" % e) from None


def _track_scene_cut(track_scene_cut, track, track_motion, track_lookback, track_backtrack):
    """``annotate_images`` / ``annotate_stream`` / ``get_annotated_frame``'s ``track_scene_cut`` checked -> the percentage, or None."""
    if track_scene_cut is None:
        return None
    if track is None or track_motion is None:
        raise ValueError("track_scene_cut=%r compares every frame with the frame the block match keeps: it needs track=(thr, hold, grow) and "
                         "track_motion=R" % (track_scene_cut,))
    for name, value in (("track_lookback", track_lookback), ("track_backtrack", track_backtrack)):
        if value is not None:
            raise ValueError("track_scene_cut=%r together with %s=%r is not supported: a backward chain would have to stop at a cut"
                             % (track_scene_cut, name, value))
    return ops.track_cut_option(track_scene_cut)


def track_trails_from_args(args):
    """(host only) The trails the command line asks for -> (N, W) as ``submit_batch(track_trails=...)`` takes it (N = ops.TRACK_TRAILS[0][2]
    = 16 for a bare ``--track_trails``, W = ``--trail_width`` or 3), or None without the flag.  ValueError, with the reason, for
    ``--trail_width`` without ``--track_trails``, ``--track_trails`` without ``--track`` or with ``--no_draw``, and for an N outside 2..64
    or a W outside 1..9."""
    if args.track_trails is None:
        if args.trail_width is not None:
            raise ValueError("--trail_width=%s is the width the trails are drawn with: it needs --track_trails" % args.trail_width)
        return None
    if not args.track:
        raise ValueError("--track_trails=%s draws the paths of the tracker's ids: it needs --track" % args.track_trails)
    if args.no_draw:
        raise ValueError("--track_trails together with --no_draw is not supported: a run that draws nothing draws no trails")
    try:
        return ops.track_trails_option((args.track_trails, args.trail_width))
    except ValueError as e:
        raise ValueError("--track_trails / --trail_width: %s" % e) from None


def _track_trails(track_trails, track, draw):
    """``annotate_images`` / ``annotate_stream`` / ``get_annotated_frame``'s ``track_trails`` checked -> (N, W), or None."""
    if track_trails is None:
        return None
    if track is None:
        raise ValueError("track_trails=%r draws the paths of the tracker's ids: it needs track=(thr, hold, grow)" % (track_trails,))
    if not draw:
        raise ValueError("track_trails=%r together with draw=False is not supported: a run that draws nothing draws no trails" % (track_trails,))
    return ops.track_trails_option(track_trails)


def count_from_args(args, class_mapping):
    """(host only) The line count the command line asks for -> ((lines, classes, W) as ``submit_batch(count=...)`` takes it, the path of
    ``--counts_out`` or None), or (None, None) without ``--count_line``.  ValueError, with the reason, for ``--count_classes`` /
    ``--count_width`` / ``--counts_out`` without ``--count_line``, ``--count_line`` without ``--track``, more than 8 lines, a tuple that is
    not four integers X1,Y1,X2,Y2, A = B, an unknown class name and a W outside 1..9."""
    if not args.count_line:
        for flag, value in (("--count_classes", args.count_classes), ("--count_width", args.count_width), ("--counts_out", args.counts_out)):
            if value is not None:
                raise ValueError("%s=%s is a setting of the line count: it needs --count_line X1,Y1,X2,Y2" % (flag, value))
        return None, None
    if not args.track:
        raise ValueError("--count_line counts the tracker's ids as they cross the line: it needs --track")
    lines = []
    for text in args.count_line:
        try:
            line = tuple(int(v) for v in text.split(","))
        except ValueError:
            line = ()
        if len(line) != 4:
            raise ValueError("--count_line %s: four integers X1,Y1,X2,Y2" % text)
        lines.append(line)
    names = [n.strip() for n in (args.count_classes or "all").split(",") if n.strip()]
    if not names:
        raise ValueError("--count_classes takes comma-separated class names, or all")
    try:
        classes = "all" if names == ["all"] else ops.redact_class_list(_names_by_index(class_mapping), names)
        return ops.count_option(lines, classes, args.count_width), args.counts_out
    except ValueError as e:
        raise ValueError("--count_line / --count_classes / --count_width: %s" % e) from None


def _count(count, track):
    """``annotate_images`` / ``annotate_stream``'s ``count`` checked -> (lines, classes, W), or None."""
    if count is None:
        return None
    if track is None:
        raise ValueError("count=%r counts the tracker's ids as they cross a line: it needs track=(thr, hold, grow)" % (count,))
    try:
        lines, classes, width = count
    except (TypeError, ValueError):
        raise ValueError("count=%r: (lines, classes, width)" % (count,)) from None
    return ops.count_option(lines, classes, width)


COUNTS_HEADER = "frame,line,direction,id,cls"


def counts_rows(frame_no, crossings, names):
    """(host only) The ``--counts_out`` rows of one frame: ``frame,line,direction,id,cls`` per crossing (line, dir, id, cls), frames from
    1, direction + or -, the class by its name in ``names`` (names by index)."""
    return ["%d,%d,%s,%d,%s" % (frame_no, line, "+" if d else "-", tid, names[cls] if 0 <= cls < len(names) else cls)
            for line, d, tid, cls in crossings]


def print_counts(n_lines, totals, per_class, events_dropped):
    """(host only) The lines printed at the end of a counted list: one per counting line with its two totals, the totals per class (from
    the crossings listed), and a warning when crossings were left out of the lists."""
    for l in range(n_lines):
        print("line {}: +{} -{}".format(l, totals[l][1], totals[l][0]))
    for name in sorted(per_class):
        print("crossings of {}: +{} -{}".format(name, per_class[name][1], per_class[name][0]))
    if events_dropped:
        print("warning: {} crossings did not fit their frames' lists: the counts file is short by that many rows; the totals are exact"
              .format(events_dropped))


class CountsLog:
    """Where the crossings of a counted sequence go: the ``--counts_out`` file (``path`` None: none) and the totals per class name.  A
    sequence report (``_reports``): ``n_lines`` and ``state()``, the count state, are what its summary is printed from."""
    output = "counts_out"

    def __init__(self, path, names, n_lines=0, state=None):
        self.names, self.per_class, self.n_lines, self.state = list(names), {}, n_lines, state
        self.file = open(path, "w") if path is not None else None
        if self.file is not None:
            self.file.write(COUNTS_HEADER + "\n")

    def add(self, frame_no, crossings):
        for _, d, _, cls in crossings:
            self.per_class.setdefault(self.names[cls] if 0 <= cls < len(self.names) else str(cls), [0, 0])[d] += 1
        if self.file is not None:
            self.file.writelines(row + "\n" for row in counts_rows(frame_no, crossings, self.names))

    def frame(self, pos, label, frame, dets, marks):
        self.add(pos + 1, marks["crossings"])

    def end(self):                                        # (host only: the state read back)
        self.close()
        totals = ops.count_totals(self.state())
        print_counts(self.n_lines, totals["totals"], self.per_class, totals["events_dropped"])

    def close(self):
        if self.file is not None:
            self.file.close()
            self.file = None


def _write_counts(counts_out, frame_no, crossings, class_mapping):
    """``counts_out``: None, a ``CountsLog``, or a text file that receives the frame's CSV rows (no header)."""
    if isinstance(counts_out, CountsLog):
        counts_out.add(frame_no, crossings)
    elif counts_out is not None:
        counts_out.writelines(row + "\n" for row in counts_rows(frame_no, crossings, _names_by_index(class_mapping)))


def _count_state(training_manager, eng):
    """The count state of ``eng``, or of the eager path with None."""
    return eng.count_state() if eng is not None else _eager_states(training_manager.class_mapping).count_state()


def reset_counts(training_manager, detector, in_flight=1, post=None):
    """Zero totals and no entries before a new sequence: the count state of the engine ``in_flight`` names, or the eager path's.
    (``reset_tracks`` ends the ids and keeps the totals.)"""
    eng = _engine(training_manager, detector, in_flight, post)
    if eng is not None:
        eng.count_reset()
    else:
        _eager_states(training_manager.class_mapping).reset_counts()


def zone_from_args(args, class_mapping):
    """(host only) The zones the command line asks for -> ((zones, classes, W, anchor) as ``submit_batch(zone=...)`` takes it, the path of
    ``--zones_out`` or None), or (None, None) without ``--zone``.  ValueError, with the reason, for ``--zone_classes`` / ``--zone_width`` /
    ``--zone_anchor`` / ``--zones_out`` without ``--zone``, ``--zone`` without ``--track``, more than 8 zones, a value that is not an even
    number of at least six integers, equal consecutive vertices, an unknown class name, a W outside 1..9 and an unknown anchor."""
    if not args.zone:
        for flag, value in (("--zone_classes", args.zone_classes), ("--zone_width", args.zone_width), ("--zone_anchor", args.zone_anchor),
                            ("--zones_out", args.zones_out)):
            if value is not None:
                raise ValueError("%s=%s is a setting of the zones: it needs --zone X1,Y1,X2,Y2,X3,Y3[,...]" % (flag, value))
        return None, None
    if not args.track:
        raise ValueError("--zone tests the tracker's ids against the zone: it needs --track")
    zones = []
    for text in args.zone:
        try:
            flat = tuple(int(v) for v in text.split(","))
        except ValueError:
            flat = ()
        if len(flat) < 6 or len(flat) % 2:
            raise ValueError("--zone %s: an even number of integers X1,Y1,X2,Y2,X3,Y3[,...], three vertices at least" % text)
        zones.append(tuple(zip(flat[0::2], flat[1::2])))
    names = [n.strip() for n in (args.zone_classes or "all").split(",") if n.strip()]
    if not names:
        raise ValueError("--zone_classes takes comma-separated class names, or all")
    try:
        classes = "all" if names == ["all"] else ops.redact_class_list(_names_by_index(class_mapping), names)
        return ops.zone_option(zones, classes, args.zone_width, args.zone_anchor), args.zones_out
    except ValueError as e:
        raise ValueError("--zone / --zone_classes / --zone_width / --zone_anchor: %s" % e) from None


def _zone(zone, track):
    """``annotate_images`` / ``annotate_stream``'s ``zone`` checked -> (zones, classes, W, anchor), or None."""
    if zone is None:
        return None
    if track is None:
        raise ValueError("zone=%r tests the tracker's ids against the zones: it needs track=(thr, hold, grow)" % (zone,))
    try:
        zones, classes, width, anchor = zone
    except (TypeError, ValueError):
        raise ValueError("zone=%r: (zones, classes, width, anchor)" % (zone,)) from None
    return ops.zone_option(zones, classes, width, anchor)


ZONES_HEADER = "frame,zone,kind,id,cls,dwell"


def zones_rows(frame_no, events, names):
    """(host only) The ``--zones_out`` rows of one frame: ``frame,zone,kind,id,cls,dwell`` per event (zone, kind, id, cls, dwell), frames
    from 1, kind enter, exit or lost, the class by its name in ``names`` (names by index), the dwell in frames (0 for enter)."""
    return ["%d,%d,%s,%d,%s,%d" % (frame_no, z, ops.ZONE_KINDS[kind], tid, names[cls] if 0 <= cls < len(names) else cls, dwell)
            for z, kind, tid, cls, dwell in events]


def print_zones(n_zones, totals):
    """(host only) The lines printed at the end of a list with zones, from ``ops.zone_totals``' form: one per zone -- visitors, peak, stays
    and the mean dwell in frames over the completed stays --, and a warning when events were left out of the lists."""
    for z in range(n_zones):
        stays, dwell = totals["stays"][z], totals["dwell"][z]
        mean = "{:.1f} frames".format(dwell / stays) if stays else "-"
        print("zone {}: visitors {} peak {} stays {} mean dwell {}".format(z, totals["visitors"][z], totals["peak"][z], stays, mean))
    if totals["events_dropped"]:
        print("warning: {} zone events did not fit their frames' lists: the zones file is short by that many rows; the totals are exact"
              .format(totals["events_dropped"]))


class ZonesLog:
    """Where the zone events of a sequence go: the ``--zones_out`` file (``path`` None: none).  A sequence report (``_reports``):
    ``n_zones`` and ``state()``, the zone state, are what its summary is printed from."""
    output = "zones_out"

    def __init__(self, path, names, n_zones=0, state=None):
        self.names, self.n_zones, self.state = list(names), n_zones, state
        self.file = open(path, "w") if path is not None else None
        if self.file is not None:
            self.file.write(ZONES_HEADER + "\n")

    def add(self, frame_no, events):
        if self.file is not None:
            self.file.writelines(row + "\n" for row in zones_rows(frame_no, events, self.names))

    def frame(self, pos, label, frame, dets, marks):
        self.add(pos + 1, marks["zones"]["events"])

    def end(self):                                        # (host only: the state read back)
        self.close()
        print_zones(self.n_zones, ops.zone_totals(self.state()))

    def close(self):
        if self.file is not None:
            self.file.close()
            self.file = None


def _write_zones(zones_out, frame_no, events, class_mapping):
    """``zones_out``: None, a ``ZonesLog``, or a text file that receives the frame's CSV rows (no header)."""
    if isinstance(zones_out, ZonesLog):
        zones_out.add(frame_no, events)
    elif zones_out is not None:
        zones_out.writelines(row + "\n" for row in zones_rows(frame_no, events, _names_by_index(class_mapping)))


REID_HEADER = "frame,id,tracker_id,cls,distance,gap"


def reid_rows(frame_no, events, names):
    """(host only) The ``--reid_out`` rows of one frame: ``frame,id,tracker_id,cls,distance,gap`` per event (pid, tid, cls, distance, gap),
    frames from 1, the class by its name in ``names`` (names by index), the distance 0..8192, the gap in frames."""
    return ["%d,%d,%d,%s,%d,%d" % (frame_no, pid, tid, names[cls] if 0 <= cls < len(names) else cls, dist, gap)
            for pid, tid, cls, dist, gap in events]


class ReidLog:
    """Where the re-identifications of a sequence go: the ``--reid_out`` file (``path`` None: none), and how many there were.  A
    sequence report (``_reports``)."""
    output = "reid_out"

    def __init__(self, path, names):
        self.names, self.total = list(names), 0
        self.file = open(path, "w") if path is not None else None
        if self.file is not None:
            self.file.write(REID_HEADER + "\n")

    def add(self, frame_no, events):
        self.total += len(events)
        if self.file is not None:
            self.file.writelines(row + "\n" for row in reid_rows(frame_no, events, self.names))

    def frame(self, pos, label, frame, dets, marks):
        self.add(pos + 1, marks["reid"])
        _print_reid(label, marks["reid"])

    def end(self):
        self.close()
        print("re-identified: {}".format(self.total))

    def close(self):
        if self.file is not None:
            self.file.close()
            self.file = None


def _write_reid(reid_out, frame_no, events, class_mapping):
    """``reid_out``: None, a ``ReidLog``, or a text file that receives the frame's CSV rows (no header)."""
    if isinstance(reid_out, ReidLog):
        reid_out.add(frame_no, events)
    elif reid_out is not None:
        reid_out.writelines(row + "\n" for row in reid_rows(frame_no, events, _names_by_index(class_mapping)))


def _print_reid(label, events):
    for ev in events:
        print("re-identified: {} id {}".format(label, ev[0]))


def _det_thresholds(det_threshold, track_low, track, eager=False):
    """``annotate_images`` / ``annotate_stream`` / ``get_annotated_frame``'s ``det_threshold`` and ``track_low`` checked -> (T, L): T the
    score threshold of the output (None: DET_THRESHOLD), L the low threshold of the weak rule (DESIGN §8 "Weak rule") or None.  ``eager``:
    the caller runs the eager path (a foreign model), which has no captured pass to run the rule in.  ValueError with the reason
    (ops.track_weak_option's; the eager path's refusal of an L)."""
    T, L = ops.track_weak_option(DET_THRESHOLD if det_threshold is None else det_threshold, track_low, track is not None)
    if L is not None and eager:
        raise ValueError("track_low=%r runs the tracker's weak rule inside the captured passes: the eager path (a foreign model) cannot"
                         % (track_low,))
    return T, L


def det_thresholds_from_args(args):
    """(host only) The thresholds the command line asks for -> {} without the two flags, else the ``det_threshold=`` / ``track_low=`` that
    ``annotate_images`` takes.  ValueError, with the reason, for ``--track_low`` without ``--track``, for a ``--track_low`` that is not
    under ``--det_threshold`` and for values outside 0..1."""
    try:
        ops.track_weak_option(DET_THRESHOLD if args.det_threshold is None else args.det_threshold, args.track_low, bool(args.track))
    except ValueError as e:
        raise ValueError("--det_threshold / --track_low: %s" % e) from None
    out = {} if args.det_threshold is None else {"det_threshold": args.det_threshold}
    if args.track_low is not None:
        out["track_low"] = args.track_low
    return out


def _track_reid(track_reid, track):
    """``annotate_images`` / ``annotate_stream`` / ``get_annotated_frame``'s ``track_reid`` checked -> (pct, keep), or None."""
    if track_reid is None:
        return None
    if track is None:
        raise ValueError("track_reid=%r gives the tracker's ids back: it needs track=(thr, hold, grow)" % (track_reid,))
    try:
        pct, keep = track_reid
    except (TypeError, ValueError):
        raise ValueError("track_reid=%r: (pct, keep)" % (track_reid,)) from None
    return ops.track_reid_option(pct, keep)


def track_reid_from_args(args):
    """(host only) The re-identification the command line asks for -> ((pct, keep) as ``submit_batch(track_reid=...)`` takes it, the path
    of ``--reid_out`` or None), or (None, None) without ``--track_reid``.  ValueError, with the reason, for ``--reid_keep`` / ``--reid_out``
    without ``--track_reid``, ``--track_reid`` without ``--track`` or together with ``--track_lookback`` / ``--track_backtrack``, and for
    values out of range."""
    if args.track_reid is None:
        for flag, value in (("--reid_keep", args.reid_keep), ("--reid_out", args.reid_out)):
            if value is not None:
                raise ValueError("%s=%s is a setting of the re-identification: it needs --track_reid" % (flag, value))
        return None, None
    if not args.track:
        raise ValueError("--track_reid gives the tracker's ids back: it needs --track")
    for flag, value in (("--track_lookback", args.track_lookback), ("--track_backtrack", args.track_backtrack)):
        if value is not None:
            raise ValueError("--track_reid together with %s is not supported: the window of a delayed pass holds the tracker's own ids" % flag)
    try:
        return ops.track_reid_option(args.track_reid, args.reid_keep), args.reid_out
    except ValueError as e:
        raise ValueError("--track_reid / --reid_keep: %s" % e) from None


def _zone_state(training_manager, eng):
    """The zone state of ``eng``, or of the eager path with None."""
    return eng.zone_state() if eng is not None else _eager_states(training_manager.class_mapping).zone_state()


def reset_zones(training_manager, detector, in_flight=1, post=None):
    """An empty zone state, totals included, before a new sequence: the state of the engine ``in_flight`` names, or the eager path's.
    (``reset_tracks`` ends the ids and keeps the totals.)"""
    eng = _engine(training_manager, detector, in_flight, post)
    if eng is not None:
        eng.zone_reset()
    else:
        _eager_states(training_manager.class_mapping).reset_zones()


def heatmap_from_args(args, class_mapping):
    """(host only) The heat map the command line asks for -> ((classes, A, S) as ``submit_batch(heat=...)`` takes it, the path of
    ``--heatmap_out`` or None), or (None, None) without ``--heatmap``.  classes: "all", or the tuple of names (of ``class_mapping``, the
    active one) in the order given.  ValueError, with the reason, for ``--heatmap_alpha`` / ``--heatmap_decay`` / ``--heatmap_out`` without
    ``--heatmap``, an unknown class name, an A outside 1..255, an S outside 0..15 and a ``--heatmap_out`` that does not end in .png."""
    if args.heatmap is None:
        for flag, value in (("--heatmap_alpha", args.heatmap_alpha), ("--heatmap_decay", args.heatmap_decay), ("--heatmap_out", args.heatmap_out)):
            if value is not None:
                raise ValueError("%s=%s is a setting of the heat map: it needs --heatmap CLASSES" % (flag, value))
        return None, None
    names = [n.strip() for n in args.heatmap.split(",") if n.strip()]
    if not names:
        raise ValueError("--heatmap takes comma-separated class names, or all")
    try:
        classes = "all" if names == ["all"] else ops.redact_class_list(_names_by_index(class_mapping), names)
        heat = ops.heat_option(classes, args.heatmap_alpha, args.heatmap_decay)
    except ValueError as e:
        raise ValueError("--heatmap / --heatmap_alpha / --heatmap_decay: %s" % e) from None
    return heat, _heatmap_out(args.heatmap_out, heat)


def _heatmap(heatmap):
    """``annotate_images`` / ``annotate_stream`` / ``get_annotated_frame``'s ``heatmap`` checked -> (classes, A, S), or None."""
    if heatmap is None:
        return None
    try:
        classes, alpha, decay = () if isinstance(heatmap, str) else heatmap
    except (TypeError, ValueError):
        raise ValueError("heatmap=%r: (classes, alpha, decay)" % (heatmap,)) from None
    return ops.heat_option(classes, alpha, decay)


def _heatmap_out(heatmap_out, heatmap):
    """``heatmap_out`` checked against ``heatmap`` -> the path, or None."""
    if heatmap_out is None:
        return None
    if heatmap is None:
        raise ValueError("heatmap_out=%r is where the heat map is written: it needs heatmap=(classes, alpha, decay)" % (heatmap_out,))
    if not str(heatmap_out).lower().endswith(".png"):
        raise ValueError("heatmap_out=%r: the map is written as an 8-bit grey PNG, a path that ends in .png" % (heatmap_out,))
    return str(heatmap_out)


def heatmap_paths(path, sizes):
    """(host only) ``--heatmap_out``'s files for the frame sizes ``sizes`` ((h, w) each) -> {(h, w): path}: ``path`` itself for one size,
    ``<stem>_<w>x<h>.png`` for each of several."""
    sizes = sorted(sizes)
    if len(sizes) <= 1:
        return {hw: path for hw in sizes}
    return {(h, w): "%s_%dx%d%s" % (path[:-4], w, h, path[-4:]) for h, w in sizes}


def write_heatmaps(path, states):
    """``states``: {(h, w): a heat state's host copy (numpy)}.  Every size that saw a frame is written as an 8-bit grey PNG of the draw
    step's t values (ops.heat_levels) with PIL -> the paths written."""
    from PIL import Image as PilImage
    met = {hw: st for hw, st in states.items() if int(st[0]) > 0}
    paths = heatmap_paths(path, met)
    for (h, w), out in paths.items():
        PilImage.fromarray(ops.heat_levels(met[(h, w)], h, w), mode="L").save(out)
    return [paths[hw] for hw in sorted(paths)]


def _heat_states(training_manager, eng):
    """The host copies of the heat states of ``eng``, or of the eager path with None: {(h, w): numpy int32}."""
    import torch
    torch.cuda.synchronize()
    states = eng.edit_states if eng is not None else _eager_states(training_manager.class_mapping)
    return {hw: st.cpu().numpy() for hw, st in states.heat.items()}


def reset_heat(training_manager, detector, in_flight=1, post=None):
    """A cold heat map before a new sequence: the states of the engine ``in_flight`` names, or the eager path's."""
    eng = _engine(training_manager, detector, in_flight, post)
    if eng is not None:
        eng.heat_reset()
    else:
        _eager_states(training_manager.class_mapping).reset_heat()


def remove_from_args(args, class_mapping):
    """(host only) The removal the command line asks for -> ((classes, S, T, M) as ``submit_batch(remove=...)`` takes it, the path of
    ``--plate_out`` or None), or (None, None) without ``--remove``.  classes: "all", or the tuple of names (of ``class_mapping``, the
    active one) in the order given.  ValueError, with the reason, for ``--remove_settle`` / ``--remove_tol`` / ``--remove_margin`` /
    ``--plate_out`` without ``--remove``, an unknown class name, an S outside 1..255, a T outside 0..255, an M outside 0..64 and a
    ``--plate_out`` that does not end in .png."""
    if args.remove is None:
        moving = bool(getattr(args, "redact_moving", False))          # (the plate's three settings go with either flag)
        for flag, value in (("--remove_settle", args.remove_settle), ("--remove_tol", args.remove_tol), ("--remove_margin", args.remove_margin),
                            ("--plate_out", args.plate_out)):
            if value is not None and not (moving and flag != "--plate_out"):
                raise ValueError("%s=%s is a setting of the removal: it needs --remove CLASSES" % (flag, value)
                                 + ("" if flag == "--plate_out" else " (or --redact_moving)"))
        return None, None
    names = [n.strip() for n in args.remove.split(",") if n.strip()]
    if not names:
        raise ValueError("--remove takes comma-separated class names, or all")
    try:
        classes = "all" if names == ["all"] else ops.plate_class_list(_names_by_index(class_mapping), names)
        remove = ops.plate_option(classes, args.remove_settle, args.remove_tol, args.remove_margin)
    except ValueError as e:
        raise ValueError("--remove / --remove_settle / --remove_tol / --remove_margin: %s" % e) from None
    return remove, _plate_out(args.plate_out, remove)


def _remove(remove):
    """``annotate_images`` / ``annotate_stream`` / ``get_annotated_frame``'s ``remove`` checked -> (classes, S, T, M), or None."""
    if remove is None:
        return None
    try:
        classes, settle, tol, margin = () if isinstance(remove, str) else remove
    except (TypeError, ValueError):
        raise ValueError("remove=%r: (classes, settle, tol, margin)" % (remove,)) from None
    return ops.plate_option(classes, settle, tol, margin)


def _plate_out(plate_out, remove):
    """``plate_out`` checked against ``remove`` -> the path, or None."""
    if plate_out is None:
        return None
    if remove is None:
        raise ValueError("plate_out=%r is where the background plate is written: it needs remove=(classes, settle, tol, margin)" % (plate_out,))
    if not str(plate_out).lower().endswith(".png"):
        raise ValueError("plate_out=%r: the plate is written as an RGB PNG, a path that ends in .png" % (plate_out,))
    return str(plate_out)


def plate_summaries(states):
    """``states``: {(h, w, rgb): a plate state's host copy (numpy)} -> {(h, w, rgb): (frames, known, the (h, w, 3) plate as R, G, B with
    unknown pixels black)} for every state that saw a frame.  A size whose frames came in both channel orders (frames decoded by
    different decoders) has learned two plates, and both are reported."""
    met = {}
    for (h, w, rgb), st in sorted(states.items()):
        frames, known, plate, _ = ops.plate_image(st, h, w)
        if frames > 0:
            met[(h, w, rgb)] = (frames, known, plate if rgb else plate[:, :, ::-1])
    return met


def _plate_order_tag(key, summaries):
    """"" for a size met in one channel order; else which of its two plates this is."""
    h, w, rgb = key
    if (h, w, not rgb) not in summaries:
        return ""
    return "rgb" if rgb else "bgr"


def print_plates(summaries):
    """One line per frame size met: ``plate 1242x375: 128 frames, 97.3 % known``; a size met in both channel orders has a line per order,
    ``plate 1242x375 (bgr frames): ...`` and ``plate 1242x375 (rgb frames): ...``."""
    for key, (frames, known, _) in sorted(summaries.items()):
        h, w, _ = key
        tag = _plate_order_tag(key, summaries)
        print("plate {}x{}{}: {} frames, {:.1f} % known".format(w, h, " (%s frames)" % tag if tag else "", frames, 100.0 * known / (h * w)))


def write_plates(path, summaries):
    """Every plate of ``plate_summaries``'s result written as an RGB PNG with PIL, named as ``heatmap_paths`` names its files -- ``path``
    itself for one size, ``<stem>_<w>x<h>.png`` for several --, with ``_bgr`` / ``_rgb`` behind the size where one size has two plates
    -> the paths written."""
    from PIL import Image as PilImage
    by_size = heatmap_paths(path, {key[:2] for key in summaries})
    paths = {}
    for key in sorted(summaries):
        out, tag = by_size[key[:2]], _plate_order_tag(key, summaries)
        paths[key] = "%s_%s%s" % (out[:-4], tag, out[-4:]) if tag else out
        PilImage.fromarray(np.ascontiguousarray(summaries[key][2]), mode="RGB").save(paths[key])
    return [paths[key] for key in sorted(paths)]


def _plate_states(training_manager, eng):
    """The host copies of the plate states of ``eng``, or of the eager path with None: {(h, w, rgb): numpy int32}."""
    import torch
    torch.cuda.synchronize()
    states = eng.edit_states if eng is not None else _eager_states(training_manager.class_mapping)
    return {key: st.cpu().numpy() for key, st in states.plate.items()}


def _region_weights(training_manager, eng, h, w, option):
    """W, (h, w) uint16, of the plane of the region option ``option`` for frames of (h, w) in the states of ``eng``, or of the eager
    path with None."""
    states = eng.edit_states if eng is not None else _eager_states(training_manager.class_mapping)
    return ops.redact_region_weights(states.region_plane(h, w, option))


def reset_plate(training_manager, detector, in_flight=1, post=None):
    """An empty plate before a new sequence: the states of the engine ``in_flight`` names, or the eager path's."""
    eng = _engine(training_manager, detector, in_flight, post)
    if eng is not None:
        eng.plate_reset()
    else:
        _eager_states(training_manager.class_mapping).reset_plate()


def reset_moving(training_manager, detector, in_flight=1, post=None):
    """An empty moving state before a new sequence: the states of the engine ``in_flight`` names, or the eager path's.  (The plate the
    net compares with is ``reset_plate``'s.)"""
    eng = _engine(training_manager, detector, in_flight, post)
    if eng is not None:
        eng.moving_reset()
    else:
        _eager_states(training_manager.class_mapping).reset_moving()


def _lookback_frames(track_lookback, track, eng, B):
    """``annotate_images`` / ``annotate_stream``'s ``track_lookback`` checked -> the look-back of their passes, or None."""
    if track_lookback is None:
        return None
    if track is None:
        raise ValueError("track_lookback=%r hides the tracker's new tracks in earlier frames: it needs track=(thr, hold, grow)" % (track_lookback,))
    if eng is None:
        raise ValueError("track_lookback=%r delays the output by one pass: the eager path (a foreign model) returns every frame at once and "
                         "cannot" % (track_lookback,))
    if track_lookback == TRACK_LOOKBACK_AUTO and not isinstance(track_lookback, bool):
        return min(ops.TRACK_LOOKBACK[2], B)
    n = ops.track_lookback_option(track_lookback)
    if n > B:                                             # (what submit_batch would refuse at the first pass)
        raise ValueError("track_lookback=%d reaches further back than a pass of %d frames holds: at most %d here" % (n, B, B))
    return n


def mot_lines(frame_no, dets, class_mapping):
    """The MOTChallenge lines of one frame: ``frame,id,left,top,width,height,prob,cls,-1,-1`` per LIVE tracked det ("track_id" > 0, no
    "held"), in row order; left / top the smaller corner, width / height the corners' distance, prob with six decimals, cls the index."""
    out = []
    for d in dets:
        if d.get("held") or d.get("backfilled") or d.get("track_id", 0) <= 0:
            continue
        x1, y1, x2, y2 = [int(v) for v in d["bbox"]]
        out.append("%d,%d,%d,%d,%d,%d,%.6f,%d,-1,-1" % (frame_no, d["track_id"], min(x1, x2), min(y1, y2), abs(x2 - x1), abs(y2 - y1),
                                                       float(d["prob"]), class_mapping[d["cls_name"]]))
    return out


def _write_tracks(tracks_out, frame_no, dets, class_mapping):
    if tracks_out is not None:
        tracks_out.writelines(line + "\n" for line in mot_lines(frame_no, dets, class_mapping))


def reset_tracks(training_manager, detector, in_flight=1, post=None):
    """Forget every track before a new sequence: the state of the engine ``in_flight`` names, or the eager path's."""
    eng = _engine(training_manager, detector, in_flight, post)
    if eng is not None:
        eng.track_reset()
    else:
        _eager_states(training_manager.class_mapping).reset_tracks()


def _print_drawn(dets, width, height):
    for det in dets:
        if not det.get("held") and not det.get("backfilled") and drawn(det, width, height):       # (held and back-filled rows are never drawn)
            print(det)


def _output_needs(name, option, text):
    """The check of an output against its option; the one-frame form's wording leaves the value out."""
    def check(v, c):
        if v[name] is not None and v[option] is None:
            raise ValueError((name if c.form == "frame" else "%s=%r" % (name, v[name])) + text)
    return check


def _normalised(name, check, *others):
    """The step that replaces option ``name`` by ``check(its value, the values of the options ``others``)``."""
    def step(v, c):
        v[name] = check(v[name], *(v[o] for o in others))
    return step


def _check_motion(v, c):
    if v["track_motion"] is not None and v["track"] is None:
        raise ValueError("track_motion=%r moves the boxes of the tracker: it needs track=(thr, hold, grow)" % (v["track_motion"],))
    if c.form == "draw" and v["track_motion"] is not None:
        v["track_motion"] = ops.track_motion_radius(v["track_motion"])


def _check_thresholds(v, c):
    v["det_threshold"], v["track_low"] = _det_thresholds(v["det_threshold"], v["track_low"], v["track"])


def _check_remove_names(v, c):
    if v["remove"] is not None and v["remove"][0] != "all":
        ops.plate_class_list(_names_by_index(c.owner if isinstance(c.owner, dict) else c.owner.class_mapping), v["remove"][0])


def _check_moving(v, c):
    v["redact_moving"] = _redact_moving(v["redact_moving"], v["remove"], c.owner)


def _check_reid_delayed(v, c):
    if v["track_reid"] is not None and c.form == "frame" and v["track_lookback"] is not None:
        raise ValueError("track_reid=%r together with track_lookback= is not supported" % (v["track_reid"],))
    if v["track_reid"] is not None and c.form == "list" and (v["track_lookback"] is not None or v["track_backtrack"] is not None):
        raise ValueError("track_reid=%r together with track_lookback= / track_backtrack= is not supported: the window of a delayed pass "
                         "holds the tracker's own ids" % (v["track_reid"],))


def _check_region_fits(v, c):
    mask = None if v["redact_region"] is None else v["redact_region"][1]
    if mask is not None and mask.shape != tuple(c.frame.shape[:2]):
        raise ValueError("redact_region: the mask is %dx%d, %s %dx%d" % (mask.shape[1], mask.shape[0], "the frame" if c.form == "draw" else
                                                                          "frame %s is" % (c.label,), c.frame.shape[1], c.frame.shape[0]))


def _check_out_fits(v, c):
    if v["out_size"] is not None:
        if c.form == "draw":
            ops.scale_option(v["out_size"], c.frame.shape[:2])
        else:
            scaled_size(v["out_size"], c.label, c.frame.shape[1], c.frame.shape[0])
        v["out_size"] = ops.scale_form(v["out_size"])


def _check_one_frame(v, c):
    if v["detect_every"] is not None:
        raise ValueError("detect_every=%r runs the detector once per pass of several frames: get_annotated_frame detects its one frame and "
                         "cannot; use annotate_images or annotate_stream" % (v["detect_every"],))
    for name in ("track_backtrack", "track_lookback"):
        if v[name] is not None:
            raise ValueError("%s=%r delays the output: get_annotated_frame returns its frame at once and cannot; use annotate_images "
                             "or annotate_stream" % (name, v[name]))


_check_post = _normalised("post", lambda post: None if post is None else ops.det_post_option(post))
_check_out_size = _normalised("out_size", lambda out_size: None if out_size is None else ops.scale_form(out_size))
_check_cut = _normalised("track_scene_cut", lambda cut, track, motion: _track_scene_cut(cut, track, motion, None, None), "track", "track_motion")
_check_counts_out = _output_needs("counts_out", "count", " is where the crossings are written: it needs count=(lines, classes, width)")
_check_zones_out = _output_needs("zones_out", "zone", " is where the zone events are written: it needs zone=(zones, classes, width, anchor)")
_check_reid_out = _output_needs("reid_out", "track_reid", " is where the re-identifications are written: it needs track_reid=(pct, keep)")
_check_shape, _check_region = _normalised("redact_shape", _redact_shape, "redact"), _normalised("redact_region", _redact_region)
_check_reid, _check_count, _check_zone = _normalised("track_reid", _track_reid, "track"), _normalised("count", _count, "track"), _normalised("zone", _zone, "track")
_check_trails = _normalised("track_trails", _track_trails, "track", "draw")
_check_heatmap, _check_remove = _normalised("heatmap", _heatmap), _normalised("remove", _remove)
# The engine-independent checks of each form, IN THE ORDER the form has always run them: with two violations the first one is reported,
# and the three entry points grew different orders.  A list leaves ``detect_every``, ``track_lookback``, ``track_backtrack``,
# ``track_scene_cut`` and, behind them, ``track_trails`` to ``_tracking_options``, where the engine is known.
_CHECKS = {
    "list": (_check_motion, _check_thresholds, _check_post, _check_heatmap, _normalised("heatmap_out", _heatmap_out, "heatmap"), _check_remove,
             _normalised("plate_out", _plate_out, "remove"), _check_remove_names, _check_moving, _normalised("moving_out", _moving_out, "redact_moving"),
             _check_count, _check_counts_out, _check_zone, _check_zones_out, _check_reid, _check_reid_out, _check_reid_delayed,
             _check_out_size, _check_shape, _check_region),
    "frame": (_check_post, _check_shape, _check_region, _check_region_fits, _check_out_fits, _check_reid, _check_reid_out,
              _check_reid_delayed, _check_count, _check_counts_out, _check_zone, _check_zones_out, _check_one_frame, _check_motion,
              _check_cut, _check_trails, _check_heatmap, _check_remove, _check_moving, _check_thresholds),
    "draw": (_check_shape, _check_region, _check_region_fits, _check_out_fits, _check_reid, _check_trails, _check_heatmap, _check_remove,
             _check_moving, _check_count, _check_zone, _check_motion, _check_cut),
}
OPTION_OUTPUTS = ("tracks_out", "heatmap_out", "counts_out", "zones_out", "plate_out", "reid_out", "moving_out")
# what a form does not take: an unknown keyword there, as it always was
_NOT_TAKEN = {"list": (), "frame": ("heatmap_out", "plate_out"),
              "draw": ("track_lookback", "detect_every", "track_backtrack", "post", "det_threshold", "track_low") + OPTION_OUTPUTS}
# option -> submit_batch's keyword, for every option that is one, in the order the passes' keywords were always built in
_PASS_KEYWORDS = {"track": "track", "track_motion": "track_motion", "track_lookback": "track_lookback", "detect_every": "detect_every",
                  "track_backtrack": "track_backtrack", "track_scene_cut": "track_scene_cut", "track_trails": "track_trails", "heatmap": "heat",
                  "remove": "remove", "redact_moving": "redact_moving", "count": "count", "zone": "zone", "track_reid": "track_reid",
                  "out_size": "out_size", "redact_shape": "redact_shape", "redact_region": "redact_region"}
_PASS_ONLY = ("track_lookback", "detect_every", "track_backtrack", "out_size")      # steps of a pass, not of a frame's editing chain


@dataclasses.dataclass(frozen=True)
class AnnotateOptions:
    """The options of one annotated sequence, checked and normalised: what ``annotate_images``, ``annotate_stream``,
    ``get_annotated_frame`` and ``draw_eager`` take as keywords (``checked``), what the command line states (``from_args``), and what
    they hand on: the keywords of ``submit_batch`` (``pass_keywords``) and of a one-frame edit (``edit_keywords``).  It mirrors
    ``entry.PassSpec`` on the caller's side: a new option is a field here, its check in ``_CHECKS``, its keyword in ``_PASS_KEYWORDS``
    and, when it keeps state over a sequence, its report in ``_reports``.  Without an option no pass, key, printed line or output byte
    is another.
    ``redact``: (classes, mode, size, margin) as ``redact_from_args`` returns it -- those classes' boxes are hidden in every frame inside
    its pass, in front of the drawing step and of whichever encoder writes the frame; None: nothing is.  ``draw`` False: no boxes, no labels.
    ``track``: (thr, hold, grow) as ``track_from_args`` returns it -- the list is ONE sequence in list order: the tracker's state is reset
    at the start, every tracked detection is labelled ``cls#id`` and lost tracks are held (and redacted) for ``hold`` frames; None: no
    tracking.  ``tracks_out``: a text file that receives the MOT lines, frame i of the list under the number i + 1.
    ``track_motion``: the search radius as ``track_motion_from_args`` returns it (with ``track``) -- every track's box is moved with the
    pixels under it from frame to frame, so a held box follows its object; None: held boxes stand still.
    ``track_lookback``: the frames as ``track_lookback_from_args`` returns them (with ``track``; TRACK_LOOKBACK_AUTO: as many as a pass
    holds, at most 8) -- every new track is followed BACK over that many frames and hidden there too (DESIGN §8 "Look-back rule").  Every
    group then goes through a full pass of B frames, a pass returns the frames of the pass before it and a flush ends the list: each
    frame is written and printed when it is emitted, the same lines in the same order.  The eager path refuses it.
    ``detect_every``: K as ``detect_every_from_args`` returns it (with ``track`` and ``track_motion``, not with ``track_lookback``) -- the
    detector runs on every K-th frame only and a pass takes B * K frames; on the frames between, every track's box follows the pixels under
    it (DESIGN §8 "Interval rule"), is drawn, redacted and written to ``tracks_out`` with the prob of its last match.  Nothing is matched,
    aged or born between two detected frames: ``hold`` counts detected frames.  The K-th frames are counted per GROUP, not over the list:
    a group is a run of at most B * K consecutive frames of one geometry, it is cut where the geometry changes, and its frames 0, K,
    2K, ... are the detected ones (a group whose key frames fill under half a pass goes through one-image passes of K frames, the same
    key frames).  With frames of one size, a video, every group but the last is full and that is every K-th frame of the list; in a list
    of mixed sizes a detected frame follows every change of geometry.  The eager path refuses it.
    ``track_backtrack``: the frames as ``track_backtrack_from_args`` returns them (with ``detect_every``, not with ``track_lookback``;
    TRACK_BACKTRACK_AUTO: as many as a pass of B * K frames holds, at most 16; at least K - 1) -- at every detected frame every track is
    followed BACK through the frames in front of it (DESIGN §8 "Back-track rule"): a continued track as far as the detected frame before,
    a new one over that many frames, and the boxes found are hidden there too, so a frame between two detections is covered from both
    sides.  Every group of at most B * K frames then goes through one full (padded) pass, a pass returns the frames of the pass before it
    and a flush follows a change of geometry and the end of the list, as with ``track_lookback``.  The eager path refuses it.
    ``track_scene_cut``: the percentage as ``track_scene_cut_from_args`` returns it (with ``track`` and ``track_motion``, with or without
    ``detect_every``; not with ``track_lookback`` or ``track_backtrack``, whose backward chains would have to stop at a cut) -- a frame
    whose 4 x 4-region luma histogram differs from the frame before by that share of the largest distance there is, is a hard cut (DESIGN
    §8 "Cut rule"): every track ends in front of it, so no id is inherited by the new scene and no held box of the old scene is redacted
    in it; between two detected frames nothing is shown behind a cut until the next detected frame.  A line ``scene cut: <path>`` is
    printed in front of that frame's lines.  A fade or a dissolve is not detected.  None: every byte and line is what it was.
    ``track_trails``: (N, W) as ``track_trails_from_args`` returns it (with ``track``, in every form above; not with ``draw`` False) -- the
    path of every id is kept on the device and each frame shows the last N points of the ids live in it as a line W pixels wide in the
    colour of the id (DESIGN §8 "Trail rule"), over the redaction and under the boxes; a delayed pass draws them in the order its frames
    are emitted.  The printed lines and ``tracks_out`` are unchanged.  None: every byte and line is what it was.
    ``heatmap``: (classes, A, S) as ``heatmap_from_args`` returns it (with every option above, ``draw`` False included) -- a map on the
    device that starts cold with the list gains 256 per box of those classes in every frame (every detection; with ``track`` the live
    tracked rows, in a delayed pass the emitted frames'), loses ceil(v / 2^S) per frame, and is blended into each frame at weight A for
    the hottest pixel, over the redaction and under the trails, boxes and labels (DESIGN §8 "Heat rule").  ``heatmap_out``: a path ending
    in .png that receives the map at the end of the list, 8-bit grey, one file per frame size met (``<stem>_<w>x<h>.png`` for several).
    The printed lines and ``tracks_out`` are unchanged.  None: every byte and line is what it was.
    ``count=(lines, classes, W)`` (``--count_line X1,Y1,X2,Y2``, repeatable up to 8 times, with ``--track`` in any of the forms above;
    ``--count_classes``, ``--count_width``) counts the tracks whose box centre crosses a line, once per id, line and direction
    (ops.count_update / ops.count_draw_u8, csrc/count.hip; DESIGN §8 "Count rule"): each frame shows the lines and a label ``L{l} +{pos}
    -{neg}`` per line over the redaction, heat map and trails and under the boxes, ``counts_out=PATH`` (``--counts_out``) receives a CSV row
    ``frame,line,direction,id,cls`` per crossing, and at the end one line per counting line and the totals per class are printed.  A list
    starts from zero totals; ``get_annotated_frame(count=, counts_out=)`` and the eager path take the option as one-frame calls that continue
    the state (``reset_counts`` zeroes it).  On the command line a value that begins with a minus sign needs the ``=`` form:
    ``--count_line=-5,0,-5,100``.
    ``zone=(zones, classes, W, anchor)`` (``--zone X1,Y1,X2,Y2,X3,Y3[,...]``, repeatable up to 8 times, with ``--track`` in any of the forms
    above; ``--zone_classes``, ``--zone_width``, ``--zone_anchor centre|bottom``) tests every track's box centre, or the middle of its bottom
    edge, against polygon zones with an exact even-odd rule (ops.zone_update / ops.zone_draw_u8, csrc/zone.hip; DESIGN §8 "Zone rule"): each
    frame shows the occupied zones tinted, every zone's outline and a label ``Z{z} {occupancy}/{visitors}`` behind the heat map and under
    every line, ``zones_out=PATH`` (``--zones_out``) receives a CSV row ``frame,zone,kind,id,cls,dwell`` per event, kind enter, exit or lost,
    and at the end one line per zone is printed: visitors, peak, stays and the mean dwell of the completed stays.  A list starts from an
    empty state; ``get_annotated_frame(zone=, zones_out=)`` and the eager path take the option as one-frame calls that continue the state
    (``reset_zones`` starts over).  ``--no_draw`` still counts.  A value that begins with a minus sign needs the ``=`` form: ``--zone=-5,0,9,0,9,9``.
    ``remove=(classes, S, T, M)`` (``--remove CLASSES``, class names of the active mapping or ``all``; ``--remove_settle S``, 1..255;
    ``--remove_tol T``, 0..255; ``--remove_margin M``, 0..64; the defaults 8, 10 and 8 are PROVISIONAL: nobody has measured them on real
    footage) paints the objects of those classes out of fixed-camera footage (ops.plate_update / ops.plate_fill_u8, csrc/plate.hip; DESIGN §8
    "Plate rule"): a background plate on the device learns every pixel that no box of ANY class touches -- held and back-filled tracked rows
    too -- and that stays within T of the value its run began with for S frames, and the boxes of the classes, grown by M, are filled with
    it.  Where the plate is not known yet the redaction shows, if ``--redact`` covers the classes, else black.  An object that stands still
    and is never detected becomes background after S frames: that is the rule's limit.  A ``--track_scene_cut`` cut empties the plate.  A
    list starts from an empty plate; ``get_annotated_frame(remove=)`` and the eager path continue it as one-frame calls (``reset_plate``
    empties it).  ``plate_out=PATH.png`` (``--plate_out``) writes the plate at the end as an RGB PNG with unknown pixels black, one per
    frame size met, named as ``--heatmap_out`` names its files, and one line per size is printed: ``plate 1242x375: 128 frames, 97.3 %
    known`` (a size met in both channel orders has two plates: a line and a file for each).  With every other option, ``--no_draw`` included, with and without ``--track``.
    ``track_reid=(pct, keep)`` (``--track_reid [PCT]``, 1..100, bare: 25; ``--reid_keep N``, 1..4095 frames, default 250; both defaults are
    PROVISIONAL: nobody has measured them on real footage; with ``--track`` in every form but ``--track_lookback`` / ``--track_backtrack``)
    gives an object that was hidden for longer than ``--track_hold`` frames its old id back (ops.track_reid_update, csrc/track_reid.hip;
    DESIGN §8 "Re-identify rule"): every live tracked row gets a colour signature, and a new track whose signature lies within PCT percent
    of that of an id the tracker gave up at most N frames ago carries that id -- in the labels, ``--tracks_out``, the printed ``track_id``,
    the trails, the count lines (which then count it once) and the zones.  A line ``re-identified: <path> id <pid>`` is printed in front
    of that frame's lines and ``re-identified: N`` at the end; ``reid_out=PATH`` (``--reid_out``) receives a CSV row
    ``frame,id,tracker_id,cls,distance,gap`` per event.  A list starts from an empty memory; ``get_annotated_frame(track_reid=)`` and the
    eager path continue it as one-frame calls (``reset_tracks`` empties it).  A ``--track_scene_cut`` cut empties it too.
    ``post``: the post-process option as ``args_util.post_from_args`` returns it (``ops.det_post_option``: mode, nms_thresh, sigma,
    min_score, vote_iou) -- soft-NMS and box voting inside the captured passes (DESIGN §8 "Post-process rule"), on the eager path through
    ``ops.detections_post``: which boxes every frame reports, with decayed scores in the soft modes; everything above then works on those
    boxes.  The passes belong to an engine of their own.  None: no pass, engine key, printed line or output byte changes.
    ``out_size``: ("size", W, H) or ("scale", N) as ``out_size_from_args`` returns it -- every frame is scaled DOWN on the device as the
    last step of its pass, behind every edit and in front of whichever encoder writes it (DESIGN §8 "Scale rule": the exact area mean, in
    integers; labels shrink with the picture): the device encoders encode, and the read-back copies, the smaller frame; the host encoders
    simply receive it.  ("scale", N) applies per frame size in a list of mixed sizes; ("size", W, H) is refused with the name of the
    first frame that is smaller than it (or more than 16 times its size along a side).  The printed lines, ``tracks_out``, ``counts_out``
    and ``zones_out`` stay in SOURCE coordinates.  None: no pass, key, printed line or output byte changes.
    ``redact_shape``: (shape, feather) as ``redact_shape_from_args`` returns it (with ``redact``, and with every option above) -- every
    box the redaction hides, held and back-filled ones too, hides the ellipse inscribed in the box grown by the margin ("ellipse"), and
    the replacement fades into the scene over ``feather`` pixels OUTSIDE the shape, so nothing the hard shape hides shows (DESIGN §8
    "Shape rule", ops.redact_shaped_u8).  The plate of ``remove``, the tracker, the heat map and the drawn boxes keep their rectangles.
    None and ("box", 0): no pass, key, printed line or output byte changes.
    ``det_threshold``: T, a float in 0..1 (``--det_threshold``; None: DET_THRESHOLD = 0.0, the reference script's): the score under which
    a detection is not reported; with or without ``track``.  ``track_low``: L < T (``--track_low``, with ``track``): the weak rule
    (DESIGN §8 "Weak rule", the ``strong=`` form of the tracker call): the passes emit rows down to L (submit_batch's det_threshold = L,
    track_strong = T), a row with a score in [L, T) may only continue a track that no row of T or more continued, and every other such
    row is dropped -- so an object whose score dips stays covered by the detector's own box, under its id, and nothing new is reported
    under T.  "num dets", the printed lines and ``tracks_out`` show the kept rows.  Refused by name without ``track``, for L >= T and
    outside 0..1, and on the eager path (a foreign model).  None and None: no pass, key, printed line or output byte changes.
    ``redact_region``: (regions, mask, mode, size, feather) as ``redact_region_from_args`` returns it (with every option above, with and
    without ``redact`` and ``track``) -- static areas, polygons in source-frame pixels and a painted mask whose bytes >= 128 hide, are
    hidden in EVERY frame whatever the detector says (DESIGN §8 "Region rule"): what replaces them comes from the untouched frame, they
    are blended in behind the plate fill of ``remove`` and under the heat map and everything drawn, and the edge fades outwards over
    ``feather`` pixels.  Polygons apply to every frame size; a mask is held to one, and a frame it does not fit is refused by name.
    ``plate_out`` then shows every pixel of an area black.  A line ``redact regions 1242x375: 2 regions + mask, 12.3 % of the frame
    hidden`` is printed per frame size at the end; every other printed line and file is unchanged.  None: no pass, key, printed line or
    output byte changes.
    ``redact_moving``: True, a dict of ops.redact_moving_option's keywords or its 12 values, as ``redact_moving_from_args`` returns it
    (with every option above, with and without ``remove`` and ``track``) -- the moving net (DESIGN §8 "Moving rule"): on fixed-camera
    footage whatever differs from the plate is hidden in every frame, detected or not.  The list starts from an EMPTY moving state and
    an empty plate; without ``remove`` the plate is learned all the same, with the option's (S, T, M), and nothing is painted out; with
    it the three are ``remove``'s, and one stated here that differs is refused by name.  The defaults 24, 8, 4 and 8 are PROVISIONAL.
    Until a pixel's background is known it is shown (unknown "hide" blanks it instead): the first S frames are not protected by the
    net under the default.  Delayed passes run the net on the frames they emit.  ``moving_out``: a path; a CSV ``frame,cells,covered``
    is written there.  A line ``moving net 1242x375: 128 frames, mean 3.2 % hidden, peak 17.0 %`` is printed per frame size at the
    end.  None: no pass, key, printed line or output byte changes.
    The outputs: ``tracks_out`` an open text file, the others paths (``heatmap_out`` / ``plate_out``: ending in .png).
    One frame at a time (``get_annotated_frame``, ``draw_eager``) every state CONTINUES from the call before: ``reset_tracks`` (ids,
    trails, the re-identify memory), ``reset_heat``, ``reset_counts``, ``reset_zones``, ``reset_plate`` and ``reset_moving`` start a
    new sequence; ``counts_out`` / ``zones_out`` / ``reid_out`` are then open text files that receive the frame's rows without a header,
    ``moving_out`` a ``MovingLog``; a mask of ``redact_region`` must have the frame's size."""
    redact: object = None
    draw: bool = True
    track: object = None
    track_motion: object = None
    track_lookback: object = None
    detect_every: object = None
    track_backtrack: object = None
    track_scene_cut: object = None
    track_trails: object = None
    heatmap: object = None
    count: object = None
    zone: object = None
    remove: object = None
    track_reid: object = None
    post: object = None
    out_size: object = None
    redact_shape: object = None
    det_threshold: object = None                          # checked: T, a float (DET_THRESHOLD when not stated)
    track_low: object = None
    redact_region: object = None
    redact_moving: object = None
    tracks_out: object = None
    heatmap_out: object = None
    counts_out: object = None
    zones_out: object = None
    plate_out: object = None
    reid_out: object = None
    moving_out: object = None

    @classmethod
    def checked(cls, owner, form="list", frame=None, label=None, **stated):
        """The keywords of an entry point -> the value, every engine-independent check run once (``_CHECKS``).  ``owner``: the class
        mapping, or the training manager that holds it (read only by the options that name classes).  ``form``: "list"
        (``annotate_images`` / ``annotate_stream``), "frame" (``get_annotated_frame``, which refuses ``detect_every``, ``track_lookback``
        and ``track_backtrack``) or "draw" (``draw_eager``); the last two check a mask and an ``out_size`` against ``frame``, the frame
        ``label``.  TypeError for a keyword the form does not take, ValueError with the reason for everything else."""
        values = dict(vars(cls(**stated)))
        for name in _NOT_TAKEN[form]:
            if name in stated:
                raise TypeError("got an unexpected keyword argument %r" % name)
        context = _Context(owner, form, frame, label)
        for check in _CHECKS[form]:
            check(values, context)
        return cls(**values)

    @classmethod
    def from_args(cls, args, class_mapping, stack):
        """(host only) What the command line states -> the value, through the ``*_from_args`` functions (each ValueError names the
        flag); ``tracks_out`` is opened on ``stack``.  The entry point that takes the value's fields checks them against each other."""
        v = dict(redact=redact_from_args(args, class_mapping), draw=not args.no_draw, track=track_from_args(args))
        v["track_motion"] = track_motion_from_args(args)
        if v["track"] is not None and args.tracks_out:
            v["tracks_out"] = stack.enter_context(open(args.tracks_out, "w"))
        v["track_lookback"] = track_lookback_from_args(args)
        v["detect_every"] = detect_every_from_args(args)
        v["track_backtrack"] = track_backtrack_from_args(args)
        v["track_scene_cut"] = track_scene_cut_from_args(args)
        v["track_trails"] = track_trails_from_args(args)
        v["heatmap"], v["heatmap_out"] = heatmap_from_args(args, class_mapping)
        v["remove"], v["plate_out"] = remove_from_args(args, class_mapping)
        v["redact_moving"], v["moving_out"] = redact_moving_from_args(args, class_mapping, v["remove"])
        v["count"], v["counts_out"] = count_from_args(args, class_mapping)
        v["track_reid"], v["reid_out"] = track_reid_from_args(args)
        v["zone"], v["zones_out"] = zone_from_args(args, class_mapping)
        from .args_util import post_from_args
        v["post"] = post_from_args(args)                  # (dependent options are refused by name)
        v["out_size"] = out_size_from_args(args)
        v["redact_shape"] = redact_shape_from_args(args)
        v["redact_region"] = redact_region_from_args(args)
        return cls(**v, **det_thresholds_from_args(args))

    @property
    def uploaded_threshold(self):
        """The score threshold the passes upload: under the weak rule the LOW one (the tracker is told ``det_threshold``)."""
        return self.det_threshold if self.track_low is None else self.track_low

    def pass_keywords(self, sink_keywords=()):
        """The keywords of ``submit_batch`` behind ``batch``, for a sink's encoder keywords.  An option that is not stated is absent,
        ``redact`` and ``draw`` too unless one is: the pass, and its key, are then the ones without the argument."""
        kw = dict(sink_keywords, annotate=True)
        kw.update((keyword, getattr(self, name)) for name, keyword in _PASS_KEYWORDS.items() if getattr(self, name) is not None)
        if self.track_low is not None:                    # the weak rule: the passes emit rows down to ``track_low``
            kw["track_strong"] = self.det_threshold
        if self.redact is not None or not self.draw:
            kw.update(redact=self.redact, draw=self.draw)
        return kw

    def edit_keywords(self):
        """The fields of the ``entry.PassSpec`` of a one-frame edit (``frame_edit.EditChain``): ``pass_keywords`` without the steps that
        belong to a pass."""
        kw = {k: v for k, v in self.pass_keywords().items() if k not in _PASS_ONLY and k != "track_strong"}
        if self.track_motion is not None:
            kw["track_motion"] = ops.track_motion_radius(self.track_motion)
        redact = self.redact if self.redact is None else (self.redact[0] if self.redact[0] == "all" else tuple(self.redact[0]),) + tuple(self.redact[1:])
        return dict(kw, redact=redact, draw=self.draw)


_Context = collections.namedtuple("_Context", "owner form frame label")


class TracksLog:
    """A sequence report (``_reports``): the MOT lines of a tracked sequence go to ``file`` (None: none)."""
    output = None

    def __init__(self, file, class_mapping):
        self.file, self.class_mapping = file, class_mapping

    def frame(self, pos, label, frame, dets, marks):
        _write_tracks(self.file, pos + 1, dets, self.class_mapping)

    def end(self):
        pass

    close = end


class _EndReport:
    """A sequence report (``_reports``) that only speaks at the end of the list: ``end`` is the function given."""
    output = None

    def __init__(self, end):
        self.end = end

    def frame(self, pos, label, frame, dets, marks):
        pass

    def close(self):
        pass


def _reports(o, training_manager, detector, eng, region_sizes):
    """The reports of a sequence with the options ``o``: one object per active feature that keeps state over the sequence, yielded
    behind the reset of that state, with ``frame(pos, label, frame, dets, marks)`` for every frame a pass returns, ``end()`` for the
    summary and ``close()``; ``output`` names the option under which the eager path's frames find it.  THE ORDER IS BEHAVIOUR: it is
    the order of a frame's printed lines and of the summaries at the end of the list.  (The resets run in it too; they empty
    independent states on one stream, so their order does not show.)  ``region_sizes``: the set of (h, w) the sink's check fills."""
    mapping = training_manager.class_mapping
    states = lambda: eng.edit_states if eng is not None else _eager_states(mapping)
    reset = lambda of: of(training_manager, detector, 1 if eng is None else eng.in_flight, o.post)
    if o.track is not None:                               # a new sequence; its frames are submitted in input order, as every list's are
        reset(reset_tracks)
        yield TracksLog(o.tracks_out, mapping)
    if o.count is not None:                               # zero totals for the list
        reset(reset_counts)
        yield CountsLog(o.counts_out, _names_by_index(mapping), len(o.count[0]), lambda: _count_state(training_manager, eng))
    if o.zone is not None:                                # an empty state for the list
        reset(reset_zones)
        yield ZonesLog(o.zones_out, _names_by_index(mapping), len(o.zone[0]), lambda: _zone_state(training_manager, eng))
    if o.track_reid is not None:                          # (an empty memory for the list: reset_tracks above emptied it)
        yield ReidLog(o.reid_out, _names_by_index(mapping))
    if o.heatmap is not None:                             # a cold map for the list; its t values as grey PNG files at the end
        reset(reset_heat)
        if o.heatmap_out is not None:
            yield _EndReport(lambda: write_heatmaps(o.heatmap_out, _heat_states(training_manager, eng)))
    if o.remove is not None or o.redact_moving is not None:      # an empty plate for the list, under the moving net too
        reset(reset_plate)
    if o.remove is not None:                              # the plate as an RGB PNG at the end, unknown pixels black

        def plates():
            summaries = plate_summaries(_plate_states(training_manager, eng))
            print_plates(summaries)
            if o.plate_out is not None:
                if o.redact_region is not None:           # the plate picture never shows a static area in clear
                    summaries = {key: (n, known, blacken_plate(plate, ops.redact_region_weights(states().region_plane(key[0], key[1], o.redact_region))))
                                 for key, (n, known, plate) in summaries.items()}
                write_plates(o.plate_out, summaries)
        yield _EndReport(plates)
    if o.redact_moving is not None:                       # an empty moving state for the list
        reset(reset_moving)
        yield MovingLog(o.moving_out)
    if o.redact_region is not None:                       # (the planes' headers read back)

        def regions():
            for h, w in sorted(region_sizes):
                print(region_line(w, h, o.redact_region, ops.redact_region_stats(states().region_plane(h, w, o.redact_region))))
        yield _EndReport(regions)


def get_annotated_frame(training_manager, detector, frame, img, resize_min, resize_max, frame_no=1, **options):
    """annotate_video.py:27-44: detect on ``img`` (an InMemoryImage of ``frame``), draw into ``frame`` in place, return it -- with
    ``out_size`` the scaled frame, a new (H, W, 3) array, in its place.  ``options``: the options of ``AnnotateOptions`` in their
    one-frame form; the frame's rows go to the outputs under the number ``frame_no``, which also stands where a list prints the path
    (``scene cut: <frame_no>``, ``re-identified: <frame_no> id <pid>``)."""
    return _annotated_frame(training_manager, detector, frame, img, resize_min, resize_max, frame_no,
                            AnnotateOptions.checked(training_manager, "frame", frame, frame_no, **options))


def _annotated_frame(training_manager, detector, frame, img, resize_min, resize_max, frame_no, o):
    """``get_annotated_frame`` with its options checked: ``o``, an ``AnnotateOptions``."""
    eng = _engine(training_manager, detector, 1, o.post)
    _det_thresholds(o.det_threshold, o.track_low, o.track, eager=eng is None)      # (a foreign model refuses an L, in front of any work)
    resized_imgs, resized_ratios = resize_imgs([img], min_size=resize_min, max_size=resize_max)
    info = {}
    if eng is not None:
        pixels = eng.host_pixels(resized_imgs[0])
        ticket = eng.submit_batch([resized_imgs[0]], [resized_ratios[0]], o.uploaded_threshold, [pixels], batch=1,
                                  **dict(o.pass_keywords(), redact=o.redact, draw=o.draw))
        num_rois, dets, out, *more = eng.collect_batch(ticket)[0]
        info = more[0] if more else info                          # (a ``track_scene_cut`` pass: the frame's marks behind its payload)
        if info.get("scene_cut"):
            print("scene cut: {}".format(frame_no))
        _print_reid(frame_no, info.get("reid", ()))
        print("num rois: {}".format(num_rois))
        if o.out_size is None:
            frame[...] = out
        else:
            frame = out
    else:
        dets = voc_dets.get_dets(training_manager, detector, resized_imgs[0], resized_ratios[0], stride=STRIDE, det_threshold=o.det_threshold,
                                 post=o.post)
        frame = _edit_eager(frame, dets, training_manager.class_mapping, o, info)
        if info.get("scene_cut"):
            print("scene cut: {}".format(frame_no))
        _print_reid(frame_no, info.get("reid", ()))
    if o.track is not None:
        _write_tracks(o.tracks_out, frame_no, dets, training_manager.class_mapping)
    if o.track_reid is not None:
        _write_reid(o.reid_out, frame_no, info["reid"], training_manager.class_mapping)
    if o.count is not None:
        _write_counts(o.counts_out, frame_no, info["crossings"], training_manager.class_mapping)
    if o.zone is not None:
        _write_zones(o.zones_out, frame_no, info["zones"]["events"], training_manager.class_mapping)
    if o.redact_moving is not None and o.moving_out is not None:
        o.moving_out.add(frame_no, img.height, img.width, info["moving"])
    _print_drawn(dets, img.width, img.height)
    return frame


def _read_rgb(path):
    from PIL import Image as PilImage
    with PilImage.open(path) as im:
        if im.mode != "RGB":
            im = im.convert("RGB")
        return np.asarray(im)


def _write_png(path, rgb):
    from PIL import Image as PilImage
    PilImage.fromarray(rgb).save(path, compress_level=PNG_COMPRESS_LEVEL)


def _write_jpg(path, rgb, quality, subsampling=444, huffman="standard"):
    from PIL import Image as PilImage
    PilImage.fromarray(rgb).save(path, format="JPEG", quality=quality, subsampling=2 if subsampling == 420 else 0,
                                 optimize=huffman == "optimized")


def _write_bytes(path, data):
    with open(path, "wb") as f:
        f.write(data)


JPEG_SUFFIXES = (".jpg", ".jpeg")
JPEG_DECODERS = ("host", "device", "device_full")


PNG_DECODERS = ("host", "device", "device_full")


def frame_filenames(input_dir, jpeg_decoder="host", png_decoder="host"):
    """``png_filenames`` and, with ``jpeg_decoder`` = "device" or "device_full", the ``*.jpg`` / ``*.jpeg`` names too: the input frames, sorted.
    ``png_decoder`` ("host" / "device" / "device_full": who decodes the ``*.png`` frames) is checked and changes no name."""
    from .feed import jpeg_decoder_option, png_decoder_option
    png_decoder_option(png_decoder, "png_decoder")
    if jpeg_decoder_option(jpeg_decoder, "jpeg_decoder") == "host":
        return png_filenames(input_dir)
    return sorted(f for f in os.listdir(input_dir) if f.endswith(".png") or f.lower().endswith(JPEG_SUFFIXES))


class _FileFrame:
    """A .jpg or .png input frame the device decodes: the file's bytes and the size its header states (entry.DetectionEntry.host_pixels
    asks ``raw_file()``); ``raw_rgb`` decodes on the host for whoever still wants pixels.  ``png_planned``: what feed.plan_png made, under the PNG decoder setting in force, of
    a .png file on the decode thread (its zlib stream and plan), so that ``host_pixels`` does not parse it again."""

    def __init__(self, data, path, file_size, width=None, height=None, png_planned=None):
        self.data, self._image_path, self.file_size, self.png_planned = data, path, file_size, png_planned
        self.height = int(file_size[0]) if height is None else height
        self.width = int(file_size[1]) if width is None else width
        self._pixels = None

    def raw_file(self):
        return self.data

    def raw_size(self):
        return self.file_size

    @property
    def raw_rgb(self):
        import io
        from PIL import Image
        with Image.open(io.BytesIO(self.data)) as im:
            return np.asarray(im.convert("RGB"))

    raw = property(lambda s: s.raw_rgb[:, :, ::-1])

    def resize(self, scale_ratio):
        return _FileFrame(self.data, self._image_path, self.file_size, int(round(scale_ratio * self.width)), int(round(scale_ratio * self.height)),
                          self.png_planned)

    def resize_within_bounds(self, min_size, max_size):
        ratio = shapes._bounds_ratio(self.width, self.height, min_size, max_size)
        return self.resize(ratio), ratio


class _Frame:
    """A file-backed frame decoded ahead of time: the reference's InMemoryImage (width, height, resize) whose pixels are
    uploaded in the decoder's RGB order (entry.DetectionEntry.host_pixels: the device resize swaps channels to BGR)."""

    def __init__(self, rgb, width=None, height=None):
        self.rgb = rgb
        self.height = int(rgb.shape[0]) if height is None else height
        self.width = int(rgb.shape[1]) if width is None else width

    raw = property(lambda s: s.rgb[:, :, ::-1])
    raw_rgb = property(lambda s: s.rgb)

    def resize(self, scale_ratio):
        return _Frame(self.rgb, int(round(scale_ratio * self.width)), int(round(scale_ratio * self.height)))

    def resize_within_bounds(self, min_size, max_size):
        ratio = shapes._bounds_ratio(self.width, self.height, min_size, max_size)
        return self.resize(ratio), ratio


def _load_frame(path, device_decode, device_png):
    """(decode thread) One input frame file: a ``_FileFrame`` when a device decoder in force (``device_decode``: the JPEG setting,
    ``device_png``: the PNG one) takes the file, else a ``_Frame`` decoded by PIL."""
    frame = None
    if device_decode != "host" and path.lower().endswith(JPEG_SUFFIXES):
        with open(path, "rb") as f:
            data = f.read()
        for planner in (ops.jpeg_dec_plan,) + ((ops.jpeg_dec_full_plan,) if device_decode == "device_full" else ()):
            try:
                plan = planner(data)
                frame = _FileFrame(data, path, (int(plan.h), int(plan.w)))
                break
            except ops.JpegUnsupported:
                pass                                      # (progressive under "device", CMYK, ...: PIL below)
    elif device_png != "host" and path.lower().endswith(".png"):
        from .feed import plan_png
        with open(path, "rb") as f:
            data = f.read()
        # None: a file the chosen planner refuses ("device": palette, 16-bit, interlaced, ...; "device_full": 16-bit grey, ...): PIL below
        planned = plan_png(data, device_png)
        if planned is not None:
            frame = _FileFrame(data, path, (int(planned[1].h), int(planned[1].w)), png_planned=planned)
    if frame is None:
        frame = _Frame(_read_rgb(path))
    return frame


class _Y4mFrame:
    """A frame of a YUV4MPEG2 stream: its planes and the stream's plan (entry.DetectionEntry.host_pixels finds ``y4m_plan`` and
    ``raw_file()`` and lets the device convert); ``raw_rgb`` converts on the host (y4m.decode_host) for whoever still wants pixels."""

    def __init__(self, data, plan, path, width=None, height=None):
        self.data, self.y4m_plan, self._image_path = data, plan, path
        self.height = int(plan.h) if height is None else height
        self.width = int(plan.w) if width is None else width
        self._pixels = None

    def raw_file(self):
        return self.data

    def raw_size(self):
        return int(self.y4m_plan.h), int(self.y4m_plan.w)

    @property
    def raw_rgb(self):
        return y4m.decode_host(self.data, self.y4m_plan)

    raw = property(lambda s: s.raw_rgb[:, :, ::-1])

    def resize(self, scale_ratio):
        return _Y4mFrame(self.data, self.y4m_plan, self._image_path, int(round(scale_ratio * self.width)), int(round(scale_ratio * self.height)))

    def resize_within_bounds(self, min_size, max_size):
        ratio = shapes._bounds_ratio(self.width, self.height, min_size, max_size)
        return self.resize(ratio), ratio


def stream_frames(reader):
    """(label, frame) per frame of a ``y4m.Y4mReader``: the label ``<name>#<frame index>`` stands where a frame file's path does."""
    for i, data in enumerate(reader):
        label = "%s#%d" % (reader.name, i)
        yield label, _Y4mFrame(data, reader.plan, label)


def directory_frames(input_dir, image_filenames, jpeg_decoder=None, png_decoder=None):
    """(path, frame) per frame file of a directory, for ``annotate_stream``: what ``annotate_images`` reads, as a stream."""
    if jpeg_decoder is not None:
        entry.set_jpeg_decoder(jpeg_decoder)
    if png_decoder is not None:
        entry.set_png_decoder(png_decoder)
    for f in image_filenames:
        path = os.path.join(input_dir, f)
        yield path, _load_frame(path, entry.jpeg_decoder(), entry.png_decoder())


def _encoder_options(png_encoder, png_compress, frame_format, jpeg_encoder, jpeg_quality, jpeg_subsampling, jpeg_huffman):
    """The frame-file encoder arguments of ``annotate_images`` checked (``png_options``, ``jpeg_options``, ``jpeg_size_options``) -> (the
    encoder's keywords of submit_batch -- none with a host encoder: the pass, and its key, without the arguments --, does the pass encode?,
    .jpg files?, ``write_host(path, rgb)`` of the host encoder, ``encode(bgr device frame)`` -> the file's bytes: the device encoder outside
    a pass, for the eager path)."""
    png_encoder, png_compress = png_options(png_encoder, png_compress)
    frame_format, jpeg_encoder, jpeg_quality = jpeg_options(frame_format, jpeg_encoder, jpeg_quality, png_encoder, png_compress)
    jpeg_subsampling, jpeg_huffman = jpeg_size_options(frame_format, jpeg_subsampling, jpeg_huffman)
    jpg = frame_format == "jpg"
    on_device = (jpeg_encoder if jpg else png_encoder) == "device"
    if jpg:
        kwargs = dict(encode="jpeg", quality=jpeg_quality, subsampling=jpeg_subsampling, huffman=jpeg_huffman) if on_device else {}
        write_host = lambda path, rgb: _write_jpg(path, rgb, jpeg_quality, jpeg_subsampling, jpeg_huffman)
        encode = lambda dev: ops.jpeg_bytes(dev, quality=jpeg_quality, bgr=True, subsampling=jpeg_subsampling, huffman=jpeg_huffman)
    else:
        kwargs = dict(encode="png" if png_compress == "runs" else "png-" + png_compress) if on_device else {}
        write_host = _write_png
        encode = lambda dev: ops.png_bytes(dev, bgr=True, compress=png_compress)
    return kwargs, on_device, jpg, write_host, encode


def _tracking_options(eng, o):
    """The tracking options of a list, ``o``'s, checked against the engine (None: the eager path) -> (``o`` with them as the passes
    take them: the K of a ``detect_every`` pass, the look-back of a ``track_lookback`` / ``track_backtrack`` pass, ...; do the passes
    return the frames of the pass before them?)."""
    B = None if eng is None else eng.batch
    every = _detect_every(o.detect_every, o.track, o.track_motion, o.track_lookback, eng, B)
    lookback = _lookback_frames(o.track_lookback, o.track, eng, B)
    backtrack = _backtrack_frames(o.track_backtrack, every, o.track_lookback, eng, B)
    cut = _track_scene_cut(o.track_scene_cut, o.track, o.track_motion, o.track_lookback, o.track_backtrack)
    trails = _track_trails(o.track_trails, o.track, o.draw)
    return (dataclasses.replace(o, detect_every=every, track_lookback=lookback, track_backtrack=backtrack, track_scene_cut=cut, track_trails=trails),
            lookback is not None or backtrack is not None)


class _Sink:
    """Where the annotated frames go.  ``kwargs``: the encoder's keywords of submit_batch; ``check(label, frame)`` refuses an input frame
    the sink cannot take; ``emit(pos, out)`` hands frame ``pos`` as its pass returned it to ``write(pos, out)`` on the ``threads`` writer
    threads -- at most 4 * WRITE_THREADS wait there: encoded frames must not pile up in memory --; ``emit_eager(pos, bgr)`` writes the eager
    path's frame at once; ``finish()`` waits for every write, then calls ``flush``; ``close()`` ends the threads."""

    def __init__(self, threads, kwargs, write, emit_eager, check=lambda label, frame: None, flush=lambda: None):
        self.kwargs, self._write, self.emit_eager, self.check, self._flush = kwargs, write, emit_eager, check, flush
        self._pool, self._writes = ThreadPoolExecutor(max_workers=threads), []

    def emit(self, pos, out):
        self._writes.append(self._pool.submit(self._write, pos, out))
        while len(self._writes) > 4 * WRITE_THREADS:
            self._writes.pop(0).result()

    def finish(self):
        for f in self._writes:
            f.result()
        del self._writes[:]
        self._flush()

    def close(self):
        self._pool.shutdown(wait=True)


def _y4m_sink(writer, video_chroma=None, out_size=None):
    """One YUV4MPEG2 stream through a ``y4m.Y4mWriter``: every frame is converted to the writer's chroma mode and range inside its pass
    and written by ONE thread, so in stream order; every input frame must have the writer's size -- with ``out_size`` its SCALED size
    must be the writer's."""
    import torch
    if video_chroma is not None and video_chroma != writer.chroma:
        raise ValueError("video_chroma=%r, the writer's stream is C%s" % (video_chroma, writer.chroma))

    def check(label, frame):
        size = (frame.width, frame.height) if out_size is None else scaled_size(out_size, label, frame.width, frame.height)
        if size != (writer.w, writer.h):
            raise ValueError("%s is %dx%d%s, the output stream's frames are %dx%d: one video stream holds frames of one size"
                             % (label, frame.width, frame.height, "" if out_size is None else " (scaled: %dx%d)" % size, writer.w, writer.h))

    record = lambda bgr: ops.y4m_encode_u8(torch.from_numpy(bgr).cuda(), writer.chroma, writer.range, bgr=True).cpu().numpy().tobytes()
    return _Sink(1, dict(encode="y4m", y4m=(writer.chroma, writer.range)), lambda pos, out: writer.write(out),
                 lambda pos, bgr: writer.write(record(bgr)), check, writer.flush)


def _file_sink(out_dir, names, *encoders):
    """Frame files in ``out_dir``, written on WRITE_THREADS threads through the encoders that ``encoders`` (``_encoder_options``'
    arguments) choose.  ``names``: the input frames' file names -- frame ``pos`` keeps its own, with the extension .jpg for JPEG frames --,
    or None: ``frame_%06d.png`` / ``.jpg``."""
    import torch
    kwargs, on_device, jpg, write_host, encode = _encoder_options(*encoders)
    pathlib.Path(out_dir).mkdir(parents=True, exist_ok=True)
    if names is None:
        name = lambda pos: "frame_%06d.%s" % (pos, "jpg" if jpg else "png")
    else:
        name = lambda pos: os.path.splitext(names[pos])[0] + ".jpg" if jpg else names[pos]
    if on_device:
        write = lambda pos, data: _write_bytes(os.path.join(out_dir, name(pos)), data)
        write_eager = lambda pos, bgr: write(pos, encode(torch.from_numpy(bgr).cuda()))
    else:
        write = lambda pos, rgb: write_host(os.path.join(out_dir, name(pos)), rgb)
        write_eager = lambda pos, bgr: write(pos, bgr[:, :, ::-1])
    return _Sink(max(1, WRITE_THREADS), kwargs, write, write_eager)


def _loaded_stream(source, prepare, ahead):
    """``prepare(label, frame)`` of every (label, frame) of the iterator ``source``, in order, read by ONE thread (a stream is sequential)
    that stays ``ahead`` frames in front of the consumer."""
    read, pending = ThreadPoolExecutor(max_workers=1), collections.deque()

    def load():                                           # (reader thread) -> the prepared frame, or None at the end
        try:
            label, frame = next(source)
        except StopIteration:
            return None
        return prepare(label, frame)

    try:
        while True:
            while len(pending) < ahead:
                pending.append(read.submit(load))
            got = pending.popleft().result()
            if got is None:
                for f in pending:                         # (reads behind the end: each finds the source exhausted)
                    f.result()
                return
            yield got
    finally:
        read.shutdown(wait=True, cancel_futures=True)


def _loaded_files(paths, prepare, ahead):
    """``prepare(path)`` of every frame file of the list ``paths``, in order, decoded on DECODE_THREADS threads that stay ``ahead`` files in
    front of the consumer."""
    decode, pending, n = ThreadPoolExecutor(max_workers=max(1, DECODE_THREADS)), {}, len(paths)
    try:
        for i in range(n):
            for j in range(i, min(n, i + ahead)):
                if j not in pending:
                    pending[j] = decode.submit(prepare, paths[j])
            yield pending.pop(i).result()
    finally:
        decode.shutdown(wait=True, cancel_futures=True)


def _run_passes(eng, loaded, emit, pass_kwargs, every, delayed, backtrack, det_threshold=DET_THRESHOLD):
    """The pipelined loop: the frames of ``loaded`` -- an in-order generator of (label, frame, resized, ratio, pixels) that reads ahead --
    are grouped into runs of at most B * K of one geometry, a group goes through one pass of B (padded) when it fills at least half of it
    (as get_dets_by_cls) and through one-frame passes else, ``eng.in_flight`` passes are in flight, and ``emit(pos, label, frame, result)``
    gets every frame's result in order.  ``pass_kwargs``: what every submit_batch takes behind ``batch``; ``every`` / ``delayed`` /
    ``backtrack``: ``_tracking_options``' -- a delayed pass is always a full one, returns the group before its own, and a flush submit
    follows a change of geometry and the last group.  ``det_threshold``: the score threshold every pass uploads."""
    B = eng.batch
    F = B * (every or 1)                                  # frames of a full pass
    window = []
    waiting, last_key = collections.deque(), [None]      # delayed passes: the groups whose frames a later pass emits; the geometry of the last pass

    def finish():
        part, ticket = window[0]
        try:
            results = eng.collect_batch(ticket)
        finally:
            window.pop(0)
        if delayed:                                       # (the pass returned the group before its own, or nothing)
            part = waiting.popleft() if results else ()
        for (pos, label, frame), result in zip(part, results):
            emit(pos, label, frame, result)

    def flush():                                          # the frames the look-back window still holds
        if last_key[0] is not None:
            window.append(((), eng.submit_batch([], [], det_threshold, [], batch=B, **pass_kwargs)))
            last_key[0] = None
            if len(window) >= eng.in_flight:
                finish()

    def submit(group):
        parts = [(group, B)] if B > 1 and len(group) >= max(2, B // 2) else [([g], 1) for g in group]
        if delayed:                                       # full passes only: a window belongs to one size of pass; a new geometry: a new window
            parts = [(group, B)]
            if last_key[0] not in (None, eng.geometry_of(group[0][5])):
                flush()
            last_key[0] = eng.geometry_of(group[0][5])
        if every is not None and backtrack is None:       # the key frames 0, K, ... of a pass go to the network, every frame goes up
            parts = _every_parts(group, B, every)
        for part, take in parts:
            keys = part[::every or 1]
            ticket = eng.submit_batch([g[3] for g in keys], [g[4] for g in keys], det_threshold, [g[5] for g in part], batch=take, **pass_kwargs)
            window.append(([(g[0], g[1], g[2]) for g in part], ticket))
            if delayed:
                waiting.append(window[-1][0])
            if len(window) >= eng.in_flight:
                finish()

    try:
        group, key = [], None
        for pos, (label, frame, resized, ratio, pixels) in enumerate(loaded):
            k = eng.geometry_of(pixels)
            if group and (k != key or len(group) == F):
                submit(group)
                group = []
            group.append((pos, label, frame, resized, ratio, pixels))
            key = k
        if group:
            submit(group)
        flush()
        while window:
            finish()
    finally:
        loaded.close()                                    # (ends the read-ahead threads)
        for _, ticket in window:                          # an exception mid-stream: no slot stays marked busy
            ticket.slot.event.synchronize()
            ticket.slot.busy = False


def _run_eager(training_manager, detector, frames, sink, resize_min, resize_max, o):
    """The eager path (foreign models): the reference's loop, one (label, frame) of ``frames`` at a time through ``get_annotated_frame``'s
    work (``o``: the checked options, their outputs the sequence's reports); a stream's frame is converted on the device."""
    for pos, (label, src) in enumerate(frames):
        sink.check(label, src)
        print("processing {}".format(label))
        if isinstance(src, _Y4mFrame):
            frame = ops.y4m_decode_u8(src.data, src.y4m_plan, bgr=True).cpu().numpy()
        else:
            frame = np.ascontiguousarray(src.raw)
        img = shapes.InMemoryImage(data=frame, width=frame.shape[1], height=frame.shape[0])
        sink.emit_eager(pos, _annotated_frame(training_manager, detector, frame, img, resize_min, resize_max, pos + 1, o))


def _sized_check(sink, o, region_sizes):
    """``sink.check`` with the options' own checks of a frame's size in front of it, on both paths: a frame the ``out_size`` target or
    the ``redact_region`` mask does not fit is refused by name.  ``region_sizes`` receives the (h, w) of the frames met."""
    check, mask = sink.check, None if o.redact_region is None else o.redact_region[1]

    def sized(label, frame):
        if o.out_size is not None:
            scaled_size(o.out_size, label, frame.width, frame.height)
        if mask is not None and mask.shape != (frame.height, frame.width):
            raise ValueError("redact_region: the mask is %dx%d, %s is %dx%d: a mask is held to one frame size"
                             % (mask.shape[1], mask.shape[0], label, frame.width, frame.height))
        region_sizes.add((frame.height, frame.width))
        check(label, frame)
    return sized


def _annotate(training_manager, detector, frames, loaded_from, make_sink, resize_min, resize_max, options=None, **stated):
    """What ``annotate_images`` and ``annotate_stream`` share.  ``frames``: the (label, frame) iterator the eager path reads;
    ``loaded_from(prepare, ahead)``: the read-ahead generator of the captured path (``_loaded_stream`` / ``_loaded_files``);
    ``make_sink()``: the ``_Sink``; ``options``: the checked ``AnnotateOptions`` (None: ``stated``, its keywords, checked here -- in
    front of any capture)."""
    o = options if options is not None else AnnotateOptions.checked(training_manager, **stated)
    sink, reports, region_sizes = make_sink(), [], set()
    if o.out_size is not None or o.redact_region is not None:
        sink.check = _sized_check(sink, o, region_sizes)
    try:
        dtype = getattr(getattr(detector, "head", None), "dtype", "f32")
        eng = _engine(training_manager, detector, entry.default_in_flight(dtype), o.post)
        _det_thresholds(o.det_threshold, o.track_low, o.track, eager=eng is None)      # (a foreign model refuses an L)
        o, delayed = _tracking_options(eng, o)
        for report in _reports(o, training_manager, detector, eng, region_sizes):
            reports.append(report)
        if eng is None:
            _run_eager(training_manager, detector, frames, sink, resize_min, resize_max,
                       dataclasses.replace(o, **{r.output: r for r in reports if r.output is not None}))
        else:
            def prepare(label, frame):                    # (read-ahead thread) -> (label, frame, resized, ratio, pixels)
                sink.check(label, frame)
                resized, ratio = frame.resize_within_bounds(resize_min, resize_max)
                return label, frame, resized, ratio, eng.host_pixels(resized)

            def emit(pos, label, frame, result):
                num_rois, dets, out, *marks = result      # (the frame's marks behind its payload, when an option leaves any)
                marks = marks[0] if marks else {}
                if marks.get("scene_cut"):
                    print("scene cut: {}".format(label))
                for report in reports:
                    report.frame(pos, label, frame, dets, marks)
                print("processing {}".format(label))
                print("num rois: {}".format(num_rois))
                _print_drawn(dets, frame.width, frame.height)
                sink.emit(pos, out)

            every = o.detect_every
            _run_passes(eng, loaded_from(prepare, 2 * eng.in_flight * eng.batch * (every or 1)), emit, o.pass_keywords(sink.kwargs), every, delayed,
                        o.track_backtrack, det_threshold=o.uploaded_threshold)
        sink.finish()
        for report in reports:                            # (host only: the states read back)
            report.end()
    finally:
        for report in reports:
            report.close()
        sink.close()


def annotate_stream(training_manager, detector, reader, writer_or_out_dir, resize_min, resize_max, video_chroma=None, png_encoder=None,
                    png_compress=None, frame_format=None, jpeg_encoder=None, jpeg_quality=None, jpeg_subsampling=None, jpeg_huffman=None,
                    **options):
    """``annotate_images`` for a video stream.  ``reader``: a ``y4m.Y4mReader`` (its frames are converted on the device inside the
    passes), or any iterable of (label, frame) such as ``directory_frames``.  ``writer_or_out_dir``: a ``y4m.Y4mWriter`` -- every
    annotated frame is converted to the writer's chroma mode and range inside its pass (submit_batch(encode="y4m")) and written in order;
    every frame must then have the writer's size, with ``out_size`` its SCALED size -- or a directory, which receives ``frame_%06d.png``
    / ``.jpg`` through the encoders the other arguments choose, as ``annotate_images`` writes them.  The same pipeline: look-ahead
    bounded at 2 * in_flight * B frames, passes of B frames of one geometry, output in stream order.  Prints what ``annotate_images``
    prints, the label in the path's place.  ``options``: the options of ``AnnotateOptions``, as ``annotate_images`` takes them."""
    source = stream_frames(reader) if isinstance(reader, y4m.Y4mReader) else iter(reader)
    o = AnnotateOptions.checked(training_manager, **options)
    if isinstance(writer_or_out_dir, y4m.Y4mWriter):
        make_sink = lambda: _y4m_sink(writer_or_out_dir, video_chroma, o.out_size)
    else:
        make_sink = lambda: _file_sink(writer_or_out_dir, None, png_encoder, png_compress, frame_format, jpeg_encoder, jpeg_quality, jpeg_subsampling,
                                      jpeg_huffman)
    _annotate(training_manager, detector, source, lambda prepare, ahead: _loaded_stream(source, prepare, ahead), make_sink, resize_min, resize_max, o)


def annotate_images(training_manager, detector, input_dir, out_dir, image_filenames, resize_min, resize_max, png_encoder=None,
                    png_compress=None, frame_format=None, jpeg_encoder=None, jpeg_quality=None, jpeg_decoder=None, jpeg_subsampling=None,
                    jpeg_huffman=None, png_decoder=None, **options):
    """annotate_video.py:15-24, pipelined (see the module docstring); output and printed lines as the one-by-one loop.
    ``png_encoder``: "host" (PIL on the writer threads) or "device" (encoded inside the pass); None = ``default_png_encoder()``.
    ``png_compress``: the device encoder's mode, "runs" or "huffman"; None = ``default_png_compress()``.
    ``frame_format``: "png" or "jpg" (each output keeps its stem and gets the extension .jpg); None = ``default_frame_format()``.
    ``jpeg_encoder``: "host" or "device", as ``png_encoder``; ``jpeg_quality``: 1..100, None = JPEG_QUALITY.
    ``jpeg_subsampling``: 444 or 420, ``jpeg_huffman``: "standard" or "optimized" -- of JPEG frames, whichever encoder writes them;
    None = ``default_jpeg_subsampling()`` / ``default_jpeg_huffman()``.
    ``jpeg_decoder``: "host", "device" or "device_full" (csrc/jpeg_dec_full.hip: progressive files too): who decodes ``.jpg`` INPUT
    frames the device decoder supports (captured path only); None =
    what ``entry.jpeg_decoder()`` says (FRCNN_ENTRY_JPEG_DECODER, default "host").
    ``png_decoder``: "host", "device" or "device_full" (csrc/png_dec_full.hip: palette, 1/2/4/16-bit, grey + alpha and Adam7 files too):
    who decodes ``.png`` INPUT frames the device decoder supports (captured path only; the decode
    threads then only read the file and check its chunks); None = what ``entry.png_decoder()`` says (FRCNN_ENTRY_PNG_DECODER, default "host").
    ``options``: what is done to the frames -- redaction, tracking, counting and the rest --, as keywords: the fields of
    ``AnnotateOptions``, whose docstring describes each.  ValueError, in front of any capture, for what they refuse."""
    if jpeg_decoder is not None:
        entry.set_jpeg_decoder(jpeg_decoder)
    if png_decoder is not None:
        entry.set_png_decoder(png_decoder)
    device_decode, device_png = entry.jpeg_decoder(), entry.png_decoder()      # "host", "device" or "device_full" each
    paths = [os.path.join(input_dir, f) for f in image_filenames]
    make_sink = lambda: _file_sink(out_dir, image_filenames, png_encoder, png_compress, frame_format, jpeg_encoder, jpeg_quality, jpeg_subsampling,
                                  jpeg_huffman)
    _annotate(training_manager, detector, ((path, _Frame(_read_rgb(path))) for path in paths),
              lambda prepare, ahead: _loaded_files(paths, lambda path: prepare(path, _load_frame(path, device_decode, device_png)), ahead),
              make_sink, resize_min, resize_max, AnnotateOptions.checked(training_manager, **options))


def build_parser():
    """The reference's command line (annotate_video.py:48-64) plus voc_dets' --network / --anchor_scales: a weights file does not
    carry the architecture."""
    import argparse
    p = argparse.ArgumentParser(description="Draw the detector's boxes and labels on a directory of PNG frames")
    p.add_argument("step3_model_path", metavar="step3_model_path", type=str,
                   help="weights of the RPN trained in step 3 (Keras .h5 or this package's .npz)")
    p.add_argument("step4_model_path", metavar="step4_model_path", type=str,
                   help="weights of the detector from step 4 (must be compatible with the RPN)")
    p.add_argument("input_dir", type=str, help="directory of the video's frames as *.png; or a YUV4MPEG2 stream: a .y4m path, or - for stdin")
    p.add_argument("--kitti", dest="kitti", action="store_true", help="KITTI classes instead of Pascal VOC")
    p.add_argument("--resize_dims", dest="resize_dims", default="600,1000",
                   help="resize parameters, e.g. 600,1000 for a min size of 600 pixels and a max of 1000")
    p.add_argument("--out_dir", dest="out_dir", default=".", help="where the annotated frames are written")
    p.add_argument("--network", dest="network", choices=("vgg16", "resnet50", "resnet101"), default="resnet50")
    p.add_argument("--anchor_scales", dest="anchor_scales", default="128,256,512")
    p.add_argument("--dtype", dest="dtype", choices=("f32", "bf16"), default="f32",
                   help="precision the networks are served in: bf16 = the bf16 conv path on the matrix cores (the reference has no such flag: it runs fp32 only)")
    p.add_argument("--png_encoder", dest="png_encoder", choices=PNG_ENCODERS, default=default_png_encoder(),
                   help="who encodes the annotated frames: host = PIL on writer threads, device = inside the detection pass on the GPU "
                        "(FRCNN_ANNOTATE_PNG_ENCODER sets the default)")
    p.add_argument("--png_compress", dest="png_compress", choices=PNG_COMPRESS, default=default_png_compress(),
                   help="the device encoder's mode: runs = Sub filter, fixed Huffman codes; huffman = adaptive row filters and a dynamic "
                        "Huffman code per band, smaller files (FRCNN_ANNOTATE_PNG_COMPRESS sets the default; needs --png_encoder device)")
    p.add_argument("--frame_format", dest="frame_format", choices=FRAME_FORMATS, default=default_frame_format(),
                   help="how the annotated frames are written: png (lossless), or jpg = <stem>.jpg, baseline JPEG without chroma "
                        "subsampling (FRCNN_ANNOTATE_FRAME_FORMAT sets the default)")
    p.add_argument("--jpeg_encoder", dest="jpeg_encoder", choices=JPEG_ENCODERS, default=default_jpeg_encoder(),
                   help="who encodes JPEG frames: host = PIL on writer threads, device = inside the detection pass on the GPU "
                        "(FRCNN_ANNOTATE_JPEG_ENCODER sets the default; needs --frame_format jpg)")
    p.add_argument("--jpeg_decoder", dest="jpeg_decoder", choices=JPEG_DECODERS, default=None,
                   help="who decodes .jpg INPUT frames: host (PIL), device (csrc/jpeg_dec.hip; input_dir's *.jpg / *.jpeg are then "
                        "taken beside its *.png) or device_full (progressive files too: csrc/jpeg_dec_full.hip); default: "
                        "FRCNN_ENTRY_JPEG_DECODER, else host")
    p.add_argument("--png_decoder", dest="png_decoder", choices=PNG_DECODERS, default=None,
                   help="who decodes .png INPUT frames: host (PIL), device (csrc/png_dec.hip: 8-bit grey / RGB / RGBA without interlace) or "
                        "device_full (csrc/png_dec_full.hip: palette, 1/2/4/16-bit, grey + alpha and Adam7 files too); PIL for the files the "
                        "chosen planner refuses; "
                        "default: FRCNN_ENTRY_PNG_DECODER, else host")
    p.add_argument("--jpeg_quality", dest="jpeg_quality", type=int, default=None,
                   help="IJG quality of JPEG frames, 1..100 (default %d; needs --frame_format jpg)" % JPEG_QUALITY)
    p.add_argument("--jpeg_subsampling", dest="jpeg_subsampling", type=int, choices=JPEG_SUBSAMPLINGS, default=default_jpeg_subsampling(),
                   help="chroma of JPEG frames: 444 = full resolution, 420 = halved both ways, with either encoder "
                        "(FRCNN_ANNOTATE_JPEG_SUBSAMPLING sets the default; needs --frame_format jpg)")
    p.add_argument("--jpeg_huffman", dest="jpeg_huffman", choices=JPEG_HUFFMANS, default=default_jpeg_huffman(),
                   help="Huffman tables of JPEG frames: standard = Annex K.3, optimized = built from each frame's symbol counts, smaller "
                        "files, with either encoder (FRCNN_ANNOTATE_JPEG_HUFFMAN sets the default; needs --frame_format jpg)")
    p.add_argument("--out_video", dest="out_video", default=None, metavar="PATH|-",
                   help="write ONE YUV4MPEG2 stream (PATH, or - for stdout: every printed line then goes to stderr) instead of frame files; "
                        "range and the F / A tags are the input stream's (a frame directory: limited range, F25:1, and one frame size)")
    p.add_argument("--video_chroma", dest="video_chroma", choices=VIDEO_CHROMAS, default=None,
                   help="chroma of the stream --out_video writes: 420jpeg (the default) or 444")
    p.add_argument("--out_size", dest="out_size", default=None, metavar="WxH",
                   help="scale every annotated frame DOWN to W x H on the device, behind every edit and in front of the encoder (an exact "
                        "area mean; labels shrink with the picture); at most the frame's size and at least 1/16 of it along each side; "
                        "boxes printed and written to --tracks_out / --counts_out / --zones_out stay in source coordinates")
    p.add_argument("--out_scale", dest="out_scale", type=int, default=None, metavar="N",
                   help="as --out_size with both sides divided by N (2..16) and rounded up, per frame size; not together with --out_size")
    p.add_argument("--redact", dest="redact", default=None, metavar="CLASSES",
                   help="hide the detected objects of these classes: comma-separated names of the active class mapping, or all; a box that "
                        "crosses the frame's border is hidden too")
    p.add_argument("--redact_mode", dest="redact_mode", choices=REDACT_MODES, default=None,
                   help="how they are hidden: pixelate (the default) = the means of an N x N pixel grid, blur = a box blur of radius N, "
                        "fill = black (needs --redact)")
    p.add_argument("--redact_size", dest="redact_size", type=int, default=None, metavar="N",
                   help="pixelate: the cell's side, 2..64 (default 16); blur: the radius, 1..32 (default 12); none with fill (needs --redact)")
    p.add_argument("--redact_margin", dest="redact_margin", type=int, default=None, metavar="N",
                   help="pixels added around every redacted box (default 0; needs --redact)")
    p.add_argument("--redact_shape", dest="redact_shape", choices=ops.REDACT_SHAPES, default=None,
                   help="what of every redacted box is hidden: box (default) = all of it; ellipse = the ellipse inscribed in the box "
                        "grown by --redact_margin, not clipped to the frame (needs --redact)")
    p.add_argument("--redact_feather", dest="redact_feather", type=int, default=None, metavar="N",
                   help="the redaction fades into the scene over N pixels OUTSIDE the shape, 0..32 (default 0: a hard edge; needs --redact)")
    p.add_argument("--redact_region", dest="redact_region", action="append", default=None, metavar="X1,Y1,X2,Y2,X3,Y3[,...]",
                   help="hide a static area in EVERY frame, whatever is detected: a polygon of 3..16 vertices in source-frame pixels, each "
                        "coordinate -32768..65535, even-odd interior; repeatable up to 8 times; a value that begins with a minus sign needs "
                        "the = form (--redact_region=-5,0,9,0,9,9)")
    p.add_argument("--redact_mask", dest="redact_mask", default=None, metavar="PATH.png",
                   help="a painted mask of the frames' size, any file PIL opens, read as 8-bit grey: every pixel >= 128 is hidden in every "
                        "frame; with or without --redact_region")
    p.add_argument("--region_mode", dest="region_mode", choices=REDACT_MODES, default=None,
                   help="what replaces a static area (default: fill; needs --redact_region or --redact_mask)")
    p.add_argument("--region_size", dest="region_size", type=int, default=None, metavar="N",
                   help="pixelate: the cell's side, 2..64 (default 16); blur: the radius, 1..32 (default 12); none with fill (needs "
                        "--redact_region or --redact_mask)")
    p.add_argument("--region_feather", dest="region_feather", type=int, default=None, metavar="N",
                   help="a static area fades into the scene over N pixels OUTSIDE it, 0..32 (default 0; needs --redact_region or "
                        "--redact_mask)")
    p.add_argument("--redact_moving", dest="redact_moving", action="store_true",
                   help="fixed-camera footage: hide whatever differs from the learned background plate, whether the detector saw it or "
                        "not; the first --remove_settle frames are not protected (the background is not known yet)")
    p.add_argument("--moving_tol", dest="moving_tol", type=int, default=None, metavar="D",
                   help="how far a channel may lie from the plate, 0..255 (default 24, provisional: not measured on real footage; needs "
                        "--redact_moving)")
    p.add_argument("--moving_min", dest="moving_min", type=int, default=None, metavar="K",
                   help="the differing pixels that make an 8 x 8 cell vote, 1..64 (default 8, provisional; needs --redact_moving)")
    p.add_argument("--moving_hold", dest="moving_hold", type=int, default=None, metavar="H",
                   help="the frames a cell stays hidden behind its last vote, 0..255 (default 4, provisional; needs --redact_moving)")
    p.add_argument("--moving_grow", dest="moving_grow", type=int, default=None, metavar="G",
                   help="the pixels the hidden cells grow by, 0..32 (default 8, provisional; needs --redact_moving)")
    p.add_argument("--moving_feather", dest="moving_feather", type=int, default=None, metavar="F",
                   help="the hidden set fades into the scene over F pixels OUTSIDE it, 0..32 (default 0; needs --redact_moving)")
    p.add_argument("--moving_unknown", dest="moving_unknown", choices=("show", "hide"), default=None,
                   help="a pixel whose background is not known yet: show it (default) or hide it, which blanks the start of a sequence "
                        "(needs --redact_moving)")
    p.add_argument("--moving_except", dest="moving_except", default=None, metavar="CLASSES",
                   help="comma-separated class names, or all: the boxes of these classes are never hidden by the net (needs "
                        "--redact_moving)")
    p.add_argument("--moving_mode", dest="moving_mode", choices=REDACT_MODES, default=None,
                   help="what replaces what the net hides (default: pixelate; needs --redact_moving)")
    p.add_argument("--moving_size", dest="moving_size", type=int, default=None, metavar="N",
                   help="pixelate: the cell's side, 2..64 (default 16); blur: the radius, 1..32 (default 12); none with fill (needs "
                        "--redact_moving)")
    p.add_argument("--moving_out", dest="moving_out", default=None, metavar="PATH",
                   help="write a CSV frame,cells,covered: the moving cells and the hidden pixels of every frame (needs --redact_moving)")
    p.add_argument("--no_draw", dest="no_draw", action="store_true", help="draw no boxes and no labels (with --redact: only hide)")
    p.add_argument("--track", dest="track", action="store_true",
                   help="join the detections of consecutive frames into tracks: labels read cls#id, and a track the detector loses is held "
                        "(and, with --redact, stays hidden) for --track_hold frames")
    p.add_argument("--track_iou", dest="track_iou", type=int, default=None, metavar="PCT",
                   help="a detection continues a track of its class when their boxes overlap by at least PCT percent IoU, 1..100 "
                        "(default 30; needs --track)")
    p.add_argument("--track_hold", dest="track_hold", type=int, default=None, metavar="N",
                   help="frames a lost track is held, 0..255 (default 8; 0: ids only; needs --track)")
    p.add_argument("--track_grow", dest="track_grow", type=int, default=None, metavar="N",
                   help="pixels a held box grows by on every side per frame held, 0..64 (default 0; needs --track)")
    p.add_argument("--track_motion", dest="track_motion", type=int, nargs="?", const=ops.TRACK_MOTION_RADIUS[2], default=None, metavar="R",
                   help="move every track's box with the pixels under it from frame to frame (a block match of at most R pixels either "
                        "way, 1..16, default 8), so a held box follows its object (needs --track)")
    p.add_argument("--track_lookback", dest="track_lookback", type=int, nargs="?", const=TRACK_LOOKBACK_AUTO, default=None, metavar="N",
                   help="hide every new track in the N frames BEFORE its first detection too (1..16 and at most the frames of one pass; "
                        "bare: as many as a pass holds, at most 8); the output runs one pass behind the input (needs --track)")
    p.add_argument("--det_threshold", dest="det_threshold", type=float, default=None, metavar="T",
                   help="report detections with a score of T or more only, 0..1 (default 0.0: every detection, as the reference script)")
    p.add_argument("--track_low", dest="track_low", type=float, default=None, metavar="L",
                   help="with --track and --det_threshold T: a detection with a score in [L, T) may continue a track that no stronger "
                        "detection continued, and is dropped otherwise; it never starts a track (needs L < T; no default: none has been "
                        "measured on real footage)")
    p.add_argument("--detect_every", dest="detect_every", type=int, default=None, metavar="K",
                   help="run the detector on every K-th frame only, 2..16; on the frames between, every track's box follows the pixels "
                        "under it by block matching and is drawn, redacted and written to --tracks_out with the prob of its last match. "
                        "Nothing is matched, aged or born there: --track_hold counts DETECTED frames and a held box does not grow in "
                        "between (needs --track --track_motion; not with --track_lookback)")
    p.add_argument("--track_backtrack", dest="track_backtrack", type=int, nargs="?", const=TRACK_BACKTRACK_AUTO, default=None, metavar="N",
                   help="with --detect_every K: at every detected frame follow every track BACK through the frames in front of it and hide "
                        "it there too -- a continued track as far as the detected frame before, a new one over N frames (1..16, at least "
                        "K - 1 and at most the B * K frames of one pass; bare: as many as a pass holds, at most 16) -- so a frame between two "
                        "detections is covered from both sides; the output runs one pass behind the input (needs --track --track_motion "
                        "--detect_every; not with --track_lookback)")
    p.add_argument("--track_scene_cut", dest="track_scene_cut", type=int, nargs="?", const=ops.TRACK_CUT_PCT[2], default=None, metavar="PCT",
                   help="end every track at a hard cut: a frame whose 4x4-region luma histogram differs from the frame before by PCT percent "
                        "of the largest distance there is (1..100; bare: 40, a provisional default that no real footage has been measured "
                        "for) starts a new scene -- no id is carried into it and no held box of the old scene is redacted in it; a line "
                        "'scene cut: <path>' is printed in front of that frame's lines; fades and dissolves are not detected (needs --track "
                        "--track_motion; with or without --detect_every; not with --track_lookback or --track_backtrack)")
    p.add_argument("--track_reid", dest="track_reid", type=int, nargs="?", const=ops.TRACK_REID_PCT[2], default=None, metavar="PCT",
                   help="give an object that returns after more than --track_hold frames its old id back: a new track whose colour signature "
                        "lies within PCT percent of the largest distance there is (1..100; bare: 25, a provisional default that no real "
                        "footage has been measured for) of that of an id the tracker gave up carries that id in labels, files, trails, "
                        "counts and zones; a line 're-identified: <path> id <id>' is printed in front of that frame's lines and "
                        "'re-identified: N' at the end (needs --track; not with --track_lookback or --track_backtrack)")
    p.add_argument("--reid_keep", dest="reid_keep", type=int, default=None, metavar="N",
                   help="the frames an id that is gone is remembered, 1..4095 (default 250, provisional; needs --track_reid)")
    p.add_argument("--reid_out", dest="reid_out", default=None, metavar="PATH",
                   help="write a CSV row frame,id,tracker_id,cls,distance,gap per re-identification (needs --track_reid)")
    p.add_argument("--track_trails", dest="track_trails", type=int, nargs="?", const=ops.TRACK_TRAILS[0][2], default=None, metavar="N",
                   help="draw the path of every track: the last N centres of its box (2..64; bare: 16) as a line in the colour of its id, "
                        "over the redaction and under the boxes; a trail ends where its id ends (needs --track; with every tracking option; "
                        "not with --no_draw)")
    p.add_argument("--trail_width", dest="trail_width", type=int, default=None, metavar="W",
                   help="the width of the trails in pixels, 1..9 (default 3; needs --track_trails)")
    p.add_argument("--heatmap", dest="heatmap", default=None, metavar="CLASSES",
                   help="blend an occupancy heat map into every frame: where the boxes of these classes (comma-separated names of the active "
                        "mapping, or all) have been since the first frame, black through red and yellow to white at the hottest pixel, over the "
                        "redaction and under the trails, boxes and labels; with --track the live tracked boxes count, held ones do not")
    p.add_argument("--heatmap_alpha", dest="heatmap_alpha", type=int, default=None, metavar="A",
                   help="the weight of the hottest pixel's colour, 1..255 (default 160; needs --heatmap)")
    p.add_argument("--heatmap_decay", dest="heatmap_decay", type=int, default=None, metavar="S",
                   help="every frame takes ceil(v / 2^S) off every pixel of the map, 1..15; 0 (the default): the map never cools (needs --heatmap)")
    p.add_argument("--heatmap_out", dest="heatmap_out", default=None, metavar="PATH.png",
                   help="write the map at the end of the list as an 8-bit grey PNG, one per frame size met (needs --heatmap)")
    p.add_argument("--remove", dest="remove", default=None, metavar="CLASSES",
                   help="paint the objects of these classes (comma-separated names of the active mapping, or all) out of every frame with a "
                        "background plate learned from the frames themselves, for fixed-camera footage: a pixel that no box of any class "
                        "touches and that holds still for S frames becomes background; until the background under a box is known the "
                        "redaction shows there (with --redact of the same classes), else black.  An object that stands still and is never "
                        "detected becomes background")
    p.add_argument("--remove_settle", dest="remove_settle", type=int, default=None, metavar="S",
                   help="the frames a pixel must hold still to become background, 1..255 (default 8, provisional: not measured on real "
                        "footage; needs --remove or --redact_moving)")
    p.add_argument("--remove_tol", dest="remove_tol", type=int, default=None, metavar="T",
                   help="how far a channel may lie from the value its run began with, 0..255 (default 10, provisional; needs --remove or --redact_moving)")
    p.add_argument("--remove_margin", dest="remove_margin", type=int, default=None, metavar="M",
                   help="the pixels every box grows by, 0..64 (default 8, provisional; needs --remove or --redact_moving)")
    p.add_argument("--plate_out", dest="plate_out", default=None, metavar="PATH.png",
                   help="write the plate at the end of the list as an RGB PNG with unknown pixels black, one per frame size met (needs --remove)")
    p.add_argument("--count_line", dest="count_line", action="append", default=None, metavar="X1,Y1,X2,Y2",
                   help="count the tracks whose box centre crosses the line from (X1,Y1) to (X2,Y2), in source-frame pixels (-32768..65535), "
                        "once per id and direction; a value that begins with a minus sign is written --count_line=-5,0,-5,100; repeatable up to 8 "
                        "times; each line is drawn with its totals 'L{l} +{pos} -{neg}' over "
                        "the redaction, heat map and trails and under the boxes, and the totals are printed at the end (needs --track)")
    p.add_argument("--zone", dest="zone", action="append", default=None, metavar="X1,Y1,X2,Y2,X3,Y3[,...]",
                   help="a polygon zone of 3..16 vertices in source-frame pixels (-32768..65535): who is inside (the centre of the box, or "
                        "with --zone_anchor bottom the middle of its bottom edge), how many ids have visited and how long they stayed; a value "
                        "that begins with a minus sign is written --zone=-5,0,9,0,9,9; repeatable up to 8 times (needs --track)")
    p.add_argument("--zone_classes", dest="zone_classes", default=None, metavar="CLASSES",
                   help="the classes the zones see: comma-separated names of the active mapping, or all (the default; needs --zone)")
    p.add_argument("--zone_width", dest="zone_width", type=int, default=None, metavar="W",
                   help="the width the zones' outlines are drawn with in pixels, 1..9 (default 3; needs --zone)")
    p.add_argument("--zone_anchor", dest="zone_anchor", choices=("centre", "bottom"), default=None,
                   help="the point of a box that is tested: its centre (the default) or the middle of its bottom edge (needs --zone)")
    p.add_argument("--zones_out", dest="zones_out", default=None, metavar="PATH",
                   help="write a CSV row frame,zone,kind,id,cls,dwell per zone event, kind enter, exit or lost (needs --zone)")
    p.add_argument("--count_classes", dest="count_classes", default=None, metavar="CLASSES",
                   help="the classes that count: comma-separated names of the active mapping, or all (the default; needs --count_line)")
    p.add_argument("--count_width", dest="count_width", type=int, default=None, metavar="W",
                   help="the width the counting lines are drawn with in pixels, 1..9 (default 3; needs --count_line)")
    p.add_argument("--counts_out", dest="counts_out", default=None, metavar="PATH",
                   help="write every crossing as a CSV row frame,line,direction,id,cls: frames from 1, direction + or -, the class by name "
                        "(needs --count_line)")
    p.add_argument("--tracks_out", dest="tracks_out", default=None, metavar="PATH",
                   help="write the tracks as MOTChallenge lines frame,id,left,top,width,height,prob,cls,-1,-1 (needs --track)")
    from .args_util import add_post_arguments
    add_post_arguments(p)                                 # --nms, --nms_thresh, --nms_sigma, --nms_min_score, --box_vote
    return p


VIDEO_CHROMAS = ("420jpeg", "444")


def is_stream_input(input_dir):
    """Does the command line's ``input_dir`` name a YUV4MPEG2 stream (``-``: stdin, or a ``.y4m`` path) rather than a frame directory?"""
    return input_dir == "-" or input_dir.lower().endswith(".y4m")


def video_options(args):
    """The video arguments checked (before any model is loaded) -> (stream input?, out_video or None, video_chroma).  ValueError for
    --video_chroma without --out_video and for --out_video with options that choose how frame FILES are encoded."""
    out_video = args.out_video
    if args.video_chroma is not None and out_video is None:
        raise ValueError("--video_chroma=%s is a setting of the stream --out_video writes: it needs --out_video" % args.video_chroma)
    if out_video is not None:
        if args.frame_format != "png" or args.png_encoder != "host" or args.png_compress != "runs" or args.jpeg_encoder != "host" \
                or args.jpeg_quality is not None or args.jpeg_subsampling != 444 or args.jpeg_huffman != "standard":
            raise ValueError("--out_video writes one YUV4MPEG2 stream: --frame_format / --png_* / --jpeg_* encoder options choose how frame "
                             "FILES are written and do not go with it")
    return is_stream_input(args.input_dir), out_video, args.video_chroma or "420jpeg"


def out_size_from_args(args):
    """(host only) The output scale the command line asks for -> ("size", W, H) for --out_size WxH, ("scale", N) for --out_scale N, as
    ``submit_batch(out_size=...)`` takes it, or None.  ValueError for both flags together, a size that is not WxH, a side of 0 and a
    divisor outside 2..16."""
    if args.out_size is not None and args.out_scale is not None:
        raise ValueError("--out_size=%s and --out_scale=%s both state the output size: give one" % (args.out_size, args.out_scale))
    if args.out_scale is not None:
        return ops.scale_form(("scale", args.out_scale))
    if args.out_size is None:
        return None
    m = re.fullmatch(r"\s*(\d+)\s*[xX]\s*(\d+)\s*", args.out_size)
    if not m:
        raise ValueError("--out_size=%s: WxH, two positive integers" % args.out_size)
    return ops.scale_form(("size", int(m.group(1)), int(m.group(2))))


def scaled_size(out_size, label, width, height):
    """(host only) The (width, height) frame ``label`` of (width, height) has behind the scale step; ValueError that names the frame
    when the rule refuses the target for it."""
    try:
        H, W = ops.scale_option(out_size, (height, width))
    except ValueError as e:
        raise ValueError("%s (%dx%d): %s" % (label, width, height, e)) from None
    return W, H


def _frame_size(path):
    from PIL import Image as PilImage
    with PilImage.open(path) as im:
        return im.size                                    # (width, height)


def main(argv=None):
    """annotate_video.py:47-82: load the two models, annotate every PNG of input_dir into out_dir."""
    import contextlib
    import sys
    args = build_parser().parse_args(argv)
    stream_in, out_video, video_chroma = video_options(args)
    with contextlib.ExitStack() as stack:
        if out_video == "-":                              # the stream owns stdout: everything printed goes to stderr
            video_out = sys.stdout.buffer
            stack.enter_context(contextlib.redirect_stdout(sys.stderr))
        else:
            video_out = None
        _main(args, stream_in, out_video, video_chroma, video_out, stack)


def _main(args, stream_in, out_video, video_chroma, video_out, stack):
    import sys
    from . import resnet, vgg
    from .args_util import anchor_scales_from_str, resize_dims_from_str
    from .data.voc_data_helpers import KITTI_CLASS_MAPPING, VOC_CLASS_MAPPING
    from .det_util import DetTrainingManager
    from .util import get_anchors
    frame_format = jpeg_options(args.frame_format, args.jpeg_encoder, args.jpeg_quality,
                                *png_options(args.png_encoder, args.png_compress))[0]                     # (before any model is loaded)
    jpeg_size_options(frame_format, args.jpeg_subsampling, args.jpeg_huffman)
    os.environ.setdefault("GPU_MAX_HW_QUEUES", voc_dets.ENTRY_HW_QUEUES)      # (as voc_dets.main: passes in flight want > 4 queues)
    class_mapping = KITTI_CLASS_MAPPING if args.kitti else VOC_CLASS_MAPPING
    options = AnnotateOptions.from_args(args, class_mapping, stack)                                         # (before any model is loaded)
    anchors = get_anchors(anchor_scales_from_str(args.anchor_scales))
    if args.network == "vgg16":
        rpn = vgg.rpn_from_h5(args.step3_model_path, anchors_per_loc=len(anchors), dtype=args.dtype)
        detector = vgg.det_from_h5(args.step4_model_path, num_classes=len(class_mapping), dtype=args.dtype)
        preprocess = vgg.preprocess
    else:
        depth = 50 if args.network == "resnet50" else 101
        rpn = resnet.rpn_from_h5(args.step3_model_path, anchors_per_loc=len(anchors), depth=depth, dtype=args.dtype)
        detector = resnet.det_from_h5(args.step4_model_path, num_classes=len(class_mapping), depth=depth, dtype=args.dtype)
        preprocess = resnet.preprocess
    manager = DetTrainingManager(rpn_model=rpn, class_mapping=class_mapping, preprocess_func=preprocess, anchor_dims=anchors)
    resize_min, resize_max = resize_dims_from_str(args.resize_dims)
    if stream_in or out_video is not None:
        if stream_in:
            fin = sys.stdin.buffer if args.input_dir == "-" else stack.enter_context(open(args.input_dir, "rb"))
            reader = y4m.Y4mReader(fin, name="<stdin>" if args.input_dir == "-" else args.input_dir)
            w, h, yrange, tags = int(reader.plan.w), int(reader.plan.h), reader.plan.range_name, reader.plan.tags
        else:
            names = frame_filenames(args.input_dir, args.jpeg_decoder or entry.jpeg_decoder())
            if not names:
                raise ValueError("%s holds no frames" % args.input_dir)
            reader = directory_frames(args.input_dir, names, args.jpeg_decoder, args.png_decoder)
            (w, h), yrange, tags = _frame_size(os.path.join(args.input_dir, names[0])), "limited", {"F": "25:1"}
        if out_video is not None:
            fout = video_out if video_out is not None else stack.enter_context(open(out_video, "wb"))
            if options.out_size is not None:              # the header carries the scaled size
                w, h = scaled_size(options.out_size, "<stdin>" if args.input_dir == "-" else args.input_dir, w, h)
            sink = y4m.Y4mWriter(fout, w, h, video_chroma, yrange, {k: tags[k] for k in ("F", "A") if k in tags})
            annotate_stream(manager, detector, reader, sink, resize_min, resize_max, **vars(options))
        else:
            annotate_stream(manager, detector, reader, args.out_dir, resize_min, resize_max, png_encoder=args.png_encoder,
                            png_compress=args.png_compress, frame_format=args.frame_format, jpeg_encoder=args.jpeg_encoder,
                            jpeg_quality=args.jpeg_quality, jpeg_subsampling=args.jpeg_subsampling, jpeg_huffman=args.jpeg_huffman,
                            **vars(options))
        return
    annotate_images(training_manager=manager, detector=detector, input_dir=args.input_dir, out_dir=args.out_dir,
                    image_filenames=frame_filenames(args.input_dir, args.jpeg_decoder or entry.jpeg_decoder()), resize_min=resize_min,
                    resize_max=resize_max, jpeg_decoder=args.jpeg_decoder, png_decoder=args.png_decoder,
                    png_encoder=args.png_encoder, png_compress=args.png_compress, frame_format=args.frame_format,
                    jpeg_encoder=args.jpeg_encoder, jpeg_quality=args.jpeg_quality, jpeg_subsampling=args.jpeg_subsampling,
                    jpeg_huffman=args.jpeg_huffman, **vars(options))


if __name__ == "__main__":
    main()
