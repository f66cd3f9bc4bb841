"""The reference's INFERENCE ENTRY POINTS on the captured device pipeline.

``voc_dets.get_dets`` / ``get_dets_by_cls`` (voc_dets.py:20-111) reach the device through
``DetTrainingManager.get_det_inputs`` (det_util.py:136-158) and ``detector.predict`` (voc_dets.py:49), crossing to
numpy twice per image (det_util.py:41, 49-55).  When the manager's ``rpn_model`` and the ``detector`` are this package's
models, the same call runs here as ONE captured pass per image:

    image.data (uint8 BGR)  ->  one H2D copy [pixels | resize_ratio, det_threshold]
                            ->  hipGraph: resnet.preprocess on the device, backbone, RPN heads, decode, top-8000,
                                NMS to 300, the reference's padded RoI list, RoI crop-resize, detector head, post-process
                            ->  one packed D2H copy [n_dets, n_rois | boxes | classes | scores]

* A captured pass is specific to an image SIZE (VOC has dozens after ``util.resize_imgs``): ``GraphCache`` keeps them per
  (height, width), least-recently-used first out under a byte budget; a size is captured at its first sighting.
  ``resize_ratio`` and ``det_threshold`` are per-image VALUES, read from device memory by the post-process
  (frcnn_detections_dyn), so they are not part of the key.
* ``get_dets_by_cls`` keeps several images in flight (one HIP stream each; a size seen several times in a row gets as
  many captured instances as are in flight) and hands results back in submission order, so the returned dict is the
  reference's, entry for entry.
* The frame is uploaded as DECODED (``image.raw``: the file's own size, 0.56 MB for a 500x375 VOC frame) and resized on the
  device inside the captured pass (frcnn_resize_cubic_u8: OpenCV's 8-bit INTER_CUBIC in integers, bit-identical to the host
  restatement in shapes._resize, which takes ~90 ms per frame in numpy); such a pass is keyed by (height, width, source
  height, source width, flip).  ``get_dets_by_cls`` decodes the JPEGs of the next images on a small thread pool meanwhile.
* A foreign ``preprocess_func`` (anything but resnet.preprocess / vgg.preprocess) is called on the host, as the reference
  does (det_util.py:36), and its float image is uploaded instead of the bytes; a foreign ``detector`` (any other object
  with Keras' ``predict``) keeps voc_dets' eager path.
* Weights that change (load_weights, a training step, set_weights) bump ``models.weights_epoch()``; every captured pass
  holds pointers to packed filters, so the cache is dropped and re-captured on the next call.
"""
import collections
import ctypes
import dataclasses
import os
import time

import numpy as np
import torch

from . import _lib, models, ops
from ._lib import FrcnnError
from .frame_edit import EditChain, EditStates
from .pipeline import BatchedInferencePipeline, InferencePipeline, no_gc
from .shapes import declares as _declares

MEAN_BGR = (103.939, 116.779, 123.68)           # resnet.preprocess / vgg.preprocess (resnet.py:64-75, vgg.py:52-57)
# submit_batch(encode=...) of an annotating pass -> the device PNG encoder's compress mode (ops.png_encode_u8)
PNG_ENCODES = {"png": "runs", "png-huffman": "huffman"}
# submit_batch(encode="jpeg", quality=q): the device JPEG encoder (ops.jpeg_encode_u8) at the end of an annotating pass
JPEG_ENCODE = "jpeg"
JPEG_MODE = (444, "standard")          # ... its default (subsampling, huffman): frcnn_jpeg_encode_u8; any other pair: frcnn_jpeg_opt_encode_u8
# submit_batch(encode="y4m", y4m=(chroma, range)): the drawn frames as YUV4MPEG2 records (ops.y4m_encode_frames_u8), all B in one launch
Y4M_ENCODE = "y4m"
Y4M_MODE = ("420jpeg", "limited")
PRE_NMS_TOP_N, MAX_PROPOSALS = 8000, 300        # det_util.py:151-156
TRACK_CAPACITY = 64                             # slots of an engine's tracker state (submit_batch(track=...))


def _default_budget():
    env = os.environ.get("FRCNN_GRAPH_CACHE_BYTES")
    if env:
        return int(float(env))
    total = torch.cuda.get_device_properties(torch.cuda.current_device()).total_memory
    return total // 4                           # 72 GB of an MI355X's 288: ~150 captured 600x1000 fp32 passes


def default_in_flight(dtype="f32"):
    """Captured passes in flight for get_dets_by_cls: four (FRCNN_ENTRY_IN_FLIGHT overrides).  What matters more is that the PROCESS has
    more hardware queues than ROCm's default four (GPU_MAX_HW_QUEUES, read when the runtime starts; voc_dets.main sets 8): on four, the
    passes' staging copies, replays and read-backs queue behind one another -- 497 img/s through get_dets_by_cls against 542-547 on 8 or
    16 queues, where 4 / 5 / 6 / 8 / 12 passes in flight measure 545 / 526 / 542 / 535 / 497 (fp32, four images per pass, 256 frames;
    scripts/dev/r6_entry_child_sweep.sh).  (Until round 6 this returned up to 12 on 12 queues: right for one-image passes.)"""
    env = int(os.environ.get("FRCNN_ENTRY_IN_FLIGHT", "0"))
    return env if env > 0 else 4


def default_batch(dtype="f32"):
    """Images per captured pass where neighbouring images share a geometry (FRCNN_ENTRY_BATCH / FRCNN_ENTRY_BATCH_F32)."""
    if dtype == "bf16":
        return max(1, int(os.environ.get("FRCNN_ENTRY_BATCH", "8")))
    return max(1, int(os.environ.get("FRCNN_ENTRY_BATCH_F32", "4")))


# The reference pads the last batch of 64 RoIs with copies of its first RoI and scores the copies too (voc_dets.py:42-51).  A copy
# has the box, class and score of its original, so the per-class NMS that follows (threshold 0.5) keeps exactly one of them where it
# would have kept the original: the returned list is the same with or without the copies.  The captured passes therefore score the
# kept proposals only (300 rows instead of 320: 6 % less detector-head work); FRCNN_ENTRY_PAD=1 scores the padded list as the eager
# path does.  tests/test_entry_gpu.py compares the two paths detection by detection.
PAD_TO_BATCH = os.environ.get("FRCNN_ENTRY_PAD", "0") != "0"
# eager passes in front of a capture: ONE sizes the split-K workspace, lowers what is lowered lazily and leaves the magnitude-record
# arena's high-water mark (round 6: two until then; a capture is ~2/3 warm-up, and a list of mixed sizes captures per geometry)
WARMUP_PASSES = max(1, int(os.environ.get("FRCNN_ENTRY_WARMUP", "1")))
# Padded canvases (round 6): a list of MANY image sizes is served by passes captured per canvas CLASS with the images' true sizes as
# device values (pipeline: ``extents``), instead of one capture per geometry.  A canvas has EVEN sides, multiples of CANVAS_GRANULE; an
# image sits at offset (H & 1, W & 1) (csrc/boxes.hip: the offset stands for the extra zero row / column SAME padding puts in front of
# an odd side; a VGG16 frame sits at (0, 0): no VGG16 layer's padding depends on the size -- the base's ``extents_class`` says which).
# voc_dets.get_dets_by_cls switches canvases on for a call whose list holds more than CANVAS_MIN_GEOMETRIES sizes and
# PLANS the classes from the list's size histogram (DetectionEntry.plan_canvases): few classes, each worth its captures.
# file-backed frames go up in the decoder's channel order and are swapped to BGR by the device resize (0: reverse on the host as before)
RGB_UPLOAD = os.environ.get("FRCNN_ENTRY_RGB_UPLOAD", "1") != "0"
# who decodes a file-backed frame: "host" (PIL, the default) or "device" (ops.jpeg_decode_batch_u8 in front of the replay, for the files
# its planner supports, in per-geometry and canvas passes alike; PIL for the rest) or "device_full" (as "device", and
# ops.jpeg_decode_full_batch_u8 beside it for the progressive files ITS planner supports).  FRCNN_ENTRY_JPEG_DECODER, or
# ``set_jpeg_decoder`` (voc_dets / annotate_video --jpeg_decoder), which wins.
_JPEG_DECODER = None


def set_jpeg_decoder(value):
    """"host" / "device" / "device_full" for every DetectionEntry of the process from now on; None: back to FRCNN_ENTRY_JPEG_DECODER."""
    global _JPEG_DECODER
    from .feed import jpeg_decoder_option
    _JPEG_DECODER = None if value is None else jpeg_decoder_option(value, "jpeg_decoder")


def jpeg_batch():
    """FRCNN_ENTRY_JPEG_BATCH (read at every call: a test or a benchmark may set it): "1", the default, decodes all files of a pass in
    one ops.jpeg_decode_batch_u8; "0" keeps one ops.jpeg_decode_u8 (and one upload) per file, so that the two can be measured."""
    value = os.environ.get("FRCNN_ENTRY_JPEG_BATCH") or "1"
    if value not in ("0", "1"):
        raise ValueError("FRCNN_ENTRY_JPEG_BATCH=%r: 0 or 1" % value)
    return value == "1"


def jpeg_decoder():
    from .feed import jpeg_decoder_option
    return _JPEG_DECODER or jpeg_decoder_option(os.environ.get("FRCNN_ENTRY_JPEG_DECODER"), "FRCNN_ENTRY_JPEG_DECODER")


class JpegFile:
    """What ``host_pixels`` hands ``submit_batch`` in place of the decoded array when the device decodes: the file and its plan."""
    __slots__ = ("data", "plan", "name")

    def __init__(self, data, plan, name):
        self.data, self.plan, self.name = data, plan, name


# who decodes a file-backed .png frame: "host" (PIL, the default), "device" (ops.png_decode_batch_u8 in front of the replay, beside the
# JPEG decoder's call when a pass mixes both; PIL for the files its planner refuses) or "device_full" (ops.png_decode_full_batch_u8 in its
# place: palette, 1/2/4/16-bit, grey + alpha and Adam7 files too; PIL for what ITS planner refuses).  FRCNN_ENTRY_PNG_DECODER, or
# ``set_png_decoder`` (annotate_video --png_decoder), which wins.
_PNG_DECODER = None


def set_png_decoder(value):
    """"host" / "device" / "device_full" for every DetectionEntry of the process from now on; None: back to FRCNN_ENTRY_PNG_DECODER."""
    global _PNG_DECODER
    from .feed import png_decoder_option
    _PNG_DECODER = None if value is None else png_decoder_option(value, "png_decoder")


def png_decoder():
    from .feed import png_decoder_option
    return _PNG_DECODER or png_decoder_option(os.environ.get("FRCNN_ENTRY_PNG_DECODER"), "FRCNN_ENTRY_PNG_DECODER")


class PngFile(JpegFile):
    """A .png frame the device decodes: ``data`` is its zlib stream (the IDAT payloads back to back), ``plan`` a ``_lib.PngDecPlan``;
    under "device_full" ``plan`` is a ``_lib.PngDecFullPlan`` and a palette file's 768 staged palette bytes follow the stream in ``data``.
    A JpegFile to everything that only asks for the frame's size (plan.h, plan.w) and stages ``data``."""
    __slots__ = ()


class Y4mFile(JpegFile):
    """A frame of a YUV4MPEG2 stream (annotate_video.annotate_stream): ``data`` is the frame's planes, ``plan`` a ``_lib.Y4mPlan``.  The
    device converts it to R,G,B in its source segment beside the other kinds' decodes (ops.Y4M_DECODER: one launch, no workspace, no
    status)."""
    __slots__ = ()


# host_pixels: the item kind by the label of the decoder whose planner made the plan
_FILE_KINDS = {"JPEG": JpegFile, "PNG": PngFile, "Y4M": Y4mFile}
CANVAS_GRANULE = int(os.environ.get("FRCNN_ENTRY_CANVAS_GRANULE", "32"))
CANVAS_MIN_GEOMETRIES = int(os.environ.get("FRCNN_ENTRY_CANVAS_MIN", "4"))
# captured passes kept per canvas class: with several classes interleaving in a list, two of one class in flight at once is the common
# worst case; a third would be a capture (~20-35 ms) to save a wait of a few ms -- get_dets_by_cls waits instead (should_wait)
CANVAS_SLOTS_PER_CLASS = int(os.environ.get("FRCNN_ENTRY_CANVAS_SLOTS", "2"))


# the plan's cost model, in image-times: a captured pass costs about this many images' worth of host time per class (15-25 ms per
# capture, a class has a few passes in flight); padded pixels cost the trunk's and the RPN's share of an image's time (the head's
# 300 RoIs do not grow with the canvas)
CANVAS_CAPTURE_IMAGES = float(os.environ.get("FRCNN_ENTRY_CANVAS_CAPTURE_IMAGES", "12"))
CANVAS_PIXEL_SHARE = float(os.environ.get("FRCNN_ENTRY_CANVAS_PIXEL_SHARE", "0.4"))
CANVAS_MAX_CLASSES = int(os.environ.get("FRCNN_ENTRY_CANVAS_MAX_CLASSES", "8"))
CANVAS_EXTRA_SLOT = int(os.environ.get("FRCNN_ENTRY_WINDOW_EXTRA", "0"))      # (voc_dets.WINDOW_EXTRA: passes submitted beyond the streams)
# passes a class may hold = factor x passes in flight x its share of the list, at least CANVAS_SLOT_MIN once it fills more than one pass.
# bench.py's mixed list (three classes, 52 / 31 / 17 %), first call / again, img/s: factor 1.5 (4 + 2 + 2 = 8 captures) 446 / 558; 1.0
# (3 + 2 + 2 = 7) 468-478 / 557-559; 1.0 with a minimum of one (3 + 2 + 1 = 6) 427-457 / 552-553; 0.75 (4 captures) 465-480 / 533
CANVAS_SLOT_FACTOR = float(os.environ.get("FRCNN_ENTRY_CANVAS_SLOT_FACTOR", "1.0"))
CANVAS_SLOT_MIN = int(os.environ.get("FRCNN_ENTRY_CANVAS_SLOT_MIN", "2"))
CANVAS_BYTES_PER_PIXEL = 600                             # a captured fp32 pass's memory per canvas pixel, before one of its class has been measured
# (600 is the f32 ResNet figure and the first guess for VGG16 too; for VGG16 it is UNMEASURED.  By reckoning: a captured pass's pool
# re-uses what the pass has freed, so its per-pixel part is about block 1's two full-resolution 64-channel maps, 2 x 256 B in f32 and
# 2 x 128 B in bf16 -- but a part that does not scale with pixels (head, proposals, staging) sits on top and dominates small canvases,
# so the guess may fall on either side.  Either side is safe: the guess only trims slot ALLOWANCES before the first capture of a
# class; GraphCache evicts by the MEASURED nbytes of the passes it holds, and the next plan_canvases reads that figure instead.)


def canvas_side(n, granule=None):
    """The smallest canvas side for a true side ``n``: even, a multiple of the granule, with room for the offset of an odd side."""
    g = CANVAS_GRANULE if granule is None else granule
    assert g > 0 and g % 2 == 0, "canvas granule: a positive even number"
    n = int(n)
    return -(-(n + (n & 1)) // g) * g


def plan_canvas_classes(counts, existing=(), capture_images=None, pixel_share=None, max_new=None, granule=None):
    """{(H, W): canvas (Hc, Wc)} for a histogram ``counts`` = {(H, W): number of images}: start with every geometry on its own smallest
    canvas (or on an ``existing`` class -- a pass already captured -- when the padding costs less than a capture), then merge the pair
    of classes whose union canvas lowers  sum over NEW classes of capture_images + sum over images of pixel_share * (canvas area /
    image area - 1)  the most, until no merge lowers it and at most ``max_new`` new classes are left.  Deterministic: the same
    histogram and the same existing classes give the same plan (a second call over the same list captures nothing)."""
    cap = CANVAS_CAPTURE_IMAGES if capture_images is None else capture_images
    share = CANVAS_PIXEL_SHARE if pixel_share is None else pixel_share
    max_new = CANVAS_MAX_CLASSES if max_new is None else max_new
    ex = set(tuple(e) for e in existing)
    area = lambda c: c[0] * c[1]

    def padding(geos, c):
        return sum(n * share * (area(c) / float(h * w) - 1.0) for (h, w), n in geos)

    def cost(c, geos):
        return (0.0 if c in ex else cap) + padding(geos, c)
    classes = {}
    for (h, w), n in sorted(counts.items()):
        own = (canvas_side(h, granule), canvas_side(w, granule))
        best, best_cost = own, cost(own, [((h, w), n)])
        for e in sorted(ex):
            if e[0] >= own[0] and e[1] >= own[1]:
                c = padding([((h, w), n)], e)
                if c < best_cost:
                    best, best_cost = e, c
        classes.setdefault(best, []).append(((h, w), n))
    while len(classes) > 1:
        keys, best = sorted(classes), None
        for i, a in enumerate(keys):
            for b in keys[i + 1:]:
                u = (max(a[0], b[0]), max(a[1], b[1]))
                if a in ex and b in ex and u not in (a, b):
                    continue                                  # (two captured classes: nothing to save by leaving both)
                third = classes[u] if (u in classes and u not in (a, b)) else []
                delta = cost(u, classes[a] + classes[b] + third) - cost(a, classes[a]) - cost(b, classes[b]) - (cost(u, third) if third else 0.0)
                if best is None or delta < best[0]:
                    best = (delta, a, b, u)
        if best is None or (best[0] >= 0.0 and sum(1 for k in keys if k not in ex) <= max_new):
            break
        _, a, b, u = best
        merged = classes.pop(a) + classes.pop(b) + classes.pop(u, [])
        classes[u] = merged
    return {g: c for c, geos in classes.items() for g, _ in geos}


class _PinnedArena:
    """Pinned host memory for the captured passes' staging, handed out in 4 KB-aligned pieces from a few large blocks: a capture
    took two hipHostMalloc calls (frame staging, detection read-back), several milliseconds each, and a list of mixed image sizes
    captures per geometry.  Pieces are not returned one by one: a block goes back when every slot cut from it has been closed."""
    BLOCK = 64 << 20

    def __init__(self):
        self.blocks = []                                 # [tensor, used bytes, live pieces]

    def take(self, nbytes, zero=False):
        nbytes = max(int(nbytes), 16)
        need = (nbytes + 4095) // 4096 * 4096
        for blk in self.blocks:
            if blk[0].numel() - blk[1] >= need:
                break
        else:
            blk = [torch.empty(max(self.BLOCK, need), dtype=torch.uint8).pin_memory(), 0, 0]
            self.blocks.append(blk)
        piece = blk[0][blk[1]:blk[1] + nbytes]
        blk[1] += need
        blk[2] += 1
        if zero:
            piece.zero_()
        piece._arena_block = blk
        return piece

    @staticmethod
    def give_back(piece):
        blk = getattr(piece, "_arena_block", None)
        if blk is None:
            return
        blk[2] -= 1
        if blk[2] == 0:
            blk[1] = 0                                   # every piece of the block is gone: the block starts over


_CAPTURE_STREAM = None


def _capture_stream():
    global _CAPTURE_STREAM
    if _CAPTURE_STREAM is None:
        _CAPTURE_STREAM = torch.cuda.Stream()
    return _CAPTURE_STREAM


@dataclasses.dataclass(frozen=True)
class PassSpec:
    """The options of one captured pass, checked and normalised: what ``submit_batch``'s keywords say (``checked``), what the cache key
    says of them (``key_tail``) and what ``_capture_slot`` builds the pass from.  The default is the plain detection pass, and every
    canvas pass.  A new option is a field here, its check in ``checked`` and its tag in ``key_tail``."""
    annotate: bool = False
    encode: object = None
    quality: object = None
    jpeg_mode: tuple = JPEG_MODE
    y4m_mode: tuple = Y4M_MODE
    redact: object = None
    redact_shape: object = None                          # (shape, feather), ops.redact_shape_option's form; None: ("box", 0), the plain redaction
    draw: bool = True
    track: object = None
    track_motion: object = None
    track_lookback: object = None
    detect_every: object = None
    track_backtrack: object = None
    track_scene_cut: object = None
    track_trails: object = None
    heat: object = None
    count: object = None
    zone: object = None                                  # (zones, classes, W, anchor), ops.zone_option's form: frame_edit.EditChain reads it
    remove: object = None                                # (classes, S, T, M), ops.plate_option's form
    track_reid: object = None                            # (pct, keep), ops.track_reid_option's form
    out_size: object = None                              # ("size", W, H) or ("scale", N), ops.scale_form's form: the scale step's target
    track_strong: object = None                          # T, a float: the Weak rule's ``strong`` (the uploaded det_threshold is then the LOW one)
    redact_region: object = None                         # (regions, mask, mode, size, feather), ops.redact_region_option's form
    redact_moving: object = None                         # (D, K, H, G, F, unknown, EXCEPT, mode, size, S, T, M), ops.redact_moving_option's form

    @classmethod
    def checked(cls, engine, batch, annotate=False, encode=None, quality=None, subsampling=None, huffman=None, y4m=None, redact=None, draw=True,
                track=None, track_motion=None, track_lookback=None, detect_every=None, track_backtrack=None, track_scene_cut=None,
                track_trails=None, heat=None, count=None, zone=None, remove=None, track_reid=None, out_size=None, redact_shape=None,
                track_strong=None, redact_region=None, redact_moving=None):
        """``submit_batch``'s keywords (its docstring says what each means) for a pass of ``batch`` images (None: ``engine.batch``) on
        ``engine`` -> the spec.  FrcnnError with the reason.  ``track_lookback`` / ``track_backtrack`` are still as given: ``sized`` checks
        them, behind ``submit_batch``'s flush, which reads neither."""
        if (redact is not None or not draw) and not annotate:
            raise FrcnnError("submit_batch: redact= and draw=False change the frame an ANNOTATING pass returns: pass annotate=True")
        if track is not None:
            if not annotate:
                raise FrcnnError("submit_batch: track= tracks the detections of an ANNOTATING pass: pass annotate=True")
            track = engine.track_option(track)
        if track_motion is not None:
            if track is None:
                raise FrcnnError("submit_batch: track_motion= moves the boxes of the tracker: pass track=(thr, hold, grow) too")
            track_motion = engine.track_motion_option(track_motion)
        if track_lookback is not None and track is None:
            raise FrcnnError("submit_batch: track_lookback= hides the tracker's new tracks in earlier frames: pass track=(thr, hold, grow) too")
        if track_backtrack is not None:
            if track_lookback is not None:
                raise FrcnnError("submit_batch: track_backtrack= together with track_lookback= is not supported: the back-track rule hides a new "
                                 "track in the earlier frames itself, and a pass has one window")
            if detect_every is None:
                raise FrcnnError("submit_batch: track_backtrack= follows the tracks of a detected frame back over the frames between two "
                                 "detections: pass detect_every=K (with track= and track_motion=) too")
        if detect_every is not None:
            if track_motion is None:
                raise FrcnnError("submit_batch: detect_every= follows the tracks by block matching between two detected frames: pass "
                                 "track=(thr, hold, grow) and track_motion=R too")
            if track_lookback is not None:
                raise FrcnnError("submit_batch: detect_every= together with track_lookback= is not supported: the look-back window keeps one "
                                 "tracked buffer per detected frame")
            if not engine.device_preprocess:
                raise FrcnnError("submit_batch: detect_every= needs the device-side preprocess: a foreign preprocess_func uploads float "
                                 "pixels of the key frames only, and the block match reads the uint8 pixels of every source frame")
            detect_every = engine.detect_every_option(detect_every, engine.batch if batch is None else batch)
        if track_scene_cut is not None:
            if track_motion is None:
                raise FrcnnError("submit_batch: track_scene_cut= compares every frame with the frame the block match keeps: pass "
                                 "track=(thr, hold, grow) and track_motion=R too")
            for name, value in (("track_lookback", track_lookback), ("track_backtrack", track_backtrack)):
                if value is not None:
                    raise FrcnnError("submit_batch: track_scene_cut= together with %s= is not supported: a backward chain would have to "
                                     "stop at a cut" % name)
            if not engine.device_preprocess:
                raise FrcnnError("submit_batch: track_scene_cut= needs the device-side preprocess: a foreign preprocess_func uploads float "
                                 "pixels, and the cut rule reads the uint8 pixels of every source frame")
            track_scene_cut = engine.track_scene_cut_option(track_scene_cut)
        if track_trails is not None:
            if track is None:
                raise FrcnnError("submit_batch: track_trails= draws the paths of the tracker's ids: pass track=(thr, hold, grow) too")
            if not draw:
                raise FrcnnError("submit_batch: track_trails= together with draw=False is not supported: a pass that draws nothing draws "
                                 "no trails")
            track_trails = engine.track_trails_option(track_trails)
        if heat is not None:
            if not annotate:
                raise FrcnnError("submit_batch: heat= blends the heat map into the frame an ANNOTATING pass returns: pass annotate=True")
            if not engine.device_preprocess:
                raise FrcnnError("submit_batch: heat= needs the device-side preprocess: a foreign preprocess_func uploads float pixels, and "
                                 "the heat map is blended into the uint8 source frame")
            heat = engine.heat_option(heat)
        if count is not None:
            if track is None:
                raise FrcnnError("submit_batch: count= counts the tracker's ids as they cross a line: pass track=(thr, hold, grow) too")
            count = engine.count_option(count)
        if zone is not None:
            if track is None:
                raise FrcnnError("submit_batch: zone= tests the tracker's ids against the zones: pass track=(thr, hold, grow) too")
            zone = engine.zone_option(zone)
        if remove is not None:
            if not annotate:
                raise FrcnnError("submit_batch: remove= paints the objects out of the frame an ANNOTATING pass returns: pass annotate=True")
            if not engine.device_preprocess:
                raise FrcnnError("submit_batch: remove= needs the device-side preprocess: a foreign preprocess_func uploads float pixels, "
                                 "and the plate is learned from the uint8 source frame")
            remove = engine.remove_option(remove)
        if track_reid is not None:
            if track is None:
                raise FrcnnError("submit_batch: track_reid= gives the tracker's ids back: pass track=(thr, hold, grow) too")
            for name, value in (("track_lookback", track_lookback), ("track_backtrack", track_backtrack)):
                if value is not None:
                    raise FrcnnError("submit_batch: track_reid= together with %s= is not supported: the window of a delayed pass holds "
                                     "the tracked buffers of earlier passes, whose ids are the tracker's" % name)
            if not engine.device_preprocess:
                raise FrcnnError("submit_batch: track_reid= needs the device-side preprocess: a foreign preprocess_func uploads float "
                                 "pixels, and the signatures are read from the uint8 source frame")
            track_reid = engine.track_reid_option(track_reid)
        if track_strong is not None:
            if track is None:
                raise FrcnnError("submit_batch: track_strong= tells the tracker which rows are strong: pass track=(thr, hold, grow) too")
            try:
                track_strong = ops.track_weak_option(track_strong, None)[0]
            except ValueError as e:
                raise FrcnnError("submit_batch: track_strong: %s" % e) from None
        if redact is not None:
            redact = engine.redact_option(redact)
        if redact_shape is not None:
            if redact is None:
                raise FrcnnError("submit_batch: redact_shape= shapes the redaction: pass redact=(classes, mode, size, margin) too")
            redact_shape = engine.redact_shape_option(redact_shape)
        if redact_region is not None:
            if not annotate:
                raise FrcnnError("submit_batch: redact_region= hides static areas in the frame an ANNOTATING pass returns: pass annotate=True")
            redact_region = engine.redact_region_option(redact_region)
        if redact_moving is not None:
            if not annotate:
                raise FrcnnError("submit_batch: redact_moving= hides what differs from the plate in the frame an ANNOTATING pass returns: "
                                 "pass annotate=True")
            if not engine.device_preprocess:
                raise FrcnnError("submit_batch: redact_moving= needs the device-side preprocess: a foreign preprocess_func uploads float "
                                 "pixels, and the plate is learned from the uint8 source frame")
            redact_moving = engine.redact_moving_option(redact_moving, remove)
        if out_size is not None:
            if not annotate:
                raise FrcnnError("submit_batch: out_size= scales the frame an ANNOTATING pass returns: pass annotate=True")
            try:
                out_size = ops.scale_form(out_size)
            except ValueError as e:
                raise FrcnnError("submit_batch: %s" % e) from None
        jpeg_mode, y4m_mode = JPEG_MODE, Y4M_MODE
        if encode == Y4M_ENCODE:
            y4m_mode = Y4M_MODE if y4m is None else tuple(y4m)
            if len(y4m_mode) != 2 or y4m_mode[0] not in _lib.Y4M_OUT_CHROMAS or y4m_mode[1] not in _lib.Y4M_RANGES:
                raise FrcnnError("submit_batch: y4m=%r: (chroma, range) with chroma one of %s and range one of %s"
                                 % (y4m, ", ".join(_lib.Y4M_OUT_CHROMAS), ", ".join(_lib.Y4M_RANGES)))
            if quality is not None or subsampling is not None or huffman is not None:
                raise FrcnnError("submit_batch: quality / subsampling / huffman go with encode=\"%s\" only" % JPEG_ENCODE)
        elif y4m is not None:
            raise FrcnnError("submit_batch: y4m=%r goes with encode=\"%s\" only" % (y4m, Y4M_ENCODE))
        if encode == Y4M_ENCODE:
            pass
        elif encode == JPEG_ENCODE:
            if not annotate:
                raise FrcnnError("submit_batch: encode=\"%s\" encodes the ANNOTATED frame: pass annotate=True" % encode)
            if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
                raise FrcnnError("submit_batch: encode=\"%s\" takes quality= an integer in 1..100, got %r" % (encode, quality))
            quality = int(quality)
            jpeg_mode = (JPEG_MODE[0] if subsampling is None else subsampling, JPEG_MODE[1] if huffman is None else huffman)
            if isinstance(jpeg_mode[0], bool) or jpeg_mode[0] not in _lib.JPEG_OPT_SUBSAMPLINGS or not isinstance(jpeg_mode[1], str) \
                    or jpeg_mode[1] not in _lib.JPEG_OPT_HUFFMANS:
                raise FrcnnError("submit_batch: subsampling=%r (444, 420), huffman=%r (\"standard\", \"optimized\")" % (subsampling, huffman))
        elif subsampling is not None or huffman is not None:
            raise FrcnnError("submit_batch: subsampling=%r / huffman=%r go with encode=\"%s\" only" % (subsampling, huffman, JPEG_ENCODE))
        elif quality is not None:
            raise FrcnnError("submit_batch: quality=%r goes with encode=\"%s\" only" % (quality, JPEG_ENCODE))
        elif encode is not None and encode not in PNG_ENCODES:
            raise FrcnnError("submit_batch: encode=%r (None, %s)" % (encode, ", ".join('"%s"' % e for e in PNG_ENCODES)))
        if encode and not annotate:
            raise FrcnnError("submit_batch: encode=\"%s\" encodes the ANNOTATED frame: pass annotate=True" % encode)
        return cls(annotate=annotate, encode=encode, quality=quality, jpeg_mode=jpeg_mode, y4m_mode=y4m_mode, redact=redact, draw=draw, track=track,
                   track_motion=track_motion, track_lookback=track_lookback, detect_every=detect_every, track_backtrack=track_backtrack,
                   track_scene_cut=track_scene_cut, track_trails=track_trails, heat=heat, count=count, zone=zone, remove=remove,
                   track_reid=track_reid, out_size=out_size, redact_shape=redact_shape, track_strong=track_strong,
                   redact_region=redact_region, redact_moving=redact_moving)

    def region_fits(self, hw):
        """FrcnnError, by name, when the mask of ``redact_region`` is not the size ``hw`` = (h, w) of the pass's source frames."""
        mask = self.redact_region[1] if self.redact_region is not None else None
        if mask is not None and mask.shape != (int(hw[0]), int(hw[1])):
            raise FrcnnError("submit_batch: redact_region: the mask is %dx%d, the pass's source frames are %dx%d"
                             % (mask.shape[1], mask.shape[0], hw[1], hw[0]))

    def out_hw(self, hw):
        """The size (H, W) of the frames a pass over source frames of ``hw`` = (h, w) encodes and returns: the scale step's target, or
        ``hw`` itself without ``out_size``.  FrcnnError, with the reason, for a target the scale rule refuses for this frame size and for
        one the pass's encoder refuses."""
        if self.out_size is None:
            return int(hw[0]), int(hw[1])
        try:
            H, W = ops.scale_option(self.out_size, hw)
        except ValueError as e:
            raise FrcnnError("submit_batch: %s" % e) from None
        try:                                             # (the encoder's own word on the size it would be handed)
            if self.encode == JPEG_ENCODE:
                ops.jpeg_bound(H, W, *self.jpeg_mode)
            elif self.encode == Y4M_ENCODE:
                ops.y4m_frame_bytes(H, W, self.y4m_mode[0])
            elif self.encode:
                ops.png_bound(H, W, PNG_ENCODES[self.encode])
        except FrcnnError as e:
            raise FrcnnError("submit_batch: out_size %dx%d with encode=\"%s\": %s" % (W, H, self.encode, e)) from None
        return H, W

    @property
    def delayed(self):
        """Does the pass return the frames of the pass before it (a look-back or back-track pass)?"""
        return self.track_lookback is not None or self.track_backtrack is not None

    def sized(self, engine, B):
        """The look-back of a delayed pass checked against the B images of the pass -> the spec with it normalised."""
        if self.track_lookback is not None:
            return dataclasses.replace(self, track_lookback=engine.track_lookback_option(self.track_lookback, B))
        if self.track_backtrack is not None:
            K = self.detect_every
            return dataclasses.replace(self, track_backtrack=engine.track_backtrack_option(self.track_backtrack, K, B * K))
        return self

    def key_tail(self, B):
        """What an ANNOTATING pass of B images appends to its geometry in the cache key: (444, "standard") is the pass without the pair,
        and every option that is not stated leaves the key what it was."""
        key = ((B,) if B > 1 else ()) + (("annotate", self.encode) if self.encode else ("annotate",)) + ((self.quality,) if self.quality else ())
        if self.encode == JPEG_ENCODE and self.jpeg_mode != JPEG_MODE:
            key = key + self.jpeg_mode
        if self.encode == Y4M_ENCODE:
            key = key + self.y4m_mode
        if self.redact is not None:
            key = key + ("redact",) + self.redact
        if self.redact_shape is not None:                # (never ("box", 0): that is the pass without it)
            key = key + ("shape",) + self.redact_shape
        if not self.draw:
            key = key + ("nodraw",)
        if self.track is not None:
            key = key + ("track",) + self.track
        for tag, value in (("motion", self.track_motion), ("lookback", self.track_lookback), ("every", self.detect_every),
                           ("backtrack", self.track_backtrack), ("cut", self.track_scene_cut)):
            if value is not None:
                key = key + (tag, value)
        if self.track_trails is not None:
            key = key + ("trails",) + self.track_trails
        if self.heat is not None:
            key = key + ("heat",) + self.heat
        if self.count is not None:
            key = key + ("count",) + self.count
        if self.zone is not None:
            key = key + ("zone",) + self.zone
        if self.remove is not None:
            key = key + ("remove",) + self.remove
        if self.track_reid is not None:
            key = key + ("track_reid",) + self.track_reid
        if self.out_size is not None:
            key = key + ("scale",) + self.out_size
        if self.track_strong is not None:
            key = key + ("weak", self.track_strong)
        if self.redact_region is not None:
            key = key + ("region",) + ops.redact_region_key(self.redact_region)
        if self.redact_moving is not None:
            key = key + ("moving",) + self.redact_moving
        return key


class _Slot:
    """One captured pass for one image size (or canvas class), with its staging on both sides of PCIe.  Every field exists on every slot;
    what a kind of pass does not use stays None (``tabs`` / ``frame_io``: exact passes; ``chain``: annotating passes, the
    ``EditChain`` that holds their tracked buffers and lists; ``extents`` / ``_ext_raw``: canvas passes; ``png_*``:
    annotating passes that encode on the device -- a PNG or, with ``quality``, a JPEG file; ``first_copy``: the bytes of a JPEG row that
    are read back with every replay)."""
    __slots__ = ("key", "pipe", "graph", "out", "io_dev", "io_pin", "dyn_host", "out_pin", "event", "busy", "nbytes", "x_f32", "ws", "tabs", "u8_resized",
                 "batch", "pix_hosts", "out_packed", "amax", "_out_raw", "ready", "extents", "seg", "canvas", "_ext_raw", "annotate", "frame_io",
                 "encode", "png_dev", "png_ws", "png_bound", "png_pin", "_png_raw", "quality", "first_copy", "jpeg_mode",
                 "jpg_pin", "jpg_dev", "jpg_ws", "jpg_status", "jpg_status_pin", "jpg_names", "jpg_area", "jpg_items", "jpg_used",
                 "jpg_count", "png_items", "png_dec", "full_items", "jpg_decs", "y4m_items", "y4m_mode", "redact", "nodraw", "chain",
                 "track", "track_pin", "_track_raw", "n_frames_host", "n_frames_dev", "track_motion",
                 "track_lookback", "lb_pin", "_lb_raw", "every", "frames", "track_backtrack", "spec",
                 "track_scene_cut", "cuts_pin", "_cuts_raw", "track_trails", "heat", "count", "count_pin", "_count_raw", "zone", "zone_pin", "_zone_raw",
                 "remove", "track_reid", "reid_pin", "_reid_raw", "out_size", "scale_dev", "pix_out", "moving", "moving_pin", "_moving_raw")

    def __init__(self):
        for name in self.__slots__:
            setattr(self, name, None)
        self.busy = self.canvas = self.annotate = False


def _close_slot(s):
    """Release a captured pass NOW, from the thread that owns it: the hipGraph is destroyed here (torch.cuda.CUDAGraph.reset) and the
    references to its tensors are dropped, so that nothing is left for a garbage-collector finalizer to do later from whatever thread
    happens to collect (a finalizer issuing HIP calls inside another capture crashed a launch).  Idle slots only."""
    assert not s.busy, "closing a captured pass with an image in flight"
    if s.ready is not None:
        s.ready.synchronize()                            # (never replayed: its warm-up pass may still be writing the slot's buffers)
    if s.graph is not None:
        s.event.synchronize()                            # its last replay (and the copies behind it) are done
        s.graph.reset()
    if s.pipe is not None and hasattr(s.pipe, "close"):
        s.pipe.close()
    for name in s.__slots__:
        _PinnedArena.give_back(getattr(s, name))         # (the fields cut from the pinned arena: only those carry a block)
    s.__init__()                                         # every field back to its default: the slot holds nothing


class GraphCache:
    """Captured passes by image size, least-recently-used first out under a byte budget.  ``acquire(key, make)`` hands out
    an idle slot of that size or captures a new one; busy slots (an image in flight) are never evicted."""

    def __init__(self, byte_budget):
        self.byte_budget = int(byte_budget)
        self._slots = collections.OrderedDict()          # key -> [slots]; order = recency
        self.nbytes = 0
        self.captures = self.evictions = self.hits = 0

    def __len__(self):
        return sum(len(v) for v in self._slots.values())

    def keys(self):
        return list(self._slots)

    def acquire(self, key, make):
        slots = self._slots.get(key)
        if slots is not None:
            self._slots.move_to_end(key)
            for s in slots:
                if not s.busy:
                    self.hits += 1
                    return s
        slot = make()
        self.captures += 1
        self._slots.setdefault(key, []).append(slot)
        self._slots.move_to_end(key)
        self.nbytes += slot.nbytes
        self._evict(keep=slot)
        return slot

    def _evict(self, keep):
        if self.nbytes <= self.byte_budget:
            return
        dropped = False
        for key in list(self._slots):                    # oldest size first
            slots = self._slots[key]
            for s in list(slots):
                if self.nbytes <= self.byte_budget:
                    break
                if s.busy or s is keep:
                    continue
                slots.remove(s)
                self.nbytes -= s.nbytes
                self.evictions += 1
                _close_slot(s)
                dropped = True
            if not slots:
                del self._slots[key]
            if self.nbytes <= self.byte_budget:
                break
        if dropped:
            s = slots = None                             # (the loop variables still hold the last slot examined: its pool must be free to go)
            torch.cuda.empty_cache()                     # a dropped graph's private pool goes back to the device

    def clear(self):
        assert not any(s.busy for v in self._slots.values() for s in v), "graph cache cleared with images in flight"
        for v in self._slots.values():
            for s in v:
                _close_slot(s)
        self._slots.clear()
        self.nbytes = 0
        torch.cuda.empty_cache()


class Ticket:
    __slots__ = ("slot", "image", "own", "emitted", "frames")

    def __init__(self, slot, image, own=None, emitted=None, frames=None):
        # ``own`` / ``emitted`` (look-back passes): the record of this submit's group and of the group whose frames this pass emits;
        # ``frames``: the source frames of the submit (more than its images in a ``detect_every`` pass)
        self.slot, self.image, self.own, self.emitted = slot, image, own, emitted
        self.frames = len(image) if frames is None else frames


class DetectionEntry:
    """voc_dets.get_dets for one (manager, detector) pair: ``submit(image, resize_ratio, det_threshold)`` enqueues an image,
    ``collect(ticket)`` returns ``(num_rois, dets)`` with ``dets`` the reference's list of
    ``{'bbox': int array [x1,y1,x2,y2], 'cls_name', 'prob'}`` in its order (voc_dets.py:73-86)."""

    def __init__(self, manager, detector, num_rois=64, stride=16, in_flight=1, byte_budget=None, f32_engine=None, post=None):
        self.manager, self.detector = manager, detector
        # the post-process option (ops.det_post_option: soft-NMS / box voting), fixed per engine: every pass it captures -- exact, canvas,
        # annotating -- runs it; None = the reference's rule, the kernels and bytes of an engine built before the option existed
        self.post = None if post is None else ops.det_post_option(post)
        # the matrix path of the fp32 convolutions inside the captured passes (ops.f32_engine): by default the large launches run
        # on the fp16 matrix cores by a two-way operand split with a scaled low part -- fp32-grade results (csrc/conv_h3.hip:
        # error against fp64 under the native kernel's), three matrix instructions per block of products; FRCNN_F32_ENGINE=bf16x6
        # selects the exact three-way bf16 split (six), FRCNN_F32_ENGINE=native keeps v_mfma_f32_32x32x2_f32 everywhere
        self.f32_engine = f32_engine or os.environ.get("FRCNN_F32_ENGINE", "f16x3")
        self.num_rois, self.stride, self.in_flight = int(num_rois), stride, max(1, int(in_flight))
        # images per captured pass.  The bf16 detector makes ONE head pass over the RoIs of eight images and runs its trunk at batch
        # eight (pipeline.BatchedInferencePipeline: what configs[3]'s headline times); get_dets_by_cls groups neighbouring images of
        # one size into such passes.  The f32 ResNet models take four per pass since round 5 (the TRUNK is what gains: its launches are
        # latency-bound at one image -- 0.59 -> 0.445 ms per image at four; the head is unchanged, as DESIGN 11 found in round 2).
        head = getattr(detector, "head", None)
        self.batch = 1
        if hasattr(head, "forward_batched") and getattr(head, "hoist", False):
            self.batch = default_batch(getattr(head, "dtype", "f32"))
        from . import resnet, vgg
        self.device_preprocess = manager.preprocess_func in (resnet.preprocess, vgg.preprocess)
        self.rev_class_mapping = dict((v, k) for k, v in manager.class_mapping.items())
        self.cache = GraphCache(_default_budget() if byte_budget is None else byte_budget)
        self._streams = [torch.cuda.Stream() for _ in range(self.in_flight)]
        self._seq = 0
        self._epoch = models.weights_epoch()
        self.capture_seconds = 0.0
        # canvas passes need the base's extent masks (nets.ResNetBase, nets.VggBase: ``extents_class`` names the table of true sizes it
        # reads and where an image sits in its canvas) and the device-side preprocess
        net = getattr(getattr(manager.rpn_model, "base", None), "net", None)
        self._extents_class = getattr(net, "extents_class", None)
        # (FRCNN_ENTRY_CANVAS=0 switches them off: every geometry then gets passes of its own, as in round 5; =1 switches them on for a base
        # whose canvases are opt-in -- VGG16, ``canvas_by_default`` False until its mixed-list rate is measured.)  Measured on bench.py's
        # mixed_sizes legs (256 frames, 36 geometries) for ResNet: see DESIGN 5 / 7.
        want = os.environ.get("FRCNN_ENTRY_CANVAS", "1" if getattr(net, "canvas_by_default", False) else "0") != "0"
        self.canvas_capable = self.device_preprocess and self._extents_class is not None and want
        self.canvas = False                              # set per call by voc_dets.get_dets_by_cls
        self._canvas_of = {}                             # (H, W) -> canvas class: the plan (plan_canvases) + sizes seen outside it
        self._canvas_slots = {}                          # canvas class -> captured passes it may hold (its share of the list x in_flight)
        self._taps_dev = {}
        self._pinned = _PinnedArena()                    # (per engine: the blocks go when the engine goes)
        self.capture_breakdown = {}
        # the engine's ONE set of editing states (their pointers are in the graphs): a tracker of TRACK_CAPACITY slots, fewer when the
        # post-process's rows leave less room under the drawing and redaction kernels' 512 rows; a trail outlives its track by a frame,
        # and behind a scene cut the old scene's trails wait for their expiry while every slot already has a new id: twice the slots
        cap = min(TRACK_CAPACITY, _lib.REDACT_MAX_ROWS - -(-MAX_PROPOSALS // self.num_rois) * self.num_rois)
        self.edit_states = EditStates(self.class_names(), cap, min(2 * cap, ops.TRACK_MAX))
        self._lookback_waiting = {}                      # (h, w, B) -> the record of the group its window holds ({"images", "n_rois"})
        self._lookback_last = None                       # (key, capture) of the last look-back submit: what a flush submit replays

    def class_names(self):
        """This engine's class names by class index ("" for an index no class has)."""
        rev = self.rev_class_mapping
        return [rev.get(i, "") for i in range(max(rev) + 1)]

    def annotate_tables(self, draw=True):
        """The drawing tables of ops.annotate_u8 for this engine's classes (``EditStates.annotate_tables``)."""
        return self.edit_states.annotate_tables(draw)

    def redact_table(self, classes):
        """The class table of ops.redact_u8 for ``classes`` ("all" or a tuple of names) of this engine's classes (uploaded once each)."""
        return self.edit_states.redact_table(classes)

    def redact_option(self, redact):
        """``submit_batch``'s ``redact`` checked and normalised -> (classes, mode, size, margin): classes "all" or a tuple of this
        engine's class names, size the mode's default for None.  FrcnnError, with the reason, for anything else."""
        try:
            classes, mode, size, margin = redact
        except (TypeError, ValueError):
            raise FrcnnError("submit_batch: redact=%r: (classes, mode, size, margin)" % (redact,)) from None
        try:
            classes = "all" if classes == "all" or tuple(classes) == ("all",) else ops.redact_class_list(self.class_names(), classes)
            size = ops.redact_size(mode, size)
        except ValueError as e:
            raise FrcnnError("submit_batch: %s" % e) from None
        if isinstance(margin, bool) or not isinstance(margin, (int, np.integer)) or margin < 0:
            raise FrcnnError("submit_batch: redact margin=%r: an integer >= 0" % (margin,))
        return classes, mode, size, int(margin)

    def redact_shape_option(self, redact_shape):
        """``submit_batch``'s ``redact_shape`` checked and normalised -> (shape, feather), or None for ("box", 0), which IS the plain
        redaction: one spec, one key.  FrcnnError, with the reason, for anything else."""
        try:
            shape, feather = redact_shape
        except (TypeError, ValueError):
            raise FrcnnError("submit_batch: redact_shape=%r: (shape, feather)" % (redact_shape,)) from None
        try:
            option = ops.redact_shape_option(shape, feather)
        except ValueError as e:
            raise FrcnnError("submit_batch: %s" % e) from None
        return None if option == ("box", 0) else option

    def redact_region_option(self, redact_region):
        """``submit_batch``'s ``redact_region`` checked and normalised -> (regions, mask, mode, size, feather)
        (ops.redact_region_option).  FrcnnError, with the reason, for anything else."""
        try:
            regions, mask, mode, size, feather = redact_region
        except (TypeError, ValueError):
            raise FrcnnError("submit_batch: redact_region=%r: (regions, mask, mode, size, feather)" % (redact_region,)) from None
        try:
            return ops.redact_region_option(regions, mask, mode, size, feather)
        except ValueError as e:
            raise FrcnnError("submit_batch: %s" % e) from None

    # ------------------------------------------------------------------ heat map
    def heat_state(self, h, w):
        """The engine's heat state for source frames of (h, w) (device int32, ops.heat_state), made on first use: one per size, shared by
        every pass submitted with ``heat=`` whatever its other options.  ``heat_reset()`` empties it; ``track_reset()`` does not."""
        return self.edit_states.heat_state(h, w)

    def heat_reset(self):
        """A cold map for every size: the states are zeroed on the ordered stream, behind the heat passes submitted so far."""
        with torch.cuda.stream(self.track_stream):
            self.edit_states.reset_heat()

    def heat_option(self, heat):
        """``submit_batch``'s ``heat`` checked and normalised -> (classes, A, S): classes "all" or a tuple of this engine's class names,
        None for A or S replaced by the defaults (160, 0).  FrcnnError, with the reason, for anything else."""
        try:
            classes, alpha, decay = () if isinstance(heat, str) else heat
        except (TypeError, ValueError):
            raise FrcnnError("submit_batch: heat=%r: (classes, alpha, decay)" % (heat,)) from None
        try:
            classes, alpha, decay = ops.heat_option(classes, alpha, decay)
            if classes != "all":
                classes = ops.redact_class_list(self.class_names(), classes)
        except ValueError as e:
            raise FrcnnError("submit_batch: heat=%r: %s" % (heat, e)) from None
        return classes, alpha, decay

    # ------------------------------------------------------------------ tracking
    @property
    def track_stream(self):
        """The ONE stream every pass submitted with ``track=`` replays on, in submit order: frame i + 1 needs frame i's state."""
        return self._streams[0]

    def track_state(self):
        """The engine's tracker state (device int32, ops.track_state), made on first use: ``edit_states.track_capacity`` slots."""
        if self.edit_states.track_capacity < 1:
            rows = -(-MAX_PROPOSALS // self.num_rois) * self.num_rois
            raise FrcnnError("track=: the post-process's %d rows leave no room for held rows (at most %d rows in all)" % (rows, _lib.REDACT_MAX_ROWS))
        return self.edit_states.tracker()

    def track_trails_state(self, length):
        """The engine's trail state for trails of ``length`` points (device int32, ops.track_trails_state), made on first use, of
        ``track_trails_capacity()`` trails.  ``track_reset()`` empties it."""
        return self.edit_states.trails_state(length)

    def track_trails_capacity(self):
        """The trails of the engine's trail state: twice the tracker's slots, at most ops.TRACK_MAX."""
        return self.edit_states.trail_capacity

    @staticmethod
    def track_trails_option(value):
        """``submit_batch``'s ``track_trails`` checked -> (N, W).  FrcnnError with the reason."""
        try:
            return ops.track_trails_option(value)
        except ValueError as e:
            raise FrcnnError("submit_batch: track_trails=%r: %s" % (value, e)) from None

    track_trails_expire = staticmethod(EditChain.trails_expire)

    # ------------------------------------------------------------------ line counts
    def count_state(self):
        """The engine's count state (device int32, ops.count_state), made on first use, of ``track_trails_capacity()`` entries: one,
        shared by every pass submitted with ``count=``.  ``count_reset()`` empties it, totals included; ``track_reset()`` drops its
        entries -- the ids end -- and leaves the totals.  ``ops.count_totals`` reads it."""
        return self.edit_states.count_state()

    def count_reset(self):
        """Zero totals and no entries: the state is zeroed on the ordered stream, behind the counting passes submitted so far."""
        with torch.cuda.stream(self.track_stream):
            self.edit_states.reset_counts()

    def count_option(self, count):
        """``submit_batch``'s ``count`` checked and normalised -> (lines, classes, W): lines a tuple of 1..8 (ax, ay, bx, by), classes
        "all" or a tuple of this engine's class names, W 1..9 (None: 3).  FrcnnError, with the reason, for anything else."""
        try:
            lines, classes, width = count
        except (TypeError, ValueError):
            raise FrcnnError("submit_batch: count=%r: (lines, classes, width)" % (count,)) from None
        try:
            lines, classes, width = ops.count_option(lines, classes, width)
            if classes != "all":
                classes = ops.redact_class_list(self.class_names(), classes)
        except ValueError as e:
            raise FrcnnError("submit_batch: count=%r: %s" % (count, e)) from None
        return lines, classes, width

    # ------------------------------------------------------------------ background plate
    def plate_state(self, h, w, rgb=None):
        """The engine's plate state for source frames of (h, w) (device int32, ops.plate_state; ``ops.plate_image`` reads it): one per
        size and channel order, shared by every pass submitted with ``remove=`` whatever its other options.  ``rgb`` None: the one
        there is of that size (made for B, G, R frames if there is none), else the one of that channel order.  ``plate_reset()`` empties
        it; ``track_reset()`` does not."""
        if rgb is None:
            made = [k[2] for k in self.edit_states.plate if k[:2] == (int(h), int(w))]
            if len(made) > 1:
                raise FrcnnError("plate_state: frames of %dx%d were met in both channel orders: say rgb=True or rgb=False" % (w, h))
            rgb = made[0] if made else False
        return self.edit_states.plate_state(h, w, rgb)

    def plate_reset(self):
        """An empty plate for every size: the states are zeroed on the ordered stream, behind the remove passes submitted so far."""
        with torch.cuda.stream(self.track_stream):
            self.edit_states.reset_plate()

    # ------------------------------------------------------------------ moving net
    def moving_state(self, h, w, rgb=None):
        """The engine's moving state for source frames of (h, w) (device uint8, ops.redact_moving_state; ``ops.redact_moving_left``
        reads it): one per size and channel order, beside the plate state of the same key, shared by every pass submitted with
        ``redact_moving=``.  ``rgb`` as ``plate_state``'s.  ``moving_reset()`` empties it; ``track_reset()`` does not."""
        if rgb is None:
            made = [k[2] for k in self.edit_states.moving if k[:2] == (int(h), int(w))]
            if len(made) > 1:
                raise FrcnnError("moving_state: frames of %dx%d were met in both channel orders: say rgb=True or rgb=False" % (w, h))
            rgb = made[0] if made else False
        return self.edit_states.moving_state(h, w, rgb)

    def moving_reset(self):
        """No cell held, for every size: the states are zeroed on the ordered stream, behind the passes submitted so far.  (The plate the
        net compares with is ``plate_reset()``'s.)"""
        with torch.cuda.stream(self.track_stream):
            self.edit_states.reset_moving()

    def redact_moving_option(self, redact_moving, remove=None):
        """``submit_batch``'s ``redact_moving`` checked and normalised -> ops.redact_moving_option's form: True or () for every default,
        else a dict of ops.redact_moving_option's keywords or its 12-tuple; the EXCEPT names must be this engine's; with ``remove``
        (normalised) the plate's (S, T, M) are the remove option's -- a pass has one plate update --, and a settle, plate_tol or margin
        stated here that differs is refused by name (ops.redact_moving_form).  FrcnnError, with the reason."""
        try:
            return ops.redact_moving_form(redact_moving, remove, self.class_names())
        except ValueError as e:
            text = str(e)
            raise FrcnnError("submit_batch: %s" % (text if text.startswith("redact_moving") else "redact_moving: " + text)) from None

    def remove_option(self, remove):
        """``submit_batch``'s ``remove`` checked and normalised -> (classes, S, T, M): classes "all" or a tuple of this engine's class
        names, None for S, T or M replaced by the (provisional) defaults (8, 10, 8).  FrcnnError, with the reason, for anything else."""
        try:
            classes, settle, tol, margin = () if isinstance(remove, str) else remove
        except (TypeError, ValueError):
            raise FrcnnError("submit_batch: remove=%r: (classes, settle, tol, margin)" % (remove,)) from None
        try:
            classes, settle, tol, margin = ops.plate_option(classes, settle, tol, margin)
            if classes != "all":
                classes = ops.plate_class_list(self.class_names(), classes)
        except ValueError as e:
            raise FrcnnError("submit_batch: remove=%r: %s" % (remove, e)) from None
        return classes, settle, tol, margin

    # ------------------------------------------------------------------ re-identification
    def reid_state(self):
        """The engine's re-identify state (device int32, ops.track_reid_state), made on first use, of twice the tracker's slots (256 at
        most): one, shared by every pass submitted with ``track_reid=``.  ``reid_reset()`` empties it, and so does ``track_reset()``
        (the tracker's ids start over).  ``ops.track_reid_totals`` reads it."""
        return self.edit_states.reid_state()

    def reid_reset(self):
        """Forget every look: the state is zeroed on the ordered stream, behind the passes submitted so far.  An object that returns
        from now on is a new id; the tracker's own ids go on."""
        with torch.cuda.stream(self.track_stream):
            self.edit_states.reset_reid()

    def track_reid_option(self, track_reid):
        """``submit_batch``'s ``track_reid`` checked and normalised -> (pct, keep): None for either replaced by the PROVISIONAL defaults
        25 and 250, which nobody has measured on real footage.  FrcnnError, with the reason, for anything else."""
        try:
            pct, keep = track_reid
        except (TypeError, ValueError):
            raise FrcnnError("submit_batch: track_reid=%r: (pct, keep)" % (track_reid,)) from None
        try:
            return ops.track_reid_option(pct, keep)
        except ValueError as e:
            raise FrcnnError("submit_batch: track_reid=%r: %s" % (track_reid, e)) from None

    # ------------------------------------------------------------------ zones
    def zone_state(self):
        """The engine's zone state (device int32, ops.zone_state), made on first use, of ``track_trails_capacity()`` entries: one,
        shared by every pass submitted with ``zone=``.  ``zone_reset()`` empties it, totals included; ``track_reset()`` drops its
        entries -- the ids end, without events, open stays are not counted -- and leaves the totals.  ``ops.zone_totals`` reads it."""
        return self.edit_states.zone_state()

    def zone_reset(self):
        """Zero totals and no entries: the state is zeroed on the ordered stream, behind the zone passes submitted so far."""
        with torch.cuda.stream(self.track_stream):
            self.edit_states.reset_zones()

    def zone_option(self, zone):
        """``submit_batch``'s ``zone`` checked and normalised -> (zones, classes, W, anchor): zones a tuple of 1..8 polygons of 3..16
        (x, y), classes "all" or a tuple of this engine's class names, W 1..9 (None: 3), anchor 0 / 1 ("centre" / "bottom", None:
        centre).  FrcnnError, with the reason, for anything else."""
        try:
            zones, classes, width, anchor = zone
        except (TypeError, ValueError):
            raise FrcnnError("submit_batch: zone=%r: (zones, classes, width, anchor)" % (zone,)) from None
        try:
            zones, classes, width, anchor = ops.zone_option(zones, classes, width, anchor)
            if classes != "all":
                classes = ops.redact_class_list(self.class_names(), classes)
        except ValueError as e:
            raise FrcnnError("submit_batch: zone=%r: %s" % (zone, e)) from None
        return zones, classes, width, anchor

    def track_reset(self):
        """Forget every track: the states are zeroed on the tracking stream, behind the tracked passes submitted so far
        (``EditStates.reset_tracks``: the motion headers, the look-back windows, the trails and the count entries with them)."""
        self.track_state()
        with torch.cuda.stream(self.track_stream):
            self.edit_states.reset_tracks()
        self._lookback_waiting.clear()
        self._lookback_last = None

    def track_lookback_window(self, h, w, B, rows=None):
        """-> (the engine's look-back window for passes of B source frames of (h, w) (ops.track_lookback_state), its ``back``), made on
        first use, by a pass that knows the ``rows`` of its packed buffers.  ``track_reset()`` empties it."""
        return self.edit_states.lookback_window(h, w, B, rows)

    @staticmethod
    def track_lookback_option(n, B):
        """``submit_batch``'s ``track_lookback`` checked against the pass's B frames -> the look-back.  FrcnnError with the reason."""
        try:
            n = ops.track_lookback_option(n)
        except ValueError as e:
            raise FrcnnError("submit_batch: track_lookback=%r: %s" % (n, e)) from None
        if n > B:
            raise FrcnnError("submit_batch: track_lookback=%d reaches further back than a pass of %d frames holds: a frame would be emitted "
                             "before a later pass could fill it (use passes of at least %d frames)" % (n, B, n))
        return n

    @staticmethod
    def track_backtrack_option(n, K, F):
        """``submit_batch``'s ``track_backtrack`` checked against the pass's interval and its F source frames -> the look-back.
        FrcnnError with the reason."""
        try:
            return ops.track_backtrack_option(n, K, F)
        except ValueError as e:
            raise FrcnnError("submit_batch: track_backtrack=%r: %s" % (n, e)) from None

    def track_motion_state(self, h, w):
        """The engine's motion state for source frames of (h, w) (ops.track_motion_state), made on first use: the passes submitted with
        ``track_motion=`` keep their last frame in it."""
        return self.edit_states.motion_state(h, w)

    def track_table(self, redact_classes=None):
        """The class table of ops.track_update: the classes the drawing rule draws united with ``redact_classes`` (uploaded once each)."""
        return self.edit_states.track_table(redact_classes)

    @staticmethod
    def track_option(track):
        """``submit_batch``'s ``track`` checked -> (thr, hold, grow) (None in a place: its default).  FrcnnError with the reason."""
        try:
            thr, hold, grow = track
            return ops.track_option(thr, hold, grow)
        except (TypeError, ValueError) as e:
            raise FrcnnError("submit_batch: track=%r: (thr, hold, grow): %s" % (track, e)) from None

    @staticmethod
    def detect_every_option(k, B):
        """``submit_batch``'s ``detect_every`` checked against the pass's B network images -> K, 2..16 with B * K frames in one tracker
        call.  FrcnnError with the reason."""
        try:
            k = ops.track_interval_option(k)
        except ValueError as e:
            raise FrcnnError("submit_batch: detect_every=%r: %s" % (k, e)) from None
        if B * k > _lib.TRACK_MAX_FRAMES:
            raise FrcnnError("submit_batch: detect_every=%d with batch=%d is a pass of %d frames: one tracker call takes at most %d "
                             "(FRCNN_TRACK_MAX_FRAMES)" % (k, B, B * k, _lib.TRACK_MAX_FRAMES))
        return k

    @staticmethod
    def track_scene_cut_option(pct):
        """``submit_batch``'s ``track_scene_cut`` checked -> the threshold in percent, 1..100.  FrcnnError with the reason."""
        try:
            return ops.track_cut_option(pct)
        except ValueError as e:
            raise FrcnnError("submit_batch: track_scene_cut=%r: %s" % (pct, e)) from None

    @staticmethod
    def track_motion_option(radius):
        """``submit_batch``'s ``track_motion`` checked -> the search radius, 1..16.  FrcnnError with the reason."""
        try:
            return ops.track_motion_radius(radius)
        except ValueError as e:
            raise FrcnnError("submit_batch: track_motion=%r: %s" % (radius, e)) from None

    # ------------------------------------------------------------------ eligibility
    @staticmethod
    def usable(manager, detector, num_rois):
        rpn = getattr(manager, "rpn_model", None)
        if not (isinstance(rpn, models.RpnModel) and isinstance(detector, models.DetModel)):
            return False                                # a foreign Keras-style model: voc_dets keeps the eager path
        if not manager.conv_only or detector.base is not None:
            return False                                # the detector must take the RPN's conv map (voc_dets.py:177-183)
        n_rows = -(-MAX_PROPOSALS // int(num_rois)) * int(num_rois)
        return 0 < n_rows <= 512                        # frcnn_detections: one workgroup, <= 512 scored rows

    # ------------------------------------------------------------------ capture
    def _device_taps(self, dst, src):
        t = self._taps_dev.get((dst, src))
        if t is None:
            if len(self._taps_dev) > 256:
                self._taps_dev.clear()
            t = self._taps_dev[(dst, src)] = torch.from_numpy(ops.resize_cubic_taps(dst, src)).cuda()
        return t

    def _stage(self, s, seg, fine):
        """The slot's staging on both sides of PCIe: [B frame segments of ``seg`` bytes | B x (resize_ratio, det_threshold)]; a
        ``detect_every`` pass has ``s.frames`` = B * K segments in front of its B pairs.
        -> (the pinned side as a numpy array, the device view the pass reads the pairs from: (B, 2) f64, one image's (2,) for B = 1)."""
        B, off = s.batch, s.frames * seg
        s.seg = seg
        tail = 16 if s.track or s.heat or s.remove or s.moving else 0     # a tracking, heat or remove pass: | the count of real frames, int32 (ops.track_update's n_frames)]
        s.io_dev = torch.zeros(off + 16 * B + tail, dtype=torch.uint8, device="cuda")
        fine("buffers: device staging")
        s.io_pin = self._pinned.take(off + 16 * B + tail, zero=True)
        fine("buffers: pinned staging")
        host = s.io_pin.numpy()
        if tail:                                         # (0 until a submit says otherwise: warm-up and capture leave the state alone)
            s.n_frames_host = host[off + 16 * B:off + 16 * B + 4].view(np.int32)
            s.n_frames_dev = s.io_dev[off + 16 * B:off + 16 * B + 4].view(torch.int32)
        s.dyn_host = host[off:off + 16 * B].view(np.float64).reshape(B, 2)
        s.dyn_host[:] = (1.0, 0.0)
        dyn_dev = s.io_dev[off:off + 16 * B].view(torch.float64).view(B, 2)
        return host, (dyn_dev if B > 1 else dyn_dev[0])

    def _exact_pass(self, s, fine, H, W, src, flip):
        """The buffers and the pass of an exact-geometry slot; resize and preprocess are INSIDE the pass.  ``src`` = (source height,
        source width): the pass starts from the decoded frame at the file's size and resizes (and flips) it on the device; None: the
        uploaded pixels are already (H, W).  An annotating pass then edits each uploaded source frame where it lies (``s.chain``, an
        ``EditChain``: redaction, heat map, trails, count lines, boxes and labels, in the order its docstring states); with ``s.encode`` == "png" or "png-huffman" it then encodes the drawn frame as a PNG file on
        the device (ops.png_encode_u8, compress "runs" or "huffman") into the slot's own buffer, which is what such a pass reads back
        instead of the raw frame; with ``s.encode`` == "jpeg" as a JPEG file at ``s.quality`` in ``s.jpeg_mode`` = (subsampling, huffman)
        (ops.jpeg_encode_u8)."""
        B, pipe, annotate = s.batch, s.pipe, s.annotate
        F, K = s.frames, s.every or 1                               # source frames of the pass; the network sees every K-th (F = B unless ``detect_every``)
        in_h, in_w = src if src is not None else (H, W)
        npix = in_h * in_w * 3
        pix_bytes = npix if self.device_preprocess else 4 * npix
        host, dyn = self._stage(s, (pix_bytes + 15) // 16 * 16, fine)
        seg = s.seg
        if self.device_preprocess:
            s.pix_hosts = [host[i * seg:i * seg + npix].reshape(in_h, in_w, 3) for i in range(F)]
            u8 = [s.io_dev[i * seg:i * seg + npix].view(in_h, in_w, 3) for i in range(F)]
            s.x_f32 = torch.empty((B, H, W, 3), dtype=torch.float32, device="cuda")
            if src is not None:
                s.tabs = (torch.from_numpy(ops.resize_cubic_taps(W, in_w)).cuda(), torch.from_numpy(ops.resize_cubic_taps(H, in_h)).cuda())
                s.u8_resized = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
        else:
            assert B == 1 and not annotate and src is None
            s.pix_hosts = [host[:pix_bytes].view(np.float32).reshape(H, W, 3)]
            s.x_f32 = s.io_dev[:pix_bytes].view(torch.float32).view(1, H, W, 3)
        # annotating pass: frame i is read back from its staging segment into the slot's own pinned segment after the replay
        s.frame_io = [(s.io_dev[i * seg:i * seg + npix], s.io_pin[i * seg:i * seg + npix]) for i in range(F)] if annotate and not s.encode else None
        uploaded_rgb = src is not None and bool(int(flip) & 2)      # the channel order the frames were uploaded in (host_pixels: flip bit 1)
        if annotate:
            # the editing chain (``EditChain``: its docstring states the order) over the frames as uploaded, ``seg`` bytes apart in the
            # staging area.  A delayed pass edits, encodes and returns the frames of the pass BEFORE it, which the chain's window emits
            # (a ``track_backtrack`` pass is such a pass over its F = B * K source frames: F is B everywhere else)
            if s.track:
                self.track_state()                                  # (refuses an engine whose rows leave no room for a tracker)
            chain = s.chain = EditChain(self.edit_states, s.spec, F, K, (in_h, in_w), uploaded_rgb)
            out = [chain.lb_frames[i] for i in range(F)] if s.track_lookback else u8
            if s.track_lookback and s.frame_io is not None:         # (raw read-back: the emitted frame, into the slot's pinned segment)
                s.frame_io = [(out[i].view(-1), s.io_pin[i * seg:i * seg + npix]) for i in range(F)]
        # the scale step (DESIGN §8 "Scale rule"): the last edit, in front of every encoder.  Each edited frame is scaled into the slot's
        # scaled area, ``sc_seg`` bytes a frame, and THAT is what the encoders read and a pass without one copies back
        enc_h, enc_w = s.spec.out_hw((in_h, in_w))
        enc_pix = enc_h * enc_w * 3
        if s.out_size:
            sc_seg = (enc_pix + 15) // 16 * 16
            s.scale_dev = torch.zeros(F * sc_seg, dtype=torch.uint8, device="cuda")
            scaled = [s.scale_dev[i * sc_seg:i * sc_seg + enc_pix].view(enc_h, enc_w, 3) for i in range(F)]
            if s.frame_io is not None:
                s.frame_io = [(scaled[i].view(-1), s.io_pin[i * seg:i * seg + enc_pix]) for i in range(F)]
                s.pix_out = [host[i * seg:i * seg + enc_pix].reshape(enc_h, enc_w, 3) for i in range(F)]
        if s.encode == JPEG_ENCODE:
            # a frame's row: [its length, int32 | pad to 16 | the file, at most jpeg_bound bytes].  The bound is 6.5 times the raw frame
            # (every block at its longest), which is device memory only: a replay reads back the row's first ``first_copy`` bytes -- the
            # length, the header and a quarter of the raw frame's size, more than a photograph takes at quality 90 -- and collect_batch
            # fetches the rest of a longer file.
            subsampling, huffman = s.jpeg_mode
            s.png_bound = ops.jpeg_bound(enc_h, enc_w, subsampling, huffman)
            s.png_dev = torch.zeros((F, 16 + (s.png_bound + 15) // 16 * 16), dtype=torch.uint8, device="cuda")
            s.first_copy = min(16 + ops.jpeg_header_bytes() + enc_pix // 4, 16 + s.png_bound)
            s.png_ws = torch.empty(ops.jpeg_workspace_bytes(enc_h, enc_w, subsampling, huffman), dtype=torch.uint8, device="cuda")
            png_out = [(s.png_dev[i][16:16 + s.png_bound], s.png_dev[i][0:4].view(torch.int32)) for i in range(F)]
        elif s.encode == Y4M_ENCODE:
            # a frame's row: its record [Y | Cb | Cr], ops.y4m_frame_bytes long: the slot's output area is B records back to back
            chroma, yrange = s.y4m_mode
            s.png_bound = ops.y4m_frame_bytes(enc_h, enc_w, chroma)
            s.png_dev = torch.zeros((F, s.png_bound), dtype=torch.uint8, device="cuda")
        elif s.encode:
            # a frame's row: [the file, at most png_bound bytes | pad to 16 | its length, int32 | pad]: one fixed-size copy brings both back
            # (the bound is 0.5 % over the raw frame).  File-backed frames were uploaded in the decoder's order (host_pixels: flip bit 1).
            compress = PNG_ENCODES[s.encode]
            s.png_bound = ops.png_bound(enc_h, enc_w, compress)
            len_at = (s.png_bound + 15) // 16 * 16
            s.png_dev = torch.zeros((F, len_at + 16), dtype=torch.uint8, device="cuda")
            s.png_ws = torch.empty(ops.png_workspace_bytes(enc_h, enc_w, compress), dtype=torch.uint8, device="cuda")     # (the frames of a pass encode one after another)
            png_out = [(s.png_dev[i][:s.png_bound], s.png_dev[i][len_at:len_at + 4].view(torch.int32)) for i in range(F)]

        def run():
            if self.device_preprocess:
                for i in range(B):                                  # (a ``detect_every`` pass: segments 0, K, 2K, ... feed the network)
                    frame = u8[i * K]
                    if src is not None:                             # shapes.Image.data: INTER_CUBIC resize (+ flip) of the decoded frame
                        frame = ops.resize_cubic_u8(u8[i * K], H, W, flip=flip, tabs=s.tabs, out=s.u8_resized)
                    ops.preprocess_u8(frame, MEAN_BGR, out=s.x_f32[i:i + 1])     # resnet.preprocess + the f32 feed cast, bit for bit
            res = pipe.forward_dev(s.x_f32, dyn=dyn)
            if annotate:                                            # the frames edited where they lie (their only reader is done)
                chain.update(s.io_dev, seg, res["det_packed"], s.n_frames_dev)
                for i in range(F):
                    chain.edit(i, out[i])
                    if s.encode == Y4M_ENCODE:
                        continue                                    # (all B frames in one launch behind the loop)
                    final = out[i]
                    if s.out_size:
                        final = ops.downscale_u8(out[i], enc_h, enc_w, out=scaled[i])
                    if s.encode == JPEG_ENCODE:
                        ops.jpeg_encode_u8(final, quality=s.quality, bgr=not uploaded_rgb, out=png_out[i][0], out_len=png_out[i][1],
                                           workspace=s.png_ws, subsampling=subsampling, huffman=huffman)
                    elif s.encode:
                        ops.png_encode_u8(final, bgr=not uploaded_rgb, out=png_out[i][0], out_len=png_out[i][1], workspace=s.png_ws,
                                              compress=compress)
                if s.encode == Y4M_ENCODE:
                    frames, stride = (chain.lb_frames.view(-1), npix) if s.track_lookback else (s.io_dev, seg)
                    if s.out_size:                                  # (all F frames scaled in one launch, then encoded in one)
                        ops.downscale_u8(frames.as_strided((F, in_h, in_w, 3), (stride, 3 * in_w, 3, 1)), enc_h, enc_w,
                                         out=s.scale_dev.as_strided((F, enc_h, enc_w, 3), (sc_seg, 3 * enc_w, 3, 1)))
                        frames, stride = s.scale_dev, sc_seg
                    ops.y4m_encode_frames_u8(frames, stride, F, enc_h, enc_w, chroma, yrange, bgr=not uploaded_rgb, out=s.png_dev)
            return res
        return run

    def _canvas_pass(self, s, fine, Hc, Wc):
        """The buffers and the pass of a slot over B canvases of (Hc, Wc): the frames' resize + preprocess stay OUTSIDE the graph (their
        sizes are per image: a few eager launches in front of every replay, _canvas_preprocess), the graph holds trunk .. post-process
        with the images' true extents read from ``s.extents`` (device words)."""
        B = s.batch
        host, dyn = self._stage(s, (Hc * Wc * 3 + 15) // 16 * 16, fine)      # a frame's segment: any source of at most the canvas's pixel count
        s.pix_hosts = [host[i * s.seg:(i + 1) * s.seg] for i in range(B)]
        s.u8_resized = torch.empty((B, s.seg), dtype=torch.uint8, device="cuda")
        s.x_f32 = torch.zeros((B, Hc, Wc, 3), dtype=torch.float32, device="cuda")
        fine("buffers: canvases")
        s._ext_raw = self._pinned.take(self._extents_class.LEVELS * B * 8)
        s.extents = self._extents_class(B, pinned=s._ext_raw)
        for i in range(B):
            s.extents.set(i, Hc, Wc)                                # (warm-up and capture run over the full canvas)
        s.extents.upload()
        return lambda: s.pipe.forward_dev(s.x_f32, dyn=dyn, extents=s.extents)

    def _capture_slot(self, B, canvas, H, W, src=None, flip=False, spec=PassSpec()):
        """One captured pass over B frames, each with its own [resize_ratio, det_threshold] pair (B > 1:
        pipeline.BatchedInferencePipeline): of the exact geometry (H, W, src, flip) (_exact_pass), or with ``canvas`` of the canvas class
        (H, W) (_canvas_pass).  ``spec`` (``PassSpec``) says what the pass does and fills the slot's fields of the same names.
        ``encode``: "png" / "png-huffman" for an annotating pass that ends in the device PNG encoder, "jpeg" for one that
        ends in the device JPEG encoder at ``quality`` in ``jpeg_mode`` = (subsampling, huffman), "y4m" for one that ends in the YUV4MPEG2
        encoder in ``y4m_mode`` = (chroma, range).  ``redact`` = (classes, mode, size, margin) (``redact_option``): an annotating pass that
        hides those classes' boxes in each frame (ops.redact_u8) in front of the drawing step; ``draw`` False: one that draws nothing.
        ``track`` = (thr, hold, grow): an annotating pass that runs the engine's tracker over its frames (ops.track_update);
        ``track_motion`` = R: with the motion step of radius R in front of every frame's match (ops.track_update_motion);
        ``track_lookback`` = L: with the look-back call behind the tracker (ops.track_lookback): the pass edits, encodes and returns the
        frames of the pass before it.  ``detect_every`` = K: a pass over B * K source frames whose network sees every K-th
        (ops.track_update_interval); with ``track_backtrack`` = L: the back-track call behind it (ops.track_backtrack), a delayed pass as
        a look-back pass is, over its B * K source frames.  Which of these calls an annotating pass makes, and in which order, is the
        chain's to say (``frame_edit.EditChain``, built by _exact_pass from ``spec``)."""
        t0 = time.perf_counter()
        with no_gc():                                               # (collects first, at most once per second: a collection costs more than the capture)
            m = self.manager
            kw = dict(stride=self.stride, pre_nms_top_n=PRE_NMS_TOP_N, max_proposals=MAX_PROPOSALS, roi_batch=self.num_rois, pad_to_batch=PAD_TO_BATCH,
                      bg_idx=m.class_mapping["bg"])
            if self.post is not None:
                kw["post"] = self.post
            if B > 1:
                pipe = BatchedInferencePipeline(m.rpn_model, self.detector, m.anchor_dims, B, **kw)
            else:
                pipe = InferencePipeline(m.rpn_model, self.detector, m.anchor_dims, **kw)
            reserved0 = torch.cuda.memory_reserved()
            stamps = []
            stamp = lambda name: stamps.append((name, time.perf_counter()))
            fine = stamp if canvas else (lambda name: None)         # (a canvas capture's "buffers" are booked piece by piece)
            stamp("pipeline")
            s = _Slot()
            s.key, s.pipe, s.batch, s.canvas, s.spec = (("canvas", H, W) if canvas else (H, W)), pipe, B, canvas, spec
            s.annotate, s.encode, s.quality, s.jpeg_mode, s.y4m_mode = spec.annotate, spec.encode, spec.quality, spec.jpeg_mode, spec.y4m_mode
            s.redact, s.nodraw, s.track, s.track_motion = spec.redact, (None if spec.draw else True), spec.track, spec.track_motion
            s.track_lookback, s.track_backtrack = spec.track_lookback or spec.track_backtrack, spec.track_backtrack      # (both: the delayed path is one)
            s.every, s.frames = spec.detect_every, B * (spec.detect_every or 1)
            s.track_scene_cut, s.track_trails, s.heat, s.count = spec.track_scene_cut, spec.track_trails, spec.heat, spec.count
            s.zone, s.remove, s.track_reid, s.out_size = spec.zone, spec.remove, spec.track_reid, spec.out_size
            s.moving = spec.redact_moving
            run = self._canvas_pass(s, fine, H, W) if canvas else self._exact_pass(s, fine, H, W, src, flip)
            shared = self.in_flight > 1
            # one image in flight: split-K on the small grids (a latency tool); several: plain launches, tiles for a shared chip
            # (fp32 models keep split-K also beside other passes, as bench.py's headline does: the small grids of rpn_conv1 / stage 4 then run
            # the split engine's split-K form; the bf16 engine loses with it when several passes share the chip)
            dtype = getattr(getattr(self.detector, "head", None), "dtype", "f32")
            s.ws = ops.NO_SPLIT_K if ((shared and (dtype == "bf16" or os.environ.get("FRCNN_ENTRY_NO_SPLITK"))) or B > 1) else ops.ConvWorkspace()
            fine("buffers: extents")
            s.io_dev.copy_(s.io_pin)
            fine("buffers: first upload")
            s.amax = ops.AmaxArena() if self.f32_engine == "f16x3" else None      # the pass's magnitude records (fixed addresses across replays)
            # Warm-up and capture on ONE side stream, with no device-wide synchronisation: the passes of other geometries that are in flight on
            # the engine's streams keep running (round 6: torch.cuda.graph's enter -- synchronize, empty_cache -- and two more synchronize calls
            # drained them at every capture, and a list of mixed image sizes captures per geometry).  The warm-up pass writes the slot's own
            # buffers, as the replays will: ``s.ready`` orders the first replay behind it.
            side = _capture_stream()
            side.wait_stream(torch.cuda.current_stream())
            stamp("buffers")
            with torch.cuda.stream(side), ops.conv_workspace(s.ws), ops.tile_policy(shared), ops.f32_engine(self.f32_engine), ops.amax_arena(s.amax):
                for _ in range(WARMUP_PASSES):
                    run()
                stamp("warm-up enqueue")
                s.ready = torch.cuda.Event()
                s.ready.record(side)
                s.graph = torch.cuda.CUDAGraph()
                s.graph.capture_begin(pool=torch.cuda.graph_pool_handle(), capture_error_mode="thread_local")
                try:
                    s.out = run()
                    stamp("capture enqueue")
                finally:
                    s.graph.capture_end()
            stamp("instantiate")
            packed = s.out["det_packed"]
            s.out_packed = packed if isinstance(packed, (list, tuple)) else [packed]
            s._out_raw = self._pinned.take(4 * B * s.out_packed[0].numel())
            s.out_pin = s._out_raw.view(torch.int32).view((B,) + tuple(s.out_packed[0].shape))
            if s.encode:                                            # (taken behind the capture: a failed one never held it)
                shape = (s.frames, s.first_copy) if s.encode == JPEG_ENCODE else tuple(s.png_dev.shape)
                s._png_raw = self._pinned.take(shape[0] * shape[1], zero=True)
                s.png_pin = s._png_raw[:shape[0] * shape[1]].view(shape)
            if s.track:
                track_out = s.chain.host_tracked
                s._track_raw = self._pinned.take(4 * track_out.numel())
                s.track_pin = s._track_raw.view(torch.int32)[:track_out.numel()].view(tuple(track_out.shape))
            if s.track_scene_cut:
                s._cuts_raw = self._pinned.take(4 * s.frames)
                s.cuts_pin = s._cuts_raw.view(torch.int32)[:s.frames]
            if s.count:
                count_lists = s.chain.count_lists
                s._count_raw = self._pinned.take(4 * count_lists.numel())
                s.count_pin = s._count_raw.view(torch.int32)[:count_lists.numel()].view(tuple(count_lists.shape))
            if s.zone:
                zone_lists = s.chain.zone_lists
                s._zone_raw = self._pinned.take(4 * zone_lists.numel())
                s.zone_pin = s._zone_raw.view(torch.int32)[:zone_lists.numel()].view(tuple(zone_lists.shape))
            if s.track_reid:
                reid_lists = s.chain.reid_lists
                s._reid_raw = self._pinned.take(4 * reid_lists.numel())
                s.reid_pin = s._reid_raw.view(torch.int32)[:reid_lists.numel()].view(tuple(reid_lists.shape))
            if s.moving:
                moving_stats = s.chain.moving_stats
                s._moving_raw = self._pinned.take(4 * moving_stats.numel())
                s.moving_pin = s._moving_raw.view(torch.int32)[:moving_stats.numel()].view(tuple(moving_stats.shape))
            if s.track_lookback:                                    # [the B emitted buffers | the count word]
                words = s.chain.lb_out[1].numel() + 4
                s._lb_raw = self._pinned.take(4 * words)
                s.lb_pin = s._lb_raw.view(torch.int32)[:words]
            s.event = torch.cuda.Event()
            s.nbytes = max(int(torch.cuda.memory_reserved() - reserved0), int(s.io_dev.numel() + s.x_f32.numel() * 4))
            stamp("read-back buffers")
            self.capture_seconds += time.perf_counter() - t0
            self._book_capture(t0, stamps)
            return s

    def _book_capture(self, t0, stamps):
        """Where a capture's host time goes (stats()["capture_breakdown_ms"], summed over the engine's captures)."""
        prev = t0
        for name, t in stamps:
            self.capture_breakdown[name] = self.capture_breakdown.get(name, 0.0) + (t - prev) * 1e3
            prev = t

    # ------------------------------------------------------------------ the call
    def _check_epoch(self):
        self.manager.rpn_model._flush_trainer()
        self.detector._flush_trainer()
        if models.weights_epoch() != self._epoch:
            self.cache.clear()
            self._epoch = models.weights_epoch()

    def prefetchable(self, image):
        """True when ``host_pixels(image)`` is pure host work (a JPEG decode) that another thread may do ahead of time; images
        without ``raw`` and foreign preprocess functions are fetched inline (their ``data`` may use the device)."""
        return self.device_preprocess and _declares(image, "raw") and _declares(image, "height")

    def host_pixels(self, image):
        """What ``submit`` uploads for this image -- safe to call from another thread ahead of time (JPEG decode).
        Returns (array, H, W, src or None, flip)."""
        if self.device_preprocess and _declares(image, "raw") and _declares(image, "height"):
            H, W, flip = int(image.height), int(image.width), bool(getattr(image, "flipped", False))
            jpeg_dev, png_dev = jpeg_decoder(), png_decoder()
            y4m_plan = getattr(image, "y4m_plan", None)
            if RGB_UPLOAD and isinstance(y4m_plan, _lib.Y4mPlan) and _declares(image, "raw_file"):
                # a frame of a YUV4MPEG2 stream: its planes go up, the device converts them (no setting: there is no host codec to prefer)
                return Y4mFile(image.raw_file(), y4m_plan, getattr(image, "_image_path", None) or str(getattr(image, "name", "?"))), H, W, \
                    (int(y4m_plan.h), int(y4m_plan.w)), 2 | int(flip)
            if RGB_UPLOAD and (jpeg_dev != "host" or png_dev != "host"):
                from . import feed
                # None: in-memory pixels, or a file the device decoders do not take
                planned = feed.plan_entry_file(image, jpeg=jpeg_dev, png=png_dev)
                if planned is not None:
                    data, plan = planned
                    kind = _FILE_KINDS[ops.decoder_of(plan).label]
                    return kind(data, plan, getattr(image, "_image_path", None) or str(getattr(image, "name", "?"))), H, W, \
                        (int(plan.h), int(plan.w)), 2 | int(flip)
            rgb = getattr(image, "raw_rgb", None) if RGB_UPLOAD else None
            if rgb is not None:
                # a file-backed frame goes up as the decoder delivers it (RGB); the device resize writes B, G, R (flip bit 1) -- a resize to
                # its own size when none is needed: taps {0, 1, 0, 0}, i.e. a copy with the channels swapped
                rgb = np.asarray(rgb)
                if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
                    raise TypeError("image pixels must be uint8 (h, w, 3) (shapes.py:19-29), got %s %s" % (rgb.dtype, rgb.shape))
                return rgb, H, W, (int(rgb.shape[0]), int(rgb.shape[1])), 2 | int(flip)
            raw = np.asarray(image.raw)
            if raw.dtype != np.uint8 or raw.ndim != 3 or raw.shape[2] != 3:
                raise TypeError("image pixels must be uint8 BGR (h, w, 3) (shapes.py:19-29), got %s %s" % (raw.dtype, raw.shape))
            if raw.shape[:2] == (H, W) and not flip:
                return raw, H, W, None, False
            return raw, H, W, (int(raw.shape[0]), int(raw.shape[1])), flip
        data = image.data
        if self.device_preprocess:
            data = np.asarray(data)
            if data.dtype != np.uint8:
                raise TypeError("image.data must be uint8 BGR (shapes.py:19-29), got %s" % data.dtype)
        else:
            data = self.manager.preprocess_func(data)               # det_util.py:36 (float64 on the host, cast on feed)
        return data, int(data.shape[0]), int(data.shape[1]), None, False

    def plan_canvases(self, counts):
        """Before a call over a list whose sizes are known (voc_dets.get_dets_by_cls reads the headers): the canvas classes for that
        histogram {(H, W): images} (plan_canvas_classes; classes with a captured pass count as free) and how many passes each may
        hold in flight -- its share of the list times ``in_flight``, at least one, two when it fills more than one pass."""
        existing = {k[1:3] for k in self.cache.keys() if k[:1] == ("canvas",)}
        plan = plan_canvas_classes(counts, existing=existing)
        self._canvas_of.update(plan)
        per_class, total = collections.Counter(), float(sum(counts.values())) or 1.0
        for g, c in plan.items():
            per_class[c] += counts[g]
        for c, n in per_class.items():
            want = int(np.ceil(CANVAS_SLOT_FACTOR * self.in_flight * n / total - 1e-9))
            self._canvas_slots[("canvas",) + c] = max(1 if (n <= self.batch or CANVAS_SLOT_MIN < 2) else 2, min(self.in_flight, want))
            if want >= self.in_flight:                            # the class that fills every stream: one pass more, queued behind the oldest
                self._canvas_slots[("canvas",) + c] += CANVAS_EXTRA_SLOT
        # ... within the cache's byte budget: passes beyond it would only evict each other (a pass costs what one of its class did, else
        # CANVAS_BYTES_PER_PIXEL of its canvases: ~1.4 GB per four 600 x 1000 images)
        def cost(c):
            known = [sl.nbytes for k, v in self.cache._slots.items() if k[:3] == ("canvas",) + c for sl in v]
            return max(known) if known else CANVAS_BYTES_PER_PIXEL * self.batch * c[0] * c[1]
        live = [c for c in per_class]
        while sum(self._canvas_slots[("canvas",) + c] * cost(c) for c in live) > 0.9 * self.cache.byte_budget:
            c = max(live, key=lambda k: (self._canvas_slots[("canvas",) + k], -per_class[k]))     # (the fullest allowance; among equals the rarest class)
            if self._canvas_slots[("canvas",) + c] <= 1:
                break
            self._canvas_slots[("canvas",) + c] -= 1
        return plan

    def canvas_class(self, H, W):
        """The canvas (Hc, Wc) of a true size: the plan's, else the smallest known class that holds it with at most a third more
        pixels, else its own smallest canvas (which becomes a class)."""
        c = self._canvas_of.get((H, W))
        if c is None:
            own = (canvas_side(H), canvas_side(W))
            fits = [k for k in set(self._canvas_of.values()) if k[0] >= own[0] and k[1] >= own[1] and 3 * k[0] * k[1] <= 4 * own[0] * own[1]]
            c = self._canvas_of[(H, W)] = min(fits, key=lambda k: (k[0] * k[1], k)) if fits else own
            if len(self._canvas_of) > 4096:
                self._canvas_of.clear()
        return c

    def canvas_ok(self, pixels):
        """Can this frame go through a canvas pass?  (device preprocess, a source no larger than its canvas)"""
        arr, H, W, src, flip = pixels
        if not (self.canvas_capable and (isinstance(arr, JpegFile) or getattr(arr, "dtype", None) == np.uint8)):
            return False
        Hc, Wc = self.canvas_class(H, W)
        size = arr.plan.h * arr.plan.w * 3 if isinstance(arr, JpegFile) else int(np.prod(arr.shape))
        return size <= Hc * Wc * 3

    @staticmethod
    def geometry_of(pixels):
        """The exact geometry of a ``host_pixels`` result (resized size, source size, flip)."""
        _, H, W, src, flip = pixels
        return (H, W) if src is None else (H, W) + src + (flip,)

    def geometry(self, pixels):
        """The captured-pass key of a ``host_pixels`` result: images with equal keys can share a batched pass.  In canvas mode the key
        is the canvas CLASS of the image's size."""
        if self.canvas and self.canvas_ok(pixels):
            return ("canvas",) + self.canvas_class(pixels[1], pixels[2])
        return self.geometry_of(pixels)

    def probe_geometry(self, image):
        """``geometry(host_pixels(image))`` WITHOUT decoding the pixels (a file's header gives its size), or None when that cannot be
        known cheaply.  get_dets_by_cls counts how often each geometry occurs in its list before it decides what to capture."""
        if not (self.device_preprocess and hasattr(image, "raw_size") and hasattr(image, "height")):
            return None
        try:
            size = image.raw_size()
        except Exception:                                       # noqa: BLE001 -- an unreadable header: the decode will say what is wrong
            return None
        if size is None:
            return None
        H, W, flip = int(image.height), int(image.width), bool(getattr(image, "flipped", False))
        if self.canvas and self.canvas_capable:
            Hc, Wc = self.canvas_class(H, W)
            if size[0] * size[1] <= Hc * Wc:
                return ("canvas", Hc, Wc)
        if RGB_UPLOAD and getattr(image, "_pixels", 0) is None and hasattr(type(image), "raw_rgb"):      # file-backed: uploaded as RGB (host_pixels; the
            # attribute is looked up on the CLASS: hasattr on the instance would run the property, i.e. decode the JPEG)
            return (H, W, int(size[0]), int(size[1]), 2 | int(flip))
        if tuple(size) == (H, W) and not flip:
            return (H, W)
        return (H, W, int(size[0]), int(size[1]), flip)

    def should_wait(self, pixels, batch):
        """Before a ``submit_batch`` of these frames: True when every captured pass of their canvas class is in flight and the class
        already has the passes its plan allows (CANVAS_SLOTS_PER_CLASS outside a plan) -- collecting an older ticket frees one sooner
        than a capture would make another."""
        key = self.geometry(pixels[0])
        if key[0] != "canvas":
            return False
        slots = self.cache._slots.get(key + ((batch,) if batch > 1 else ()))
        return slots is not None and len(slots) >= self._canvas_slots.get(key, CANVAS_SLOTS_PER_CLASS) and all(sl.busy for sl in slots)

    def exact_geometry(self, image):
        """``probe_geometry`` with canvas mode off: the image's OWN geometry (get_dets_by_cls counts the distinct ones)."""
        was, self.canvas = self.canvas, False
        try:
            return self.probe_geometry(image)
        finally:
            self.canvas = was

    def has_geometry(self, key):
        """A captured pass of this geometry (one image per pass, or the batched form) is already in the cache."""
        return key in self.cache._slots or (key + (self.batch,)) in self.cache._slots

    def submit(self, image, resize_ratio, det_threshold=0.0, pixels=None):
        """``pixels``: the result of ``host_pixels(image)`` when the caller fetched it ahead of time."""
        return self.submit_batch([image], [resize_ratio], det_threshold, [self.host_pixels(image) if pixels is None else pixels], batch=1)

    def submit_batch(self, images, resize_ratios, det_threshold, pixels, batch=None, **options):
        """Up to ``batch`` images of ONE geometry (``geometry(pixels[i])`` equal) in one captured pass; a short group is padded with
        copies of its first frame, whose results nobody reads.  ``collect_batch`` returns the images' results in order.
        ``annotate``: a pass of its own (cache key tagged "annotate", never a canvas pass) that also draws the detections into each
        uploaded frame and reads the frame back; ``collect_batch`` then returns (num_rois, dets, frame).  ``encode`` = "png" (annotating
        passes only; again a pass of its own, key tagged "annotate", "png"): the drawn frame is encoded as a PNG file inside the pass
        and the FILE is read back; ``collect_batch`` then returns (num_rois, dets, png) with ``png`` the file's bytes.  "png-huffman":
        the same through the encoder's huffman mode (key tagged "annotate", "png-huffman": one more pass of its own, buffers sized by
        that mode's bound).  ``encode`` = "jpeg" with ``quality`` = 1..100 (stated by the caller: it is part of the pass): the drawn
        frame is encoded as a baseline JPEG file at that IJG quality (ops.jpeg_encode_u8; key tagged "annotate", "jpeg", quality) and
        ``collect_batch`` returns (num_rois, dets, jpg).  ``quality`` with any other ``encode`` is an error.  ``subsampling`` = 444 / 420
        and ``huffman`` = "standard" / "optimized" (encode="jpeg" only; None: 444, "standard") select the encoder's mode; any pair but the
        default is a pass of its own, its key tagged with the pair behind the quality -- (444, "standard") IS the pass without them.
        ``encode`` = "y4m" with ``y4m`` = (chroma, range) ("420jpeg" / "444", "limited" / "full"; None: Y4M_MODE): the B drawn frames are
        converted to YUV4MPEG2 records [Y | Cb | Cr] in one launch (ops.y4m_encode_frames_u8; key tagged "annotate", "y4m", chroma, range)
        and ``collect_batch`` returns (num_rois, dets, record).  ``y4m`` with any other ``encode`` is an error.
        ``redact`` = (classes, mode, size, margin) (annotating passes only; a pass of its own, the annotating key with ("redact", classes,
        mode, size, margin) appended): classes a tuple of class names or "all", mode "pixelate" / "blur" / "fill", size the cell side /
        blur radius (None: the mode's default; 0 for "fill"), margin >= 0 pixels around each box.  Every box of those classes is hidden in
        the frame (ops.redact_u8, DESIGN §8 "Redaction rule") before the drawing step, so in front of every ``encode``.  ``draw`` = False
        (annotating passes only; key tagged ("nodraw",)): nothing is drawn.  Without the two, every key is what it was.
        ``track`` = (thr, hold, grow) (annotating passes only; a pass of its own, the annotating key with ("track", thr, hold, grow)
        appended; None in a place: 30, 8, 0): the engine's tracker (DESIGN §8 "Tracking rule", ops.track_update) runs over the pass's
        frames in order, behind the post-process: every live row of a tracked class gets a stable id, which the label shows as
        ``cls#id``, and a track the detector has lost is HELD for ``hold`` frames, its box grown by ``grow`` pixels per frame -- held
        boxes are redacted (with ``redact``) and never drawn.  ``collect_batch``'s dets then carry "track_id" (0: untracked), and the
        held rows follow the live ones as dets with "held" = their age.  Passes with ``track`` replay on ONE stream of the engine
        (``track_stream``) in submit order, whatever ``in_flight`` is: submit the frames in the order they were shot, and call
        ``track_reset()`` between two sequences.  A short group's padding frames do not count.
        ``track_motion`` = R (tracking passes only; ("motion", R) appended behind the track tail of the key; 1..16): the motion step
        (DESIGN §8 "Motion rule", ops.track_update_motion) runs in front of every frame's match: each track's box is moved by the best
        integer shift, at most R pixels either way, of the pixels under it between the frame before and this one, so a held box follows
        its object and a fast object is matched where it now is.  The engine keeps the last frame of each source size; ``track_reset()``
        forgets them too.  Without it every key and byte of a tracking pass is what it was.
        ``track_lookback`` = L (tracking passes only; ("lookback", L) appended behind the track / motion tail of the key; 1..16 and at most
        the pass's B): the look-back rule (DESIGN §8 "Look-back rule", ops.track_lookback) runs behind the tracker: every track born in the
        pass is followed back over L frames and hidden there, and the pass edits, encodes and returns the frames of the look-back pass
        submitted BEFORE it: ``collect_batch`` of submit k returns the results of submit k - 1 (none for the first; ``ticket.emitted``
        holds their images), with the back-filled rows as dets with "backfilled" = k behind the held ones.  A submit with NO images is the
        flush: it replays the LAST look-back pass submitted, whatever its other arguments say (they are not read, ``track_lookback`` only marks
        it), with no frame, and returns the last group.  Collect look-back tickets in submit order.  An engine follows ONE look-back
        sequence at a time: flush before the geometry, the pass size or any option changes (``annotate_images`` / ``annotate_stream``
        do), and do not interleave two sequences.
        ``detect_every`` = K (tracking passes with ``track_motion`` only; ("every", K) appended behind the track / motion tail of the key;
        2..16 with batch * K at most 64): the network sees every K-th frame only (DESIGN §8 "Interval rule", ops.track_update_interval).
        ``pixels`` then holds up to batch * K source frames of one geometry IN ORDER, ``images`` / ``resize_ratios`` the KEY frames
        0, K, 2K, ... among them only: len(images) == ceil(len(pixels) / K).  Between two key frames the block match alone moves every
        track's box; nothing is matched, aged or born there, so ``hold`` counts key frames and a held box does not grow in between.  The
        redaction, the drawing step and the encoder run over every source frame, and ``collect_batch`` returns one result per source frame,
        in order: a key frame's as a tracking pass returns it, a between frame's with num_rois 0 and dets made of the tracks -- the live
        ones with "track_id" and "propagated": True (the prob is that of the track's last match), then the held ones.  Not together with
        ``track_lookback`` (the look-back window holds one tracked buffer per network image); as every annotating pass, never a canvas
        pass (its key is the exact geometry), and refused by name on an engine whose foreign preprocess uploads float pixels.
        ``track_backtrack`` = L (``detect_every`` passes only; ("backtrack", L) appended behind ("every", K); None in L's place: min(16,
        batch * K); 1..16, at least K - 1 and at most batch * K): the back-track rule (DESIGN §8 "Back-track rule", ops.track_backtrack)
        runs behind the interval call: every tracked live row of a key frame is followed BACKWARDS -- a track the key frame continues
        through the between frames in front of it, a new one over L frames -- so a between frame is hidden from both sides: by the box
        propagated forwards and by the one tracked back from the next detection.  The pass is a delayed pass exactly as a
        ``track_lookback`` pass is -- ``collect_batch`` of submit k returns the results of submit k - 1, one per SOURCE frame, a submit
        with no images is the flush, one sequence at a time --; its between frames keep "propagated": True on their live dets, and the
        back-filled rows are dets with "backfilled" = k.  Not together with ``track_lookback``.
        ``track_scene_cut`` = PCT (tracking passes with ``track_motion`` only, with or without ``detect_every``; ("cut", PCT) appended
        behind the tags above; 1..100, None in PCT's place is not the default here: ops.track_cut_option() is, 40, provisional): the cut
        rule (DESIGN §8 "Cut rule", ops.track_update_cut) takes the place of the motion or interval call: a frame whose 4 x 4-region luma
        histogram differs from that of the frame before by PCT percent of the largest distance there is, is a hard cut, and every track
        ends in front of it -- no id continues across it, no held row crosses it, and a between frame behind it has no dets until the
        next key frame.  Every result of such a pass carries one more element behind its payload, a dict: {"scene_cut": True} for a frame
        that is a cut, {} else.  Refused by name without ``track_motion``, together with ``track_lookback`` or ``track_backtrack`` (their
        backward chains would have to stop at a cut) and on an engine whose foreign preprocess uploads float pixels.  Without it every
        key and byte is what it was.
        ``track_trails`` = (N, W) (tracking passes only, every form of them; ("trails", N, W) appended behind all the tags above; N 2..64
        points, W 1..9 pixels, an integer N or None in either place: ops.track_trails_option's defaults 16 and 3): the trail rule (DESIGN §8
        "Trail rule") draws the path of every id: one ops.track_trails_update behind the tracker call -- in a delayed pass behind the
        look-back / back-track call, over the EMITTED buffers and their count -- appends the centre of every live tracked row to the trail
        of its id in the engine's trail state (``track_trails_state``, emptied by ``track_reset()``), and each frame's trails are drawn
        (ops.track_trails_draw_u8) over its redaction and under its boxes and labels, in the colour of the id, the highest id on top.  A
        trail leaves (hold + 1) * K frames behind its last point (``track_trails_expire``), K = ``detect_every`` or 1.  The results are
        what they are without it: only the frames' bytes change.  Refused by name without ``track`` and with ``draw`` False; as every
        annotating pass, on an engine with a foreign preprocess.  Without it every key and byte is what it was.
        ``heat`` = (classes, A, S) (annotating passes, with every other option, ``draw`` False included; ("heat", classes, A, S) appended
        behind all the tags above; classes "all" or names, A the blend weight 1..255, S the decay 0..15, None for the defaults 160 and 0):
        the heat rule (DESIGN §8 "Heat rule") keeps where the objects of those classes have been: for each frame one ops.heat_update --
        every detection of a plain pass, the LIVE rows of a tracking pass (a ``detect_every`` between frame's propagated rows among them),
        in a delayed pass the EMITTED frames' -- into the engine's heat state of the frame size (``heat_state``; it lives across passes
        and submits until ``heat_reset()``; ``track_reset()`` leaves it), and one ops.heat_draw_u8 that blends the map into the frame over
        its redaction and under its trails, boxes and labels.  The map depends on the order of the frames: such passes replay in submit
        order on one stream, as tracking passes do, whatever ``in_flight`` is.  The results are what they are without it: only the
        frames' bytes change.  Refused by name without ``annotate``, on an engine with a foreign preprocess and for options out of
        range.  Without it every key and byte is what it was.
        ``count`` = (lines, classes, W) (tracking passes only, every form of them; ("count", lines, classes, W) appended behind all the
        tags above; lines 1..8 tuples (ax, ay, bx, by) in source-frame pixels, -32768..65535, A != B; classes "all" or names; W the width
        the lines are drawn with, 1..9, None: 3): the count rule (DESIGN §8 "Count rule") counts every id once per line and direction as
        the centre of its box crosses: one ops.count_update behind the tracker call -- in a delayed pass behind the look-back /
        back-track call, over the EMITTED buffers and their count, gated by the pass's own count, exactly where the trail update sits --
        steps the engine's count state (``count_state``; ``count_reset()`` zeroes it, ``track_reset()`` drops its entries and keeps the
        totals), and each frame's lines and labels "L{l} +{pos} -{neg}" are drawn (ops.count_draw_u8) over its redaction, heat and trails
        and under its boxes and labels; ``draw`` False still counts and draws no line.  The count lists come back with the dets: every
        result of such a pass carries, in ONE trailing dict (the one that carries "scene_cut"), "crossings": [(line, dir, id, cls), ...]
        -- dir 1 for +, cls the class index.  An entry leaves (hold + 1) * K frames behind its last step.  Refused by name without
        ``track`` and for options out of range.  Without it every key and byte is what it was.
        ``zone`` = (zones, classes, W, anchor) (tracking passes only, every form of them; ("zone", zones, classes, W, anchor) appended
        behind ("count", ...); zones 1..8 polygons of 3..16 (x, y) in source-frame pixels, -32768..65535; classes "all" or names; W the
        width of the outlines, 1..9, None: 3; anchor "centre" or "bottom"): the zone rule (DESIGN §8 "Zone rule"): one ops.zone_update
        behind the count update, over the same buffers, count and gate, steps the engine's zone state (``zone_state``; ``zone_reset()``
        zeroes it, ``track_reset()`` drops its entries and keeps the totals), and each frame's occupied zones are tinted and all
        outlines and labels "Z{z} {occupancy}/{visitors}" drawn (ops.zone_draw_u8) behind its heat map and under every line; ``draw``
        False still counts.  Every result of such a pass carries in its ONE trailing dict "zones": {"occupancy": [per zone],
        "events": [(zone, kind, id, cls, dwell)]}, kind 1 enter, 0 exit, 2 lost.  Refused by name without ``track`` and for options out
        of range.  Without it every key and byte is what it was.
        ``remove`` = (classes, S, T, M) (annotating passes, with every other option, without ``track`` too; ("remove", classes, S, T, M)
        appended behind ("zone", ...); classes "all" or names, S the settle 1..255, T the tolerance 0..255, M the margin 0..64, None for
        the PROVISIONAL defaults 8, 10 and 8, which nobody has measured on real footage): the plate rule (DESIGN §8 "Plate rule") paints
        the objects of those classes out.  For each frame one ops.plate_update learns the background from the untouched frame outside
        EVERY row of the buffer the edits read -- the packed detections of a plain pass, every tracked row of a tracking pass, held ones
        too, the emitted rows of a delayed pass, back-filled ones too -- into the engine's plate state of the frame size and channel
        order (``plate_state``; it lives across passes and submits until ``plate_reset()``; ``track_reset()`` leaves it; a
        ``track_scene_cut`` frame's cut word empties it), and one ops.plate_fill_u8 behind the redaction copies the plate into the boxes
        of the classes: where it is not known yet the redaction shows, if ``redact`` covers the classes, else black.  The plate depends
        on the order of the frames: such passes replay in submit order on one stream, as heat passes do.  An object that stands still
        and is never detected becomes background after S frames.  The results are what they are without it: only the frames' bytes
        change.  Refused by name without ``annotate``, on an engine with a foreign preprocess and for options out of range.  Without it
        every key and byte is what it was.
        ``track_reid`` = (pct, keep) (tracking passes, every form but the delayed ones; ("track_reid", pct, keep) appended last, behind
        ("remove", ...); pct 1..100, keep 1..4095 frames, None for the PROVISIONAL defaults 25 and 250, which nobody has measured on
        real footage): the re-identify rule (DESIGN §8 "Re-identify rule"): one ops.track_reid_update behind the tracker call gives a
        track whose colour signature lies within pct percent of that of an id the tracker gave up at most keep frames ago that id
        back, in the engine's re-identify state (``reid_state``; ``reid_reset()`` and ``track_reset()`` empty it; a
        ``track_scene_cut`` frame's cut word too).  Everything behind it -- trails, counts (whose entries then live max(expire, keep)
        frames), zones, labels, the "track_id" of the returned dets -- sees those ids.  Every result of such a pass carries in its ONE
        trailing dict "reid": [(pid, tid, cls, distance, gap)].  Refused by name without ``track``, with ``track_lookback`` /
        ``track_backtrack``, on an engine with a foreign preprocess and for options out of range.  Without it every key and byte is
        what it was.
        ``out_size`` = ("size", W, H) or ("scale", N) (annotating passes, with every other option; ("scale",) + the option appended LAST,
        behind ("track_reid", ...); N a divisor 2..16: H = ceil(h / N), W = ceil(w / N)): the scale rule (DESIGN §8 "Scale rule"): each
        frame, behind ALL its edits -- labels shrink with the picture --, is scaled down to (H, W) by the exact area mean (one
        ops.downscale_u8 into the slot's scaled area; with encode="y4m" one call over all frames behind the loop), and the scaled frame
        is what every encoder reads -- its bound and workspace are those of (H, W) -- and what a pass without an encoder copies back:
        ``collect_batch`` returns the (H, W, 3) frame.  A delayed pass scales the frames it emits.  The dets, the tracked rows and every
        list stay in SOURCE coordinates.  Refused by name, in front of any capture: without ``annotate``; a target the rule refuses for
        the pass's frame size (larger than it, less than 1/16 of it along a side, a side of 0); a size the pass's encoder refuses, with
        the encoder's own reason.  Without it every key and byte is what it was.
        ``redact_shape`` = (shape, feather) (passes with ``redact`` only; ("shape", shape, feather) appended directly behind ("redact",
        ...); shape "box" / "ellipse", feather 0..32 pixels, None in a place: "box", 0): the shape rule (DESIGN §8 "Shape rule"): the
        redaction step is ops.redact_shaped_u8 instead of ops.redact_u8 -- every box, held and back-filled ones too, hides the ellipse
        inscribed in it, NOT clipped to the frame, and the replacement fades out over ``feather`` pixels OUTSIDE the shape.  Nothing else
        of the pass knows: the plate steps, the tracker, the heat map and the drawn boxes keep their rectangles.  ("box", 0) and None ARE
        the pass without it: one spec, one key.  Refused by name, in front of any capture: without ``redact``, for an unknown shape and
        for a feather out of range.  Without it every key and byte is what it was.
        ``track_strong`` = T (tracking passes only, every form of them; ("weak", T) appended LAST, behind ("scale", ...); a float in
        0..1): the weak rule (DESIGN §8 "Weak rule"): the tracker call of the pass is its ``strong=T`` form.  ``det_threshold`` stays the
        value that is uploaded -- what the post-process emits down to, the LOW threshold --, and a row whose score is under T may only
        continue a track that no strong row continued; every other such row is dropped from the tracked buffer's live part.  The dets
        ``collect_batch`` returns for a frame are then the KEPT rows -- built from the tracked buffer's live rows, which carry bbox, cls
        and prob of the packed rows they came from, with their "track_id" --, so "num dets" and everything written from them show kept
        rows only; every consumer of the tracked buffer (redaction, plate, heat, trails, count, zone, reid, look-back, back-track,
        drawing) reads it as it is.  Refused by name without ``track`` and for a T outside 0..1.  Without it every key and byte is what
        it was.
        ``redact_region`` = (regions, mask, mode, size, feather) (annotating passes, with every other option, with and without ``redact``
        and ``track``; ("region", regions, the mask's digest or None, mode, size, feather) appended LAST, behind ("weak", ...); regions
        0..8 polygons in ``zone``'s grammar, mask None or a (h, w) uint8 array of the pass's SOURCE size whose bytes >= 128 hide, at
        least one of the two; mode "fill" / "pixelate" / "blur", None: "fill"; size None: the mode's default; feather 0..32, None: 0):
        the region rule (DESIGN §8 "Region rule") hides static areas whatever the detector says: one plane of weights per source size
        is built once in the engine's editing states, each frame's ops.redact_region_prepare reads the UNTOUCHED frame beside the plate
        update, and its ops.redact_region_apply_u8 blends behind the plate fill and under the heat map and everything drawn.  A
        delayed pass hides the areas in the frames it emits.  The results are what they are without it: only the frames' bytes change.
        Refused by name, in front of any capture: without ``annotate``, for values out of range, with neither polygons nor mask, and
        for a mask that is not the pass's source size.  Without it every key and byte is what it was.
        ``redact_moving`` = True, a dict of ops.redact_moving_option's keywords or its 12 values (annotating passes with the device
        preprocess, with every other option, with and without ``remove`` and ``track``; ("moving", D, K, H, G, F, unknown, EXCEPT, mode,
        size, S, T, M) appended LAST, behind ("region", ...); the defaults D 24, K 8, H 4, G 8 are PROVISIONAL, nobody has measured them on
        real footage): the moving rule (DESIGN §8 "Moving rule") hides whatever differs from the plate, detected or not.  Each frame's
        ops.redact_moving_build runs right behind its plate update -- which a pass without ``remove`` runs too, with the option's (S, T, M)
        and no fill; with ``remove`` the three are the remove option's -- into the engine's moving state of the frame size and channel
        order (``moving_state``; it lives across passes until ``moving_reset()``; ``track_reset()`` leaves it), and the frame is blended
        under the resulting plane behind the static regions and under everything drawn.  Like remove passes these replay in input order
        on the ordered stream and carry the real-frame count word; a delayed pass runs the net on the frames it emits.  Each result's
        trailing dict carries "moving": {"cells": n, "covered": n}.  Refused by name, in front of any capture: without ``annotate``,
        with a foreign preprocess, for values out of range and for an EXCEPT name that is no class.  Without it every key and byte is
        what it was.
        The order of all these steps in a pass is stated once, in ``frame_edit.EditChain``'s docstring."""
        spec = PassSpec.checked(self, batch, **options)            # (an unknown keyword: its TypeError)
        self._check_epoch()
        B = self.batch if batch is None else batch
        if spec.delayed and len(images) == 0:                       # the flush
            if self._lookback_last is None:
                raise FrcnnError("submit_batch: a flush (no images) follows a look-back submit; none is waiting")
            s = self.cache.acquire(*self._lookback_last)
            return self._replay(s, [], [], [], det_threshold)
        if spec.detect_every is not None:
            detect_every = spec.detect_every
            if not 1 <= len(pixels) <= B * detect_every or len(images) != -(-len(pixels) // detect_every) or len(images) != len(resize_ratios):
                raise FrcnnError("submit_batch: detect_every=%d with batch=%d takes 1..%d source frames in pixels and their key frames 0, %d, ... "
                                 "in images / resize_ratios: got %d frames, %d images, %d ratios"
                                 % (detect_every, B, B * detect_every, detect_every, len(pixels), len(images), len(resize_ratios)))
        else:
            assert 1 <= len(images) <= B and len(images) == len(pixels) == len(resize_ratios)
        _, H, W, src, flip = pixels[0]
        spec = spec.sized(self, B)
        spec.out_hw(src if src is not None else (H, W))            # (refuses a target this frame size or the encoder cannot take)
        spec.region_fits(src if src is not None else (H, W))       # (refuses a mask of another size)
        if spec.annotate:
            if not self.device_preprocess:
                raise FrcnnError("annotating passes need the device-side preprocess (a foreign preprocess_func uploads float pixels)")
            key = self.geometry_of(pixels[0])
            assert all(self.geometry_of(p) == key for p in pixels), "one pass, one geometry"
            key = key + spec.key_tail(B)
        else:
            key = self.geometry(pixels[0])
            assert all(self.geometry(p) == key for p in pixels), "one pass, one geometry"
            key = key + ((B,) if B > 1 else ())
        if key[0] == "canvas":
            s = self.cache.acquire(key, lambda: self._capture_slot(B, True, key[1], key[2]))
        else:
            capture = lambda: self._capture_slot(B, False, H, W, src, flip, spec)
            s = self.cache.acquire(key, capture)
            if spec.delayed:
                self._lookback_last = (key, capture)
        return self._replay(s, images, pixels, resize_ratios, det_threshold)

    def _replay(self, s, images, pixels, resize_ratios, det_threshold):
        """The upload, the replay and the read-back copies of one submit on slot ``s`` -> its ticket.  No images: a look-back pass's flush."""
        B = s.batch
        metas, files = [], []
        for i in range(B if images else 0):
            j = i if i < len(images) else 0
            s.dyn_host[i, 0], s.dyn_host[i, 1] = float(resize_ratios[j]), float(det_threshold)
        for i in range(s.frames if images else 0):                  # (B of them, but in a ``detect_every`` pass: every source frame goes up)
            j = i if i < len(pixels) else 0
            if isinstance(pixels[j][0], JpegFile):
                files.append((i, pixels[j][0]))
            if s.canvas:
                metas.append(self._canvas_frame(s, i, pixels[j]))
            elif not isinstance(pixels[j][0], JpegFile):
                np.copyto(s.pix_hosts[i], pixels[j][0], casting="same_kind")      # into pinned memory (f64 -> f32 cast for a foreign preprocess)
        if s.track or s.heat or s.remove or s.moving:               # (a heat, remove or moving pass too: their states depend on the order of the frames)
            s.n_frames_host[0] = len(pixels) if images else -1      # goes up with the frames: the padding does not advance the tracker; -1: a flush
            st = self.track_stream
        else:
            st = self._streams[self._seq % self.in_flight]
            self._seq += 1
        with torch.cuda.stream(st):
            if s.ready is not None:
                st.wait_event(s.ready)                             # (the first replay of a fresh pass: behind its warm-up)
                s.ready = None
            if files:
                self._stage_files(s, files)
            else:
                s.jpg_names = None
            s.io_dev.copy_(s.io_pin, non_blocking=True)
            if files:
                self._decode_files(s, files)                        # each file's frame into its source segment, behind the io copy
            if s.canvas:
                self._canvas_preprocess(s, metas)
            s.graph.replay()
            if files:
                s.jpg_status_pin.copy_(s.jpg_status, non_blocking=True)
            own = emitted = None
            if s.track_lookback:                                    # this pass returns the group its window held; its own group waits
                (in_h, in_w), lb_out = s.chain.hw, s.chain.lb_out
                own = {"images": list(images), "n_rois": None, "frames": len(pixels)} if images else None
                emitted = self._lookback_waiting.pop((in_h, in_w, s.frames), None)
                if own is not None:
                    self._lookback_waiting[(in_h, in_w, s.frames)] = own
                words = lb_out[1].numel()
                s.lb_pin[:words].copy_(lb_out[1].view(-1), non_blocking=True)
                s.lb_pin[words:].copy_(lb_out[2], non_blocking=True)
            for i in range(len(images)):
                s.out_pin[i].copy_(s.out_packed[i], non_blocking=True)
            for i in range(len(pixels) if s.track else 0):
                s.track_pin[i].copy_(s.chain.host_tracked[i], non_blocking=True)      # (with track_reid: the buffers with pids)
            if s.track_scene_cut:
                s.cuts_pin.copy_(s.chain.cuts, non_blocking=True)
            if s.count:                                             # the count lists come back with the dets
                s.count_pin.copy_(s.chain.count_lists, non_blocking=True)
            if s.zone:
                s.zone_pin.copy_(s.chain.zone_lists, non_blocking=True)
            if s.track_reid:
                s.reid_pin.copy_(s.chain.reid_lists, non_blocking=True)
            if s.moving:                                            # the frames' moving stats come back with the dets
                s.moving_pin.copy_(s.chain.moving_stats, non_blocking=True)
            for i in range(emitted["frames"] if emitted else 0 if s.track_lookback else len(pixels)):
                if s.encode == JPEG_ENCODE:
                    s.png_pin[i].copy_(s.png_dev[i][:s.first_copy], non_blocking=True)
                elif s.encode:
                    s.png_pin[i].copy_(s.png_dev[i], non_blocking=True)
                elif s.annotate:
                    s.frame_io[i][1].copy_(s.frame_io[i][0], non_blocking=True)
            s.event.record(st)
        s.busy = True
        return Ticket(s, list(images), own, emitted, len(pixels))

    def _stage_files(self, s, files):
        """Host side of a pass whose frames the device decodes: [item table | the files' bytes back to back] into the slot's one pinned
        area (grow-only; the slot is idle, so nothing reads the old one), room for them and for the decoder's workspace on the device.
        ``files``: (frame index, JpegFile) of the pass's file-backed frames; item k is files[k], its output frame i's source segment.  A
        file that fills several frames (the padding of a short group) is staged once."""
        B = s.frames
        kind_of = lambda f: 3 if isinstance(f, Y4mFile) else 2 if isinstance(f, PngFile) else int(isinstance(f.plan, _lib.JpegDecFullPlan))
        files.sort(key=lambda t: kind_of(t[1]))                     # (in place, stable: the baseline .jpg items, the progressive ones, the .png items, the y4m frames)
        nj, nf, npng = (sum(1 for _, f in files if kind_of(f) == k) for k in (0, 1, 2))
        item = ctypes.sizeof(_lib.JpegDecBatchItem)
        first_full = B * (item + ctypes.sizeof(_lib.PngDecFullBatchItem))      # [B JPEG items | B PNG items], room for the larger kind of PNG item
        # ... | B progressive items] only in a pass that holds such a file: their items are 5 KB each; ... | B y4m items] behind them
        first_y4m = self._first_y4m_item(B, nf)
        table = (first_y4m + B * ctypes.sizeof(_lib.Y4mBatchItem) + 255) // 256 * 256
        at, seen, file_off = 0, {}, []
        for _, f in files:
            if id(f) not in seen:
                seen[id(f)] = at
                at += len(f.data)
            file_off.append(seen[id(f)])
        if s.jpg_pin is None or s.jpg_pin.numel() < table + at:
            size = table + (at + at // 4 + 255) // 256 * 256
            s.jpg_pin = torch.empty(size, dtype=torch.uint8).pin_memory()
            s.jpg_area = torch.empty(size, dtype=torch.uint8, device="cuda")
        s.jpg_dev = s.jpg_area[table:]                               # the file area; the table lies in front of it
        plans = [f.plan for _, f in files]
        # one kind of PNG item per pass: with a full-format plan among them (png_decoder "device_full") revision-1 plans, which a pass
        # can only hold when the setting changed under way, are restated as full-format ones
        np_ = nj + nf                                                # the first .png item
        ny = np_ + npng                                              # the first y4m item
        full = any(isinstance(p, _lib.PngDecFullPlan) for p in plans[np_:ny])
        s.png_dec = ops.PNG_DECODERS["device_full" if full else "device"]
        if full:
            plans[np_:ny] = [ops.png_dec_full_of(p) if isinstance(p, _lib.PngDecPlan) else p for p in plans[np_:ny]]
        # per decoder: its items of the pass
        kinds = ((ops.JPEG_DECODER, 0, nj), (ops.JPEG_FULL_DECODER, nj, np_), (s.png_dec, np_, ny), (ops.Y4M_DECODER, ny, len(plans)))
        ws_off, need = [], 0
        for dec, lo, hi in kinds:
            for k in range(lo, hi, dec.batch_max):                  # (a call takes batch_max items: its regions behind the last call's)
                offs, total = dec.layout(plans[k:min(hi, k + dec.batch_max)])
                ws_off += [need + o for o in offs]
                need += total
        if s.jpg_ws is None or s.jpg_ws.numel() < need:
            s.jpg_ws = torch.empty(need + need // 4, dtype=torch.uint8, device="cuda")
        if s.jpg_status is None:
            s.jpg_status = torch.zeros(B, dtype=torch.int32, device="cuda")
            s.jpg_status_pin = torch.zeros(B, dtype=torch.int32).pin_memory()
        out_off = [i * s.seg for i, _ in files]
        # (a palette lies behind its stream in the file's staged bytes: DeviceDecoder.items)
        s.jpg_items, s.full_items, s.png_items, s.y4m_items = (dec.items(plans[lo:hi], file_off[lo:hi], out_off[lo:hi], ws_off[lo:hi])
                                                               for dec, lo, hi in kinds)
        s.jpg_count = nj
        s.jpg_decs = [dec for dec, lo, hi in kinds for _ in range(lo, hi)]     # item k's decoder
        s.jpg_used = table + at
        s.jpg_names = [f.name for _, f in files]                    # (item k's status word is word k, in the order of ``kinds``)
        host = s.jpg_pin.numpy()
        for items, first in ((s.jpg_items, 0), (s.png_items, B * item), (s.full_items, first_full), (s.y4m_items, first_y4m)):
            if len(items):
                host[first:first + ctypes.sizeof(items)] = np.frombuffer(items, dtype=np.uint8)
        for f in {id(f): f for _, f in files}.values():
            host[table + seen[id(f)]:table + seen[id(f)] + len(f.data)] = np.frombuffer(f.data, dtype=np.uint8)

    @staticmethod
    def _first_y4m_item(B, progressive):
        """Where the y4m items lie in a slot's staged table: behind the JPEG, the PNG and (in a pass that holds one) the progressive items."""
        return B * (ctypes.sizeof(_lib.JpegDecBatchItem) + ctypes.sizeof(_lib.PngDecFullBatchItem)
                    + (ctypes.sizeof(_lib.JpegDecFullBatchItem) if progressive else 0))

    def _decode_files(self, s, files):
        """Device side, on the pass's stream between the io copy and the canvas preprocess / the replay: one upload of the staged area,
        the status words cleared, one batched decode of every file into its frame's source segment (R,G,B as PIL delivers it: the pass's
        resize swaps, flip bit 1).  FRCNN_ENTRY_JPEG_BATCH=0: an upload and a single-file decode per file instead."""
        item, table = ctypes.sizeof(_lib.JpegDecBatchItem), s.jpg_area.numel() - s.jpg_dev.numel()
        nj, batched = s.jpg_count, jpeg_batch()
        if batched or len(files) > nj:                              # (the progressive and the .png items are always decoded as a batch)
            s.jpg_area[:s.jpg_used].copy_(s.jpg_pin[:s.jpg_used], non_blocking=True)
        s.jpg_status.zero_()
        # per decoder: its items, its first status word, where its items lie in the staged area; the .png items' launches go first
        first_full = s.frames * (item + ctypes.sizeof(_lib.PngDecFullBatchItem))
        for dec, items, word, first in ((ops.Y4M_DECODER, s.y4m_items, nj + len(s.full_items) + len(s.png_items),
                                         self._first_y4m_item(s.frames, len(s.full_items))),
                                        (s.png_dec, s.png_items, nj + len(s.full_items), s.frames * item),
                                        (ops.JPEG_FULL_DECODER, s.full_items, nj, first_full), (ops.JPEG_DECODER, s.jpg_items, 0, 0)):
            if dec is ops.JPEG_DECODER and not batched:
                continue
            size = ctypes.sizeof(dec.item_type)
            for k in range(0, len(items), dec.batch_max):
                n = min(dec.batch_max, len(items) - k)
                part = (dec.item_type * n).from_buffer(items, k * size)
                dec.decode(s.jpg_dev, part, s.io_dev, status=s.jpg_status[word + k:word + k + n], workspace=s.jpg_ws,
                           items_dev=s.jpg_area[first + k * size:first + (k + n) * size])
        if batched:
            return
        for k, (i, f) in enumerate(files[:nj]):
            it = s.jpg_items[k]
            lo, n, frame = table + int(it.file_off), len(f.data), int(f.plan.h) * int(f.plan.w) * 3
            s.jpg_area[lo:lo + n].copy_(s.jpg_pin[lo:lo + n], non_blocking=True)
            out = s.io_dev[i * s.seg:i * s.seg + frame].view(int(f.plan.h), int(f.plan.w), 3)
            ops.jpeg_decode_u8(s.jpg_area[lo:lo + n], f.plan, out=out, status=s.jpg_status[k:k + 1], workspace=s.jpg_ws)

    def _canvas_frame(self, s, i, pixels):
        """Frame i of a canvas pass, host side: the frame goes into its staging segment at ITS size, its true size into the extents.
        -> what _canvas_preprocess needs to know about it."""
        arr, H, W, src, flip = pixels
        oy, ox = s.extents.offset_of(H, W)                          # ResNet: (H & 1, W & 1); VGG16: (0, 0)
        _, Hc, Wc = s.key
        if isinstance(arr, JpegFile):                               # the device decodes it into the segment (_decode_files): only its size here
            in_h, in_w = int(arr.plan.h), int(arr.plan.w)
            assert in_h * in_w * 3 <= s.seg and H + oy <= Hc and W + ox <= Wc, "one pass, one canvas class"
        else:
            arr = np.ascontiguousarray(arr)
            in_h, in_w = arr.shape[0], arr.shape[1]
            assert arr.dtype == np.uint8 and arr.nbytes <= s.seg and H + oy <= Hc and W + ox <= Wc, "one pass, one canvas class"
            s.pix_hosts[i][:arr.nbytes] = arr.reshape(-1)
        s.extents.set(i, H, W)
        return in_h, in_w, H, W, src, flip, (oy, ox)

    def _canvas_preprocess(self, s, metas):
        """The eager launches in front of a canvas pass's replay, on its stream: the true sizes go up as extents, every frame is resized
        (and flipped) to ITS (H, W) and preprocessed into the corner of its canvas."""
        s.extents.upload()
        for i, (in_h, in_w, H, W, src, flip, offset) in enumerate(metas):
            frame = s.io_dev[i * s.seg:i * s.seg + in_h * in_w * 3].view(in_h, in_w, 3)
            if src is not None:                                     # shapes.Image.data: INTER_CUBIC resize (+ flip) of the decoded frame
                frame = ops.resize_cubic_u8(frame, H, W, flip=flip, tabs=(self._device_taps(W, in_w), self._device_taps(H, in_h)),
                                            out=s.u8_resized[i][:H * W * 3].view(H, W, 3))
            ops.preprocess_u8_canvas(frame, MEAN_BGR, s.x_f32[i], offset=offset)

    def collect_batch(self, ticket):
        """-> [(num_rois, dets)] for the images of a ``submit_batch`` ticket; [(num_rois, dets, frame)] for an annotating one, ``frame``
        the annotated source frame (uint8 (h, w, 3), in the channel order it was uploaded in); [(num_rois, dets, png)] for one that
        encodes, ``png`` the annotated frame as the bytes of a PNG file (RGB), or of a JPEG file for encode="jpeg"."""
        s = ticket.slot
        try:
            s.event.synchronize()
            rev = self.rev_class_mapping
            res = []
            if s.jpg_names:
                words = s.jpg_status_pin.numpy()
                for i, name in enumerate(s.jpg_names):
                    if name is not None and int(words[i]):          # (the .jpg items' words, then the .png items')
                        ops.raise_damaged(s.jpg_decs[i], int(words[i]), name)
            if s.amax is not None and ticket.image:          # (a look-back flush brings no image: its pass's detections are not read, nor copied back)
                bits = int(s.out_pin[0].numpy()[2])                 # the pass's f16x3 status word (pipeline._pass_status)
                if bits:
                    raise FrcnnError("f16x3 pass not trustworthy (%s): status %d; run the image on the native or bf16x6 engine" % (ops.h3_status_text(bits), bits))
            if s.track_lookback:
                return self._collect_lookback(ticket)
            K = s.every or 1
            for f in range(ticket.frames):
                if f % K:                                           # a between frame of a ``detect_every`` pass: its dets are the tracks
                    _, _, dets = ops.tracked_dets(s.track_pin[f].numpy(), rev, propagated=True)
                    res.append((0, dets) + self._payload(s, f) + self._marks(s, f))
                    continue
                i = f // K
                packed = s.out_pin[i].numpy()
                nd, n_rois = int(packed[0]), int(packed[1])
                if s.track and s.spec.track_strong is not None:    # the weak rule: the dets are the rows of the tracked buffer, the kept ones
                    n_live, _, dets = ops.tracked_dets(s.track_pin[f].numpy(), rev)      # first, then the held (as a delayed pass reads its own)
                    if n_live > nd:
                        raise FrcnnError("tracker: %d live rows for %d detections" % (n_live, nd))
                    res.append((n_rois, dets) + self._payload(s, f) + self._marks(s, f))
                    continue
                rows = (packed.size - 4) // 7
                bbox = packed[4:4 + 4 * nd].reshape(nd, 4).astype(np.int64)
                cls = packed[4 + 4 * rows:4 + 4 * rows + nd].copy()
                prob = packed[4 + 5 * rows:4 + 5 * rows + nd].view(np.float32).copy()
                dets = [{"bbox": bbox[k], "cls_name": rev[int(cls[k])], "prob": prob[k]} for k in range(nd)]
                if s.track:                                         # the live rows' ids, then the held rows
                    n_live, ids, held = ops.tracked_dets(s.track_pin[f].numpy(), rev, start=nd)
                    if n_live != nd:
                        raise FrcnnError("tracker: %d live rows for %d detections" % (n_live, nd))
                    for k in range(nd):
                        dets[k]["track_id"] = int(ids[k])
                    dets += held
                res.append((n_rois, dets) + self._payload(s, f) + self._marks(s, f))
            return res
        finally:
            s.busy = False                               # whatever happened while decoding the records: the slot is free again

    @staticmethod
    def _marks(s, i):
        """What frame i of a collected ``track_scene_cut``, ``count`` or ``zone`` pass returns behind its payload: ONE dict -- "scene_cut":
        True for a frame that is a cut, "crossings": [(line, dir, id, cls)] in a counting pass (the events of the frame's count list, dir 1
        for +), "zones": {"occupancy": [per zone], "events": [(zone, kind, id, cls, dwell)]} in a zone pass (the frame's zone list), "reid":
        [(pid, tid, cls, distance, gap)] in a ``track_reid`` pass (the frame's reid list), "moving": {"cells", "covered"} in a
        ``redact_moving`` pass (the frame's moving stats) --;
        () for every other pass."""
        if not s.track_scene_cut and not s.count and not s.zone and not s.track_reid and not s.moving:
            return ()
        marks = {"scene_cut": True} if s.track_scene_cut and int(s.cuts_pin[i]) else {}
        if s.count:
            marks["crossings"] = ops.count_events(s.count_pin[i].numpy())
        if s.zone:                                       # "zones": the frame's occupancy per zone and its events (zone, kind, id, cls, dwell)
            zlist = s.zone_pin[i].numpy()
            marks["zones"] = {"occupancy": ops.zone_occupancy(zlist, len(s.zone[0])), "events": ops.zone_events(zlist)}
        if s.track_reid:                                 # "reid": the frame's re-identifications (pid, tid, cls, distance, gap)
            marks["reid"] = ops.track_reid_events(s.reid_pin[i].numpy())
        if s.moving:                                     # "moving": the moving cells of the frame and the pixels hidden under its plane
            stats = s.moving_pin[i].numpy()
            marks["moving"] = {"cells": int(stats[1]), "covered": int(stats[2])}
        return (marks,)

    def _payload(self, s, i):
        """What frame i of a collected pass returns behind (num_rois, dets): () , (the frame,) or (the encoded file's bytes,)."""
        if s.encode == JPEG_ENCODE:
            row = s.png_pin[i].numpy()
            n = int(row[0:4].view(np.int32)[0])
            if not 0 < n <= s.png_bound:
                raise FrcnnError("device JPEG encoder: length word %d outside (0, %d]" % (n, s.png_bound))
            data = row[16:min(16 + n, s.first_copy)].tobytes()
            if 16 + n > s.first_copy:               # a file longer than the first copy: its remainder now (synchronous)
                data += s.png_dev[i][s.first_copy:16 + n].cpu().numpy().tobytes()
            return (data,)
        elif s.encode == Y4M_ENCODE:
            return (s.png_pin[i].numpy().tobytes(),)      # the frame's record: a fixed size, no length word
        elif s.encode:
            row = s.png_pin[i].numpy()
            n = int(row[-16:-12].view(np.int32)[0])
            if not 0 < n <= s.png_bound:
                raise FrcnnError("device PNG encoder: length word %d outside (0, %d]" % (n, s.png_bound))
            return (row[:n].tobytes(),)
        else:
            return ((s.pix_out or s.pix_hosts)[i].copy(),) if s.annotate else ()

    def _collect_lookback(self, ticket):
        """``collect_batch`` of a look-back pass: this submit's num_rois are kept for the pass that will emit its frames, and the results
        are those of the group this pass emitted, read from the emitted tracked buffers."""
        s, rev = ticket.slot, self.rev_class_mapping
        if ticket.own is not None:
            ticket.own["n_rois"] = [int(s.out_pin[i].numpy()[1]) for i in range(len(ticket.image))]
        group = ticket.emitted
        if group is None:
            return []
        if group["n_rois"] is None:
            raise FrcnnError("collect_batch: look-back tickets are collected in submit order")
        lb = s.lb_pin.numpy()
        words = (lb.size - 4) // s.frames
        if int(lb[-4]) != group["frames"]:
            raise FrcnnError("look-back window: %d frames emitted for a group of %d" % (int(lb[-4]), group["frames"]))
        K = s.every or 1                                            # (a ``track_backtrack`` pass: one result per source frame)
        res = []
        for i in range(group["frames"]):
            _, _, dets = ops.tracked_dets(lb[i * words:(i + 1) * words], rev, propagated=bool(i % K))
            res.append((0 if i % K else group["n_rois"][i // K], dets) + self._payload(s, i) + self._marks(s, i))
        return res

    def collect(self, ticket):
        return self.collect_batch(ticket)[0]

    def stats(self):
        c = self.cache
        post = {} if self.post is None else {"post": dict(zip(ops.DET_POST_FIELDS, self.post))}      # (only an engine that has the option says so)
        return {**post, "graphs": len(c), "sizes": len(c.keys()), "bytes": c.nbytes, "byte_budget": c.byte_budget, "captures": c.captures,
                "hits": c.hits, "evictions": c.evictions, "capture_seconds": round(self.capture_seconds, 3), "in_flight": self.in_flight,
                "device_preprocess": self.device_preprocess, "f32_engine": self.f32_engine, "images_per_pass": self.batch,
                "canvas_slots": {"%dx%d" % k[1:3]: v for k, v in self._canvas_slots.items()},      # canvas class "HcxWc" -> captured passes its plan allows
                "capture_breakdown_ms": {k: round(v, 1) for k, v in self.capture_breakdown.items()}}


def for_models(manager, detector, num_rois=64, stride=16, in_flight=1, post=None):
    """The DetectionEntry of this (manager, detector, num_rois, stride, in_flight[, post]), built on first use and kept on the
    manager; None when the pair cannot take the captured path (voc_dets then runs the eager one).  ``post``: the post-process option
    (ops.det_post_option); an engine with it is a table entry of its own beside the one without."""
    if not torch.cuda.is_available() or not DetectionEntry.usable(manager, detector, num_rois):
        return None
    table = manager.__dict__.setdefault("_entries", {})
    key = (id(detector), int(num_rois), stride, int(in_flight))
    if post is not None:
        post = ops.det_post_option(post)
        key += (post,)
    eng = table.get(key)
    if eng is None or eng.detector is not detector:
        global _QUEUES_SAID
        if not _QUEUES_SAID and in_flight > 1 and int(os.environ.get("GPU_MAX_HW_QUEUES", "4")) < 8:
            _QUEUES_SAID = True
            import warnings
            warnings.warn("faster_rcnn_amd.entry: this process runs on %s hardware queues (GPU_MAX_HW_QUEUES; ROCm's default is 4): get_dets_by_cls measures "
                          "~9 %% slower there than on 8 (497 against 542-547 img/s).  The setting is read when the HIP runtime starts: export "
                          "GPU_MAX_HW_QUEUES=8 before the first device call, as voc_dets.main does." % os.environ.get("GPU_MAX_HW_QUEUES", "4"))
        eng = table[key] = DetectionEntry(manager, detector, num_rois, stride, in_flight, post=post)
    return eng


_QUEUES_SAID = False
