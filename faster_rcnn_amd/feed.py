"""Device-side feed of the training managers' fast paths (rpn_util.RpnTrainingManager, det_util.DetTrainingManager).

The reference hands ``train_on_batch`` host arrays: ``np.expand_dims(preprocess_func(image.data), 0)`` -- a float64 (1,H,W,3)
array, 14 MB for a 600x1000 frame (rpn_util.py:50-51, det_util.py:35-36) -- and the step's feed casts it to float32 and uploads
it.  When the manager's ``preprocess_func`` is one of this package's mean subtractions (resnet.preprocess / vgg.preprocess) the
same float32 tensor is produced ON the device from the decoded uint8 frame: one 0.6-1.8 MB upload, the INTER_CUBIC resize and
flip of ``shapes.Image.data`` (frcnn_resize_cubic_u8, the same integers as the host restatement) and frcnn_preprocess_u8 (bit for
bit float32(float64(pixel) - mean)).  tests/test_train_loop_gpu.py holds the two feeds to the same bits.
"""
import os
import numpy as np
import torch

from . import ops
from .shapes import declares as _declares

MEAN_BGR = (103.939, 116.779, 123.68)           # resnet.preprocess / vgg.preprocess (resnet.py:64-75, vgg.py:52-57)
RGB_UPLOAD = os.environ.get("FRCNN_FEED_RGB_UPLOAD", "1") != "0"
JPEG_DECODERS = ("host", "device", "device_full")


def jpeg_decoder_option(value, what):
    """A decoder setting ("host": PIL, the default; "device": ops.jpeg_decode_u8 for the files its planner supports, PIL for the rest;
    "device_full": as "device", and ops.jpeg_decode_full_batch_u8 for the progressive files ITS planner supports, PIL for the rest)
    checked: -> the value, ValueError naming ``what`` (an environment variable, an option) for anything else."""
    value = "host" if value is None or value == "" else value
    if value not in JPEG_DECODERS:
        raise ValueError("%s=%r: one of %s" % (what, value, ", ".join(JPEG_DECODERS)))
    return value


def default_jpeg_decoder():
    """FRCNN_FEED_JPEG_DECODER: who decodes a file-backed frame for ``device_image`` (read at every call: a test may set it)."""
    return jpeg_decoder_option(os.environ.get("FRCNN_FEED_JPEG_DECODER"), "FRCNN_FEED_JPEG_DECODER")


def plan_file(image, full=None):
    """(the file's bytes, its decode plan) of a file-backed image the device decoder supports, else None (in-memory pixels, no
    ``raw_file``, a file outside the supported set: the caller takes the host path).  ``full`` (None: FRCNN_FEED_JPEG_DECODER is
    "device_full"): a file the baseline planner refuses goes to the progressive planner (-> a ``_lib.JpegDecFullPlan``) before it is
    given up.  Pure host work: a thread may do it ahead."""
    if not _declares(image, "raw_file") or getattr(image, "_pixels", None) is not None:
        return None
    data = image.raw_file()
    if data is None:
        return None
    try:
        return data, ops.jpeg_dec_plan(data)
    except ops.JpegUnsupported:
        pass
    if default_jpeg_decoder() == "device_full" if full is None else full:
        try:
            return data, ops.jpeg_dec_full_plan(data)
        except ops.JpegUnsupported:
            pass
    return None


PNG_DECODERS = ("host", "device", "device_full")


def default_png_decoder():
    """FRCNN_FEED_PNG_DECODER: who decodes a file-backed .png frame for ``device_image`` (read at every call: a test may set it)."""
    return png_decoder_option(os.environ.get("FRCNN_FEED_PNG_DECODER"), "FRCNN_FEED_PNG_DECODER")


def png_decoder_option(value, what):
    """A PNG decoder setting ("host": PIL, the default; "device": ops.png_decode_batch_u8 for the files its planner supports, PIL for the
    rest; "device_full": ops.png_decode_full_batch_u8, whose planner also takes palette, 1/2/4/16-bit, grey + alpha and Adam7 files) checked: -> the value, ValueError naming ``what`` (an environment variable, an option) for anything else."""
    value = "host" if value is None or value == "" else value
    if value not in PNG_DECODERS:
        raise ValueError("%s=%r: one of %s" % (what, value, ", ".join(PNG_DECODERS)))
    return value


def plan_png(data, mode="device"):
    """(what goes to the device of a .png file's bytes: its zlib stream, the IDAT payloads back to back, followed under "device_full" for a
    palette file by its 768 staged palette bytes: item.plte_off = item.file_off + plan.stream_len; its decode plan) under the PNG decoder
    setting ``mode`` ("device": a ``PngDecPlan``; "device_full": a ``PngDecFullPlan``), or None for a file that decoder's planner
    refuses.  Pure host work."""
    dec = ops.PNG_DECODERS[mode]
    try:
        plan = dec.plan(data)
    except ops.PngUnsupported:
        return None
    return dec.stage(data, plan), plan


def plan_png_full(data):
    """``plan_png`` under "device_full"."""
    return plan_png(data, "device_full")


def plan_entry_file(image, jpeg=True, png=False):
    """``plan_file`` for the detection entry, which may decode either kind on the device: a file-backed image whose bytes start with
    the PNG signature is planned by the PNG decoder ``png`` names (a PNG decoder setting; True stands for "device", "full" for
    "device_full", False for "host") -> ``plan_png``'s pair; what an ``annotate_video._FileFrame`` planned ahead under the same setting
    is taken as it is), any other file by ``plan_file`` when ``jpeg`` (a JPEG decoder setting, or True for "device" and False for
    "host").  None: the caller takes the host path.  (``device_image``, the
    training feed, plans through ``plan_feed_file``.)"""
    return _plan_by_settings(image, {True: "device", False: "host"}.get(jpeg, jpeg), {True: "device", "full": "device_full", False: "host"}.get(png, png))


def plan_feed_file(image):
    """``plan_file`` for the training feed under its two settings: a file that starts with the PNG signature is planned by the PNG
    planner FRCNN_FEED_PNG_DECODER names (-> ``plan_png``'s pair), any other file by ``plan_file`` when
    FRCNN_FEED_JPEG_DECODER is "device" or "device_full".  None: in-memory pixels, no ``raw_file``, a setting of "host" for that kind of file, or a file
    the planner refuses: the caller takes the host path.  Pure host work: a thread may do it ahead."""
    return _plan_by_settings(image, default_jpeg_decoder(), default_png_decoder())


def _plan_by_settings(image, jpeg, png):
    full = jpeg == "device_full"
    jpeg = jpeg != "host"
    if png == "host":
        return plan_file(image, full) if jpeg else None
    if not _declares(image, "raw_file") or getattr(image, "_pixels", None) is not None:
        return None
    data = image.raw_file()
    if data is None:
        return None
    if bytes(data[:8]) == ops.PNG_SIGNATURE:
        planned = getattr(image, "png_planned", None)
        if planned is not None and ops.decoder_of(planned[1]).setting == png:
            return planned
        return plan_png(data, png)
    return plan_file(image, full) if jpeg else None


def _still_wanted(plan):
    """Does the setting that was in force when a file was planned ahead still hold?"""
    dec = ops.decoder_of(plan)
    if dec.label == "PNG":
        return default_png_decoder() == dec.setting
    return default_jpeg_decoder() in ("device_full",) + (("device",) if dec.setting == "device" else ())    # ("device_full" keeps the baseline decoder)


class _PinRing:
    """A few grow-only pinned staging areas used in turn: ``upload(array)`` copies the array into the next one and starts an
    ASYNCHRONOUS copy to the device on the current stream (a pageable source makes the runtime stage the bytes itself and block the
    host for the whole transfer: 0.25 ms for a 1.8 MB frame, on a loop whose iteration is 2 ms).  An area is reused only after the
    copy out of it has finished (its event)."""

    def __init__(self, n=6):
        self.slots = [[None, None] for _ in range(n)]
        self.i = 0

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        k, self.i = self.i, (self.i + 1) % len(self.slots)
        slot = self.slots[k]
        if slot[1] is not None:
            slot[1].synchronize()
        nbytes = max(arr.nbytes, 16)
        if slot[0] is None or slot[0].numel() < nbytes:
            slot[0] = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8).pin_memory()
            slot[1] = torch.cuda.Event()
        pin = slot[0][:arr.nbytes]
        np.copyto(pin.numpy().view(arr.dtype).reshape(arr.shape), arr)
        dev = pin.view(_TORCH_DTYPE[arr.dtype.type]).view(arr.shape).to("cuda", non_blocking=True)
        slot[1].record()
        return dev

    def host_slot(self, shape, dtype):
        """A pinned host tensor for a device -> host copy (e.g. two counters), valid until the ring comes round again."""
        k, self.i = self.i, (self.i + 1) % len(self.slots)
        slot = self.slots[k]
        if slot[1] is not None:
            slot[1].synchronize()
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        if slot[0] is None or slot[0].numel() < n:
            slot[0] = torch.empty(max(256, n), dtype=torch.uint8).pin_memory()
            slot[1] = torch.cuda.Event()
        return slot[0][:n].view(dtype).view(shape), slot[1]


_TORCH_DTYPE = {np.uint8: torch.uint8, np.int32: torch.int32, np.float32: torch.float32, np.int16: torch.int16, np.float64: torch.float64}
_RING = None


def ring():
    global _RING
    if _RING is None:
        _RING = _PinRing()
    return _RING


def upload(arr):
    """numpy array -> device tensor through pinned staging, asynchronous on the current stream."""
    return ring().upload(arr)


def device_preprocess(preprocess_func):
    from . import resnet, vgg
    return preprocess_func in (resnet.preprocess, vgg.preprocess)


# The JPEG decode of a file-backed frame (1.0 ms for a 500 x 375 VOC image) on the training loop's thread made a mixed-precision RPN iteration
# host-bound: 1.45 ms from files against 1.03 from memory.  train_util's loops name the image TWO iterations ahead (when fetching it needs no
# shuffle) and ONE background thread decodes it -- PIL releases the interpreter lock inside its decoder -- while the loop enqueues the
# step between.  FRCNN_FEED_DECODE_AHEAD=0: decode on the loop's thread.
DECODE_AHEAD = os.environ.get("FRCNN_FEED_DECODE_AHEAD", "1") != "0"
_DECODER = None
_DECODED = {}                                    # id(image) -> (image, Future of its raw_rgb)


def decode_ahead(image):
    """Start decoding a file-backed image's pixels on the background thread (device_image picks the result up).  With the device decoder
    the thread reads the file and plans it instead; an unsupported file is decoded there as before."""
    global _DECODER
    device = default_jpeg_decoder() != "host" or default_png_decoder() != "host"
    if not (DECODE_AHEAD and RGB_UPLOAD and hasattr(type(image), "raw_rgb")) or getattr(image, "_pixels", 0) is not None or id(image) in _DECODED:
        return
    if _DECODER is None:
        from concurrent.futures import ThreadPoolExecutor
        _DECODER = ThreadPoolExecutor(max_workers=1, thread_name_prefix="frcnn-decode")
    if len(_DECODED) > 8:
        _DECODED.clear()                                      # (frames asked for and never taken: forget them)
    def work():
        planned = plan_feed_file(image) if device else None
        return planned if planned is not None else image.raw_rgb
    _DECODED[id(image)] = (image, _DECODER.submit(work))


def _raw_rgb(image):
    """The decoded RGB frame, or with the device decoder (file bytes, plan) for a supported file."""
    ent = _DECODED.pop(id(image), None)
    if ent is not None and ent[0] is image:
        got = ent[1].result()
        if not isinstance(got, tuple) or _still_wanted(got[1]):
            return got
        return image.raw_rgb                                  # (planned ahead, and the setting changed since)
    planned = plan_feed_file(image)
    if planned is not None:
        return planned
    return image.raw_rgb


# Device decodes whose status word has not been looked at: (pinned int32 [1], event behind its copy, file name, its ops.DeviceDecoder).  ``check_decodes`` is
# called where a training manager has just synchronised for its own counts: it reads the words whose copy has FINISHED and waits for none.
_DECODE_STATUS = []
_STATUS_PIN, _STATUS_AT = None, 0


def _decode_on_device(data, plan, name):
    """The file decoded on the current stream -> (h, w, 3) uint8 R,G,B device tensor; its status word is queued for check_decodes."""
    dec = ops.decoder_of(plan)
    if dec.label == "PNG" or dec is ops.JPEG_FULL_DECODER:      # (a batch of one: the plan is too large to travel by value)
        rgb, status = _decode_png_on_device(dec, data, plan)
    else:
        file_dev = upload(np.frombuffer(data, dtype=np.uint8))
        rgb, status = ops.jpeg_decode_u8(file_dev, plan)
    global _STATUS_PIN, _STATUS_AT
    if _STATUS_PIN is None:
        _STATUS_PIN = torch.zeros(64, dtype=torch.int32).pin_memory()
    if len(_DECODE_STATUS) >= 32:                             # (nobody called check_decodes: the oldest word's place is needed again)
        _DECODE_STATUS[0][1].synchronize()
        check_decodes()
    word, _STATUS_AT = _STATUS_PIN[_STATUS_AT:_STATUS_AT + 1], (_STATUS_AT + 1) % 64
    word.copy_(status, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    _DECODE_STATUS.append((word, ev, name, dec))
    return rgb


def _decode_png_on_device(dec, data, plan):
    """A planned .png file (``plan_png``'s pair, made for the decoder ``dec``), or a progressive .jpg file, as a batch of one: ONE upload through the pin ring of [the
    item | the zlib stream | the palette], the decode on the current stream -> ((h, w, 3) uint8 R,G,B device tensor, its status word [1])."""
    import ctypes
    head = (ctypes.sizeof(dec.item_type) + 15) // 16 * 16
    items = dec.items([plan], [0], [0], dec.layout([plan])[0])
    staged = np.empty(head + len(data), np.uint8)
    staged[:ctypes.sizeof(items)] = np.frombuffer(items, dtype=np.uint8)
    staged[head:] = np.frombuffer(data, dtype=np.uint8)
    dev = upload(staged)
    rgb = torch.empty((int(plan.h), int(plan.w), 3), dtype=torch.uint8, device="cuda")
    status = dec.decode(dev[head:], items, rgb.view(-1), status=torch.zeros(1, dtype=torch.int32, device="cuda"), items_dev=dev[:head])
    return rgb, status


def check_decodes():
    """Raise FrcnnError for a device decode that reported a damaged file.  Never waits: a word still in flight stays for the next call."""
    if not _DECODE_STATUS:
        return
    waiting, bad = [], None
    for word, ev, name, dec in _DECODE_STATUS:
        if not ev.query():
            waiting.append((word, ev, name, dec))
        elif int(word[0]) and bad is None:
            bad = (dec, int(word[0]), name)
    _DECODE_STATUS[:] = waiting
    if bad is not None:
        ops.raise_damaged(*bad)


def device_image(image, preprocess_func):
    """(1,H,W,3) float32 device tensor == float32(np.expand_dims(preprocess_func(image.data), 0)), on the current stream."""
    if device_preprocess(preprocess_func) and _declares(image, "raw") and _declares(image, "height"):
        H, W, flip = int(image.height), int(image.width), bool(getattr(image, "flipped", False))
        # a file-backed frame goes up in the decoder's channel order (R,G,B: PIL's, the device JPEG decoder's and the device PNG decoders'); the device resize (to its own size when none is needed: a
        # copy) writes B, G, R -- the host's channel reversal cost as much as half the decode (round 6, as entry.DetectionEntry)
        rgb = _raw_rgb(image) if (RGB_UPLOAD and hasattr(type(image), "raw_rgb")) else None
        if isinstance(rgb, tuple):                               # (file bytes, plan): decoded on the device into what the resize reads
            dev = _decode_on_device(rgb[0], rgb[1], getattr(image, "_image_path", None) or getattr(image, "name", "?"))
            return ops.preprocess_u8(ops.resize_cubic_u8(dev, H, W, flip=2 | int(flip)), MEAN_BGR)
        if rgb is not None:
            rgb = np.asarray(rgb)
            if rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3:
                return ops.preprocess_u8(ops.resize_cubic_u8(upload(rgb), H, W, flip=2 | int(flip)), MEAN_BGR)
        raw = np.asarray(image.raw)
        if raw.dtype == np.uint8 and raw.ndim == 3 and raw.shape[2] == 3:
            if raw.shape[0] != H or raw.shape[1] != W:
                u8 = ops.resize_cubic_u8(upload(raw), H, W, flip=flip)
            else:
                u8 = upload(raw[:, ::-1] if flip else raw)
            return ops.preprocess_u8(u8, MEAN_BGR)
    x = np.expand_dims(preprocess_func(image.data), axis=0)
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    return t if t.dim() == 4 else t.unsqueeze(0)


class Ready:
    """Marks device tensors produced on a side stream: ``tensor._ready`` is an event the consuming streams wait for
    (train._StepDriver._run_step), and the tensors are registered with those streams so the caching allocator does not recycle them
    under a kernel that still reads them."""

    @staticmethod
    def mark(*tensors):
        ev = torch.cuda.Event()
        ev.record()
        for t in tensors:
            t._ready = ev
        return tensors


# ---- the stream the training managers' device work runs on (rpn_util.RpnTrainingManager, det_util.DetTrainingManager).  ONE per process,
# and one that shares a hardware queue with NEITHER the caller's stream NOR the training step's weight-gradient and prefix streams.
# HIP deals its hardware queues (GPU_MAX_HW_QUEUES, 4 by default) to streams as they are created; once they are taken, streams share.
# A manager stream that shares with the weight-gradient stream has its launches -- and the event the host waits on for the sampling
# counts -- queued behind the previous step's batched weight gradients: 2.7 ms per fp32 RPN iteration instead of 2.05, decided by how
# many streams the process happened to have created before (scripts/dev/stream_probe.py prints the sharing matrix: the same loop leg
# fast or slow by its place in the process).  So candidates are PROBED: a ~3 ms spin on the other stream, an event on the candidate --
# a candidate whose event completes while the spin is still running is independent of it.  More queues are NOT the answer: with
# GPU_MAX_HW_QUEUES = 8 / 12 the same loops ran at 2.5 (mixed) / 3.9 ms (fp32) per iteration.
# FRCNN_MANAGER_STREAM: "own" (default: the probed stream) | "prefix" (train._prefix_stream()) | "main" (the caller's stream).
_MANAGER_STREAM = None
MANAGER_STREAM = os.environ.get("FRCNN_MANAGER_STREAM", "own")


def _runs_beside(busy_stream, stream):
    """Does an event on ``stream`` complete while ``busy_stream`` spins?  (~3 ms per question.)"""
    first = torch.cuda.Event()
    first.record(stream)
    first.synchronize()                                      # (a stream's queue is set up at its first use: not inside the measurement)
    with torch.cuda.stream(busy_stream):
        torch.cuda._sleep(4_000_000)
        busy = torch.cuda.Event()
        busy.record(busy_stream)
    ev = torch.cuda.Event()
    ev.record(stream)
    ev.synchronize()
    beside = not busy.query()
    busy.synchronize()
    return beside


def manager_stream():
    global _MANAGER_STREAM
    if MANAGER_STREAM == "main":
        return torch.cuda.current_stream()
    if MANAGER_STREAM == "prefix":
        from . import train
        return train._prefix_stream()
    if _MANAGER_STREAM is None:
        from . import train
        cur = torch.cuda.current_stream()
        cur.synchronize()
        others = [cur, train._wgrad_stream(), train._prefix_stream()]       # (created now if the process has not trained yet: the order is fixed here)
        tried, best = [], None
        for _ in range(8):
            cand = torch.cuda.Stream()
            tried.append(cand)                               # (kept alive: a released stream's queue slot would be dealt out again)
            free = [_runs_beside(o, cand) for o in others]
            if all(free):
                best = cand
                break
            if best is None and free[0] and free[1]:
                best = cand                                  # sharing with the prefix stream only: 2.10 against 2.05 ms
        if best is None:
            import warnings
            best = tried[-1]
            warnings.warn("faster_rcnn_amd.feed: no HIP stream independent of the training step's streams found among %d candidates; the "
                          "managers' prefetch will queue behind the step's weight gradients (slower loop, same results)" % len(tried))
        _MANAGER_STREAM = best
        # the losing candidates go back (each held a hardware-queue slot for the life of the process); the queues were dealt
        # when the streams were created, so releasing them does not move the chosen one
        manager_stream.tried = len(tried)
        del tried
    return _MANAGER_STREAM
