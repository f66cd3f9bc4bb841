"""Device-tensor level wrappers over the C ABI (include/frcnn_hip.h).

torch tensors are only the container type (device memory + the current HIP stream); all
arithmetic happens inside libfrcnn_hip.so.  Every function takes/returns CUDA(=HIP) tensors
and is asynchronous on ``torch.cuda.current_stream()``.
"""
import ctypes
import dataclasses
import os

import numpy as np
import torch

from . import _lib
from . import y4m as _y4m

NMS_MAX_BOXES = 12288


_GPU_SEEN = False


def _require_gpu():
    # (torch.cuda.is_available() re-reads the environment on every call: 2 us x ~170 calls per training step)
    global _GPU_SEEN
    if not _GPU_SEEN:
        if not torch.cuda.is_available():
            raise _lib.FrcnnError("no HIP device visible: the faster_rcnn_amd ops need an MI355X (no CPU fallback)")
        _GPU_SEEN = True


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_RAW_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """The current torch stream's HIP handle.  torch.cuda.current_stream() builds a Stream object through three layers of
    Python (8 us); a training step asks ~90 times, and its mixed-precision form is bound by the host's launch rate."""
    if _RAW_STREAM is not None and _RAW_DEVICE is not None:
        return ctypes.c_void_p(_RAW_STREAM(_RAW_DEVICE()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    """Device pointer of a tensor as the plain integer ctypes' c_void_p argtype accepts (None = NULL).  (Building a c_void_p
    object per argument cost ~0.2 us x ~470 pointers per training step, whose mixed-precision form is bound by this host path.)"""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device-contiguous tensor required"
    return t.data_ptr()


def _anchor_arg(anchor_hw):
    a = np.ascontiguousarray(np.asarray(anchor_hw), dtype=np.int32)
    assert a.ndim == 2 and a.shape[1] == 2
    return a, a.ctypes.data_as(ctypes.c_void_p), a.shape[0]


def _dev(x, dtype):
    """numpy / tensor -> contiguous device tensor of dtype."""
    if isinstance(x, torch.Tensor):
        return x.to(device="cuda", dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(x)).to(device="cuda", dtype=dtype)


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")


def preprocess_u8(img_u8, mean_bgr, out=None):
    """(H,W,3) uint8 BGR image (numpy or device tensor) -> (1,H,W,3) f32 device tensor = float64(img) - mean, cast to f32
    (resnet.preprocess followed by the network's f32 input cast, bit for bit).  ``out``: write into this tensor
    (a captured graph's static input) instead of a new one."""
    _require_gpu()
    t = img_u8 if isinstance(img_u8, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img_u8, dtype=np.uint8))
    t = t.to(device="cuda").contiguous()
    assert t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3
    if out is None:
        out = torch.empty((1,) + tuple(t.shape), dtype=torch.float32, device="cuda")
    else:
        assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == t.numel()
    mean = (ctypes.c_double * 3)(*[float(v) for v in mean_bgr])
    _lib.call("frcnn_preprocess_u8", _p(t), t.shape[0] * t.shape[1], mean, _p(out), _stream())
    return out


def preprocess_u8_canvas(img_u8, mean_bgr, out, offset=None):
    """``preprocess_u8`` into a canvas: img_u8 (h,w,3) uint8 device tensor, out (1,hc,wc,3) / (hc,wc,3) f32; the image sits at ``offset``
    (rows, cols) -- default (h & 1, w & 1), which makes conv1's SAME padding on an even canvas the image's own -- zeros outside
    (frcnn_preprocess_u8_canvas)."""
    _require_gpu()
    assert img_u8.is_cuda and img_u8.dtype == torch.uint8 and img_u8.dim() == 3 and img_u8.shape[2] == 3 and img_u8.is_contiguous()
    hc, wc = int(out.shape[-3]), int(out.shape[-2])
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == hc * wc * 3
    h, w = int(img_u8.shape[0]), int(img_u8.shape[1])
    oy, ox = (h & 1, w & 1) if offset is None else (int(offset[0]), int(offset[1]))
    mean = (ctypes.c_double * 3)(*[float(v) for v in mean_bgr])
    _lib.call("frcnn_preprocess_u8_canvas", _p(img_u8), h, w, hc, wc, oy, ox, mean, _p(out), _stream())
    return out


def zero_outside(x, true_hw):
    """x (n,hc,wc,C) f32 or bf16 canvas tensor, IN PLACE: zero every cell at or beyond image i's true extent true_hw[i] = (rows, cols)
    (device int32 (n,2); frcnn_zero_outside).  Zeros cannot raise a magnitude bound: x keeps its record."""
    _require_gpu()
    assert x.dim() == 4 and x.is_contiguous() and true_hw.dtype == torch.int32 and true_hw.is_cuda and true_hw.numel() >= 2 * x.shape[0]
    n, hc, wc, c = (int(v) for v in x.shape)
    _lib.call("frcnn_zero_outside", _p(x), n, hc, wc, c * x.element_size(), _p(true_hw), _stream())
    return x


def decode_proposals_canvas(regr, anchor_hw_conv, true_rc):
    """``decode_proposals`` on canvas-shaped RPN outputs: true_rc = device int32 (2,) = the image's true (rows, cols)."""
    _require_gpu()
    keep, ap, A = _anchor_arg(anchor_hw_conv)
    regr = regr.reshape(regr.shape[-3], regr.shape[-2], regr.shape[-1]).contiguous()
    rows, cols = regr.shape[0], regr.shape[1]
    assert regr.shape[2] == 4 * A and true_rc.dtype == torch.int32 and true_rc.is_cuda and true_rc.numel() >= 2
    n = rows * cols * A
    rois = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    valid = torch.empty(n, dtype=torch.uint8, device="cuda")
    _lib.call("frcnn_decode_proposals_canvas", _p(regr), rows, cols, ap, A, _p(true_rc), _p(rois), _p(valid), _stream())
    return rois, valid


_TAPS = {}


def resize_cubic_taps(dst, src):
    """One axis' INTER_CUBIC tap table [dst][8] int32 = {4 clamped source indices, 4 fixed-point weights} (host array;
    frcnn_resize_cubic_taps: OpenCV's f32 arithmetic).  Cached: a dataset has a handful of (dst, src) pairs."""
    key = (int(dst), int(src))
    tab = _TAPS.get(key)
    if tab is None:
        tab = np.empty((key[0], 8), dtype=np.int32)
        _lib.call("frcnn_resize_cubic_taps", key[0], key[1], tab.ctypes.data_as(ctypes.c_void_p))
        if len(_TAPS) > 512:
            _TAPS.clear()
        _TAPS[key] = tab
    return tab


def resize_cubic_u8(src, dst_h, dst_w, flip=False, tabs=None, out=None):
    """cv2.resize(src, (dst_w, dst_h), interpolation=cv2.INTER_CUBIC) [+ horizontal flip] of a (h,w,3) uint8 device image
    (shapes.Image.data, shapes.py:19-29) -> (dst_h, dst_w, 3) uint8 device tensor.  ``flip``: bool, or the C ABI's bit set (1 = horizontal
    flip, 2 = the source is RGB: write B, G, R).  ``tabs``: (tab_x, tab_y) DEVICE int32
    tables to reuse (a captured pass keeps its own); ``out``: write into this tensor."""
    _require_gpu()
    assert src.is_cuda and src.dtype == torch.uint8 and src.dim() == 3 and src.shape[2] == 3 and src.is_contiguous()
    sh, sw = int(src.shape[0]), int(src.shape[1])
    if tabs is None:
        tabs = (torch.from_numpy(resize_cubic_taps(dst_w, sw)).cuda(), torch.from_numpy(resize_cubic_taps(dst_h, sh)).cuda())
    if out is None:
        out = torch.empty((dst_h, dst_w, 3), dtype=torch.uint8, device="cuda")
    _lib.call("frcnn_resize_cubic_u8", _p(src), sh, sw, _p(tabs[0]), _p(tabs[1]), int(dst_h), int(dst_w), int(flip), _p(out), _stream())
    return out


# ----------------------------------------------------------------------------- anchors
def anchors_image(rows, cols, anchor_hw, stride):
    _require_gpu()
    keep, ap, A = _anchor_arg(anchor_hw)
    out = torch.empty((rows * cols * A, 4), dtype=torch.float32, device="cuda")
    _lib.call("frcnn_anchors_image", rows, cols, ap, A, stride, _p(out), _stream())
    return out


def anchors_conv(rows, cols, anchor_hw_conv):
    _require_gpu()
    keep, ap, A = _anchor_arg(anchor_hw_conv)
    out = torch.empty((rows, cols, A, 4), dtype=torch.float32, device="cuda")
    _lib.call("frcnn_anchors_conv", rows, cols, ap, A, _p(out), _stream())
    return out


# ----------------------------------------------------------------------------- IoU
def cross_ious(boxes1, boxes2):
    """boxes1: (M,4) f32 or int16 device tensor; boxes2: (G,4) f32.  -> (M,G) f32."""
    _require_gpu()
    M, G = boxes1.shape[0], boxes2.shape[0]
    out = torch.zeros((M, G), dtype=torch.float32, device="cuda")
    b2 = boxes2.to(torch.float32).contiguous()
    if boxes1.dtype == torch.int16:
        _lib.call("frcnn_cross_ious_i16", _p(boxes1.contiguous()), M, _p(b2), G, _p(out), _stream())
    else:
        _lib.call("frcnn_cross_ious_f32", _p(boxes1.to(torch.float32).contiguous()), M, _p(b2), G, _p(out), _stream())
    return out


# ----------------------------------------------------------------------------- RPN targets
def rpn_assign(rows, cols, anchor_hw, stride, gt, img_w, img_h):
    """-> can_use (N,) u8, is_pos (N,) u8, bbreg (N,4) f32, argmax_gt (N,) i32 (device)."""
    _require_gpu()
    keep, ap, A = _anchor_arg(anchor_hw)
    gt = _dev(gt, torch.float32).reshape(-1, 4)
    G = gt.shape[0]
    n = rows * cols * A
    can_use = torch.empty(n, dtype=torch.uint8, device="cuda")
    is_pos = torch.empty(n, dtype=torch.uint8, device="cuda")
    bbreg = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    argmax = torch.empty(n, dtype=torch.int32, device="cuda")
    nbytes = _lib.load().frcnn_rpn_assign_workspace_bytes(rows, cols, A, G)
    ws = _ws(nbytes)
    _lib.call("frcnn_rpn_assign", rows, cols, ap, A, stride, _p(gt) if G else ctypes.c_void_p(0), G, int(img_w), int(img_h),
              _p(can_use), _p(is_pos), _p(bbreg), _p(argmax), _p(ws), ws.numel(), _stream())
    return can_use, is_pos, bbreg, argmax


def rpn_sample_lists(can_use, is_pos):
    """-> (pos_locs (N,) i32, neg_locs (N,) i32, counts (2,) i32): np.where(is_pos & can_use) / np.where(~is_pos & can_use) in
    ascending order, filled from the front, and their lengths (frcnn_rpn_sample_lists)."""
    _require_gpu()
    n = can_use.numel()
    pos = torch.empty(n, dtype=torch.int32, device="cuda")
    neg = torch.empty(n, dtype=torch.int32, device="cuda")
    counts = torch.empty(2, dtype=torch.int32, device="cuda")
    _lib.call("frcnn_rpn_sample_lists", _p(can_use), _p(is_pos), n, _p(pos), _p(neg), _p(counts), _stream())
    return pos, neg, counts


def rpn_pack_targets(can_use, is_pos, bbreg, cells, A, pos_locs, n_pos, off_pos, neg_locs, n_neg, off_neg):
    """Switch off the sampled positions (device int32 lists or None) IN can_use, then -> (y_class (cells,2A) f32, y_bbreg
    (cells,8A) f32) laid out like rpn_y_true's outputs (frcnn_rpn_pack_targets)."""
    _require_gpu()
    yc = torch.empty((cells, 2 * A), dtype=torch.float32, device="cuda")
    yb = torch.empty((cells, 8 * A), dtype=torch.float32, device="cuda")
    _lib.call("frcnn_rpn_pack_targets", _p(can_use), _p(is_pos), _p(bbreg), cells, A,
              _p(pos_locs), int(n_pos), _p(off_pos), 0 if off_pos is None else off_pos.numel(),
              _p(neg_locs), int(n_neg), _p(off_neg), 0 if off_neg is None else off_neg.numel(), _p(yc), _p(yb), _stream())
    return yc, yb


# ----------------------------------------------------------------------------- proposals
def decode_proposals(regr, anchor_hw_conv):
    """regr: (1,R,C,4A) or (R,C,4A) f32 device tensor -> rois (N,4) f32, valid (N,) u8."""
    _require_gpu()
    keep, ap, A = _anchor_arg(anchor_hw_conv)
    regr = regr.reshape(regr.shape[-3], regr.shape[-2], regr.shape[-1]).contiguous()
    rows, cols = regr.shape[0], regr.shape[1]
    assert regr.shape[2] == 4 * A
    n = rows * cols * A
    rois = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    valid = torch.empty(n, dtype=torch.uint8, device="cuda")
    _lib.call("frcnn_decode_proposals", _p(regr), rows, cols, ap, A, _p(rois), _p(valid), _stream())
    return rois, valid


def transform_inplace(coords, deltas):
    _require_gpu()
    assert coords.dtype == torch.float32 and deltas.dtype == torch.float32
    _lib.call("frcnn_transform_inplace", _p(coords), _p(deltas.contiguous()), coords.shape[0], _stream())
    return coords


def topk_order(scores, valid, K):
    """-> order (K,) i32 (entries >= n are -1), n (1,) i32 device."""
    _require_gpu()
    N = scores.numel()
    order = torch.empty(K, dtype=torch.int32, device="cuda")
    n_out = torch.empty(1, dtype=torch.int32, device="cuda")
    ws = _ws(_lib.load().frcnn_topk_workspace_bytes(N))
    _lib.call("frcnn_topk_order", _p(scores.contiguous()), _p(valid), N, K, _p(order), _p(n_out), _p(ws), ws.numel(), _stream())
    return order, n_out


def gather_candidates(rois, scores, order, n, K):
    _require_gpu()
    cand = torch.empty((K, 4), dtype=torch.int16, device="cuda")
    cs = torch.empty(K, dtype=torch.float32, device="cuda")
    _lib.call("frcnn_gather_candidates", _p(rois), _p(scores.contiguous()), _p(order), _p(n), K, _p(cand), _p(cs), _stream())
    return cand, cs


def nms_sorted(boxes, n, thresh, max_boxes):
    """boxes: (K,4) int16 or float64, already in descending-score order; n: (1,) i32 device.
    -> keep (max_boxes,) i32 positions, n_keep (1,) i32."""
    _require_gpu()
    K = boxes.shape[0]
    keep = torch.empty((max_boxes,), dtype=torch.int32, device="cuda")       # the call writes every slot (-1 past n_keep)
    n_keep = torch.empty(1, dtype=torch.int32, device="cuda")
    ws = _ws(_lib.load().frcnn_nms_workspace_bytes(K))
    name = {torch.int16: "frcnn_nms_i16", torch.float64: "frcnn_nms_f64"}[boxes.dtype]
    _lib.call(name, _p(boxes.contiguous()), _p(n), K, float(thresh), int(max_boxes), _p(keep), _p(n_keep), _p(ws), ws.numel(), _stream())
    return keep, n_keep


def gather_rois(cand, keep, n_keep, batch, out_rows, out=None):
    """``out``: write into this (out_rows,4) f32 tensor (a slice of a batch's RoI list) instead of a new one."""
    _require_gpu()
    if out is None:
        out = torch.empty((out_rows, 4), dtype=torch.float32, device="cuda")
    else:
        assert out.dtype == torch.float32 and tuple(out.shape) == (out_rows, 4) and out.is_contiguous()
    _lib.call("frcnn_gather_rois", _p(cand), _p(keep), _p(n_keep), batch, out_rows, _p(out), _stream())
    return out


# ----------------------------------------------------------------------------- detector targets
def roi_targets(rois_i16, gt_f32, gt_f64, gt_cls, bg_idx):
    _require_gpu()
    E, G = rois_i16.shape[0], gt_f32.shape[0]
    elig = torch.zeros(E, dtype=torch.uint8, device="cuda")
    cls = torch.full((E,), bg_idx, dtype=torch.int32, device="cuda")
    tg = torch.zeros((E, 4), dtype=torch.float32, device="cuda")
    _lib.call("frcnn_roi_targets", _p(rois_i16.contiguous()), E, _p(gt_f32.contiguous()), _p(gt_f64.contiguous()),
              _p(gt_cls.contiguous()), G, bg_idx, _p(elig), _p(cls), _p(tg), _stream())
    return elig, cls, tg


# ----------------------------------------------------------------------------- RoI crop/resize
def roi_crop_resize(feat, rois, pool, fill=None, relu=False, layout=0, planes_out=False, n_per_img=0):
    """feat: (R,C,Cf) f32 (or (1,R,C,Cf)); rois: (n,4) f32 -> (n,pool,pool,Cf) f32, or (pool,pool,n,Cf) with layout=1.
    fill (Cf,) = value of an invalid RoI (default zeros); relu clamps the output (frcnn_roi_crop_resize_fwd_ex).
    ``planes_out``: the result as a PlaneTensor for an f16x3 convolution behind it (frcnn_roi_crop_resize_fwd_planes); needs the
    map's magnitude record (its producer's), otherwise the f32 tensor comes back.
    ``n_per_img`` > 0: feat (B,R,C,Cf) holds one map per image and RoI r crops image r // n_per_img's (frcnn_roi_crop_resize_fwd_batch)."""
    _require_gpu()
    src = feat
    if n_per_img > 0:
        assert feat.dim() == 4 and feat.is_contiguous() and rois.reshape(-1, 4).shape[0] <= feat.shape[0] * n_per_img
        rows, cols, C = feat.shape[1:]
    else:
        feat = feat.reshape(feat.shape[-3], feat.shape[-2], feat.shape[-1]).contiguous()
        rows, cols, C = feat.shape
    rois = rois.reshape(-1, 4).to(torch.float32).contiguous()
    n = rois.shape[0]
    oshape = (pool, pool, n, C) if layout else (n, pool, pool, C)
    if planes_out and _tracking() and getattr(src, "_amax", None) is not None and C % 4 == 0 and n > 0:
        floor = 0.0
        if fill is not None:
            floor = getattr(fill, "_absmax", None)
            if floor is None:
                floor = float(fill.abs().max().item())
        out = PlaneTensor(oshape)
        amax_carry(out, src, floor, exponent_out=out.exponent)    # the bound and, from it, the planes' scale: known before the launch
        yp = _lib.H3Planes(planes=out.planes.data_ptr(), exponent=out.exponent.data_ptr(), status=out._amax.data_ptr() + 4)
        if n_per_img > 0:
            _lib.call("frcnn_roi_crop_resize_fwd_batch", _p(feat), rows, cols, C, _p(rois), n, n_per_img, pool, _p(fill), 1 if relu else 0, layout, None, ctypes.byref(yp), _stream())
        else:
            _lib.call("frcnn_roi_crop_resize_fwd_planes", _p(feat), rows, cols, C, _p(rois), n, pool, _p(fill), 1 if relu else 0, layout, ctypes.byref(yp), _stream())
        return out
    out = torch.empty(oshape, dtype=torch.float32, device="cuda")
    if n_per_img > 0:
        _lib.call("frcnn_roi_crop_resize_fwd_batch", _p(feat), rows, cols, C, _p(rois), n, n_per_img, pool, _p(fill), 1 if relu else 0, layout, _p(out), None, _stream())
    else:
        _lib.call("frcnn_roi_crop_resize_fwd_ex", _p(feat), rows, cols, C, _p(rois), n, pool, _p(fill), 1 if relu else 0, layout, _p(out), _stream())
    if _tracking() and getattr(src, "_amax", None) is not None:
        # a bilinear sample is a convex combination of map values; a rejected RoI yields the fill vector
        floor = 0.0
        if fill is not None:
            floor = getattr(fill, "_absmax", None)
            if floor is None:                                    # (PackedConv records it at lowering; a foreign vector costs one host sync)
                floor = float(fill.abs().max().item())
        amax_carry(out, src, floor)
    return out


class RoiResidual:
    """The RoI-resampled shortcut as the convolution behind it gathers it (include/ext/frcnn_hip_roi_res.h): the MAP ``fmap`` (B,R,C,Cf)
    or (R,C,Cf) f32, the tap table of the RoIs in the consuming launch's row order and the fill vector -- what
    ``roi_crop_resize(fmap, rois, pool, fill=fill, layout=layout, n_per_img=n_per_img)`` would have written, never materialised.
    ``conv2d(..., residual=RoiResidual(...))`` reads it where ``conv_takes_roi_res`` says so; ``shape`` is that tensor's."""

    def __init__(self, fmap, rois, pool, fill=None, layout=0, n_per_img=0):
        _require_gpu()
        assert fmap.dtype == torch.float32 and fmap.is_contiguous() and fmap.dim() in (3, 4)
        rows, cols, C = (int(v) for v in fmap.shape[-3:])
        n_maps = int(fmap.shape[0]) if fmap.dim() == 4 else 1
        assert n_per_img > 0 or n_maps == 1, "a batch of maps needs n_per_img"
        rois = rois.reshape(-1, 4).to(torch.float32).contiguous()
        n = int(rois.shape[0])
        self.map, self.fill, self.map_rows = fmap, fill, n_maps * rows * cols
        self.shape = (pool, pool, n, C) if layout else (n, pool, pool, C)
        self.taps = torch.empty((max(n * pool * pool, 1), _lib.ROI_TAP_BYTES // 4), dtype=torch.int32, device="cuda")
        _lib.call("frcnn_roi_tap_table", rows, cols, C, _p(rois), n, int(n_per_img), n_maps, int(pool), int(layout), _p(self.taps), _stream())
        self._amax = None
        if _tracking() and getattr(fmap, "_amax", None) is not None:
            amax_carry(self, fmap, self._floor())

    def _floor(self):
        """max|fill|: with the map's bound, the bound of the resampled tensor (roi_crop_resize: a convex combination of map values, or the fill vector)."""
        if self.fill is None:
            return 0.0
        floor = getattr(self.fill, "_absmax", None)
        return float(self.fill.abs().max().item()) if floor is None else floor

    def amax(self):
        """The magnitude record of the tensor this stands for: the map's record merged with max|fill|; a map without a valid record (none, or
        one of an earlier pass of its arena) is measured, as ``amax_of`` does for a resampled tensor nobody left a record on."""
        if self._amax is None:
            merged = _amax_new()
            _lib.call("frcnn_amax_merge", _p(merged), _p(amax_of(self.map)), float(self._floor()), None, _stream())
            self._amax = merged
        return self._amax

    def desc(self):
        return _lib.RoiRes(map=self.map.data_ptr(), taps=self.taps.data_ptr(), fill=self.fill.data_ptr() if self.fill is not None else None,
                           map_rows=self.map_rows, reserved=0)


def conv_takes_roi_res(x, pc, stride=1, padding="valid", act=None, layout=0, tile=0):
    """Would ``conv2d(x, pc, ..., residual=RoiResidual(...))`` gather its residual (frcnn_conv2d_roi_res_available: the f16x3 engine's
    256x128 form on sixteen waves, un-split, not the ring)?  ``x``: the tensor (f32 or PlaneTensor) the launch will read."""
    if not isinstance(pc, PackedConv):
        return False
    d = _conv_desc(tuple(x.shape), pc.kh, pc.kw, pc.cout, stride, padding, ACT[act], layout, tile or AUTO_TILE)
    eng = _split_engine(d, pc, tile or AUTO_TILE)
    code = {None: 0, "x6": 1, "h3": 2}[eng]
    got = _lib.load().frcnn_conv2d_roi_res_available(ctypes.byref(d), code, 1 if isinstance(x, PlaneTensor) else 0)
    if got < 0:
        _lib.check(got, "frcnn_conv2d_roi_res_available")
    return got == 1 and _planes_ok(d, pc, eng)


def roi_shortcut(fmap, rois, pool, x, pc, fill=None, layout=0, n_per_img=0, stride=1, padding="valid", act=None, tile=0):
    """The residual of ``conv2d(x, pc, stride, padding, act, residual=., tile=tile, layout=layout)`` when it is the RoI resampling of
    ``fmap``: a RoiResidual where that launch gathers its residual (``conv_takes_roi_res``), otherwise the resampled f32 tensor
    (``roi_crop_resize``) -- every other engine, tile and form.  Either way the convolution's result is the same, bit for bit."""
    n = rois.reshape(-1, 4).shape[0]
    if n > 0 and fmap.dtype == torch.float32 and fmap.is_contiguous() and conv_takes_roi_res(x, pc, stride, padding, act, layout, tile):
        return RoiResidual(fmap, rois, pool, fill=fill, layout=layout, n_per_img=n_per_img)
    return roi_crop_resize(fmap, rois, pool, fill=fill, layout=layout, n_per_img=n_per_img)


def avgpool_pos_major(x):
    """(h,w,n,c) f32 position-major -> (n,c): AveragePooling2D over the whole h x w window."""
    _require_gpu()
    h, w, n, c = x.shape
    out = torch.empty((n, c), dtype=torch.float32, device="cuda")
    _lib.call("frcnn_avgpool_pos_major", _p(x.contiguous()), h * w, n, c, _p(out), _stream())
    return out


def roi_crop_resize_bwd(dout, rois, rows, cols):
    _require_gpu()
    n, pool, _, C = dout.shape
    dfeat = torch.empty((rows, cols, C), dtype=torch.float32, device="cuda")
    _lib.call("frcnn_roi_crop_resize_bwd", _p(dout.contiguous()), rows, cols, C, _p(rois.reshape(-1, 4).contiguous()), n, pool, _p(dfeat), _stream())
    return dfeat


# ----------------------------------------------------------------------------- conv engine
ACT = {None: 0, "linear": 0, "none": 0, "relu": 1, "sigmoid": 2}


def same_pad(size, k, stride):
    """TF/Keras padding='same': (out, pad_before)."""
    out = -(-size // stride)
    total = max((out - 1) * stride + k - size, 0)
    return out, total // 2


def valid_out(size, k, stride):
    return (size - k) // stride + 1


# The f16x3 engine scales a whole filter by ONE power of two.  fp16 keeps full precision over 2^-12 .. 2^15 after scaling and loses bits
# gradually below (the low plane and fp16's subnormals stretch that: at 2^-30 of the largest value ~19 bits are left, at 2^-44 about
# six).  A filter whose reduction channels differ by more than 2^H3_MAX_SPREAD_LOG2 in magnitude (max |w| per input channel, largest
# against smallest non-zero) may pair its smallest-weight channels with the LARGEST activations (channel scales that a checkpoint's
# normalisation moved between weights and activations), and then the lost bits show in the sum.  Measured
# (tests/test_h3_fences_gpu.py): at a compensated spread of 2^30 the engine still reads 2.0e-7 of sum |x w| against the native kernel's
# 4.0e-7; the bar is kept well inside that, and a layer beyond it runs on the exact bf16 split.  With the weights inside the bar, ANY
# spread of the activations alone costs nothing (5.6e-7 against the native 1.3e-6 at 2^30).
H3_MAX_SPREAD_LOG2 = 24.0


def _channel_spread_log2(w_hwio, axis):
    """log2(largest / smallest non-zero) of max|w| per reduction channel (``axis`` of the HWIO filter); one host read at lowering."""
    dims = tuple(i for i in range(w_hwio.dim()) if i != axis)
    cm = w_hwio.abs().amax(dim=dims).double()
    nz = cm[cm > 0]
    if nz.numel() < 2:
        return 0.0
    return float(torch.log2(nz.max() / nz.min()).item())


class PackedConv:
    """A convolution's device-resident parameters: filter packed to [cout][packed_k], and the
    per-channel scale/shift the epilogue applies (bias and BatchNorm/Scale folded)."""

    def __init__(self, w_hwio, scale=None, shift=None):
        _require_gpu()
        w = _dev(w_hwio, torch.float32)
        self.kh, self.kw, self.cin, self.cout = (int(v) for v in w.shape)
        kp = _lib.load().frcnn_conv_packed_k(self.kh, self.kw, self.cin)
        self.w = torch.empty((self.cout, kp), dtype=torch.float32, device="cuda")
        _lib.call("frcnn_pack_conv_weights", _p(w), self.kh, self.kw, self.cin, self.cout, _p(self.w), _stream())
        self.scale = None if scale is None else _dev(scale, torch.float32)
        self.shift = None if shift is None else _dev(shift, torch.float32)
        if self.shift is not None and not isinstance(shift, torch.Tensor):
            self.shift._absmax = float(np.abs(np.asarray(shift, dtype=np.float64)).max())      # host copy of max|shift| (amax_carry's floor)
        self._h3_spread_log2 = _channel_spread_log2(w, 2)

    def x6_planes(self):
        """The filter as three bf16 planes [3][cout][packed_k] for the split-bf16 engine (frcnn_conv2d_fwd_x6), derived
        once from the packed f32 filter (6 bytes per weight beside the 4 of the f32 form)."""
        planes = getattr(self, "_x6", None)
        if planes is None or getattr(self, "_x6_src", None) is not self.w:
            planes = torch.empty((3,) + tuple(self.w.shape), dtype=torch.bfloat16, device="cuda")
            _lib.call("frcnn_pack_conv_weights_x6", _p(self.w), self.w.shape[0], self.w.shape[1], _p(planes), _stream())
            self._x6, self._x6_src = planes, self.w
        return planes


    def h3_planes(self):
        """The filter as a 16-byte header (max|w|) + two fp16 planes [2][cout][packed_k] for the f16x3 engine
        (frcnn_conv2d_fwd_h3), derived once from the packed f32 filter (4 bytes per weight)."""
        planes = getattr(self, "_h3", None)
        if planes is None or getattr(self, "_h3_src", None) is not self.w:
            planes = torch.empty(_lib.load().frcnn_conv_h3_planes_bytes(self.w.shape[0], self.w.shape[1]), dtype=torch.uint8, device="cuda")
            _lib.call("frcnn_pack_conv_weights_h3", _p(self.w), self.w.shape[0], self.w.shape[1], _p(planes), _stream())
            self._h3, self._h3_src = planes, self.w
        return planes


    def h3_bound(self):
        """(bound_c, bound_d) of frcnn_conv2d_fwd_h3_planes: |y| <= bound_c * max|x| + bound_d for ANY input -- the largest
        |scale[c]| * sum |w[.,.,.,c]| over the output channels and the largest |shift[c]| (host floats, computed once per filter)."""
        b = getattr(self, "_h3_bound", None)
        if b is None or getattr(self, "_h3_bound_src", None) is not self.w:
            l1 = self.w.abs().sum(dim=1)
            if self.scale is not None:
                l1 = l1 * self.scale.abs()
            b = (float(l1.max().item()), 0.0 if self.shift is None else float(self.shift.abs().max().item()))
            self._h3_bound, self._h3_bound_src = b, self.w
        return b


class PlaneTensor:
    """An activation tensor the way the f16x3 engine multiplies it: two fp16 planes (2, *shape) -- hi = f16(v * 2^e), lo = f16((v * 2^e
    - hi) * 2^11) -- and the device int32 ``exponent`` e, written by the launch that produced it (frcnn_conv2d_fwd_h3_planes).  Only
    convolutions read it (``conv2d`` accepts it in place of the f32 tensor); ``_amax`` is the producer's magnitude record."""
    is_planes = True

    def __init__(self, shape):
        self.shape = tuple(int(v) for v in shape)
        self.planes = torch.empty((2,) + self.shape, dtype=torch.float16, device="cuda")
        self.exponent = torch.empty(1, dtype=torch.int32, device="cuda")
        self._amax = None

    def float(self):
        """The f32 values (hi + lo * 2^-11) * 2^-e, on the device (tests / debugging: torch arithmetic)."""
        e = self.exponent.to(torch.float64)
        return ((self.planes[0].double() + self.planes[1].double() / 2048.0) * torch.pow(torch.tensor(2.0, dtype=torch.float64, device="cuda"), -e)).float()


# ---- which matrix path an fp32 convolution takes.
# "native": v_mfma_f32_32x32x2_f32 (csrc/conv_igemm.hip).  "bf16x6": the same GEMM on the bf16 matrix cores by exact
# three-way operand splitting (csrc/conv_x6.hip) for the launches where it measures faster -- large row counts, cin % 32 == 0;
# everything else stays native.  fp32-grade either way (error against fp64 at or below the native kernel's), but a
# different summation order: the two agree to f32 rounding, not bit for bit, so the library default stays "native" and a
# caller opts in for a scope (``with f32_engine("bf16x6"):`` -- bench.py and entry.DetectionEntry do, around their captures).
# "f16x3" (round 5): the same launches on the fp16 matrix cores by a two-way split with a scaled low part (csrc/conv_h3.hip):
# three matrix instructions per block of products instead of six, error against fp64 at or under the native kernel's; every
# tensor an f16x3 launch reads carries a device-resident magnitude record (``AmaxArena``, ``amax_of``) from which the launch
# derives the power of two that brings the tensor into fp16's range.
F32_ENGINE = "native"
# where the split engine measures faster than the native kernels (MI355X, configs[1] shapes, each launch alone on the chip;
# scripts/conv_shapes.py 0,74,77,71,76): the head's 14 700-row GEMMs 355 / 189 / 167 us against 530 / 275 / 269; with 64x64 tiles
# almost every trunk layer too -- stage 2 (37 101 rows) 3x3 30.9 vs 36.3 us, 1x1 23.4 vs 27.2 / 19.0 vs 20.9, stage 3's wide 1x1
# 19.6 vs 22.0 / 28.2 vs 32.6, stage 4's 1024-column 1x1 18.9 vs 20.9 / 28.7 vs 33.6 -- as long as the launch has >= 256 tiles of
# 64x64; under that (stage 4's 256-column layers: 26.8 vs 21.1 us) the native split-K launches win, except where the engine's own
# split-K form applies (rpn_conv1 176 vs 202, stage 4's 3x3 32.7 vs 34.9).  Layers with fewer than 64 columns stay native.
X6_MIN_TILES = 256              # 64x64 tiles of the output
X6_MIN_COUT = 64


class f32_engine:
    def __init__(self, name):
        assert name in ("native", "bf16x6", "f16x3")
        self.name = name

    def __enter__(self):
        global F32_ENGINE
        self.prev, F32_ENGINE = F32_ENGINE, self.name

    def __exit__(self, *exc):
        global F32_ENGINE
        F32_ENGINE = self.prev


_ENGINE_CODE = {"native": 0, "bf16x6": 1, "f16x3": 2}
_ENGINE_TAG = {0: None, 1: "x6", 2: "h3"}


def _split_engine(d, pc, tile):
    """Which split engine a forward launch takes: "x6" (bf16, six products), "h3" (fp16, three products) or None (native).
    The policy itself lives in the library (frcnn_conv2d_engine: explicit tile codes 71..78 / 81..88 pick their engine, otherwise
    the engine of the ``F32_ENGINE`` scope takes the launches where it measures faster -- >= X6_MIN_TILES output tiles of 64x64
    and >= X6_MIN_COUT columns, or its split-K form when split-K launches are allowed), so a host in another language gets the
    same choices; memoised on the cached descriptor."""
    key = ("engine", F32_ENGINE, _CONV_WS is not NO_SPLIT_K)
    memo = getattr(d, "_ws", None)
    own = memo is not None and d.tile == tile and d.cout == pc.cout and d.cin == pc.cin
    got = memo.get(key) if own else None
    if got is None:
        q = d
        if not own:
            q = _lib.ConvDesc.from_buffer_copy(d)             # (a caller asking about another tile code / filter than the descriptor's)
            q.tile, q.cin, q.cout = tile, pc.cin, pc.cout
        got = _lib.load().frcnn_conv2d_engine(ctypes.byref(q), _ENGINE_CODE[F32_ENGINE], 1 if key[2] else 0)
        if got < 0:
            _lib.check(got, "frcnn_conv2d_engine")
        if own:
            memo[key] = got
    if got == 2 and not (81 <= tile <= 88) and getattr(pc, "_h3_spread_log2", 0.0) > H3_MAX_SPREAD_LOG2:
        return "x6"                                           # an ill-scaled filter (H3_MAX_SPREAD_LOG2): the exact split (an explicit 8x tile code stands)
    return _ENGINE_TAG[got]


def _use_x6(d, pc, tile):
    return _split_engine(d, pc, tile) == "x6"


# ---- magnitude records of the f16x3 engine (include/frcnn_hip.h, "Magnitude records").  A tensor that an f16x3 launch may read
# carries ``t._amax``: a device record holding an upper bound of max|t|, written by the launch that produced the tensor.
class AmaxArena:
    """The records of ONE forward pass: a fixed pool handed out in call order, cleared by a kernel at the start of the pass, so a
    captured pass re-uses the same addresses on every replay and contains no memset node.

    ``gen`` counts the passes begun: a record handed out carries the generation it belongs to, and ``amax_of`` refuses one of an earlier
    pass (its words have been cleared, or belong to another tensor now) -- the tensor is measured again instead (a cached
    conv map, an ``out=`` buffer).  ``status()`` gathers the records' sticky status words (FRCNN_H3_*: a value above its record's
    bound, a clamped value, a non-finite record) into ONE device word to be read with the pass's outputs."""

    def __init__(self, n=192):
        _require_gpu()
        self.floats = _lib.load().frcnn_amax_record_floats()
        self.buf = torch.zeros((n, self.floats), dtype=torch.float32, device="cuda")
        self.status_word = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.i = self.high_water = self.gen = 0

    def begin(self):
        """Clear the records the passes so far have used (all of them were zero at allocation; a captured pass bakes in the count of
        its warm-up passes, which walk the same launches): ~60 records = 240 KB for a ResNet-50 pass instead of the whole pool."""
        self.high_water = max(self.high_water, self.i)
        self.i = 0
        self.gen += 1
        if self.high_water:
            _lib.call("frcnn_amax_clear", _p(self.buf), self.high_water, _stream())

    def take(self):
        assert self.i < self.buf.shape[0], "AmaxArena: more tracked tensors in a pass than records"
        r = self.buf[self.i]
        r._arena_gen = (self, self.gen)
        self.i += 1
        return r

    def status(self, out=None):
        """-> device int32 word (``out`` or the arena's own): OR of the status words of the records this pass has used so far."""
        out = self.status_word if out is None else out
        n = max(self.i, 1)
        _lib.call("frcnn_amax_status", _p(self.buf), n, _p(out), _stream())
        return out


def h3_status_text(bits):
    """Readable form of a FRCNN_H3_* status word (entry.DetectionEntry raises with it)."""
    names = [(n, b) for n, b in (("a value above its magnitude record's bound", _lib.H3_UNDER), ("values clamped to fp16's range", _lib.H3_SATURATED),
                                  ("a non-finite magnitude record (Inf in a tensor)", _lib.H3_NONFINITE)) if bits & b]
    return "; ".join(n for n, _ in names) or "clean"


_AMAX_ARENA = None
AMAX_MEASURED = 0           # tensors whose bound had to be measured by a pass of their own (no producer record): a perf counter


class amax_arena:
    """``with amax_arena(arena):`` f16x3 launches inside take their records from ``arena`` (None: one fresh allocation each)."""

    def __init__(self, arena):
        self.arena = arena

    def __enter__(self):
        global _AMAX_ARENA
        self.prev, _AMAX_ARENA = _AMAX_ARENA, self.arena
        return self.arena

    def __exit__(self, *exc):
        global _AMAX_ARENA
        _AMAX_ARENA = self.prev


def amax_begin():
    """Start of a forward pass: clear the active arena's records (no arena: nothing to do)."""
    if _AMAX_ARENA is not None:
        _AMAX_ARENA.begin()


def _amax_new(optional=False):
    """A cleared record: from the active arena, or (eager launches) a fresh allocation.  A capture without an arena cannot have one
    (a zero-filling allocation would put a memset node into the graph): an error for an f16x3 launch, None for a native layer that
    would merely have left its record for a layer behind it (``optional``)."""
    if _AMAX_ARENA is not None:
        return _AMAX_ARENA.take()
    if torch.cuda.is_current_stream_capturing():
        if optional:
            return None
        raise _lib.FrcnnError("f16x3 launches inside a capture need an ops.amax_arena (pipeline.InferencePipeline.capture makes one)")
    return torch.zeros(_lib.load().frcnn_amax_record_floats(), dtype=torch.float32, device="cuda")


def _tracking():
    return F32_ENGINE == "f16x3"


def amax_of(x):
    """The magnitude record of tensor ``x``: the one its producer attached, or a MEASURED one (one pass over x).  A measured record is
    not kept on the tensor: a tensor nobody produced is somebody's input buffer, rewritten between passes (a captured pass's static
    input), and its record lives in an arena that the next pass clears."""
    rec = getattr(x, "_amax", None)
    if rec is not None:
        stamp = getattr(rec, "_arena_gen", None)
        if stamp is not None and stamp[0].gen != stamp[1]:      # a record of an EARLIER pass of its arena: cleared or re-used since
            rec = None
            try:
                x._amax = None
            except AttributeError:
                pass
    if rec is None:
        global AMAX_MEASURED
        AMAX_MEASURED += 1
        rec = _amax_new()
        _lib.call("frcnn_amax_f32", _p(x), x.numel(), _p(rec), _stream())
    return rec


def amax_carry(dst, src, floor=0.0, exponent_out=None):
    """``dst`` was derived from ``src`` by a map that cannot exceed max(|src|, floor) (a view, max-pooling, ReLU, the bilinear RoI
    resampling with a fill vector): it inherits the bound.  floor > 0 (or a request for the bound's plane exponent) needs a record
    of its own (frcnn_amax_merge)."""
    rec = getattr(src, "_amax", None)
    stamp = getattr(rec, "_arena_gen", None) if rec is not None else None
    if stamp is not None and stamp[0].gen != stamp[1]:
        rec = None                                               # (a record of an earlier pass: see amax_of)
    if rec is None:
        if exponent_out is not None:
            rec = amax_of(src)                                   # planes need their scale: measure
        else:
            return dst
    if floor > 0.0 or exponent_out is not None:
        merged = _amax_new()
        _lib.call("frcnn_amax_merge", _p(merged), _p(rec), float(floor), _p(exponent_out), _stream())
        rec = merged
    dst._amax = rec
    return dst


def conv_accepts_planes(x_shape, pc, stride=1, padding="valid", act=None, layout=0, tile=0):
    """Would ``conv2d`` of a tensor of this shape read fp16 planes (the f16x3 engine on its 256x128 tile, un-split)?  Producers ask
    before they hand a PlaneTensor on."""
    if F32_ENGINE != "f16x3" or not isinstance(pc, PackedConv):
        return False
    d = _conv_desc(tuple(x_shape), pc.kh, pc.kw, pc.cout, stride, padding, ACT[act], layout, tile or AUTO_TILE)
    return _planes_ok(d, pc, _split_engine(d, pc, tile or AUTO_TILE))


H3_KERNEL_NAMES = {81: "k_conv_igemm_h3<2,1,2,4>", 82: "k_conv_igemm_h3_db<2,2,4,2>", 83: "k_conv_igemm_h3<2,2,2,2>", 84: "k_conv_igemm_h3<1,1,2,2>",
                   85: "k_conv_igemm_h3_db<2,1,4,4>", 86: "k_conv_igemm_h3_db<2,1,4,4>", 87: "k_conv_igemm_h3<2,1,2,2>"}


def _h3_name(d, n1=0):
    return H3_KERNEL_NAMES[_lib.load().frcnn_conv2d_h3_config(ctypes.byref(d), n1)]


X6_KERNEL_NAMES = {71: "k_conv_igemm_x6<2,1,2,4>", 72: "k_conv_igemm_x6<2,2,4,2>", 73: "k_conv_igemm_x6<2,2,2,2>", 74: "k_conv_igemm_x6<1,1,2,2>",
                   75: "k_conv_igemm_x6<1,1,2,4>", 76: "k_conv_igemm_x6_db", 77: "k_conv_igemm_x6<2,1,2,2>"}


def _x6_name(d, n1=0):
    return X6_KERNEL_NAMES[_lib.load().frcnn_conv2d_x6_config(ctypes.byref(d), n1)]


# When set to a list, every conv2d launch appends {kernel, flops, shape, relaunch()} so bench.py can
# re-issue each distinct launch back to back between one HIP-event pair on the launch stream.
CONV_PROFILE = None
CONV_KERNEL_NAMES = {1: "k_conv_igemm_f32<2,2,false>", 2: "k_conv_igemm_f32<1,1,*>", 3: "k_conv_igemm_f32<2,1,*>",
                     4: "k_conv_igemm_f32<4,2,false>", 11: "k_conv_igemm_f32_v2<2,2>", 12: "k_conv_igemm_f32_v2<1,1>",
                     13: "k_conv_igemm_f32_v2<2,1>", 14: "k_conv_igemm_f32_v2<4,2>",
                     21: "k_conv_igemm_f32_v2<2,2,1>", 22: "k_conv_igemm_f32_v2<1,1,1>",
                     23: "k_conv_igemm_f32_v2<1,1,2>", 24: "k_conv_igemm_f32_v2<1,2,2>", 25: "k_conv_igemm_f32_v2<2,1,2>", 26: "k_conv_igemm_f32_v2<2,2,2>",
                     30: "k_conv_igemm_f32_v2<1,1,2> stem", 32: "k_conv_igemm_f32_v2<1,1,1> stem", 61: "k_conv_igemm_f32_sk<2,2>", 62: "k_conv_igemm_f32_sk<1,1>", 41: "k_conv_igemm_f32_v2<1,2,1,4,2>", 42: "k_conv_igemm_f32_v2<2,1,1,2,4>", 43: "k_conv_igemm_f32_v2<1,1,1,4,2>"}


def _record_launch(kernel, shape, fn, args, keep, **extra):
    """Appends a launch to CONV_PROFILE when it is set: ``kernel()`` names its kernel (looked up only then), ``shape`` is the GEMM
    (rows, columns, k, stride) the FLOPs come from, and ``relaunch`` re-issues entry point ``fn`` with ``args`` (``keep``: what the
    re-launches need alive).  ``extra``: further keys of the record."""
    if CONV_PROFILE is None:
        return
    CONV_PROFILE.append({"kernel": kernel(), **extra, "flops": 2.0 * shape[0] * shape[1] * shape[2], "shape": shape,
                         "relaunch": lambda fn=fn, args=args, keep=keep: _lib.call(fn, *args, _stream())})


def _gemm_shape(d, pc, stride):
    return (d.n * d.ho * d.wo, pc.cout, pc.kh * pc.kw * pc.cin, stride)


def _kernel_name(d, eng, ws, n1=None):
    """The kernel an f32 forward launch on engine ``eng`` ("x6", "h3", None: native) ran, with split-K workspace ``ws``
    (n1: a two-layer launch whose first layer has n1 columns)."""
    if eng is not None:
        if ws is not None:
            return f"k_conv_igemm_{eng}<1,1,2,2> split-K"
        return (_h3_name if eng == "h3" else _x6_name)(d, n1 or 0)
    if n1 is not None:
        cfg = _lib.load().frcnn_conv2d_dual_config(ctypes.byref(d), 1 if ws is not None else 0)     # the remapped code the launch ran
        return CONV_KERNEL_NAMES.get(cfg, "?") + (" split-K" if ws is not None else "")
    cfg = _lib.load().frcnn_conv2d_config(ctypes.byref(d))
    if cfg in (61, 62) and ws is None:
        cfg -= 40                                                # balanced form needs a workspace: the plain tile ran
    return CONV_KERNEL_NAMES.get(cfg, "?") + (" split-K" if ws is not None and cfg not in (61, 62) else "")


class ConvWorkspace:
    """Split-K workspace (arrival tickets + f32 partial tiles) of frcnn_conv2d_fwd_ws.

    The C ABI wants the ticket words zero on entry and leaves them zero, so one buffer zeroed at
    allocation serves every conv launched on ONE stream (or replayed from ONE hipGraph).  Streams or
    graphs that may run concurrently need one ``ConvWorkspace`` each (pipeline.py owns one per graph).
    """

    def __init__(self, nbytes=0):
        self.buf = None
        if nbytes:
            self.get(nbytes)

    def get(self, nbytes):
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.zeros(int(nbytes), dtype=torch.uint8, device="cuda")
        return self.buf


NO_SPLIT_K = object()       # ``with conv_workspace(NO_SPLIT_K):`` = plain launches only
_CONV_WS = None             # the workspace conv launches use right now (None: per-stream default)
_STREAM_WS = {}             # eager launches: HIP stream handle -> ConvWorkspace (same-stream launches serialise)


AUTO_TILE = 0               # tile code substituted for tile=0: 0 = launch alone on the chip, 50 = beside other streams' launches


class tile_policy:
    """``with tile_policy(throughput=True):`` conv launches inside pick their tile for a chip shared with other
    images' launches (frcnn_conv_desc.tile = 50) instead of for a launch that has the chip to itself."""

    def __init__(self, throughput):
        self.code = 50 if throughput else 0

    def __enter__(self):
        global AUTO_TILE
        self.prev, AUTO_TILE = AUTO_TILE, self.code

    def __exit__(self, *exc):
        global AUTO_TILE
        AUTO_TILE = self.prev


class conv_workspace:
    """``with conv_workspace(ws):`` routes the split-K launches inside to ``ws``."""

    def __init__(self, ws):
        self.ws = ws

    def __enter__(self):
        global _CONV_WS
        self.prev, _CONV_WS = _CONV_WS, self.ws
        return self.ws

    def __exit__(self, *exc):
        global _CONV_WS
        _CONV_WS = self.prev


def _split_k_ws(need):
    """The split-K workspace tensor a launch needing `need` bytes should use right now, or None (plain launch)."""
    if not need or _CONV_WS is NO_SPLIT_K:
        return None
    holder = _CONV_WS
    if holder is None and not torch.cuda.is_current_stream_capturing():
        # a capture without an explicit workspace takes the plain launch: graphs replay concurrently
        holder = _STREAM_WS.setdefault(torch.cuda.current_stream().cuda_stream, ConvWorkspace())
    return None if holder is None else holder.get(need)


def _conv_launch(d, x, w, scale, shift, residual, mask, out, y_amax=None):
    """frcnn_conv2d_fwd_ws with the right workspace (``y_amax``: frcnn_conv2d_fwd_ws_amax, which also folds max|y| into that
    record); returns (entry point, ctypes argument tuple) for re-launches, and the workspace."""
    ws = _split_k_ws(_ws_need(d, "frcnn_conv2d_workspace_bytes"))
    head = (ctypes.byref(d), _p(x), _p(w), _p(scale), _p(shift), _p(residual), _p(mask), _p(out))
    tail = (_p(ws), ws.numel() if ws is not None else 0)
    fn, args = ("frcnn_conv2d_fwd_ws", head + tail) if y_amax is None else ("frcnn_conv2d_fwd_ws_amax", head + (_p(y_amax),) + tail)
    _lib.call(fn, *args, _stream())
    return (fn, args), ws


def _conv2d_h3_planes(d, x, pc, residual, oshape, planes_out, act, rowmap=None):
    """frcnn_conv2d_fwd_h3_planes: x a PlaneTensor or an f32 tensor, the result a PlaneTensor (planes_out) or an f32 tensor.
    ``rowmap``: the launch's rows assigned to tiles by this map (``_conv_rowmap``; plane input, no residual: frcnn_conv2d_fwd_h3_rowmap)."""
    x_in = isinstance(x, PlaneTensor)
    xp = _lib.H3Planes(planes=x.planes.data_ptr(), exponent=x.exponent.data_ptr(), status=None) if x_in else None
    y = PlaneTensor(oshape) if planes_out else torch.empty(oshape, dtype=torch.float32, device="cuda")
    ya = _amax_new()
    yp = _lib.H3Planes(planes=y.planes.data_ptr(), exponent=y.exponent.data_ptr(), status=ya.data_ptr() + 4) if planes_out else None
    bc, bd = pc.h3_bound() if planes_out else (0.0, 0.0)
    xa = amax_of(x)                                              # (a measured record is a temporary: it must outlive the launch and its re-launches)
    r_in = isinstance(residual, PlaneTensor)                     # a block's output handed on as planes: the shortcut reads them back
    r_roi = isinstance(residual, RoiResidual)                    # the RoI-resampled shortcut, gathered from its map in the epilogue
    ra = (residual.amax() if r_roi else amax_of(residual)) if (residual is not None and planes_out) else None
    rp = _lib.H3Planes(planes=residual.planes.data_ptr(), exponent=residual.exponent.data_ptr(), status=None) if r_in else None
    head = (ctypes.byref(d), None if x_in else _p(x), ctypes.byref(xp) if x_in else None, _p(xa), _p(pc.h3_planes()), _p(pc.scale), _p(pc.shift))
    tail = (_p(ra), None if planes_out else _p(y), _p(ya), ctypes.byref(yp) if planes_out else None, bc, bd)
    rm = None
    if rowmap is not None:
        assert x_in and residual is None
        rm = _lib.RowMap(row_map=rowmap[0].data_ptr(), tile_taps=rowmap[1].data_ptr(), rows=rowmap[0].numel(), reserved=0)
        fn, args = "frcnn_conv2d_fwd_h3_rowmap", (head[0],) + head[2:] + tail[1:] + (ctypes.byref(rm),)
    elif r_roi:
        rp = residual.desc()
        fn, args = "frcnn_conv2d_fwd_h3_roi_res", head + (ctypes.byref(rp),) + tail
    else:
        fn, args = "frcnn_conv2d_fwd_h3_planes_res", head + (None if r_in else _p(residual), ctypes.byref(rp) if r_in else None) + tail
    _lib.call(fn, *args, _stream())
    y._amax = ya
    # (the instantiation that reads planes is a kernel of its own; writing planes is a run-time branch of either's epilogue; the gathered
    # residual is an instantiation too, listed under the name of the launch it replaces so that per-kernel figures cover the same launches)
    # (the mapped ring likewise: the plane-reading kernel's name, a fifth word in the shape as the pooled launch has)
    _record_launch(lambda: _h3_planes_in_name(d, pc) if x_in else _h3_name(d), _gemm_shape(d, pc, d.stride) + (("rowmap",) if rm is not None else ()), fn,
                   args, (d, x, pc, residual, y, ya, xp, yp, xa, ra, rp, rm, rowmap), planes_out=bool(planes_out), roi_res=bool(r_roi),
                   **({"rowmap": True} if rm is not None else {}))
    return y


# Class-sorted row tiles (include/ext/frcnn_hip_rowmap.h): the map of a launch depends on its geometry only, so it is built once per
# geometry on the host and kept on the device for every later launch and every captured pass (fixed addresses across replays).
ROWMAP_ORDER = int(os.environ.get("FRCNN_ROWMAP_ORDER", "0"))       # dev knob: class order inside a super-group (0 raster, 1 long tiles first)
_ROWMAP_CACHE = {}


def conv_rowmap_host(d, order=None, tile_rows=_lib.ROWMAP_TILE_ROWS):
    """frcnn_conv_rowmap_build on the host, no GPU: -> (pays, row_map int32 [rows], tile_taps uint32 [rows / tile_rows], tap_tiles).
    ``pays`` False: the map saves no tap-tile against the plain launch ("not available"); it is a valid map all the same."""
    lib = _lib.load()
    order = ROWMAP_ORDER if order is None else order
    rows, tap_tiles = ctypes.c_int64(0), ctypes.c_int64(0)
    got = lib.frcnn_conv_rowmap_build(ctypes.byref(d), tile_rows, order, None, 0, None, 0, ctypes.byref(rows), ctypes.byref(tap_tiles))
    if got < 0:
        _lib.check(got, "frcnn_conv_rowmap_build")
    row_map = np.empty(rows.value, np.int32)
    taps = np.empty(rows.value // tile_rows, np.uint32)
    got = lib.frcnn_conv_rowmap_build(ctypes.byref(d), tile_rows, order, row_map.ctypes.data_as(ctypes.c_void_p), row_map.size,
                                      taps.ctypes.data_as(ctypes.c_void_p), taps.size, None, None)
    if got < 0:
        _lib.check(got, "frcnn_conv_rowmap_build")
    return got == 1, row_map, taps, tap_tiles.value


def _conv_rowmap(d, force=False):
    """The device copy of descriptor ``d``'s map, (row_map, tile_taps) int32 tensors, or None where the map does not pay (``force``: then
    too).  Built and uploaded on first use, which must lie outside a capture (a warm-up pass does it)."""
    key = (torch.cuda.current_device(), ROWMAP_ORDER, d.n, d.h, d.w, d.ho, d.wo, d.kh, d.kw, d.stride, d.pad_top, d.pad_left)
    got = _ROWMAP_CACHE.get(key)
    if got is None:
        if torch.cuda.is_current_stream_capturing():
            raise _lib.FrcnnError("conv2d(rowmap=...): the row map of this shape is uploaded on first use, which cannot happen inside a capture "
                                  "(run the pass once before capturing it)")
        pays, row_map, taps, _ = conv_rowmap_host(d)
        got = _ROWMAP_CACHE[key] = (pays, torch.from_numpy(row_map).cuda(), torch.from_numpy(taps.view(np.int32)).cuda())
    return (got[1], got[2]) if (got[0] or force) else None


def conv_takes_rowmap(x, pc, stride=1, padding="valid", act=None, layout=0, tile=0):
    """Can ``conv2d(x, pc, ..., rowmap=True)`` assign its rows to tiles by a map (frcnn_conv2d_rowmap_available: the f16x3 engine's 256x128
    ring reading planes, [roi][h][w][c] rows, un-split)?  Whether the map PAYS is a second question (``_conv_rowmap``)."""
    if not isinstance(pc, PackedConv) or not isinstance(x, PlaneTensor) or layout:
        return False
    d = _conv_desc(tuple(x.shape), pc.kh, pc.kw, pc.cout, stride, padding, ACT[act], layout, tile or AUTO_TILE)
    eng = _split_engine(d, pc, tile or AUTO_TILE)
    got = _lib.load().frcnn_conv2d_rowmap_available(ctypes.byref(d), {None: 0, "x6": 1, "h3": 2}[eng], 1)
    if got < 0:
        _lib.check(got, "frcnn_conv2d_rowmap_available")
    return got == 1 and _planes_ok(d, pc, eng)


def _h3_planes_in_name(d, pc):
    """The kernel a plane-input launch runs: the plane-reading instantiation of the 256x128 double buffer (which walks long reductions on
    its three-stage ring, csrc/conv_h3.hip h3_ring_tile: one kernel, two loops)."""
    return _h3_name(d).replace(">", ",planes>")


def _planes_ok(d, pc, eng):
    """A launch may read / write fp16 planes: the f16x3 engine on its double-buffered 256x128 tile, un-split, channel counts the 16- and
    8-byte pieces divide."""
    return (eng == "h3" and _lib.load().frcnn_conv2d_h3_config(ctypes.byref(d), 0) in (86, 85, 82) and pc.cout % 4 == 0 and pc.cin % 8 == 0
            and (_CONV_WS is NO_SPLIT_K or _ws_need(d, "frcnn_conv2d_h3_workspace_bytes") == 0))


def conv2d(x, pc, stride=1, padding="valid", act=None, residual=None, out=None, tile=0, layout=0, planes_out=False, rowmap=False):
    """x: (n,h,w,cin) f32 NHWC device tensor; pc: PackedConv -> (n,ho,wo,cout).
    layout=1: position-major tensors, x (h,w,n,cin) -> (ho,wo,n,cout) (frcnn_conv_desc.layout).
    ``planes_out``: a REQUEST to hand the result on as a PlaneTensor (the caller knows its only readers are f16x3 convolutions of the
    detector head's size); honoured when this launch runs on the engine's 256x128 tile, otherwise the f32 tensor comes back as usual.
    x may be a PlaneTensor (then the launch must be such a one: anything else raises).
    ``rowmap``: a REQUEST to assign the launch's rows to tiles by padding class, so that a tile skips the filter taps that meet only zero
    padding (include/ext/frcnn_hip_rowmap.h): honoured where ``conv_takes_rowmap`` says the launch can and the map saves tap-tiles
    ("force": wherever the launch can); the same result bit for bit either way, tensors in the same layout."""
    _require_gpu()
    x_planes = isinstance(x, PlaneTensor)
    assert (x_planes or (x.dtype == torch.float32 and x.is_contiguous())) and x.shape[-1] == pc.cin, (x.shape, pc.cin)
    d = _conv_desc(tuple(x.shape), pc.kh, pc.kw, pc.cout, stride, padding, ACT[act], layout, tile or AUTO_TILE)
    n, ho, wo = d.n, d.ho, d.wo
    oshape = (ho, wo, n, pc.cout) if layout else (n, ho, wo, pc.cout)
    res_planes = isinstance(residual, PlaneTensor)
    roi_res = isinstance(residual, RoiResidual)
    if x_planes or planes_out or res_planes or roi_res:
        ok = out is None and _planes_ok(d, pc, _split_engine(d, pc, tile or AUTO_TILE))
        if roi_res and not (ok and conv_takes_roi_res(x, pc, stride, padding, act, layout, tile)):
            raise _lib.FrcnnError("conv2d: this launch cannot gather a RoiResidual (ops.conv_takes_roi_res; frcnn_conv2d_roi_res_available)")
        if (x_planes or res_planes) and not ok:
            raise _lib.FrcnnError("conv2d: a PlaneTensor input / residual needs an f16x3 launch on the 256x128 tile (frcnn_conv2d_fwd_h3_planes)")
        if ok:
            if residual is not None:
                assert tuple(residual.shape) == tuple(oshape) and (res_planes or roi_res or residual.is_contiguous())
            rm = None
            if rowmap and residual is None and conv_takes_rowmap(x, pc, stride, padding, act, layout, tile):
                rm = _conv_rowmap(d, force=rowmap == "force")
            return _conv2d_h3_planes(d, x, pc, residual, oshape, planes_out, act, rm)
    if out is None:
        out = torch.empty(oshape, dtype=torch.float32, device="cuda")
    else:
        assert out.shape == oshape and out.is_contiguous()
    if residual is not None:
        assert residual.shape == out.shape and residual.is_contiguous()
    eng = _split_engine(d, pc, tile or AUTO_TILE)
    ya = xa = None
    if eng is None:
        ya = _amax_new(optional=True) if (_tracking() and pc.cout >= 32) else None      # a native layer in an f16x3 pass leaves max|y| for the layer behind it
        (fn, args), ws = _conv_launch(d, x, pc.w, pc.scale, pc.shift, residual, None, out, ya)
    else:
        fn = "frcnn_conv2d_fwd_" + eng
        ws = _split_k_ws(_ws_need(d, f"frcnn_conv2d_{eng}_workspace_bytes"))
        tail = (_p(pc.scale), _p(pc.shift), _p(residual), None, _p(out))
        if eng == "h3":
            ya, xa = _amax_new(), amax_of(x)
            args = (ctypes.byref(d), _p(x), _p(xa), _p(pc.h3_planes())) + tail + (_p(ya),)
        else:
            args = (ctypes.byref(d), _p(x), _p(pc.x6_planes())) + tail
        args += (_p(ws), ws.numel() if ws is not None else 0)
        _lib.call(fn, *args, _stream())
    if ya is not None or getattr(out, "_amax", None) is not None:
        out._amax = ya                                           # (an `out=` buffer must not keep the record of what it held before)
    _record_launch(lambda: _kernel_name(d, eng, ws), _gemm_shape(d, pc, stride), fn, args, (d, x, pc, residual, out, ws, ya, xa))
    return out


def conv2d_dual(x, pc, n1, stride=1, padding="valid", act1=None, act2=None, layout=0, tile=0):
    """Two layers on the same input in one launch (frcnn_conv2d_fwd_dual): ``pc`` packs the two filters concatenated along
    the output axis, the first ``n1`` output channels are layer 1.  -> (y1 (n,ho,wo,n1), y2 (n,ho,wo,cout-n1))."""
    _require_gpu()
    assert x.dtype == torch.float32 and x.is_contiguous() and x.shape[-1] == pc.cin and 0 < n1 < pc.cout
    d = _conv_desc(tuple(x.shape), pc.kh, pc.kw, pc.cout, stride, padding, 0, layout, tile or AUTO_TILE)
    lead = (d.ho, d.wo, d.n) if layout else (d.n, d.ho, d.wo)
    y1 = torch.empty(lead + (n1,), dtype=torch.float32, device="cuda")
    y2 = torch.empty(lead + (pc.cout - n1,), dtype=torch.float32, device="cuda")
    eng = _split_engine(d, pc, tile or AUTO_TILE)
    ws = a1 = a2 = xa = None
    outs = (_p(y1), n1, ACT[act1], _p(y2), ACT[act2])
    if eng == "h3":
        a1, a2, xa = _amax_new(), _amax_new(), amax_of(x)
        args = (ctypes.byref(d), _p(x), _p(xa), _p(pc.h3_planes()), _p(pc.scale), _p(pc.shift), _p(y1), n1, ACT[act1], _p(a1),
                _p(y2), ACT[act2], _p(a2))
    elif eng == "x6":
        args = (ctypes.byref(d), _p(x), _p(pc.x6_planes()), _p(pc.scale), _p(pc.shift)) + outs
    else:
        ws = _split_k_ws(_ws_need(d, "frcnn_conv2d_dual_workspace_bytes"))
        args = (ctypes.byref(d), _p(x), _p(pc.w), _p(pc.scale), _p(pc.shift)) + outs + (_p(ws), ws.numel() if ws is not None else 0)
    fn = "frcnn_conv2d_fwd_dual" + (f"_{eng}" if eng else "")
    _lib.call(fn, *args, _stream())
    if eng == "h3":
        y1._amax, y2._amax = a1, a2
    _record_launch(lambda: _kernel_name(d, eng, ws, n1), _gemm_shape(d, pc, stride), fn, args, (d, x, pc, y1, y2, ws, a1, a2, xa))
    return y1, y2


def pool2d(x, k, stride, is_max=True, planes_out=False):
    """``planes_out``: a REQUEST for the result as a PlaneTensor (the caller knows its only reader is an f16x3 convolution that reads planes:
    VGG's block<n>_conv1 behind a max-pool); honoured under the f16x3 engine with a magnitude record on x, channels in fours."""
    _require_gpu()
    n, h, w, c = x.shape
    ho, wo = valid_out(h, k, stride), valid_out(w, k, stride)
    if planes_out and F32_ENGINE == "f16x3" and _tracking() and c % 4 == 0:
        out = PlaneTensor((n, ho, wo, c))
        amax_carry(out, x, 0.0, exponent_out=out.exponent)       # a window's maximum / mean cannot exceed the largest |input|: the scale is known before the launch
        yp = _lib.H3Planes(planes=out.planes.data_ptr(), exponent=out.exponent.data_ptr(), status=out._amax.data_ptr() + 4)
        _lib.call("frcnn_pool2d_fwd_planes", _p(x.contiguous()), n, h, w, c, k, stride, 1 if is_max else 0, ctypes.byref(yp), _stream())
        return out
    out = torch.empty((n, ho, wo, c), dtype=torch.float32, device="cuda")
    _lib.call("frcnn_pool2d_fwd", _p(x.contiguous()), n, h, w, c, k, stride, 1 if is_max else 0, _p(out), _stream())
    return amax_carry(out, x)                                    # max / mean of a window never exceeds the largest |input|


def conv_takes_pool(x, pc, stride=1, padding="valid", act=None, layout=0, tile=0, window=49):
    """Would ``conv2d_avgpool(x, pc, ...)`` average inside the convolution's epilogue (frcnn_conv2d_pool_available: a 1x1 / stride-1 launch
    of the f16x3 engine's 256x128 form on sixteen waves that reads planes, [roi][7][7][c] rows, un-split, not the ring, rows a multiple of
    ``window``)?  ``x``: the tensor (f32 or PlaneTensor) the launch will read."""
    if not isinstance(pc, PackedConv) or len(x.shape) != 4:
        return False
    d = _conv_desc(tuple(x.shape), pc.kh, pc.kw, pc.cout, stride, padding, ACT[act], layout, tile or AUTO_TILE)
    eng = _split_engine(d, pc, tile or AUTO_TILE)
    code = {None: 0, "x6": 1, "h3": 2}[eng]
    got = _lib.load().frcnn_conv2d_pool_available(ctypes.byref(d), code, 1 if isinstance(x, PlaneTensor) else 0, int(window))
    if got < 0:
        _lib.check(got, "frcnn_conv2d_pool_available")
    return got == 1 and _planes_ok(d, pc, eng) and window == d.h * d.w


def conv2d_avgpool(x, pc, stride=1, padding="valid", act=None, residual=None, window=49, tile=0, layout=0):
    """``conv2d(x, pc, stride, padding, act, residual, tile=tile, layout=layout)`` followed by the average over each image's WHOLE h x w
    window (``window`` = h * w samples; the detector head: the 7 x 7 samples of a RoI) -> (n, cout) f32.  Where ``conv_takes_pool`` says so
    the average is taken inside the convolution's epilogue (frcnn_conv2d_fwd_h3_pool: the (n,h,w,cout) tensor is never written);
    everywhere else the convolution and ``pool2d`` / ``avgpool_pos_major`` run as two launches.  Either way the result is the same, bit
    for bit."""
    _require_gpu()
    if (layout == 0 and (residual is None or (isinstance(residual, torch.Tensor) and residual.dtype == torch.float32 and residual.is_contiguous()))
            and conv_takes_pool(x, pc, stride, padding, act, layout, tile, window)):
        d = _conv_desc(tuple(x.shape), pc.kh, pc.kw, pc.cout, stride, padding, ACT[act], layout, tile or AUTO_TILE)
        if residual is not None:
            assert tuple(residual.shape) == (d.n, d.ho, d.wo, pc.cout)
        xp = _lib.H3Planes(planes=x.planes.data_ptr(), exponent=x.exponent.data_ptr(), status=None)
        y = torch.empty((d.n, pc.cout), dtype=torch.float32, device="cuda")
        ya, xa = _amax_new(), amax_of(x)                         # ya: max |pooled value|, for an f16x3 reader of y
        fn = "frcnn_conv2d_fwd_h3_pool"
        args = (ctypes.byref(d), None, ctypes.byref(xp), _p(xa), _p(pc.h3_planes()), _p(pc.scale), _p(pc.shift), _p(residual), None, None,
                int(window), _p(y), _p(ya), None)
        _lib.call(fn, *args, _stream())
        y._amax = ya
        # (an instantiation of the plane-reading kernel, listed under that kernel's name with the convolution's FLOP, so that per-kernel
        # figures cover the same launches as before; the fifth word of the shape keeps it apart from the plain launches of the same GEMM
        # where launches are grouped by (kernel, shape) and timed once per group)
        _record_launch(lambda: _h3_planes_in_name(d, pc), _gemm_shape(d, pc, d.stride) + ("pool",), fn, args, (d, x, pc, residual, y, ya, xp, xa), pool=int(window))
        return y
    y = conv2d(x, pc, stride, padding, act, residual, None, tile, layout)
    if layout:
        assert window == y.shape[0] * y.shape[1]
        return avgpool_pos_major(y)
    n, h, w, c = y.shape
    assert h == w and window == h * w
    y = pool2d(y, h, h, False)
    return amax_carry(y.reshape(n, c), y)


def pool2d_extents(x, true_hw):
    """MaxPooling2D((2,2), strides=(2,2)) on the f32 tensors of a canvas pass (frcnn_pool2d_fwd_extents): x (n,hc,wc,C) need NOT be masked;
    true_hw = device int32 (n,2), image i's true (rows, cols) at x's level.  Inside floor(rows/2) x floor(cols/2) the result is
    ``pool2d(x_true, 2, 2)`` bit for bit, every other cell is zero.  Always an f32 tensor (a canvas pass hands no planes across a mask)."""
    _require_gpu()
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4
    assert true_hw.dtype == torch.int32 and true_hw.is_cuda and true_hw.numel() >= 2 * x.shape[0]
    n, h, w, c = (int(v) for v in x.shape)
    out = torch.empty((n, h // 2, w // 2, c), dtype=torch.float32, device="cuda")
    _lib.call("frcnn_pool2d_fwd_extents", _p(x), n, h, w, c, _p(true_hw), _p(out), _stream())
    return amax_carry(out, x)                                    # a maximum (or a zero) never exceeds the largest |input|


def softmax_rows(x, cols=None):
    _require_gpu()
    rows, ld = x.shape
    cols = ld if cols is None else cols
    out = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
    _lib.call("frcnn_softmax_rows", _p(x.contiguous()), rows, cols, ld, _p(out), cols, _stream())
    return out


def dense_heads_split(y, num_classes):
    """(rows, C + 4(C-1)) output of the merged dense GEMM -> (softmax class probabilities (rows, C), regressions
    (rows, 4(C-1))), both dense, in one launch."""
    _require_gpu()
    rows, ld = y.shape
    tail = ld - num_classes
    cls = torch.empty((rows, num_classes), dtype=torch.float32, device="cuda")
    reg = torch.empty((rows, tail), dtype=torch.float32, device="cuda")
    _lib.call("frcnn_dense_heads_split", _p(y.contiguous()), rows, num_classes, tail, ld, _p(cls), _p(reg), _stream())
    return cls, reg


# ----------------------------------------------------------------------------- detections
def detections(rois, n_rois, out_cls, out_reg, roi_batch, bg_idx, det_threshold, stride, resize_ratio, nms_thresh=0.5):
    """voc_dets.get_dets post-process on the device -> dict of device tensors."""
    _require_gpu()
    rows, C = out_cls.shape
    # ONE allocation, the five outputs are views into it: a client that wants the detections on the host moves
    # `det_packed` with a single copy (five small D2H copies cost ~0.25 ms of stream time per image; split_detections()
    # carves the same views out of the host copy).  Layout in 4-byte words: [n_dets, pad x3 | bbox 4R | cls R | prob R | roi R]
    packed = torch.empty(4 + 7 * rows, dtype=torch.int32, device="cuda")      # the call writes every row (-1 / 0 past n_dets)
    n_dets, det_bbox, det_cls, det_prob, det_roi = split_detections(packed, rows)
    _lib.call("frcnn_detections", _p(rois), _p(n_rois), rows, _p(out_cls.contiguous()), _p(out_reg.contiguous()), C, int(bg_idx),
              float(det_threshold), float(stride), float(resize_ratio), float(nms_thresh),
              _p(det_cls), _p(det_prob), _p(det_bbox), _p(det_roi), _p(n_dets), _stream())
    return {"det_cls": det_cls, "det_prob": det_prob, "det_bbox": det_bbox, "det_roi": det_roi, "n_dets": n_dets, "det_packed": packed}


def detections_dyn(rois, n_rois, out_cls, out_reg, roi_batch, bg_idx, stride, dyn, nms_thresh=0.5):
    """`detections` for a captured pass that serves every image of one size: resize_ratio and det_threshold are read from
    the device tensor ``dyn`` (2 x f64), the reference's padded RoI list is scored when ``roi_batch`` > 0, and word 1 of
    `det_packed` carries the number of proposals the NMS kept (frcnn_detections_dyn)."""
    _require_gpu()
    rows, C = out_cls.shape
    assert dyn.dtype == torch.float64 and dyn.numel() >= 2 and dyn.is_cuda
    packed = torch.empty(4 + 7 * rows, dtype=torch.int32, device="cuda")
    n_dets, det_bbox, det_cls, det_prob, det_roi = split_detections(packed, rows)
    _lib.call("frcnn_detections_dyn", _p(rois), _p(n_rois), int(roi_batch), rows, _p(out_cls.contiguous()), _p(out_reg.contiguous()), C,
              int(bg_idx), float(stride), float(nms_thresh), dyn.data_ptr(),
              _p(det_cls), _p(det_prob), _p(det_bbox), _p(det_roi), _p(packed), _stream())
    return {"det_cls": det_cls, "det_prob": det_prob, "det_bbox": det_bbox, "det_roi": det_roi, "n_dets": n_dets, "det_packed": packed}


DET_POST_MODES = _lib.DETECT_POST_MODES
DET_POST_FIELDS = ("mode", "nms_thresh", "sigma", "min_score", "vote_iou")


def det_post_option(post=None):
    """(host only) The post-process option checked -> (mode, nms_thresh, sigma, min_score, vote_iou) (DESIGN §8 "Post-process rule",
    include/ext/frcnn_hip_detect_post.h).  ``post``: None, a mode name, a tuple in that order (missing tail = defaults) or a dict of those
    names.  mode ``hard`` | ``soft_linear`` | ``soft_gaussian`` (None: hard); nms_thresh in [0, 1] (None: 0.5); sigma > 0 (None: 0.5);
    min_score None (the image's det_threshold) or in [0, 1]; vote_iou None (no voting) or in (0, 1].  sigma 0.5, voting at 0.5 and
    min_score = det_threshold are PROVISIONAL: their effect on mAP has not been measured on a dataset.  ValueError with the reason."""
    if post is None:
        post = ()
    if isinstance(post, str):
        post = (post,)
    if isinstance(post, dict):
        unknown = sorted(set(post) - set(DET_POST_FIELDS))
        if unknown:
            raise ValueError("post-process option: unknown field(s) %s (%s)" % (", ".join(map(repr, unknown)), ", ".join(DET_POST_FIELDS)))
        post = tuple(post.get(k) for k in DET_POST_FIELDS)
    if not isinstance(post, (tuple, list)) or len(post) > len(DET_POST_FIELDS):
        raise ValueError("post-process option %r: None, a mode name, a dict or a tuple of at most (%s)" % (post, ", ".join(DET_POST_FIELDS)))
    mode, nt, sigma, min_score, vote = tuple(post) + (None,) * (len(DET_POST_FIELDS) - len(post))
    mode = "hard" if mode is None else mode
    if mode not in DET_POST_MODES:
        raise ValueError("post-process mode %r: one of %s" % (mode, ", ".join(DET_POST_MODES)))

    def number(name, v):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or v != v:
            raise ValueError("post-process %s=%r: a number" % (name, v))
        return float(v)
    d_nt, d_sigma, _ = _lib.DETECT_POST_DEFAULTS
    nt = d_nt if nt is None else number("nms_thresh", nt)
    if not 0.0 <= nt <= 1.0:
        raise ValueError("post-process nms_thresh=%r: in [0, 1]" % nt)
    sigma = d_sigma if sigma is None else number("sigma", sigma)
    if not (sigma > 0.0 and sigma != float("inf")):
        raise ValueError("post-process sigma=%r: finite and > 0" % sigma)
    if min_score is not None:
        min_score = number("min_score", min_score)
        if not 0.0 <= min_score <= 1.0:
            raise ValueError("post-process min_score=%r: None (the image's det_threshold) or in [0, 1]" % min_score)
    if vote is not None:
        vote = number("vote_iou", vote)
        if not 0.0 < vote <= 1.0:
            raise ValueError("post-process vote_iou=%r: None (no voting) or in (0, 1]" % vote)
    return (mode, nt, sigma, min_score, vote)


def _det_post_args(post):
    mode, nt, sigma, min_score, vote = det_post_option(post)
    return nt, (DET_POST_MODES.index(mode), sigma, -1.0 if min_score is None else min_score, 0.0 if vote is None else vote)


def detections_post(rois, n_rois, out_cls, out_reg, roi_batch, bg_idx, det_threshold, stride, resize_ratio, post=None):
    """``detections`` under the post-process option ``post`` (``det_post_option``; its nms_thresh is the NMS threshold): soft-NMS and box
    voting on the device, the same outputs (frcnn_detections_post).  ``det_prob`` is the decayed score in the soft modes."""
    _require_gpu()
    nt, extra = _det_post_args(post)
    rows, C = out_cls.shape
    packed = torch.empty(4 + 7 * rows, dtype=torch.int32, device="cuda")
    n_dets, det_bbox, det_cls, det_prob, det_roi = split_detections(packed, rows)
    _lib.call("frcnn_detections_post", _p(rois), _p(n_rois), rows, _p(out_cls.contiguous()), _p(out_reg.contiguous()), C, int(bg_idx),
              float(det_threshold), float(stride), float(resize_ratio), nt,
              _p(det_cls), _p(det_prob), _p(det_bbox), _p(det_roi), _p(n_dets), *extra, _stream())
    return {"det_cls": det_cls, "det_prob": det_prob, "det_bbox": det_bbox, "det_roi": det_roi, "n_dets": n_dets, "det_packed": packed}


def detections_post_dyn(rois, n_rois, out_cls, out_reg, roi_batch, bg_idx, stride, dyn, post=None):
    """``detections_dyn`` under the post-process option ``post`` (frcnn_detections_post_dyn): a min_score of None is ``dyn[1]``."""
    _require_gpu()
    nt, extra = _det_post_args(post)
    rows, C = out_cls.shape
    assert dyn.dtype == torch.float64 and dyn.numel() >= 2 and dyn.is_cuda
    packed = torch.empty(4 + 7 * rows, dtype=torch.int32, device="cuda")
    n_dets, det_bbox, det_cls, det_prob, det_roi = split_detections(packed, rows)
    _lib.call("frcnn_detections_post_dyn", _p(rois), _p(n_rois), int(roi_batch), rows, _p(out_cls.contiguous()), _p(out_reg.contiguous()),
              C, int(bg_idx), float(stride), nt, dyn.data_ptr(),
              _p(det_cls), _p(det_prob), _p(det_bbox), _p(det_roi), _p(packed), *extra, _stream())
    return {"det_cls": det_cls, "det_prob": det_prob, "det_bbox": det_bbox, "det_roi": det_roi, "n_dets": n_dets, "det_packed": packed}


# ----------------------------------------------------------------------------- annotation
ANNOTATE_SKIP = ("DontCare", "Misc")            # classes the reference's annotate_video.py:33-34 never draws
ANNOTATE_LABEL_STRIDE = 32                      # bytes per class name in the label table (NUL included)


def annotate_tables(class_names, skip=ANNOTATE_SKIP):
    """The device tables ``annotate_u8`` reads, built once per class list: ``class_names[i]`` is the name of class index i.
    -> {"drawable": u8 [C], "labels": u8 [C][ANNOTATE_LABEL_STRIDE] NUL-terminated ASCII, "glyphs": u8 [95][7]}."""
    from .annotate_font import GLYPHS
    _require_gpu()
    names = list(class_names)
    labels = np.zeros((len(names), ANNOTATE_LABEL_STRIDE), dtype=np.uint8)
    for i, name in enumerate(names):
        raw = str(name).encode("ascii", "replace")
        if len(raw) >= ANNOTATE_LABEL_STRIDE:
            raise ValueError("class name %r longer than %d bytes" % (name, ANNOTATE_LABEL_STRIDE - 1))
        labels[i, :len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    drawable = np.array([name not in skip for name in names], dtype=np.uint8)
    return {"drawable": torch.from_numpy(drawable).cuda(), "labels": torch.from_numpy(labels).cuda(),
            "glyphs": torch.from_numpy(np.ascontiguousarray(GLYPHS)).cuda()}


def annotate_u8(frame, det_packed, tables, ids=None, tracked=False):
    """Draw the detections of ``det_packed`` (the post-process's packed buffer, device) into ``frame`` -- an (h, w, 3) uint8 device
    tensor, edited in place -- as the reference's annotate_video.py:32-41 does: a 3-pixel (0,255,0) box and the label
    "{} {:6.2f}" under it (frcnn_annotate_u8; the drawing rule is DESIGN §8's).  ``tables``: ``annotate_tables``.  Reads
    n_dets from device memory: the call can be captured in a graph.
    ``ids``: an int32 device tensor, one track id per row of ``det_packed`` -- a row whose id is > 0 is labelled "{}#{} {:6.2f}" with the
    id behind the class name (frcnn_annotate_ids_u8); None: the call and its output are what they were.
    ``tracked`` True: ``det_packed`` is one tracked buffer of ``track_update`` instead; its LIVE rows are drawn, with their ids."""
    _require_gpu()
    _frame_u8(frame)
    assert det_packed.is_cuda and det_packed.dtype == torch.int32 and det_packed.is_contiguous()
    labels = tables["labels"]
    if tracked:
        assert ids is None and det_packed.dim() == 1
        _, n_dets, _, _, det_bbox, det_cls, det_prob, ids, _ = split_tracked(det_packed)
    else:
        n_dets, det_bbox, det_cls, det_prob, _ = split_detections(det_packed)
    if ids is None:
        _lib.call("frcnn_annotate_u8", _p(frame), int(frame.shape[0]), int(frame.shape[1]), _p(det_bbox), _p(det_cls), _p(det_prob),
                  _p(n_dets), int(det_cls.numel()), _p(tables["drawable"]), _p(labels), int(labels.shape[1]), int(labels.shape[0]),
                  _p(tables["glyphs"]), _stream())
        return frame
    assert ids.is_cuda and ids.dtype == torch.int32 and ids.is_contiguous() and ids.numel() == det_cls.numel()
    _lib.call("frcnn_annotate_ids_u8", _p(frame), int(frame.shape[0]), int(frame.shape[1]), _p(det_bbox), _p(det_cls), _p(det_prob), _p(ids),
              _p(n_dets), int(det_cls.numel()), _p(tables["drawable"]), _p(labels), int(labels.shape[1]), int(labels.shape[0]),
              _p(tables["glyphs"]), _stream())
    return frame


# ----------------------------------------------------------------------------- redaction
REDACT_MODES = tuple(_lib.REDACT_MODES)         # "fill", "pixelate", "blur"
REDACT_SIZES = _lib.REDACT_SIZES                # mode -> (smallest, largest, default) ``size``


def redact_class_list(class_names, redact_classes):
    """(host only) The names ``redact_classes`` selects out of ``class_names`` (index = class index): "all" (or ("all",)) = every
    class but the background "bg" and the unnamed indices; else an iterable of names, each of which must be one of those --
    ValueError, listing them, for any other."""
    names = [str(n) for n in class_names]
    valid = [n for n in names if n and n != "bg"]
    if redact_classes == "all" or tuple(redact_classes) == ("all",):
        return tuple(valid)
    if isinstance(redact_classes, str):
        redact_classes = (redact_classes,)
    unknown = [c for c in redact_classes if c not in valid]
    if unknown:
        raise ValueError("redact: unknown class name%s %s; the classes are: %s (or \"all\")"
                         % ("s" if len(unknown) > 1 else "", ", ".join(repr(c) for c in unknown), ", ".join(valid)))
    return tuple(redact_classes)


def redact_size(mode, size=None):
    """(host only) ``size`` of ``mode`` checked, None replaced by the mode's default: the side P of a pixelate cell (2..64, default
    16), the radius r of the blur (1..32, default 12), 0 for fill.  ValueError for an unknown mode or a size out of its range."""
    if mode not in REDACT_SIZES:
        raise ValueError("redact mode %r: one of %s" % (mode, ", ".join(REDACT_MODES)))
    lo, hi, default = REDACT_SIZES[mode]
    if size is None:
        return default
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or not lo <= int(size) <= hi:
        raise ValueError("redact size %r out of range for mode \"%s\": %s" % (size, mode, "it takes none" if hi == 0 else "%d..%d" % (lo, hi)))
    return int(size)


def redact_table(class_names, redact_classes):
    """The per-class byte table ``redact_u8`` reads: device u8 [C], 1 where ``class_names[i]`` is redacted.  ``redact_classes``: names,
    or "all" for every class but the background (``redact_class_list``)."""
    _require_gpu()
    chosen = set(redact_class_list(class_names, redact_classes))
    return torch.from_numpy(np.array([str(n) in chosen for n in class_names], dtype=np.uint8)).cuda()


def redact_ws_bytes(h, w, mode="pixelate", size=None):
    """Bytes of workspace ``redact_u8`` needs for an (h, w) frame (frcnn_redact_ws_bytes): 0 for "fill"."""
    return int(_lib.load().frcnn_redact_ws_bytes(int(h), int(w), _lib.REDACT_MODES[mode], redact_size(mode, size)))


def redact_u8(frame, det_packed, table, mode="pixelate", size=None, margin=0, workspace=None, tracked=False):
    """Hide the detections of ``det_packed`` (the post-process's packed buffer, device) whose class is set in ``table``
    (``redact_table``) in ``frame`` -- an (h, w, 3) uint8 device tensor, edited in place and returned: every pixel inside a box grown by
    ``margin`` and clipped to the frame becomes 0 ("fill"), the mean of its cell of a ``size`` x ``size`` grid ("pixelate") or a box blur
    of radius ``size`` ("blur") of the SOURCE frame (frcnn_redact_u8; the rule is DESIGN §8's).  ``size`` None: the mode's default.
    ``workspace``: a u8 device tensor of at least ``redact_ws_bytes`` bytes; None allocates one.  Reads n_dets from device memory: the
    call can be captured in a graph.  ``tracked`` True: ``det_packed`` is one tracked buffer of ``track_update`` instead, and the boxes
    are all its rows, the held ones included."""
    _require_gpu()
    h, w = _frame_u8(frame)
    assert det_packed.is_cuda and det_packed.dtype == torch.int32 and det_packed.is_contiguous()
    assert table.is_cuda and table.dtype == torch.uint8 and table.dim() == 1 and table.is_contiguous()
    if mode not in _lib.REDACT_MODES:
        raise ValueError("redact mode %r: one of %s" % (mode, ", ".join(REDACT_MODES)))
    size = REDACT_SIZES[mode][2] if size is None else int(size)            # (the range is the library's to check)
    if workspace is None:
        workspace = _ws(_lib.load().frcnn_redact_ws_bytes(h, w, _lib.REDACT_MODES[mode], size))
    assert workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous()
    if tracked:                                         # (every row up to n_rows: the held ones too)
        assert det_packed.dim() == 1
        n_dets, _, _, _, det_bbox, det_cls, _, _, _ = split_tracked(det_packed)
    else:
        n_dets, det_bbox, det_cls, _, _ = split_detections(det_packed)
    _lib.call("frcnn_redact_u8", _p(frame), h, w, _p(det_bbox), _p(det_cls), _p(n_dets), int(det_cls.numel()), _p(table),
              int(table.numel()), _lib.REDACT_MODES[mode], size, int(margin), _p(workspace), int(workspace.numel()), _stream())
    return frame


REDACT_SHAPES = tuple(_lib.REDACT_SHAPES)       # "box", "ellipse"
REDACT_FEATHER = _lib.REDACT_FEATHER            # (smallest, largest) feather in pixels


def redact_shape_option(shape=None, feather=None):
    """(host only) (shape, feather) checked, None replaced by the default ("box", 0): shape "box" or "ellipse", feather the pixels the
    edge ramps outwards over, 0..32 (DESIGN §8 "Shape rule").  ValueError with the reason."""
    shape = "box" if shape is None else shape
    feather = 0 if feather is None else feather
    if not isinstance(shape, str) or shape not in _lib.REDACT_SHAPES:
        raise ValueError("redact shape %r: one of %s" % (shape, ", ".join(REDACT_SHAPES)))
    lo, hi = REDACT_FEATHER
    if isinstance(feather, bool) or not isinstance(feather, (int, np.integer)) or not lo <= int(feather) <= hi:
        raise ValueError("redact feather %r: an integer in %d..%d" % (feather, lo, hi))
    return shape, int(feather)


def redact_shaped_u8(frame, det_packed, table, mode="pixelate", size=None, margin=0, shape="box", feather=0, workspace=None, tracked=False):
    """``redact_u8`` with a shaped, soft-edged mask (frcnn_redact_shaped_u8, csrc/redact_shape.hip; DESIGN §8 "Shape rule"): every box
    is grown by ``margin`` and NOT clipped; ``shape`` "ellipse" hides the ellipse inscribed in it; the replacement is blended in with a
    weight that is full inside the shape and ramps to nothing over ``feather`` pixels OUTSIDE it, the largest weight of any row
    winning.  ("box", 0) gives ``redact_u8``'s bytes.  Every other argument, the workspace (``redact_ws_bytes``) and the return are
    ``redact_u8``'s; the shape and the feather range are the library's to check."""
    _require_gpu()
    h, w = _frame_u8(frame)
    assert det_packed.is_cuda and det_packed.dtype == torch.int32 and det_packed.is_contiguous()
    assert table.is_cuda and table.dtype == torch.uint8 and table.dim() == 1 and table.is_contiguous()
    if mode not in _lib.REDACT_MODES:
        raise ValueError("redact mode %r: one of %s" % (mode, ", ".join(REDACT_MODES)))
    if shape not in _lib.REDACT_SHAPES:
        raise ValueError("redact shape %r: one of %s" % (shape, ", ".join(REDACT_SHAPES)))
    size = REDACT_SIZES[mode][2] if size is None else int(size)            # (the range is the library's to check)
    if workspace is None:
        workspace = _ws(_lib.load().frcnn_redact_ws_bytes(h, w, _lib.REDACT_MODES[mode], size))
    assert workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous()
    if tracked:                                         # (every row up to n_rows: the held ones too)
        assert det_packed.dim() == 1
        n_dets, _, _, _, det_bbox, det_cls, _, _, _ = split_tracked(det_packed)
    else:
        n_dets, det_bbox, det_cls, _, _ = split_detections(det_packed)
    _lib.call("frcnn_redact_shaped_u8", _p(frame), h, w, _p(det_bbox), _p(det_cls), _p(n_dets), int(det_cls.numel()), _p(table),
              int(table.numel()), _lib.REDACT_MODES[mode], size, int(margin), _lib.REDACT_SHAPES[shape], int(feather), _p(workspace),
              int(workspace.numel()), _stream())
    return frame


# ----------------------------------------------------------------------------- tracking
TRACK_MAX = _lib.TRACK_MAX                     # slots of a state, at most
TRACK_DEFAULTS = _lib.TRACK_DEFAULTS            # (thr, hold, grow)


def _int_option(what, v, lo, hi, default=None, note=""):
    """(host only) What the tracker's option validators share: ``v`` as an int in lo..hi, None read as ``default``; else ValueError
    "<what>=<v>: an integer in lo..hi<note>"."""
    v = default if v is None else v
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError("%s=%r: an integer in %d..%d%s" % (what, v, lo, hi, note))
    return int(v)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _width_option(what, v, spec):
    """(host only) The width something is drawn with, ``spec`` its (smallest, largest, default)."""
    lo, hi, default = spec
    return _int_option(what, v, lo, hi, default, " (pixels)")


def _classes_option(what, classes, none_is_all, empty_ok=False):
    """(host only) The classes of an option checked -> "all" or a tuple of class names (which names there are is the caller's to check:
    ``redact_class_list``).  ``classes``: "all", one name or a list of names; None reads as "all" with ``none_is_all`` and is refused
    without.  ``empty_ok``: no name at all is a value too, and a refusal shows ``classes`` as given, not as a tuple.  ValueError
    "<what>=<classes>: ..." with the reason."""
    given = classes
    if classes is None and none_is_all:
        classes = "all"
    if isinstance(classes, str):
        classes = (classes,)
    try:
        classes = tuple(classes)
    except TypeError:
        raise ValueError("%s=%r: \"all\", a class name or a list of class names" % (what, given)) from None
    if not (classes or empty_ok) or not all(isinstance(c, str) and c for c in classes):
        raise ValueError("%s=%r: \"all\", a class name or a list of class names" % (what, given if empty_ok else classes))
    return "all" if classes == ("all",) else classes


def _frame_u8(frame):
    """What the calls that edit a frame in place take: an (h, w, 3) uint8 device tensor, contiguous -> (h, w)."""
    assert frame.is_cuda and frame.dtype == torch.uint8 and frame.dim() == 3 and frame.shape[2] == 3 and frame.is_contiguous()
    return int(frame.shape[0]), int(frame.shape[1])


def track_option(thr=None, hold=None, grow=None):
    """(host only) (thr, hold, grow) checked, None replaced by the default (30, 8, 0): thr the IoU threshold in percent, 1..100; hold the
    frames a lost track is kept, 0..255; grow the pixels a held box grows by per frame of age, 0..64.  ValueError with the reason."""
    return tuple(_int_option("track " + name, v, lo, hi, default)
                 for name, v, default, (lo, hi) in zip(("thr", "hold", "grow"), (thr, hold, grow), TRACK_DEFAULTS, _lib.TRACK_RANGES))


def track_state(capacity=64):
    """An empty tracker state of ``capacity`` slots (1..TRACK_MAX): a zeroed int32 device tensor of frcnn_track_state_bytes / 4 words,
    [n_slots, ids issued, overflow, frames | id | cls | bbox | prob | age] (include/ext/frcnn_hip_track.h)."""
    _require_gpu()
    n = int(_lib.load().frcnn_track_state_bytes(int(capacity)))
    if n == 0:
        raise _lib.FrcnnError("track_state: capacity=%r not in [1, %d]" % (capacity, TRACK_MAX))
    return torch.zeros(n // 4, dtype=torch.int32, device="cuda")


def track_capacity(state):
    return (int(state.numel()) - 4) // 8


def track_reset(state):
    """Empty the state (on the current stream): no tracks, the next id is 1, overflow and the frame count 0."""
    state.zero_()
    return state


def track_table(class_names, classes):
    """The per-class byte table ``track_update`` reads: device u8 [C], 1 where ``class_names[i]`` is tracked.  ``classes``: names, or
    "all" for every class but the background (``redact_class_list``'s reading)."""
    _require_gpu()
    chosen = set(redact_class_list(class_names, classes))
    return torch.from_numpy(np.array([str(n) in chosen for n in class_names], dtype=np.uint8)).cuda()


def track_rows(det_packed):
    """Rows of a ``det_packed`` buffer (or of each of a batch of them)."""
    one = det_packed[0] if isinstance(det_packed, (list, tuple)) or det_packed.dim() == 2 else det_packed
    return (int(one.numel()) - 4) // 7


def _track_call(who, state, det_packed, n_frames, table, h, w, thr, hold, grow, out, strong, motion=None, radius=None, interval=None,
                cut=None):
    """What the four ``track_update*`` functions do, ``who`` being the one that asks: the call prepared, checked and made -- frcnn_<who>,
    or with a ``strong`` its _weak twin -- with each optional group of the argument list stated once.  ``motion``: (mstate, frames_u8,
    frame_stride), and ``radius`` with it; ``interval``: not None where ``det_packed`` holds the KEY frames' buffers, B of them for the
    call's F frames; ``cut``: (pct, cuts, workspace).  ``out``, ``cuts`` and ``workspace`` are allocated here when None.
    -> (``out``, ``cuts``), ``cuts`` None without ``cut``."""
    _require_gpu()
    # the tensor frame 0's packed buffer starts at, the buffers' distance in words, B of them, a buffer's words
    if isinstance(det_packed, (list, tuple)):
        bufs = list(det_packed)
        assert bufs and all(b.is_cuda and b.dtype == torch.int32 and b.dim() == 1 and b.is_contiguous() and b.numel() == bufs[0].numel() for b in bufs)
        B, words = len(bufs), int(bufs[0].numel())
        step = (bufs[1].data_ptr() - bufs[0].data_ptr()) if B > 1 else 4 * words
        if B == 1 or (step % 4 == 0 and step >= 4 * words and all(bufs[i].data_ptr() - bufs[0].data_ptr() == i * step for i in range(B))):
            base, stride = bufs[0], step // 4
        else:
            base, stride = torch.stack(bufs), words
    else:
        assert det_packed.is_cuda and det_packed.dtype == torch.int32 and det_packed.is_contiguous() and det_packed.dim() in (1, 2)
        base = det_packed
        B, words = (1, int(base.numel())) if base.dim() == 1 else (int(base.shape[0]), int(base.shape[1]))
        stride = words
    mstate, frames_u8, frame_stride = motion if motion is not None else (None, None, None)
    F = B                                               # the call's frames: one per packed buffer, unless those are the key frames'
    if interval is not None:                            # -- then ``out`` or ``frames_u8`` says how many, and B has to go with it
        interval = int(interval)
        F = int(out.shape[0]) if out is not None else int(frames_u8.shape[0]) if frames_u8.dim() > 1 else B * interval
        if not _lib.TRACK_INTERVAL[0] <= interval <= _lib.TRACK_INTERVAL[1] or (F + interval - 1) // interval != B:
            raise _lib.FrcnnError("%s: interval=%d (1..%d) and %d frames do not go with %d key frames' detections"
                                  % (who, interval, _lib.TRACK_INTERVAL[1], F, B))
    motion_args = options = cut_args = ()
    if motion is not None:
        assert mstate.is_cuda and mstate.dtype == torch.uint8 and mstate.dim() == 1 and mstate.is_contiguous() and mstate.numel() == 16 + 3 * int(h) * int(w)
        assert frames_u8.is_cuda and frames_u8.dtype == torch.uint8 and frames_u8.is_contiguous()
        assert int(frames_u8.numel()) >= (F - 1) * int(frame_stride) + 3 * int(h) * int(w) and int(frame_stride) >= 0
        motion_args = (_p(mstate), _p(frames_u8), int(frame_stride))
        options = (int(radius),) if interval is None else (int(radius), interval)
    assert state.is_cuda and state.dtype == torch.int32 and state.dim() == 1 and state.is_contiguous()
    assert n_frames.is_cuda and n_frames.dtype == torch.int32 and n_frames.numel() >= 1
    assert table.is_cuda and table.dtype == torch.uint8 and table.dim() == 1 and table.is_contiguous()
    cap, rows = track_capacity(state), (words - 4) // 7
    R = rows + cap
    if out is None:
        out = torch.empty((F, 4 + 8 * R), dtype=torch.int32, device="cuda")
    assert out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (F, 4 + 8 * R)
    cuts = None
    if cut is not None:
        pct, cuts, workspace = cut
        if cuts is None:
            cuts = torch.empty(F, dtype=torch.int32, device="cuda")
        if workspace is None:
            workspace = track_cut_workspace(F)
        assert cuts.is_cuda and cuts.dtype == torch.int32 and cuts.is_contiguous() and cuts.numel() == F
        assert workspace.is_cuda and workspace.dtype == torch.int32 and workspace.is_contiguous() and workspace.numel() >= 512 * (F + 1)
        cut_args = (pct, _p(workspace), _p(cuts))
    name, weak = ("frcnn_" + who, ()) if strong is None else ("frcnn_" + who + "_weak", (float(strong),))
    _lib.call(name, _p(state), cap, *motion_args, _p(base), int(stride), F, _p(n_frames), rows, _p(table), int(table.numel()),
              int(thr), int(hold), int(grow), *options, int(h), int(w), *weak, _p(out), 4 + 8 * R, *cut_args, _stream())
    return out, cuts


def track_weak_option(det_threshold=None, low=None, track=True):
    """(host only) The pair (``det_threshold``, ``low``) of the Weak rule (DESIGN §8 "Weak rule") checked -> (T, L): T a float in 0..1, None
    read as 0.0; L None (no weak rows: the Tracking rule) or a float in 0..1 with L < T, which needs ``track``.  With an L the detector
    emits rows down to L and the tracker is told ``strong`` = T.  ValueError with the reason, by name."""
    def number(name, v):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) <= 1.0:
            raise ValueError("%s=%r: a number in 0..1" % (name, v))
        return float(v)
    T = 0.0 if det_threshold is None else number("det threshold", det_threshold)
    if low is None:
        return T, None
    L = number("track low", low)
    if not track:
        raise ValueError("track low=%r needs tracking (track): a weak row can only continue a track" % (low,))
    if not L < T:
        raise ValueError("track low=%r must be below det threshold=%r: the rows between the two are the weak ones" % (low, T))
    return T, L


def track_update(state, det_packed, n_frames, table, h, w, thr=30, hold=8, grow=0, out=None, strong=None):
    """The tracking rule (DESIGN §8 "Tracking rule", frcnn_track_update) over the frames of ``det_packed`` IN ORDER, in one launch:
    ``state`` (``track_state``) is read and advanced, and frame f's tracked buffer lands in ``out[f]`` -- -> ``out``, a (B, 4 + 8R) int32
    tensor, R = the packed buffers' rows + the state's capacity (``split_tracked`` cuts it up; ``redact_u8`` and ``annotate_u8`` take
    ``out[f]`` in a ``det_packed``'s place with ``tracked=True``).  ``det_packed``: one packed buffer of the post-process (B = 1), a
    (B, words) tensor, or a list of B buffers of one size -- used where they lie when they are evenly spaced in memory (the stride is an
    argument of the call), else gathered with one copy.  ``n_frames``: an int32 device tensor whose first word says how many of the B
    frames are real; the rest is a short pass's padding and leaves the state alone.  ``table``: ``track_table``.  (h, w): the frame's size.
    ``strong``: None, or a float for the Weak rule (DESIGN §8 "Weak rule", frcnn_track_update_weak; the same argument of the three forms
    below): a row with a score under it may only continue a track that no other row continued, and is dropped from the live part otherwise,
    so n_live <= *n_dets.  Reads *n_dets and *n_frames on the device: the call can be captured in a graph."""
    return _track_call("track_update", state, det_packed, n_frames, table, h, w, thr, hold, grow, out, strong)[0]


TRACK_MOTION_RADIUS = _lib.TRACK_MOTION_RADIUS  # (smallest, largest, the default) search radius of ``track_update_motion``


def track_motion_radius(r=None):
    """(host only) The block match's search radius checked, None replaced by the default 8: an integer in 1..16.  ValueError with the
    reason."""
    return _int_option("track motion radius", r, *TRACK_MOTION_RADIUS)


def track_motion_state(h, w):
    """A motion state for h x w frames with no reference: a zeroed uint8 device tensor of frcnn_track_motion_state_bytes = 16 + 3hw bytes,
    [kept, h, w, 0 (int32) | the kept frame (h, w, 3)] (include/ext/frcnn_hip_track_motion.h)."""
    _require_gpu()
    n = int(_lib.load().frcnn_track_motion_state_bytes(int(h), int(w)))
    if n == 0:
        raise _lib.FrcnnError("track_motion_state: frame %rx%r out of range (sides 1..%d)" % (h, w, _lib.REDACT_MAX_SIDE))
    return torch.zeros(n, dtype=torch.uint8, device="cuda")


def track_motion_reset(mstate):
    """Forget the kept frame (on the current stream): the header is zeroed, so the next frame has no reference."""
    mstate[:16].zero_()
    return mstate


def track_update_motion(state, mstate, frames_u8, frame_stride, det_packed, n_frames, table, h, w, thr=30, hold=8, grow=0, radius=8, out=None,
                        strong=None):
    """``track_update`` with the motion step in front of every frame's match (DESIGN §8 "Motion rule", frcnn_track_update_motion): every
    live slot's box is first moved by the best integer shift of the pixels under it, found by a block match of radius ``radius`` between
    the frame before and this one, so that a held box follows its object.  ``mstate`` (``track_motion_state(h, w)``) carries the last frame
    of one call to the next.  ``frames_u8``: a uint8 device tensor that holds frame f of the call, (h, w, 3) in any channel order, at
    byte ``f * frame_stride``; read only.  Everything else, ``out`` and the return value: as ``track_update``.  At most two launches per
    frame and one more per call; reads *n_dets, *n_frames and the slot count on the device: the call can be captured in a graph."""
    return _track_call("track_update_motion", state, det_packed, n_frames, table, h, w, thr, hold, grow, out, strong,
                       motion=(mstate, frames_u8, frame_stride), radius=radius)[0]


TRACK_INTERVAL = _lib.TRACK_INTERVAL            # (smallest, largest) interval of ``track_update_interval``; the public option starts at 2


def track_interval_option(k):
    """(host only) ``detect_every`` checked: an integer in 2..16, the frames from one detected frame to the next (1 is plain tracking and
    exists at the ABI only).  ValueError with the reason."""
    return _int_option("detect every", k, 2, TRACK_INTERVAL[1], note=" (the frames from one detected frame to the next)")


def track_update_interval(state, mstate, frames_u8, frame_stride, det_packed, n_frames, table, h, w, thr=30, hold=8, grow=0, radius=8, interval=1,
                          out=None, strong=None):
    """``track_update_motion`` with the detector on every ``interval``-th frame only (DESIGN §8 "Interval rule", frcnn_track_update_interval):
    ``det_packed`` holds the packed buffers of the KEY frames 0, interval, 2 interval, ... of the call -- B of them, as ``track_update``
    takes them --, ``frames_u8`` the F source frames, key and between, ``frame_stride`` bytes apart, with (F + interval - 1) // interval ==
    B; F is the rows of ``out`` (F, 4 + 8R) when given, else of a ``frames_u8`` of two or more dimensions, else B * interval.  A key frame is ``track_update_motion``'s frame; a between
    frame moves every slot by the block match and writes the slots of age 0 as live rows (their moved boxes) and the held ones behind them:
    no match, no ageing, no births, so ``hold`` counts key frames.  ``n_frames``: how many of the F frames are real.  -> ``out``.  At most
    two launches per frame and one more per call; the call can be captured in a graph."""
    return _track_call("track_update_interval", state, det_packed, n_frames, table, h, w, thr, hold, grow, out, strong,
                       motion=(mstate, frames_u8, frame_stride), radius=radius, interval=interval)[0]


TRACK_CUT_PCT = _lib.TRACK_CUT_PCT              # (smallest, largest, the default) threshold of ``track_update_cut``, in percent


def track_cut_option(pct=None):
    """(host only) The scene-cut threshold checked, None replaced by the default 40: an integer in 1..100, the share of the largest
    distance two frames' signatures can have at which the later frame is a cut.  The default is PROVISIONAL: no threshold has been
    measured on real footage.  ValueError with the reason."""
    return _int_option("track scene cut", pct, *TRACK_CUT_PCT, note=" (percent)")


def track_cut_workspace(frames):
    """The workspace of ``track_update_cut`` calls of up to ``frames`` frames: an int32 device tensor of
    frcnn_track_cut_workspace_bytes(frames) bytes, (frames + 1) signatures of 512 counters.  Nothing is carried in it between calls."""
    _require_gpu()
    n = int(_lib.load().frcnn_track_cut_workspace_bytes(int(frames)))
    if n == 0:
        raise _lib.FrcnnError("track_cut_workspace: frames=%r out of range (1..%d)" % (frames, _lib.TRACK_MAX_FRAMES))
    return torch.empty(n // 4, dtype=torch.int32, device="cuda")


def track_update_cut(state, mstate, frames_u8, frame_stride, det_packed, n_frames, table, h, w, thr=30, hold=8, grow=0, radius=8, interval=1,
                     pct=None, out=None, cuts=None, workspace=None, strong=None):
    """``track_update_interval`` (``interval`` 1: ``track_update_motion``) with the cut step in front of every frame (DESIGN §8 "Cut rule",
    frcnn_track_update_cut): a frame whose 4 x 4-region luma histogram differs from that of the frame before -- for the call's first
    frame: the kept frame of ``mstate``, when it is the frame before -- by ``pct`` percent (``track_cut_option``) of the largest distance
    there is, is a hard cut, and every track ends in front of it: no id continues across it and no held row crosses it.  ``cuts``: an
    int32 device tensor of F words, 1 where frame f is a cut; ``workspace``: ``track_cut_workspace(F)`` (both allocated here when None;
    a captured call passes them).  Everything else as ``track_update_interval``.  -> (``out``, ``cuts``).  With no cut every byte of
    ``state``, ``mstate`` and ``out`` is ``track_update_interval``'s.  Four launches per call and one per frame on top of those; the
    call can be captured in a graph."""
    pct = track_cut_option(pct) if pct is None else int(pct)
    return _track_call("track_update_cut", state, det_packed, n_frames, table, h, w, thr, hold, grow, out, strong,
                       motion=(mstate, frames_u8, frame_stride), radius=radius, interval=interval, cut=(pct, cuts, workspace))


def _id_update_args(state, tracked, n_frames, gate, table=None):
    """What ``track_trails_update``, ``count_update`` and ``zone_update`` take alike, checked -> (frames, words of a tracked buffer, its
    rows): the state, the (frames, 4 + 8 rows) tracked buffers, the device words ``n_frames`` and ``gate`` (or None), a class table."""
    assert state.is_cuda and state.dtype == torch.int32 and state.dim() == 1 and state.is_contiguous()
    assert tracked.is_cuda and tracked.dtype == torch.int32 and tracked.dim() == 2 and tracked.is_contiguous()
    assert n_frames.is_cuda and n_frames.dtype == torch.int32 and n_frames.numel() >= 1
    assert gate is None or (gate.is_cuda and gate.dtype == torch.int32 and gate.numel() >= 1)
    assert table is None or (table.is_cuda and table.dtype == torch.uint8 and table.dim() == 1 and table.is_contiguous())
    frames, words = int(tracked.shape[0]), int(tracked.shape[1])
    assert (words - 4) % 8 == 0
    return frames, words, (words - 4) // 8


def _lists_workspace(who, frames, words):
    """The lists of one of those calls of ``frames`` frames: an int32 device tensor (frames, ``words``) that every call writes whole."""
    _require_gpu()
    if not 1 <= int(frames) <= _lib.TRACK_MAX_FRAMES:
        raise _lib.FrcnnError("%s: frames=%r out of range (1..%d)" % (who, frames, _lib.TRACK_MAX_FRAMES))
    return torch.empty((int(frames), int(words)), dtype=torch.int32, device="cuda")


def _lists_arg(lists, frames, words):
    assert lists.is_cuda and lists.dtype == torch.int32 and lists.is_contiguous() and tuple(lists.shape) == (frames, words)
    return lists


def _reset_keeping_totals(state, head, keep_totals):
    """Empty a count or zone state (on the current stream); ``keep_totals``: only the count of entries and the entries behind the
    ``head`` words are zeroed."""
    if keep_totals:
        state[0:1].zero_()
        state[head:].zero_()
    else:
        state.zero_()
    return state


TRACK_TRAILS = _lib.TRACK_TRAILS                # ((smallest, largest, default) length N, the same of the width W, the largest expire)


def track_trails_option(value=None):
    """(host only) The trail option checked -> (N, W): N the points a trail keeps, 2..64, W the width it is drawn with, 1..9.  ``value``:
    None (the defaults, 16 and 3), an integer N, or a pair (N, W) either of which may be None.  ValueError with the reason."""
    (n_lo, n_hi, n_def), _, _ = TRACK_TRAILS
    if value is None or isinstance(value, (int, np.integer)):
        value = (value, None)
    try:
        n, wd = value
    except (TypeError, ValueError):
        raise ValueError("track trails=%r: N, or (N, W)" % (value,)) from None
    return _int_option("track trails length", n, n_lo, n_hi, n_def, " (points)"), _width_option("track trails width", wd, TRACK_TRAILS[1])


def _track_trails_words(capacity, length):
    n = int(_lib.load().frcnn_track_trails_list_words(int(capacity), int(length)))
    if n == 0:
        raise _lib.FrcnnError("track trails: capacity=%r not in [1, %d] or length=%r not in [%d, %d]"
                              % (capacity, TRACK_MAX, length, TRACK_TRAILS[0][0], TRACK_TRAILS[0][1]))
    return n


def track_trails_state(capacity, length):
    """An empty trail state of ``capacity`` trails of ``length`` points: a zeroed int32 device tensor of frcnn_track_trails_state_bytes / 4
    words, [n_entries, frames, dropped, 0 | per entry: id, cls, last_seen, n, pts[length][2]] (include/ext/frcnn_hip_track_trails.h).
    Zeroing it (``track_reset``) empties it."""
    _require_gpu()
    return torch.zeros(_track_trails_words(capacity, length), dtype=torch.int32, device="cuda")


def track_trails_workspace(frames, capacity, length):
    """The point lists of a ``track_trails_update`` call of ``frames`` frames: an int32 device tensor (frames, list words), a list
    [n_trails, 0, 0, 0 | per trail: id, cls, n, 0, pts[length][2]].  Every word is written by every call."""
    return _lists_workspace("track_trails_workspace", frames, _track_trails_words(capacity, length))


def track_trails_update(state, tracked, n_frames, length, expire, h, w, capacity=None, lists=None, gate=None):
    """Steps 1-4 of the trail rule (DESIGN §8 "Trail rule", frcnn_track_trails_update) over the frames of ``tracked`` IN ORDER, in one
    launch: ``tracked`` is a (frames, 4 + 8 rows) int32 tensor of tracked buffers -- ``track_update``'s ``out``, or the widened buffers a
    look-back emits --, ``n_frames`` the device word that says how many of them are real.  The centre of every live tracked row joins
    the trail of its id in ``state`` (``track_trails_state``; ``capacity``: its trails, read from its size when None), trails not seen
    for more than ``expire`` frames leave, and frame f's point list lands in ``lists[f]`` (``track_trails_workspace``; allocated here
    when None; a captured call passes it) -> ``lists``.  ``gate``: None, or a device word that is 0 when no frame of the call is real,
    whatever ``n_frames`` says (a pass whose ``n_frames`` is the count a look-back emitted passes its own frame count: a warm-up
    replay emits the same frames again).  The call can be captured in a graph."""
    _require_gpu()
    frames, words, rows = _id_update_args(state, tracked, n_frames, gate)
    length = int(length)
    if capacity is None:
        capacity = (int(state.numel()) - 4) // (4 + 2 * max(length, 1))
    if lists is None:
        lists = track_trails_workspace(frames, capacity, length)
    assert int(state.numel()) == _track_trails_words(capacity, length)
    _lists_arg(lists, frames, int(state.numel()))
    _lib.call("frcnn_track_trails_update", _p(state), int(capacity), _p(tracked), words, rows, frames, _p(n_frames), _p(gate), length,
              int(expire), int(h), int(w), _p(lists), _stream())
    return lists


def track_trails_draw_u8(frame, plist, length, width=None, rgb=False):
    """DRAW of the trail rule (frcnn_track_trails_draw_u8): the trails of ``plist`` -- one point list of ``track_trails_update`` -- drawn
    into ``frame``, an (h, w, 3) uint8 device tensor, edited in place and returned: a capsule of ``width`` pixels (None: 3) around every
    segment, in the colour of the trail's id, the highest id on top.  ``rgb``: the frame's bytes are R, G, B (False: B, G, R, as the
    encoders' ``bgr=True``).  One launch; reads the list's count from device memory, so the call can be captured in a graph."""
    _require_gpu()
    h, w = _frame_u8(frame)
    assert plist.is_cuda and plist.dtype == torch.int32 and plist.dim() == 1 and plist.is_contiguous()
    length, width = int(length), TRACK_TRAILS[1][2] if width is None else int(width)
    assert int(plist.numel()) >= 4 and (int(plist.numel()) - 4) % (4 + 2 * max(length, 1)) == 0
    _lib.call("frcnn_track_trails_draw_u8", _p(frame), h, w, _p(plist), length, width, int(bool(rgb)), _stream())
    return frame


# ----------------------------------------------------------------------------- heat map
HEAT_ALPHA, HEAT_DECAY = _lib.HEAT_ALPHA, _lib.HEAT_DECAY    # (smallest, largest, the default) of the blend weight A and of the decay S
HEAT_MAX = _lib.HEAT_MAX                        # the value a pixel of the map stops at


def heat_option(classes, alpha=None, decay=None):
    """(host only) The heat-map option checked -> (classes, A, S): classes "all" or a tuple of class names (which names there are is the
    caller's to check: ``redact_class_list``), A the blend weight of the hottest pixel, 1..255 (None: 160), S the decay, 0..15 (None: 0,
    none): every frame takes ceil(v / 2^S) off every pixel.  ValueError with the reason."""
    classes = _classes_option("heat classes", classes, False)
    out = []
    for name, v, (lo, hi, default) in (("alpha", alpha, HEAT_ALPHA), ("decay", decay, HEAT_DECAY)):
        v = default if v is None else v
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError("heat %s=%r: an integer in %d..%d" % (name, v, lo, hi))
        out.append(int(v))
    return (classes,) + tuple(out)


def heat_state_words(h, w):
    """(host only) 4-byte words of a heat state BUFFER for frames of (h, w) (frcnn_heat_state_bytes / 4): the state, 4 + h w words
    [frames, peak, saturated, 0 | map[h][w]], and the update kernel's scratch words behind it."""
    n = int(_lib.load().frcnn_heat_state_bytes(int(h), int(w)))
    if n == 0:
        raise _lib.FrcnnError("heat state: frame %rx%r out of range (sides 1..%d)" % (h, w, _lib.REDACT_MAX_SIDE))
    return n // 4


def heat_state(h, w):
    """An empty heat state for frames of (h, w): a zeroed int32 device tensor of ``heat_state_words`` words, [frames, peak, saturated, 0 |
    map[h][w] | scratch] (include/ext/frcnn_hip_heat.h).  Zeroing it (``heat_reset``) empties it; ``heat_map`` cuts the map out of it."""
    _require_gpu()
    return torch.zeros(heat_state_words(h, w), dtype=torch.int32, device="cuda")


def heat_reset(state):
    """Empty the state (on the current stream): no frames, a cold map."""
    state.zero_()
    return state


def heat_map(state, h, w):
    """(frames, peak, saturated, the (h, w) map) of a heat state, device tensor or its host copy (torch or numpy): views."""
    m = state[4:4 + int(h) * int(w)]
    return int(state[0]), int(state[1]), int(state[2]), (m.view(int(h), int(w)) if isinstance(m, torch.Tensor) else m.reshape(int(h), int(w)))


def heat_levels(state, h, w):
    """(host only) The map of a heat state's HOST copy (numpy) as the draw step sees it: uint8 (h, w), t = (v * 255) // peak, all 0 for a
    cold map -- the grey picture ``annotate_video --heatmap_out`` writes."""
    _, peak, _, m = heat_map(np.asarray(state), h, w)
    if peak <= 0:
        return np.zeros((int(h), int(w)), dtype=np.uint8)
    return (np.clip(m.astype(np.int64), 0, peak) * 255 // peak).astype(np.uint8)


def heat_update(state, h, w, det_packed, table, decay=0, frame_index=0, n_frames=None, gate=None, tracked=False):
    """UPDATE of the heat rule (DESIGN §8 "Heat rule", frcnn_heat_update) for one frame of (h, w): the map of ``state`` (``heat_state``)
    decays by ``decay`` and every pixel gains 256 per box of ``det_packed`` that covers it -- the post-process's packed buffer, every row
    of a class set in ``table`` (``redact_table``'s form), or with ``tracked`` True one tracked buffer of ``track_update`` (plain or
    widened), its LIVE rows only.  The frame counts when ``frame_index`` < *``n_frames`` (a device int32 word; None: a word that says 1,
    allocated here -- a captured call passes its own) and, with ``gate`` (a device word), *gate != 0; else nothing is written.  Two
    launches, everything guarded on the device: the call can be captured in a graph -> ``state``."""
    _require_gpu()
    assert state.is_cuda and state.dtype == torch.int32 and state.dim() == 1 and state.is_contiguous()
    assert det_packed.is_cuda and det_packed.dtype == torch.int32 and det_packed.dim() == 1 and det_packed.is_contiguous()
    assert table.is_cuda and table.dtype == torch.uint8 and table.dim() == 1 and table.is_contiguous()
    h, w = int(h), int(w)
    assert int(state.numel()) == heat_state_words(h, w)
    if n_frames is None:
        n_frames = torch.ones(1, dtype=torch.int32, device="cuda")
    assert n_frames.is_cuda and n_frames.dtype == torch.int32 and n_frames.numel() >= 1
    assert gate is None or (gate.is_cuda and gate.dtype == torch.int32 and gate.numel() >= 1)
    per = 8 if tracked else 7
    assert (int(det_packed.numel()) - 4) % per == 0
    _lib.call("frcnn_heat_update", _p(state), h, w, _p(det_packed), (int(det_packed.numel()) - 4) // per, int(bool(tracked)), _p(table),
              int(table.numel()), int(decay), int(frame_index), _p(n_frames), _p(gate), _stream())
    return state


def heat_draw_u8(frame, state, alpha=None, rgb=False):
    """DRAW of the heat rule (frcnn_heat_draw_u8): the map of ``state`` blended into ``frame``, an (h, w, 3) uint8 device tensor, edited
    in place and returned: a pixel at t = (v * 255) // peak takes the ramp's colour (black, red, yellow, white) at weight
    (``alpha`` * t) // 255 (None: 160); a cold map writes nothing.  ``rgb``: the frame's bytes are R, G, B (False: B, G, R, as the
    encoders' ``bgr=True``).  One launch; reads ``peak`` from device memory, so the call can be captured in a graph."""
    _require_gpu()
    h, w = _frame_u8(frame)
    assert state.is_cuda and state.dtype == torch.int32 and state.dim() == 1 and state.is_contiguous()
    assert int(state.numel()) == heat_state_words(h, w)
    _lib.call("frcnn_heat_draw_u8", _p(frame), h, w, _p(state), HEAT_ALPHA[2] if alpha is None else int(alpha), int(bool(rgb)), _stream())
    return frame


# ----------------------------------------------------------------------------- line counts
COUNT_MAX_LINES, COUNT_MAX_EVENTS = _lib.COUNT_MAX_LINES, _lib.COUNT_MAX_EVENTS      # the lines of a call, the events of a frame's list
COUNT_WIDTH = _lib.COUNT_WIDTH                  # (smallest, largest, the default) width W the lines are drawn with
COUNT_LIST_WORDS = _lib.COUNT_LIST_WORDS        # words of a count list: [n_events, frames, 0, 0 | totals[8][2] | events[64][4]]
COUNT_HEAD, COUNT_ENTRY = 4 + 2 * _lib.COUNT_MAX_LINES, 6                            # a state's words in front of its entries; an entry's


def count_option(lines, classes="all", width=None):
    """(host only) The count option checked -> (lines, classes, W): lines a tuple of 1..8 tuples (ax, ay, bx, by) of integers in
    -32768..65535 with A != B (one such tuple alone is one line), classes "all" or a tuple of class names (which names there are is the
    caller's to check: ``redact_class_list``), W the width the lines are drawn with, 1..9 (None: 3).  ValueError with the reason."""
    lo, hi = _lib.COUNT_COORD
    try:
        lines = tuple(lines)
        if len(lines) == 4 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in lines):
            lines = (lines,)
        lines = tuple(tuple(ln) for ln in lines)
    except TypeError:
        raise ValueError("count lines=%r: a list of (ax, ay, bx, by)" % (lines,)) from None
    if not 1 <= len(lines) <= COUNT_MAX_LINES:
        raise ValueError("count lines: %d of them, 1..%d are possible" % (len(lines), COUNT_MAX_LINES))
    for ln in lines:
        if len(ln) != 4 or not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and lo <= int(v) <= hi for v in ln):
            raise ValueError("count line %r: four integers ax, ay, bx, by in %d..%d" % (ln, lo, hi))
        if (int(ln[0]), int(ln[1])) == (int(ln[2]), int(ln[3])):
            raise ValueError("count line %r: A = B is a point, not a line" % (ln,))
    lines = tuple(tuple(int(v) for v in ln) for ln in lines)
    return lines, _classes_option("count classes", classes, True), _width_option("count width", width, COUNT_WIDTH)


def _count_lines_arg(lines):
    """``lines`` (n, 4) as the host int32 array the entry points read (keep the array alive over the call), its pointer and n."""
    a = np.ascontiguousarray(np.asarray(lines, dtype=np.int64).reshape(-1, 4).clip(-2 ** 31, 2 ** 31 - 1), dtype=np.int32)
    return a, a.ctypes.data_as(ctypes.c_void_p), int(a.shape[0])


def count_state_words(capacity):
    """(host only) 4-byte words of a count state of ``capacity`` entries (frcnn_count_state_bytes / 4): 20 + 6 capacity."""
    n = int(_lib.load().frcnn_count_state_bytes(int(capacity)))
    if n == 0:
        raise _lib.FrcnnError("count state: capacity=%r not in [1, %d]" % (capacity, TRACK_MAX))
    return n // 4


def count_state(capacity):
    """An empty count state of ``capacity`` entries: a zeroed int32 device tensor, [n_entries, frames, dropped, events_dropped |
    totals[8][2] | per entry: id, cls, last_seen, counted, px, py] (include/ext/frcnn_hip_count.h).  Zeroing it (``count_reset``) empties
    it, totals included."""
    _require_gpu()
    return torch.zeros(count_state_words(capacity), dtype=torch.int32, device="cuda")


def count_reset(state, keep_totals=False):
    """Empty the state (on the current stream): no entries, no frames, totals 0.  ``keep_totals``: only the entries leave -- the ids end,
    what was counted stays counted (``frames``, the sticky sums and the totals are kept)."""
    return _reset_keeping_totals(state, COUNT_HEAD, keep_totals)


def count_workspace(frames):
    """The count lists of a ``count_update`` call of ``frames`` frames: an int32 device tensor (frames, COUNT_LIST_WORDS).  Every word is
    written by every call."""
    lists = _lists_workspace("count_workspace", frames, COUNT_LIST_WORDS)
    assert int(_lib.load().frcnn_count_list_words()) == COUNT_LIST_WORDS
    return lists


def count_update(state, tracked, n_frames, lines, table, expire, h, w, capacity=None, lists=None, gate=None):
    """Steps 1-4 of the count rule (DESIGN §8 "Count rule", frcnn_count_update) over the frames of ``tracked`` IN ORDER, in one launch:
    ``tracked`` is a (frames, 4 + 8 rows) int32 tensor of tracked buffers -- ``track_update``'s ``out``, or the widened buffers a
    look-back emits --, ``n_frames`` the device word that says how many of them are real.  The centre of every live tracked row of a
    class set in ``table`` (device uint8 [C], ``redact_table``'s form) steps the entry of its id in ``state`` (``count_state``;
    ``capacity``: its entries, read from its size when None) and is tested against ``lines`` ((n, 4) host integers, ax, ay, bx, by); a
    crossing counts once per id, line and direction.  Entries not seen for more than ``expire`` frames leave, and frame f's count list
    lands in ``lists[f]`` (``count_workspace``; allocated here when None; a captured call passes it) -> ``lists``.  ``gate``: None, or a
    device word that is 0 when no frame of the call is real, whatever ``n_frames`` says.  The call can be captured in a graph."""
    _require_gpu()
    frames, words, rows = _id_update_args(state, tracked, n_frames, gate, table)
    if capacity is None:
        capacity = (int(state.numel()) - COUNT_HEAD) // COUNT_ENTRY
    if lists is None:
        lists = count_workspace(frames)
    assert int(state.numel()) == count_state_words(capacity)
    _lists_arg(lists, frames, COUNT_LIST_WORDS)
    keep, lines_p, n_lines = _count_lines_arg(lines)
    _lib.call("frcnn_count_update", _p(state), int(capacity), _p(tracked), words, rows, frames, _p(n_frames), _p(gate), lines_p,
              n_lines, _p(table), int(table.numel()), int(expire), int(h), int(w), _p(lists), _stream())
    return lists


def count_draw_u8(frame, clist, lines, width=None, rgb=False):
    """DRAW of the count rule (frcnn_count_draw_u8): ``lines`` drawn into ``frame``, an (h, w, 3) uint8 device tensor, edited in place and
    returned: each line a capsule of ``width`` pixels (None: 3) in PALETTE[l & 7], and above them a label "L{l} +{pos} -{neg}" per line
    with the totals of ``clist`` -- one count list of ``count_update`` --, formatted on the device.  A list of a frame that is not real
    draws nothing.  ``rgb``: the frame's bytes are R, G, B (False: B, G, R).  One launch; the list is read on the device, so the call can
    be captured in a graph."""
    _require_gpu()
    h, w = _frame_u8(frame)
    assert clist.is_cuda and clist.dtype == torch.int32 and clist.dim() == 1 and clist.is_contiguous() and int(clist.numel()) == COUNT_LIST_WORDS
    keep, lines_p, n_lines = _count_lines_arg(lines)
    _lib.call("frcnn_count_draw_u8", _p(frame), h, w, _p(clist), lines_p, n_lines,
              COUNT_WIDTH[2] if width is None else int(width), int(bool(rgb)), _stream())
    return frame


def count_totals(state):
    """(host only; reads the state back) The totals of a count state, device tensor or host copy -> {"frames", "dropped",
    "events_dropped", "entries", "totals": [(neg, pos)] * 8} -- totals[l] = (crossings of line l in direction -, in direction +)."""
    s = state.cpu().numpy() if isinstance(state, torch.Tensor) else np.asarray(state)
    return {"entries": int(s[0]), "frames": int(s[1]), "dropped": int(s[2]), "events_dropped": int(s[3]),
            "totals": [(int(s[4 + 2 * l]), int(s[5 + 2 * l])) for l in range(COUNT_MAX_LINES)]}


def count_events(clist):
    """(host only) The events of one count list's HOST copy -> [(line, dir, id, cls)], in (row, line) order."""
    c = np.asarray(clist)
    return [tuple(int(v) for v in c[COUNT_HEAD + 4 * k:COUNT_HEAD + 4 * k + 4]) for k in range(min(max(int(c[0]), 0), COUNT_MAX_EVENTS))]


# ----------------------------------------------------------------------------- zones
ZONE_MAX_ZONES, ZONE_VERTS, ZONE_MAX_EVENTS = _lib.ZONE_MAX_ZONES, _lib.ZONE_VERTS, _lib.ZONE_MAX_EVENTS
ZONE_WIDTH = _lib.ZONE_WIDTH                    # (smallest, largest, the default) width W the outlines are drawn with
ZONE_ANCHORS = ("centre", "bottom")             # the POINT of a row: index = the entry points' ``anchor``
ZONE_KINDS = ("exit", "enter", "lost")          # index = an event's kind
# words of a zone list: [n_events, frames, 0, 0 | occupancy[8] | visitors[8] | stays[8] | dwell[8] | peak[8] | events[64][5]]; of a
# state in front of its entries; of an entry; of a list in front of its events
ZONE_LIST_WORDS, ZONE_HEAD, ZONE_ENTRY, ZONE_LIST_HEAD = _lib.ZONE_LIST_WORDS, _lib.ZONE_HEAD_WORDS, _lib.ZONE_ENTRY_WORDS, 4 + 5 * _lib.ZONE_MAX_ZONES


def zone_option(zones, classes="all", width=None, anchor=None):
    """(host only) The zone option checked -> (zones, classes, W, anchor): zones a tuple of 1..8 polygons, each a tuple of 3..16 vertices
    (x, y) of integers in -32768..65535, no two consecutive ones equal (the last and the first are consecutive); a polygon may be given
    as its vertices or as the flat x1, y1, x2, y2, ..., and one polygon alone is one zone.  classes "all" or a tuple of class names
    (which names there are is the caller's to check: ``redact_class_list``), W the width of the outlines, 1..9 (None: 3), anchor 0 / 1
    from "centre" / "bottom" (None: centre).  ValueError with the reason."""
    lo, hi = _lib.ZONE_COORD
    v_lo, v_hi = ZONE_VERTS
    try:
        zones = tuple(zones)
        if zones and (all(_is_int(v) for v in zones) or all(not _is_int(p) and len(tuple(p)) == 2 and all(_is_int(v) for v in p) for p in zones)):
            zones = (zones,)                             # one polygon alone
        polys = []
        for zn in zones:
            zn = tuple(zn)
            if zn and all(_is_int(v) for v in zn):
                if len(zn) % 2:
                    raise ValueError("zone %r: an odd number of coordinates" % (zn,))
                zn = tuple(zip(zn[0::2], zn[1::2]))
            polys.append(tuple(tuple(p) for p in zn))
    except TypeError:
        raise ValueError("zones=%r: a list of polygons, each a list of (x, y)" % (zones,)) from None
    if not 1 <= len(polys) <= ZONE_MAX_ZONES:
        raise ValueError("zones: %d of them, 1..%d are possible" % (len(polys), ZONE_MAX_ZONES))
    for zn in polys:
        if not v_lo <= len(zn) <= v_hi:
            raise ValueError("zone %r: %d vertices, %d..%d are possible" % (zn, len(zn), v_lo, v_hi))
        if not all(len(p) == 2 and all(_is_int(v) and lo <= int(v) <= hi for v in p) for p in zn):
            raise ValueError("zone %r: vertices are two integers x, y in %d..%d" % (zn, lo, hi))
        for i, p in enumerate(zn):
            q = zn[(i + 1) % len(zn)]
            if (int(p[0]), int(p[1])) == (int(q[0]), int(q[1])):
                raise ValueError("zone %r: two consecutive vertices at (%d, %d)" % (zn, p[0], p[1]))
    polys = tuple(tuple((int(x), int(y)) for x, y in zn) for zn in polys)
    classes, width = _classes_option("zone classes", classes, True), _width_option("zone width", width, ZONE_WIDTH)
    anchor = 0 if anchor is None else anchor
    if isinstance(anchor, str):
        anchor = {"centre": 0, "center": 0, "bottom": 1}.get(anchor, anchor)
    if not _is_int(anchor) or int(anchor) not in (0, 1):
        raise ValueError("zone anchor=%r: \"centre\" or \"bottom\"" % (anchor,))
    return polys, classes, width, int(anchor)


def _zone_verts_arg(zones):
    """``zones`` (polygons of (x, y)) as the two host int32 arrays the entry points read (keep them alive over the call), their pointers
    and the number of zones."""
    nv = np.ascontiguousarray([len(zn) for zn in zones], dtype=np.int32)
    flat = [v for zn in zones for p in zn for v in p]
    verts = np.ascontiguousarray(np.asarray(flat, dtype=np.int64).clip(-2 ** 31, 2 ** 31 - 1), dtype=np.int32)
    return (verts, nv), verts.ctypes.data_as(ctypes.c_void_p), nv.ctypes.data_as(ctypes.c_void_p), int(nv.size)


def zone_state_words(capacity):
    """(host only) 4-byte words of a zone state of ``capacity`` entries (frcnn_zone_state_bytes / 4): 36 + 13 capacity."""
    n = int(_lib.load().frcnn_zone_state_bytes(int(capacity)))
    if n == 0:
        raise _lib.FrcnnError("zone state: capacity=%r not in [1, %d]" % (capacity, TRACK_MAX))
    return n // 4


def zone_state(capacity):
    """An empty zone state of ``capacity`` entries: a zeroed int32 device tensor, [n_entries, frames, dropped, events_dropped |
    visitors[8] | stays[8] | dwell[8] | peak[8] | per entry: id, cls, last_seen, inside, visited, since[8]]
    (include/ext/frcnn_hip_zone.h).  Zeroing it (``zone_reset``) empties it, totals included."""
    _require_gpu()
    return torch.zeros(zone_state_words(capacity), dtype=torch.int32, device="cuda")


def zone_reset(state, keep_totals=False):
    """Empty the state (on the current stream): no entries, no frames, totals 0.  ``keep_totals``: only the entries leave -- the ids end
    without an event, their open stays are not counted, and ``frames``, the sticky sums, visitors, stays, dwell and peak are kept."""
    return _reset_keeping_totals(state, ZONE_HEAD, keep_totals)


def zone_workspace(frames):
    """The zone lists of a ``zone_update`` call of ``frames`` frames: an int32 device tensor (frames, ZONE_LIST_WORDS).  Every word is
    written by every call."""
    lists = _lists_workspace("zone_workspace", frames, ZONE_LIST_WORDS)
    assert int(_lib.load().frcnn_zone_list_words()) == ZONE_LIST_WORDS
    return lists


def zone_update(state, tracked, n_frames, zones, table, expire, h, w, anchor=0, capacity=None, lists=None, gate=None):
    """Steps 1-5 of the zone rule (DESIGN §8 "Zone rule", frcnn_zone_update) over the frames of ``tracked`` IN ORDER, in one launch:
    ``tracked`` and ``n_frames`` as ``count_update`` takes them.  The point (``anchor`` 0: the centre, 1: the bottom centre) of every
    live tracked row of a class set in ``table`` (device uint8 [C], ``redact_table``'s form) is tested against ``zones`` (host polygons
    of (x, y), ``zone_option``'s form) and steps the entry of its id in ``state`` (``zone_state``; ``capacity``: its entries, read from
    its size when None): enter and exit events with the dwell, an id a visitor of a zone once.  Entries not seen for more than ``expire``
    frames leave, with a lost event per zone they were in, and frame f's zone list lands in ``lists[f]`` (``zone_workspace``; allocated
    here when None; a captured call passes it) -> ``lists``.  ``gate``: None, or a device word that is 0 when no frame of the call is
    real, whatever ``n_frames`` says.  The call can be captured in a graph."""
    _require_gpu()
    frames, words, rows = _id_update_args(state, tracked, n_frames, gate, table)
    if capacity is None:
        capacity = (int(state.numel()) - ZONE_HEAD) // ZONE_ENTRY
    if lists is None:
        lists = zone_workspace(frames)
    assert int(state.numel()) == zone_state_words(capacity)
    _lists_arg(lists, frames, ZONE_LIST_WORDS)
    keep, verts_p, nv_p, n_zones = _zone_verts_arg(zones)           # (``keep`` owns the host arrays the two pointers point into: alive over the call)
    _lib.call("frcnn_zone_update", _p(state), int(capacity), _p(tracked), words, rows, frames, _p(n_frames), _p(gate), verts_p, nv_p,
              n_zones, _p(table), int(table.numel()), int(anchor), int(expire), int(h), int(w), _p(lists), _stream())
    return lists


def zone_draw_u8(frame, zlist, zones, width=None, rgb=False):
    """DRAW of the zone rule (frcnn_zone_draw_u8) into ``frame``, an (h, w, 3) uint8 device tensor, edited in place and returned: the
    zones that ``zlist`` -- one zone list of ``zone_update`` -- says are occupied tinted with PALETTE[z & 7] at a quarter, every zone's
    outline as capsules of ``width`` pixels (None: 3), and a label "Z{z} {occupancy}/{visitors}" per zone, formatted on the device.  A
    list of a frame that is not real draws nothing.  ``rgb``: the frame's bytes are R, G, B (False: B, G, R).  One launch; the list is
    read on the device, so the call can be captured in a graph."""
    _require_gpu()
    h, w = _frame_u8(frame)
    assert zlist.is_cuda and zlist.dtype == torch.int32 and zlist.dim() == 1 and zlist.is_contiguous() and int(zlist.numel()) == ZONE_LIST_WORDS
    keep, verts_p, nv_p, n_zones = _zone_verts_arg(zones)           # (``keep`` owns the host arrays the two pointers point into: alive over the call)
    _lib.call("frcnn_zone_draw_u8", _p(frame), h, w, _p(zlist), verts_p, nv_p, n_zones,
              ZONE_WIDTH[2] if width is None else int(width), int(bool(rgb)), _stream())
    return frame


def zone_totals(state):
    """(host only; reads the state back) The totals of a zone state, device tensor or host copy -> {"entries", "frames", "dropped",
    "events_dropped", "visitors", "stays", "dwell", "peak": a list of 8 each} -- dwell[z] the frames of the completed stays in zone z."""
    s = state.cpu().numpy() if isinstance(state, torch.Tensor) else np.asarray(state)
    Z = ZONE_MAX_ZONES
    out = {"entries": int(s[0]), "frames": int(s[1]), "dropped": int(s[2]), "events_dropped": int(s[3])}
    for k, name in enumerate(("visitors", "stays", "dwell", "peak")):
        out[name] = [int(v) for v in s[4 + Z * k:4 + Z * (k + 1)]]
    return out


def zone_occupancy(zlist, n_zones=ZONE_MAX_ZONES):
    """(host only) occupancy[z] of one zone list's HOST copy, for the first ``n_zones`` zones."""
    c = np.asarray(zlist)
    return [int(v) for v in c[4:4 + int(n_zones)]]


def zone_events(zlist):
    """(host only) The events of one zone list's HOST copy -> [(zone, kind, id, cls, dwell)], kind an index of ``ZONE_KINDS``: the rows'
    enter and exit events in (row, zone) order, then the lost events in (id, zone) order."""
    c = np.asarray(zlist)
    return [tuple(int(v) for v in c[ZONE_LIST_HEAD + 5 * k:ZONE_LIST_HEAD + 5 * k + 5]) for k in range(min(max(int(c[0]), 0), ZONE_MAX_EVENTS))]


# ----------------------------------------------------------------------------- static regions
REDACT_REGION_MAX = _lib.REDACT_REGION_MAX          # polygons of one option, at most
REDACT_REGION_FEATHER = _lib.REDACT_REGION_FEATHER  # (smallest, largest) feather in pixels
REDACT_REGION_MODE = "fill"                         # the default mode: a static area has nothing worth hinting at


class RegionMask:
    """(host only) A painted mask of the region rule: ``array`` a read-only contiguous (h, w) uint8 array -- >= 128 hides --, ``digest``
    the SHA-1 of its size and bytes.  Two masks are equal when their digests are, so an option that holds one hashes and compares."""
    __slots__ = ("array", "digest")

    def __init__(self, array):
        import hashlib
        a = np.asarray(array)
        if a.dtype == np.bool_:
            a = a.astype(np.uint8) * 255
        if a.ndim != 2 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError("redact region mask: a (h, w) uint8 array (>= 128 hides), got %s %s" % (a.dtype, tuple(a.shape)))
        a = np.array(a, dtype=np.uint8, order="C")      # (a copy of the caller's: nobody writes it behind the digest)
        a.setflags(write=False)
        self.array = a
        self.digest = hashlib.sha1(b"%dx%d:" % (a.shape[1], a.shape[0]) + a.tobytes()).hexdigest()

    shape = property(lambda self: tuple(self.array.shape))

    def __eq__(self, other):
        return isinstance(other, RegionMask) and other.digest == self.digest

    def __hash__(self):
        return hash(self.digest)

    def __repr__(self):
        return "RegionMask(%dx%d, %s)" % (self.array.shape[1], self.array.shape[0], self.digest[:12])


def redact_region_option(regions=None, mask=None, mode=None, size=None, feather=None):
    """(host only) The region option checked -> (regions, mask, mode, size, feather) (DESIGN §8 "Region rule"): regions a tuple of 0..8
    polygons in ``zone_option``'s grammar and limits (3..16 vertices (x, y) of integers in -32768..65535, no two consecutive ones equal; a
    polygon as its vertices or flat; one polygon alone is one region; None: none), mask None or a (h, w) uint8 array (a ``RegionMask``
    in the result), at least one of the two; mode "fill" / "pixelate" / "blur" (None: "fill"), size as ``redact_size`` (None: the
    mode's default), feather 0..32 (None: 0).  ValueError with the reason."""
    polys = ()
    try:
        regions = () if regions is None else tuple(regions)
    except TypeError:
        raise ValueError("redact regions=%r: a list of polygons, each a list of (x, y)" % (regions,)) from None
    if regions:
        try:
            polys = zone_option(regions)[0]
        except ValueError as e:
            raise ValueError("redact region: %s" % str(e).replace("zones", "regions").replace("zone", "region")) from None
    if mask is not None and not isinstance(mask, RegionMask):
        mask = RegionMask(mask)
    if not polys and mask is None:
        raise ValueError("redact region: neither a polygon nor a mask: nothing to hide")
    mode = REDACT_REGION_MODE if mode is None else mode
    if not isinstance(mode, str) or mode not in _lib.REDACT_MODES:
        raise ValueError("redact region mode %r: one of %s" % (mode, ", ".join(REDACT_MODES)))
    try:
        size = redact_size(mode, size)
    except ValueError as e:
        raise ValueError("redact region: %s" % e) from None
    lo, hi = REDACT_REGION_FEATHER
    feather = 0 if feather is None else feather
    if not _is_int(feather) or not lo <= int(feather) <= hi:
        raise ValueError("redact region feather %r: an integer in %d..%d" % (feather, lo, hi))
    return polys, mask, mode, size, int(feather)


def redact_region_key(option):
    """(host only) ``option`` (``redact_region_option``'s form) as a cache key holds it: the mask as its digest, or None."""
    regions, mask, mode, size, feather = option
    return regions, (None if mask is None else mask.digest), mode, size, feather


def redact_region_plane_bytes(h, w):
    """Bytes of a plane for frames of (h, w) (frcnn_redact_region_plane_bytes); FrcnnError for a side out of range."""
    n = int(_lib.load().frcnn_redact_region_plane_bytes(int(h), int(w)))
    if n == 0:
        raise _lib.FrcnnError("redact region plane: frame %rx%r out of range (sides 1..%d)" % (h, w, _lib.REDACT_MAX_SIDE))
    return n


def redact_region_plane(h, w, option, out=None):
    """The plane of ``option`` (``redact_region_option``'s form) for frames of (h, w): a uint8 device tensor, [int32 h, w, feather,
    covered, full, 1, 0, 0 | uint16 W[h][w] | tile flags | private] (include/ext/frcnn_hip_redact_region.h), built by three launches
    on the current stream (frcnn_redact_region_build): once per frame size.  The mode and size of the option are not the plane's: they
    go to ``redact_region_prepare`` / ``redact_region_apply_u8``.  ``out``: a 16-byte aligned u8 device tensor of
    ``redact_region_plane_bytes(h, w)`` bytes to build into; None allocates one.  ValueError for a mask that is not (h, w)."""
    _require_gpu()
    regions, mask, _, _, feather = option
    h, w = int(h), int(w)
    if mask is not None and mask.shape != (h, w):
        raise ValueError("redact region mask of %dx%d for frames of %dx%d" % (mask.shape[1], mask.shape[0], w, h))
    plane = torch.zeros(redact_region_plane_bytes(h, w), dtype=torch.uint8, device="cuda") if out is None else out
    assert plane.is_cuda and plane.dtype == torch.uint8 and plane.dim() == 1 and plane.is_contiguous() and plane.data_ptr() % 16 == 0
    assert int(plane.numel()) == redact_region_plane_bytes(h, w)
    mask_dev = None if mask is None else torch.from_numpy(mask.array.copy()).cuda()        # (the option's array is read-only)
    keep, verts_p, nv_p, n = _zone_verts_arg(regions) if regions else (None, None, None, 0)   # (``keep``: the host arrays, alive over the call)
    _lib.call("frcnn_redact_region_build", _p(plane), h, w, verts_p, nv_p, n, _p(mask_dev), int(feather), _stream())
    return plane


def _region_call(name, frame, plane, mode, size, workspace):
    _require_gpu()
    h, w = _frame_u8(frame)
    assert plane.is_cuda and plane.dtype == torch.uint8 and plane.dim() == 1 and plane.is_contiguous()
    if mode not in _lib.REDACT_MODES:
        raise ValueError("redact region mode %r: one of %s" % (mode, ", ".join(REDACT_MODES)))
    size = REDACT_SIZES[mode][2] if size is None else int(size)            # (the range is the library's to check)
    if workspace is None:
        workspace = _ws(_lib.load().frcnn_redact_ws_bytes(h, w, _lib.REDACT_MODES[mode], size))
    assert workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous()
    _lib.call(name, _p(frame), h, w, _p(plane), _lib.REDACT_MODES[mode], size, _p(workspace), int(workspace.numel()), _stream())
    return workspace


def redact_region_prepare(frame, plane, mode=REDACT_REGION_MODE, size=None, workspace=None):
    """What replaces the hidden pixels, from ``frame`` -- the (h, w, 3) uint8 device frame NO edit has touched -- into ``workspace``
    (a u8 device tensor of ``redact_ws_bytes(h, w, mode, size)`` bytes; None allocates one) -> the workspace: the Redaction rule's phase
    one, run whatever the detections say (frcnn_redact_region_prepare).  Nothing for "fill".  The call can be captured in a graph."""
    return _region_call("frcnn_redact_region_prepare", frame, plane, mode, size, workspace)


def redact_region_apply_u8(frame, plane, mode=REDACT_REGION_MODE, size=None, workspace=None):
    """Hide the static areas of ``plane`` (``redact_region_plane``) in ``frame``, an (h, w, 3) uint8 device tensor, edited in place
    and returned: every byte with W > 0 becomes (W R + (256 - W) C + 128) >> 8, R from ``workspace`` as ``redact_region_prepare`` filled
    it from the untouched frame (DESIGN §8 "Region rule"; frcnn_redact_region_apply_u8, one launch).  A plane of another frame size
    writes nothing.  The call can be captured in a graph."""
    _region_call("frcnn_redact_region_apply_u8", frame, plane, mode, size, workspace)
    return frame


def redact_region_stats(plane):
    """(host only; reads the header back) -> {"h", "w", "feather", "covered": the pixels with W > 0, "full": those with W = 256} of a
    plane, device tensor or host copy."""
    p = plane[:4 * _lib.REDACT_REGION_HEAD_WORDS].cpu().numpy() if isinstance(plane, torch.Tensor) else np.asarray(plane)[:4 * _lib.REDACT_REGION_HEAD_WORDS]
    head = np.ascontiguousarray(p).view(np.int32)
    return {"h": int(head[0]), "w": int(head[1]), "feather": int(head[2]), "covered": int(head[3]), "full": int(head[4])}


def redact_region_weights(plane):
    """(host only; reads the plane back) W of a plane, device tensor or host copy -> a (h, w) uint16 array, 0..256."""
    p = plane.cpu().numpy() if isinstance(plane, torch.Tensor) else np.ascontiguousarray(plane)
    head = p[:8].view(np.int32)
    h, w = int(head[0]), int(head[1])
    at = 4 * _lib.REDACT_REGION_HEAD_WORDS
    return p[at:at + 2 * h * w].view(np.uint16).reshape(h, w).copy()


# ----------------------------------------------------------------------------- background plate
# (smallest, largest, the default) of the settle S, the tolerance T and the margin M.  The defaults are PROVISIONAL: nobody has measured
# them on real footage.
PLATE_SETTLE, PLATE_TOL, PLATE_MARGIN = _lib.PLATE_SETTLE, _lib.PLATE_TOL, _lib.PLATE_MARGIN


def plate_option(classes, settle=None, tol=None, margin=None):
    """(host only) The remove option checked -> (classes, S, T, M): classes "all" or a tuple of class names (which names there are is the
    caller's to check: ``redact_class_list``), S the frames a pixel must hold still to become background, 1..255 (None: 8), T how far
    a channel may lie from the run's anchor, 0..255 (None: 10), M the pixels a box grows by, 0..64 (None: 8).  The defaults are
    provisional.  ValueError with the reason."""
    classes = _classes_option("remove classes", classes, False)
    out = []
    for name, v, (lo, hi, default) in (("settle", settle, PLATE_SETTLE), ("tol", tol, PLATE_TOL), ("margin", margin, PLATE_MARGIN)):
        v = default if v is None else v
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError("remove %s=%r: an integer in %d..%d" % (name, v, lo, hi))
        out.append(int(v))
    return (classes,) + tuple(out)


def plate_class_list(class_names, classes):
    """(host only) ``redact_class_list`` for the remove classes: the same reading of "all" and of names, and the refusal of an unknown
    name says whose it is."""
    try:
        return redact_class_list(class_names, classes)
    except ValueError as e:
        text = str(e)
        raise ValueError("remove: " + (text[len("redact: "):] if text.startswith("redact: ") else text)) from None


def plate_state_words(h, w):
    """(host only) 4-byte words of a plate state BUFFER for frames of (h, w) (frcnn_plate_state_bytes / 4): the state, 4 + 2 h w words
    [frames, known, 0, 0 | px[h][w][2]], and the update kernel's scratch words behind it."""
    n = int(_lib.load().frcnn_plate_state_bytes(int(h), int(w)))
    if n == 0:
        raise _lib.FrcnnError("plate state: frame %rx%r out of range (sides 1..%d)" % (h, w, _lib.REDACT_MAX_SIDE))
    return n // 4


def plate_state(h, w):
    """An empty plate state for frames of (h, w): a zeroed int32 device tensor of ``plate_state_words`` words, [frames, known, 0, 0 |
    px[h][w][2] | scratch] (include/ext/frcnn_hip_plate.h).  Zeroing it (``plate_reset``) empties it; ``plate_image`` reads it."""
    _require_gpu()
    return torch.zeros(plate_state_words(h, w), dtype=torch.int32, device="cuda")


def plate_reset(state):
    """Empty the state (on the current stream): no frames, no pixel known."""
    state.zero_()
    return state


def plate_image(state, h, w):
    """(frames, known, the (h, w, 3) uint8 plate in the frames' byte order with unknown pixels black, the (h, w) bool mask of the known
    pixels) of a plate state, device tensor or its host copy (torch or numpy): host arrays."""
    h, w = int(h), int(w)
    host = state.detach().cpu().numpy() if isinstance(state, torch.Tensor) else np.asarray(state)
    w0 = np.ascontiguousarray(host[4:4 + 2 * h * w].reshape(h, w, 2)[:, :, 0]).view(np.uint8).reshape(h, w, 4)
    known = w0[:, :, 3] != 0
    return int(host[0]), int(host[1]), np.where(known[:, :, None], w0[:, :, :3], 0).astype(np.uint8), known


def _plate_rows(det_packed, tracked):
    per = 8 if tracked else 7
    assert det_packed.is_cuda and det_packed.dtype == torch.int32 and det_packed.dim() == 1 and det_packed.is_contiguous()
    assert (int(det_packed.numel()) - 4) % per == 0
    return (int(det_packed.numel()) - 4) // per


def plate_update(state, frame, det_packed, settle=None, tol=None, margin=None, frame_index=0, n_frames=None, gate=None, cut=None,
                 tracked=False):
    """UPDATE of the plate rule (DESIGN §8 "Plate rule", frcnn_plate_update) from ``frame``, an (h, w, 3) uint8 device tensor that no
    edit has touched yet: every pixel outside the boxes of ``det_packed`` grown by ``margin`` -- EVERY row of the post-process's packed
    buffer whatever its class, or with ``tracked`` True of one tracked buffer of ``track_update`` (plain or widened), the held and
    back-filled rows too -- that has stayed within ``tol`` of its run's anchor for ``settle`` frames becomes the plate of ``state``
    (``plate_state``); a pixel under a box starts over and keeps its plate.  The frame counts when ``frame_index`` < *``n_frames`` (a
    device int32 word; None: a word that says 1, allocated here -- a captured call passes its own) and, with ``gate`` (a device word),
    *gate != 0; else nothing is written.  ``cut``: a device int32 word; non-zero empties the plate in front of the update.  Two
    launches, everything guarded on the device: the call can be captured in a graph -> ``state``."""
    _require_gpu()
    h, w = _frame_u8(frame)
    assert state.is_cuda and state.dtype == torch.int32 and state.dim() == 1 and state.is_contiguous()
    assert int(state.numel()) == plate_state_words(h, w)
    rows = _plate_rows(det_packed, tracked)
    if n_frames is None:
        n_frames = torch.ones(1, dtype=torch.int32, device="cuda")
    assert n_frames.is_cuda and n_frames.dtype == torch.int32 and n_frames.numel() >= 1
    assert gate is None or (gate.is_cuda and gate.dtype == torch.int32 and gate.numel() >= 1)
    assert cut is None or (cut.is_cuda and cut.dtype == torch.int32 and cut.numel() >= 1)
    _lib.call("frcnn_plate_update", _p(state), h, w, _p(frame), _p(det_packed), rows, int(bool(tracked)),
              PLATE_MARGIN[2] if margin is None else int(margin), PLATE_SETTLE[2] if settle is None else int(settle),
              PLATE_TOL[2] if tol is None else int(tol), int(frame_index), _p(n_frames), _p(gate), _p(cut), _stream())
    return state


def plate_fill_u8(frame, state, det_packed, table, margin=None, keep_unknown=False, tracked=False):
    """FILL of the plate rule (frcnn_plate_fill_u8): every pixel of ``frame``, an (h, w, 3) uint8 device tensor, edited in place and
    returned, that lies in a box of ``det_packed`` (as ``plate_update`` reads it) of a class set in ``table`` (``redact_table``'s form),
    grown by ``margin``, becomes the plate's where ``state`` knows it; where it does not, black, or with ``keep_unknown`` what it is.
    One launch; reads the counts from device memory, so the call can be captured in a graph."""
    _require_gpu()
    h, w = _frame_u8(frame)
    assert state.is_cuda and state.dtype == torch.int32 and state.dim() == 1 and state.is_contiguous()
    assert table.is_cuda and table.dtype == torch.uint8 and table.dim() == 1 and table.is_contiguous()
    assert int(state.numel()) == plate_state_words(h, w)
    rows = _plate_rows(det_packed, tracked)
    _lib.call("frcnn_plate_fill_u8", _p(frame), h, w, _p(state), _p(det_packed), rows, int(bool(tracked)), _p(table), int(table.numel()),
              PLATE_MARGIN[2] if margin is None else int(margin), int(bool(keep_unknown)), _stream())
    return frame


# ----------------------------------------------------------------------------- moving net
# (smallest, largest, the default) of the tolerance D, the vote K, the hold H, the grow G and the feather F.  The defaults of D, K, H and G
# are PROVISIONAL: nobody has measured them on real footage.
REDACT_MOVING_TOL, REDACT_MOVING_VOTE, REDACT_MOVING_HOLD = _lib.REDACT_MOVING_TOL, _lib.REDACT_MOVING_VOTE, _lib.REDACT_MOVING_HOLD
REDACT_MOVING_GROW, REDACT_MOVING_FEATHER = _lib.REDACT_MOVING_GROW, _lib.REDACT_MOVING_FEATHER
REDACT_MOVING_MODE = "pixelate"
REDACT_MOVING_UNKNOWN = ("show", "hide")            # index = the rule's ``unknown``
REDACT_MOVING_KEYWORDS = ("tol", "vote", "hold", "grow", "feather", "unknown", "except_classes", "mode", "size", "settle", "plate_tol", "margin")


def redact_moving_option(tol=None, vote=None, hold=None, grow=None, feather=None, unknown=None, except_classes=None, mode=None, size=None,
                         settle=None, plate_tol=None, margin=None):
    """(host only) The moving option checked -> (D, K, H, G, F, unknown, EXCEPT, mode, size, S, T, M) (DESIGN §8 "Moving rule"): D how far
    a channel may lie from the plate, 0..255 (None: 24); K the foreground pixels that make an 8 x 8 cell vote, 1..64 (None: 8); H the
    frames a cell stays hidden behind its last vote, 0..255 (None: 4); G the pixels the hidden set grows by, 0..32 (None: 8); F the feather
    beyond that, 0..32 (None: 0); unknown "show" or "hide" (None: "show") -- what a pixel whose background is not known yet counts as --;
    EXCEPT () or a tuple of class names, "all" for every class (which names there are is the caller's to check: ``redact_class_list``):
    the boxes of those classes are never foreground; mode "fill" / "pixelate" / "blur" (None: "pixelate"), size as ``redact_size``
    (None: the mode's default); S, T, M the plate's settle, tolerance and margin as ``plate_option`` takes them (None: its defaults).
    The defaults of D, K, H and G are provisional.  ValueError with the reason."""
    out = []
    for name, v, (lo, hi, default) in (("tol", tol, REDACT_MOVING_TOL), ("vote", vote, REDACT_MOVING_VOTE), ("hold", hold, REDACT_MOVING_HOLD),
                                       ("grow", grow, REDACT_MOVING_GROW), ("feather", feather, REDACT_MOVING_FEATHER)):
        v = default if v is None else v
        if not _is_int(v) or not lo <= int(v) <= hi:
            raise ValueError("redact moving %s=%r: an integer in %d..%d" % (name, v, lo, hi))
        out.append(int(v))
    unknown = REDACT_MOVING_UNKNOWN[0] if unknown is None else unknown
    if not isinstance(unknown, str) or unknown not in REDACT_MOVING_UNKNOWN:
        raise ValueError("redact moving unknown=%r: one of %s" % (unknown, ", ".join(REDACT_MOVING_UNKNOWN)))
    classes = _classes_option("redact moving except_classes", () if except_classes is None else except_classes, False, empty_ok=True)
    mode = REDACT_MOVING_MODE if mode is None else mode
    if not isinstance(mode, str) or mode not in _lib.REDACT_MODES:
        raise ValueError("redact moving mode %r: one of %s" % (mode, ", ".join(REDACT_MODES)))
    try:
        size = redact_size(mode, size)
    except ValueError as e:
        raise ValueError("redact moving: %s" % e) from None
    try:
        _, settle, plate_tol, margin = plate_option("all", settle, plate_tol, margin)
    except ValueError as e:
        text = str(e).replace("remove ", "", 1)
        raise ValueError("redact moving %s" % ("plate_" + text if text.startswith("tol=") else text)) from None
    return tuple(out) + (unknown, classes, mode, size, settle, plate_tol, margin)


def redact_moving_form(redact_moving, remove=None, class_names=None):
    """(host only) What the entry points take as ``redact_moving`` -> ``redact_moving_option``'s form: True or () for every default, a
    dict of ``redact_moving_option``'s keywords, or its 12 values in order.  ``remove``: the pass's normalised remove option or None --
    a pass has ONE plate update, so with it the plate's (S, T, M) are the remove option's, and a ``settle`` / ``plate_tol`` / ``margin``
    stated here that differs is refused by name.  ``class_names`` (index = class index): the EXCEPT names must be among them.
    ValueError with the reason."""
    if redact_moving is True or (isinstance(redact_moving, tuple) and not redact_moving):
        kw = {}
    elif isinstance(redact_moving, dict):
        kw = dict(redact_moving)
    else:
        try:
            values = tuple(redact_moving)
        except TypeError:
            values = None
        if values is None or isinstance(redact_moving, str) or len(values) != len(REDACT_MOVING_KEYWORDS):
            raise ValueError("redact_moving=%r: True, a dict of the keywords %s, or their %d values"
                             % (redact_moving, ", ".join(REDACT_MOVING_KEYWORDS), len(REDACT_MOVING_KEYWORDS)))
        kw = dict(zip(REDACT_MOVING_KEYWORDS, values))
    unknown = [k for k in kw if k not in REDACT_MOVING_KEYWORDS]
    if unknown:
        raise ValueError("redact_moving: unknown keyword%s %s; the keywords are %s"
                         % ("s" if len(unknown) > 1 else "", ", ".join(repr(k) for k in unknown), ", ".join(REDACT_MOVING_KEYWORDS)))
    if remove is not None:
        for name, value in zip(("settle", "plate_tol", "margin"), remove[1:4]):
            if kw.get(name) is not None and kw[name] != value:
                raise ValueError("redact_moving: %s=%r, but remove= says %d: a pass has one plate update, state it once" % (name, kw[name], value))
            kw[name] = value
    option = redact_moving_option(**kw)
    if class_names is not None and option[6] not in ((), "all"):
        try:
            option = option[:6] + (redact_class_list(class_names, option[6]),) + option[7:]
        except ValueError as e:
            text = str(e)
            raise ValueError("redact moving except_classes: " + (text[len("redact: "):] if text.startswith("redact: ") else text)) from None
    return option


def redact_moving_table(class_names, except_classes):
    """The EXCEPT table ``redact_moving_build`` reads: device u8 [C], 1 where ``class_names[i]`` is excepted; () excepts nothing."""
    if except_classes == ():
        _require_gpu()
        return torch.zeros(len(class_names), dtype=torch.uint8, device="cuda")
    return redact_table(class_names, except_classes)


def redact_moving_state_bytes(h, w):
    """(host only) Bytes of a moving state BUFFER for frames of (h, w) (frcnn_redact_moving_state_bytes); FrcnnError for a side out of range."""
    n = int(_lib.load().frcnn_redact_moving_state_bytes(int(h), int(w)))
    if n == 0:
        raise _lib.FrcnnError("redact moving state: frame %rx%r out of range (sides 1..%d)" % (h, w, _lib.REDACT_MAX_SIDE))
    return n


def redact_moving_state(h, w):
    """An empty moving state for frames of (h, w): a zeroed uint8 device tensor, [int32 frames, cells_now, 0, 0 | uint8 left[ch][cw] |
    scratch] (include/ext/frcnn_hip_redact_moving.h).  Zeroing it (``redact_moving_reset``) empties it; ``redact_moving_left`` reads it."""
    _require_gpu()
    return torch.zeros(redact_moving_state_bytes(h, w), dtype=torch.uint8, device="cuda")


def redact_moving_reset(state):
    """Empty the state (on the current stream): no frames, no cell held."""
    state.zero_()
    return state


def redact_moving_left(state, h, w):
    """(host only; reads the state back) -> (frames, cells_now, the (ch, cw) uint8 array ``left``) of a moving state, device tensor or host copy."""
    host = state.detach().cpu().numpy() if isinstance(state, torch.Tensor) else np.ascontiguousarray(state)
    cell = _lib.REDACT_MOVING_CELL
    ch, cw = -(-int(h) // cell), -(-int(w) // cell)
    head = host[:16].view(np.int32)
    return int(head[0]), int(head[1]), host[16:16 + ch * cw].reshape(ch, cw).copy()


def redact_moving_build(state, plane, stats, frame, plate, det_packed, table, option, frame_index=0, n_frames=None, gate=None, cut=None,
                        tracked=False):
    """The plane of weights of one frame under the moving rule (DESIGN §8 "Moving rule", frcnn_redact_moving_build) -> ``plane``:
    ``frame``, an (h, w, 3) uint8 device tensor that no edit has touched, is compared with the plate of ``plate`` (``plate_state``, already
    updated with this same frame); a pixel that differs by more than D, outside the boxes of ``det_packed`` (as ``plate_update`` reads it)
    whose class is set in ``table`` (``redact_moving_table``), is foreground; cells of 8 x 8 vote and hold in ``state``
    (``redact_moving_state``); the moving cells grown by G and feathered by F become ``plane``, a u8 device tensor of
    ``redact_region_plane_bytes(h, w)`` bytes that ``redact_region_prepare`` / ``redact_region_apply_u8`` take; ``stats``: int32 [4]
    device, [real, cells_now, covered, full].  ``option``: ``redact_moving_option``'s form.  ``frame_index`` / ``n_frames`` / ``gate`` /
    ``cut`` as ``plate_update``'s.  Three launches, everything guarded on the device: the call can be captured in a graph."""
    _require_gpu()
    h, w = _frame_u8(frame)
    assert state.is_cuda and state.dtype == torch.uint8 and state.dim() == 1 and state.is_contiguous()
    assert plane.is_cuda and plane.dtype == torch.uint8 and plane.dim() == 1 and plane.is_contiguous()
    assert plate.is_cuda and plate.dtype == torch.int32 and plate.dim() == 1 and plate.is_contiguous()
    assert stats.is_cuda and stats.dtype == torch.int32 and stats.is_contiguous() and stats.numel() == _lib.REDACT_MOVING_STATS_WORDS
    assert table.is_cuda and table.dtype == torch.uint8 and table.dim() == 1 and table.is_contiguous()
    assert int(state.numel()) == redact_moving_state_bytes(h, w) and int(plane.numel()) == redact_region_plane_bytes(h, w)
    assert int(plate.numel()) == plate_state_words(h, w)
    rows = _plate_rows(det_packed, tracked)
    if n_frames is None:
        n_frames = torch.ones(1, dtype=torch.int32, device="cuda")
    assert n_frames.is_cuda and n_frames.dtype == torch.int32 and n_frames.numel() >= 1
    assert gate is None or (gate.is_cuda and gate.dtype == torch.int32 and gate.numel() >= 1)
    assert cut is None or (cut.is_cuda and cut.dtype == torch.int32 and cut.numel() >= 1)
    D, K, H, G, F, unknown = option[:6]
    margin = option[11]
    _lib.call("frcnn_redact_moving_build", _p(state), _p(plane), _p(stats), h, w, _p(frame), _p(plate), _p(det_packed), rows,
              int(bool(tracked)), _p(table), int(table.numel()), int(margin), int(D), int(K), int(H), int(G), int(F),
              unknown if isinstance(unknown, int) else REDACT_MOVING_UNKNOWN.index(unknown), int(frame_index), _p(n_frames), _p(gate), _p(cut),
              _stream())
    return plane


def redact_moving_stats(stats):
    """(host only; reads the stats back) -> {"real", "cells", "covered", "full"} of one frame's stats, or a list of them for an [F][4]
    tensor, device tensor or host copy."""
    host = stats.detach().cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)
    one = lambda s: {"real": int(s[0]), "cells": int(s[1]), "covered": int(s[2]), "full": int(s[3])}
    return one(host) if host.ndim == 1 else [one(s) for s in host]


# ----------------------------------------------------------------------------- output scale
SCALE_MAX_RATIO = _lib.SCALE_MAX_RATIO


def scale_form(option):
    """(host only) The output-scale option as it is stated, whatever the frames' size -> ("size", W, H) or ("scale", N) with plain ints.
    ValueError with the reason: another form, a divisor outside 2..16, a side of 0."""
    integer = lambda v: not isinstance(v, bool) and isinstance(v, (int, np.integer))
    try:
        kind, args = option[0], tuple(option[1:])
    except (TypeError, IndexError, KeyError):
        raise ValueError("out_size=%r: (\"size\", W, H) or (\"scale\", N)" % (option,)) from None
    if kind == "scale" and len(args) == 1 and integer(args[0]):
        if not 2 <= int(args[0]) <= SCALE_MAX_RATIO:
            raise ValueError("out_scale=%d: a divisor in 2..%d" % (int(args[0]), SCALE_MAX_RATIO))
        return ("scale", int(args[0]))
    if kind == "size" and len(args) == 2 and all(integer(v) for v in args):
        W, H = int(args[0]), int(args[1])
        if H < 1 or W < 1:
            raise ValueError("out_size %dx%d: both sides must be at least 1" % (W, H))
        return ("size", W, H)
    raise ValueError("out_size=%r: (\"size\", W, H) or (\"scale\", N)" % (option,))


def scale_option(option, hw):
    """(host only) The output-scale option for source frames of ``hw`` = (h, w) -> the output size (H, W): ``option`` is ("size", W, H) --
    the size itself, width first as a command line states it -- or ("scale", N), a divisor 2..16: H = ceil(h / N), W = ceil(w / N).
    ValueError with the reason for anything the scale rule (DESIGN §8 "Scale rule") refuses: a side of 0, a target larger than the source,
    a source side more than 16 times the target's."""
    h, w = int(hw[0]), int(hw[1])
    option = scale_form(option)
    if option[0] == "scale":
        N = option[1]
        H, W = (h + N - 1) // N, (w + N - 1) // N
    else:
        W, H = option[1:]
    if H > h or W > w:
        raise ValueError("out_size %dx%d is larger than the %dx%d frame: the scale step only scales down" % (W, H, w, h))
    if h > SCALE_MAX_RATIO * H or w > SCALE_MAX_RATIO * W:
        raise ValueError("out_size %dx%d is less than 1/%d of the %dx%d frame along a side" % (W, H, SCALE_MAX_RATIO, w, h))
    return H, W


def downscale_u8(frame_or_frames, H, W, out=None, n_frames=None):
    """The scale rule (DESIGN §8 "Scale rule", frcnn_downscale_u8): an (h, w, 3) uint8 device frame, or (n, h, w, 3) frames whose first
    stride may be larger than a frame, scaled down to (H, W) by the exact area mean, in integers -> ``out``, an (H, W, 3) or (n, H, W, 3)
    uint8 device tensor (allocated when None; its first stride too may be larger than a frame).  ``n_frames``: a device int32 word; the
    frames behind min(max(*n_frames, 0), n) are not written (None: all are).  One launch whatever n is; reads nothing on the host, so the
    call can be captured in a graph.  Bad arguments raise FrcnnError before anything is launched."""
    _require_gpu()
    t = frame_or_frames
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() in (3, 4) and t.shape[-1] == 3):
        raise _lib.FrcnnError("downscale_u8: frame must be an (h, w, 3) or (n, h, w, 3) uint8 device tensor")
    single = t.dim() == 3
    n, h, w = (1 if single else int(t.shape[0])), int(t.shape[-3]), int(t.shape[-2])
    H, W = int(H), int(W)
    if out is None:
        out = torch.empty(((H, W, 3) if single else (n, H, W, 3)), dtype=torch.uint8, device="cuda")
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == ((H, W, 3) if single else (n, H, W, 3))):
        raise _lib.FrcnnError("downscale_u8: out must be a uint8 device tensor of shape %s" % (((H, W, 3) if single else (n, H, W, 3)),))
    for name, x in (("frame", t), ("out", out)):                            # (a frame is contiguous; the frames may lie apart)
        if x.numel() and x.stride()[-3:] != (3 * int(x.shape[-2]), 3, 1):
            raise _lib.FrcnnError("downscale_u8: every frame of %s must be contiguous" % name)
    assert n_frames is None or (n_frames.is_cuda and n_frames.dtype == torch.int32 and n_frames.numel() >= 1)
    src_stride = 3 * h * w if single or n == 1 else int(t.stride(0))
    dst_stride = 3 * H * W if single or n == 1 else int(out.stride(0))
    _lib.call("frcnn_downscale_u8", t.data_ptr() if t.numel() else None, src_stride, n, _p(n_frames), h, w,
              out.data_ptr() if out.numel() else None, dst_stride, H, W, _stream())
    return out


# ----------------------------------------------------------------------------- re-identification
# (smallest, largest, the default) of pct and keep.  The defaults are PROVISIONAL: nobody has measured them on real footage.
TRACK_REID_PCT, TRACK_REID_KEEP, TRACK_REID_MAX = _lib.TRACK_REID_PCT, _lib.TRACK_REID_KEEP, _lib.TRACK_REID_MAX
TRACK_REID_ENTRY_WORDS, TRACK_REID_SIG_WORDS = _lib.TRACK_REID_ENTRY_WORDS, _lib.TRACK_REID_SIG_WORDS
TRACK_REID_LIST_WORDS, TRACK_REID_MAX_EVENTS = _lib.TRACK_REID_LIST_WORDS, _lib.TRACK_REID_MAX_EVENTS


def track_reid_option(pct=None, keep=None):
    """(host only) The re-identify option checked -> (pct, keep): pct the share of the largest distance two signatures can have up to
    which a new track takes an old id, 1..100 (None: 25); keep the frames an id that is gone is remembered, 1..4095 (None: 250).  Both
    defaults are PROVISIONAL: nobody has measured them on real footage.  ValueError with the reason."""
    out = []
    for name, v, (lo, hi, default) in (("pct", pct, TRACK_REID_PCT), ("keep", keep, TRACK_REID_KEEP)):
        v = default if v is None else v
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError("track reid %s=%r: an integer in %d..%d" % (name, v, lo, hi))
        out.append(int(v))
    return tuple(out)


def track_reid_state_words(capacity):
    """(host only) 4-byte words of a re-identify state of ``capacity`` entries (frcnn_track_reid_state_bytes / 4): 4 + 197 capacity."""
    n = int(_lib.load().frcnn_track_reid_state_bytes(int(capacity)))
    if n == 0:
        raise _lib.FrcnnError("track reid state: capacity=%r not in [1, %d]" % (capacity, TRACK_REID_MAX))
    return n // 4


def track_reid_state(capacity):
    """An empty re-identify state of ``capacity`` entries (1..256): a zeroed int32 device tensor, [n_entries, frames, dropped,
    reidentified | per entry: pid, tid, cls, last_seen, has_sig, sig[192]] (include/ext/frcnn_hip_track_reid.h).  Zeroing it
    (``track_reid_reset``) empties it."""
    _require_gpu()
    return torch.zeros(track_reid_state_words(capacity), dtype=torch.int32, device="cuda")


def track_reid_reset(state):
    """Empty the state (on the current stream): no entries, no frames, the sums 0."""
    state.zero_()
    return state


def track_reid_workspace(frames, rows):
    """What a ``track_reid_update`` call over ``frames`` tracked buffers of ``rows`` rows writes besides the state -> (``workspace``: int32
    (frames, rows, 193), a has-signature word and the signature of every row; ``out``: int32 (frames, 4 + 8 rows), the tracked buffers
    with pids; ``lists``: int32 (frames, TRACK_REID_LIST_WORDS)).  Nothing is carried in them between calls; a captured call passes them."""
    _require_gpu()
    n = int(_lib.load().frcnn_track_reid_workspace_bytes(int(frames), int(rows)))
    if n == 0:
        raise _lib.FrcnnError("track_reid_workspace: frames=%r (1..%d) or rows=%r (1..%d) out of range"
                              % (frames, _lib.TRACK_MAX_FRAMES, rows, _lib.REDACT_MAX_ROWS))
    frames, rows = int(frames), int(rows)
    return (torch.zeros((frames, rows, 1 + TRACK_REID_SIG_WORDS), dtype=torch.int32, device="cuda"),
            torch.zeros((frames, 4 + 8 * rows), dtype=torch.int32, device="cuda"),
            torch.zeros((frames, TRACK_REID_LIST_WORDS), dtype=torch.int32, device="cuda"))


def track_reid_update(state, frames_u8, frame_stride, tracked, n_frames, table, h, w, pct=None, keep=None, rgb=False, cuts=None,
                      capacity=None, workspace=None):
    """The re-identify rule (DESIGN §8 "Re-identify rule", frcnn_track_reid_update) over the frames of ``tracked`` IN ORDER: ``tracked``
    is a (frames, 4 + 8 rows) int32 tensor of PLAIN tracked buffers -- a ``track_update*`` call's ``out`` --, source frame f, as it was
    uploaded, lies at byte ``f * frame_stride`` of ``frames_u8`` ((h, w, 3) uint8 each; ``rgb``: the bytes are R, G, B, False: B, G, R),
    ``n_frames`` is the device word that says how many of them are real, ``table`` the tracker's class table.  Every live row gets a
    colour signature; a new tracker id whose signature lies within ``pct`` percent of the largest distance of that of an id the tracker
    gave up at most ``keep`` frames ago takes that id's place in ``state`` (``track_reid_state``; ``capacity``: its entries, read from its
    size when None).  ``cuts``: None, or the int32 device tensor of frames words a ``track_update_cut`` call wrote: a set word empties
    the table in front of its frame.  ``workspace``: ``track_reid_workspace(frames, rows)`` (allocated here when None; a captured call
    passes it) -> (out, lists): the tracked buffers with the rewritten ids, and frame f's re-identifications in ``lists[f]``
    (``track_reid_events``).  Two launches; everything is guarded on the device, so the call can be captured in a graph."""
    _require_gpu()
    assert state.is_cuda and state.dtype == torch.int32 and state.dim() == 1 and state.is_contiguous()
    assert tracked.is_cuda and tracked.dtype == torch.int32 and tracked.dim() == 2 and tracked.is_contiguous()
    assert n_frames.is_cuda and n_frames.dtype == torch.int32 and n_frames.numel() >= 1
    assert table.is_cuda and table.dtype == torch.uint8 and table.dim() == 1 and table.is_contiguous()
    frames, words = int(tracked.shape[0]), int(tracked.shape[1])
    assert (words - 4) % 8 == 0
    rows = (words - 4) // 8
    assert frames_u8.is_cuda and frames_u8.dtype == torch.uint8 and frames_u8.is_contiguous()
    assert int(frames_u8.numel()) >= (frames - 1) * int(frame_stride) + 3 * int(h) * int(w) and int(frame_stride) >= 0
    assert cuts is None or (cuts.is_cuda and cuts.dtype == torch.int32 and cuts.is_contiguous() and cuts.numel() == frames)
    if capacity is None:
        capacity = (int(state.numel()) - 4) // TRACK_REID_ENTRY_WORDS
    assert int(state.numel()) == track_reid_state_words(capacity)
    if workspace is None:
        workspace = track_reid_workspace(frames, rows)
    ws, out, lists = workspace
    assert ws.is_cuda and ws.dtype == torch.int32 and ws.is_contiguous() and tuple(ws.shape) == (frames, rows, 1 + TRACK_REID_SIG_WORDS)
    assert out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (frames, words)
    assert lists.is_cuda and lists.dtype == torch.int32 and lists.is_contiguous() and tuple(lists.shape) == (frames, TRACK_REID_LIST_WORDS)
    _lib.call("frcnn_track_reid_update", _p(state), int(capacity), _p(frames_u8), int(frame_stride), int(h), int(w), int(bool(rgb)),
              _p(tracked), words, rows, frames, _p(n_frames), _p(cuts), _p(table), int(table.numel()),
              TRACK_REID_PCT[2] if pct is None else int(pct), TRACK_REID_KEEP[2] if keep is None else int(keep), _p(ws), _p(out), words,
              _p(lists), _stream())
    return out, lists


def track_reid_events(rlist):
    """(host only) The events of one reid list's HOST copy -> [(pid, tid, cls, distance, gap)], in row order: the row the tracker calls
    tid is the object it called pid until ``gap`` frames ago; distance 0..8192."""
    c = np.asarray(rlist)
    return [tuple(int(v) for v in c[4 + 5 * k:9 + 5 * k]) for k in range(min(max(int(c[0]), 0), TRACK_REID_MAX_EVENTS))]


def track_reid_totals(state):
    """(host only; reads the state back) The sums of a re-identify state, device tensor or host copy -> {"entries", "frames", "dropped",
    "reidentified"}."""
    s = state.cpu().numpy() if isinstance(state, torch.Tensor) else np.asarray(state)
    return {"entries": int(s[0]), "frames": int(s[1]), "dropped": int(s[2]), "reidentified": int(s[3])}


TRACK_LOOKBACK = _lib.TRACK_LOOKBACK            # (smallest, largest, the default) look-back of ``track_lookback``, in frames


def track_lookback_option(n=None):
    """(host only) The look-back in frames checked, None replaced by the default 8: an integer in 1..16.  ValueError with the reason."""
    lo, hi, default = TRACK_LOOKBACK
    n = default if n is None else n
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not lo <= int(n) <= hi:
        raise ValueError("track lookback=%r: an integer in %d..%d" % (n, lo, hi))
    return int(n)


def track_lookback_state(frames, h, w, max_rows, capacity, back):
    """An empty look-back window for calls of ``frames`` frames of (h, w) whose tracked buffers have ``max_rows`` + ``capacity`` rows: a
    zeroed uint8 device tensor of frcnn_track_lookback_state_bytes bytes, [count, half, back_overflow, 0 x 5 (int32) | two halves of
    ``frames`` cells, each a widened tracked buffer of R2 = max_rows + capacity + back rows and a frame]
    (include/ext/frcnn_hip_track_lookback.h)."""
    _require_gpu()
    n = int(_lib.load().frcnn_track_lookback_state_bytes(int(frames), int(h), int(w), int(max_rows), int(capacity), int(back)))
    if n == 0:
        raise _lib.FrcnnError("track_lookback_state: frames=%r, %rx%r, max_rows=%r, capacity=%r, back=%r out of range (at most %d rows in all)"
                              % (frames, h, w, max_rows, capacity, back, _lib.REDACT_MAX_ROWS))
    return torch.zeros(n, dtype=torch.uint8, device="cuda")


def track_lookback_reset(window):
    """Empty the window (on the current stream): the header is zeroed, so no frame waits and back_overflow is 0."""
    window[:_lib.TRACK_LOOKBACK_HEADER].zero_()
    return window


def _track_window_call(who, window, frames_u8, frame_stride, tracked, n_frames, capacity, back, h, w, lookback, radius, grow, interval, out):
    """The body ``track_lookback`` and ``track_backtrack`` share: the checks (``who`` names the caller in their messages), ``out`` and the
    call of frcnn_<who>; ``interval``: the arguments the entry point takes between ``grow`` and the frame's size -- (interval,) or none."""
    _require_gpu()
    h, w, cap, back = int(h), int(w), int(capacity), int(back)
    assert window.is_cuda and window.dtype == torch.uint8 and window.dim() == 1 and window.is_contiguous()
    assert tracked.is_cuda and tracked.dtype == torch.int32 and tracked.is_contiguous() and tracked.dim() == 2
    B, words = int(tracked.shape[0]), int(tracked.shape[1])
    R = (words - 4) // 8
    rows, R2 = R - cap, R + back
    assert words == 4 + 8 * R and rows >= 1, "%s: tracked buffers of %d words for capacity=%d" % (who, words, cap)
    need = int(_lib.load().frcnn_track_lookback_state_bytes(B, h, w, rows, cap, back))
    if need and int(window.numel()) != need:
        raise _lib.FrcnnError("%s: the window has %d bytes; one for calls of %d frames of %dx%d with %d + %d + %d rows has %d "
                              "(track_lookback_state with the call's frames, rows, capacity and back)" % (who, window.numel(), B, h, w, rows, cap, back, need))
    assert frames_u8.is_cuda and frames_u8.dtype == torch.uint8 and frames_u8.is_contiguous()
    assert int(frame_stride) >= 0 and int(frames_u8.numel()) >= (B - 1) * int(frame_stride) + 3 * h * w
    assert n_frames.is_cuda and n_frames.dtype == torch.int32 and n_frames.numel() >= 1
    if out is None:
        out = (torch.zeros((B, h, w, 3), dtype=torch.uint8, device="cuda"), torch.zeros((B, 4 + 8 * R2), dtype=torch.int32, device="cuda"),
               torch.zeros(1, dtype=torch.int32, device="cuda"))
    o_frames, o_tracked, o_count = out
    assert o_frames.is_cuda and o_frames.dtype == torch.uint8 and o_frames.is_contiguous() and tuple(o_frames.shape) == (B, h, w, 3)
    assert o_tracked.is_cuda and o_tracked.dtype == torch.int32 and o_tracked.is_contiguous() and tuple(o_tracked.shape) == (B, 4 + 8 * R2)
    assert o_count.is_cuda and o_count.dtype == torch.int32 and o_count.numel() >= 1
    _lib.call("frcnn_" + who, _p(window), _p(frames_u8), int(frame_stride), _p(tracked), words, B, _p(n_frames), rows, cap, back,
              int(lookback), int(radius), int(grow), *interval, h, w, _p(o_frames), 3 * h * w, _p(o_tracked), 4 + 8 * R2, _p(o_count), _stream())
    return out


def track_lookback(window, frames_u8, frame_stride, tracked, n_frames, capacity, back, h, w, lookback=TRACK_LOOKBACK[2], radius=0, grow=0, out=None):
    """One call of the look-back rule (DESIGN §8 "Look-back rule", frcnn_track_lookback): the B frames of the call -- ``frames_u8`` holds
    frame f, (h, w, 3) uint8 as uploaded, at byte ``f * frame_stride``; ``tracked`` is ``track_update``'s (B, 4 + 8R) result for them --
    join ``window`` (``track_lookback_state``), every track born in them is followed BACKWARDS over at most ``lookback`` frames by the
    block match of radius ``radius`` (0: its box stands still) and leaves one back-filled row, age -k, in each of those frames, and the
    frames the window held before the call are emitted: -> ``out`` = (frames (B, h, w, 3) uint8, tracked (B, 4 + 8 R2) int32, count
    int32 [1]), R2 = R + ``back``; the first ``count`` entries are the emitted frames, oldest first, untouched, with their widened
    buffers (``redact_u8`` and ``annotate_u8`` take one with ``tracked=True``).  ``n_frames``: an int32 device tensor; its first word
    says how many of the B frames are real, 0 emits again and changes nothing, < 0 emits and empties the window.  Five launches; every
    count is read on the device: the call can be captured in a graph."""
    return _track_window_call("track_lookback", window, frames_u8, frame_stride, tracked, n_frames, capacity, back, h, w, lookback, radius, grow,
                              (), out)


def track_backtrack_option(n, k, frames):
    """(host only) The look-back of a back-tracking pass checked against its interval ``k`` and its ``frames`` source frames, None (or a
    bare option, True) replaced by min(16, frames): an integer in 1..16, at least k - 1 and at most ``frames``.  ValueError with the
    reason."""
    lo, hi, _ = TRACK_LOOKBACK
    k, frames = int(k), int(frames)
    if n is None or n is True:
        n = min(hi, frames)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not lo <= int(n) <= hi:
        raise ValueError("track backtrack=%r: an integer in %d..%d" % (n, lo, hi))
    n = int(n)
    if n < k - 1:
        raise ValueError("track backtrack=%d does not reach over the %d frames between two detections: frames no detection reaches would stay "
                         "uncovered; at least %d with a detection every %d frames" % (n, k - 1, k - 1, k))
    if n > frames:
        raise ValueError("track backtrack=%d reaches further back than a pass of %d frames holds: a frame would be emitted before its rows are "
                         "in place; at most %d here" % (n, frames, frames))
    return n


def track_backtrack(window, frames_u8, frame_stride, tracked, n_frames, capacity, back, h, w, lookback, radius, grow, interval, out=None):
    """One call of the back-track rule (DESIGN §8 "Back-track rule", frcnn_track_backtrack): ``track_lookback`` over the F frames of an
    interval call -- ``tracked`` is ``track_update_interval``'s (F, 4 + 8R) result with the same ``interval`` --, where every tracked live
    row of a KEY frame is followed backwards: a new track over at most ``lookback`` frames, a continued one through the between frames in
    front of its key frame.  ``window`` is a ``track_lookback_state`` for F frames; everything else, ``out`` and the return value: as
    ``track_lookback``.  With ``interval`` 1 every byte is ``track_lookback``'s.  Five launches; the call can be captured in a graph."""
    return _track_window_call("track_backtrack", window, frames_u8, frame_stride, tracked, n_frames, capacity, back, h, w, lookback, radius, grow,
                              (int(interval),), out)


def split_tracked(buf):
    """Views (n_rows, n_live, next_id, overflow, bbox, cls, prob, id, age) into ONE tracked buffer (device tensor or its host copy,
    torch or numpy), as ``split_detections`` cuts up a ``det_packed``: the four counts are one-word views, bbox is (R, 4), prob float32."""
    R = (int(buf.shape[0]) - 4) // 8
    prob = buf[4 + 5 * R:4 + 6 * R]
    prob = prob.view(torch.float32) if isinstance(prob, torch.Tensor) else prob.view(np.float32)
    bbox = buf[4:4 + 4 * R]
    bbox = bbox.view(R, 4) if isinstance(bbox, torch.Tensor) else bbox.reshape(R, 4)
    return (buf[0:1], buf[1:2], buf[2:3], buf[3:4], bbox, buf[4 + 4 * R:4 + 5 * R], prob, buf[4 + 6 * R:4 + 7 * R], buf[4 + 7 * R:4 + 8 * R])


def tracked_dets(buf, names, start=0, propagated=False):
    """(host only) ONE tracked buffer's host copy (numpy) as dets -> (n_live, the rows' ids, [{"bbox", "cls_name", "prob", "track_id"} for
    the rows from ``start`` on]): the live rows first -- with "propagated": True when ``propagated``: the rows of a between frame, which
    are the tracks themselves --, then the rows behind them with "held" = their age, or for a look-back's back-filled rows (age -k)
    "backfilled" = k.  ``names``: class index -> name.  A caller that has the live rows as dets already passes their number as ``start``
    and takes their ids from the second value."""
    n_rows, n_live, _, _, bbox, cls, prob, tid, age = split_tracked(buf)
    n_live, dets = int(n_live[0]), []
    for k in range(start, int(n_rows[0])):
        d = {"bbox": bbox[k].astype(np.int64), "cls_name": names[int(cls[k])], "prob": prob[k].copy(), "track_id": int(tid[k])}
        if k >= n_live:
            d["held" if int(age[k]) > 0 else "backfilled"] = abs(int(age[k]))
        elif propagated:
            d["propagated"] = True
        dets.append(d)
    return n_live, tid, dets


PNG_BAND_ROWS = 1       # scanlines per IDAT chunk of the device encoder (frcnn_png_band_rows(); tests/test_png_cpu.py holds the two together)
PNG_HUFF_BAND_ROWS = 8   # ... of its huffman mode (frcnn_png_huff_band_rows(); tests/test_png_huff_cpu.py)
# compress= of the png_* calls -> the prefix of their entry points: "runs" (include/ext/frcnn_hip_png.h: Sub filter, fixed Huffman codes,
# run matches) or "huffman" (include/ext/frcnn_hip_png_huff.h: adaptive row filters, a dynamic Huffman code per band)
PNG_COMPRESS = {"runs": "frcnn_png_", "huffman": "frcnn_png_huff_"}


def _png_entry(compress, what):
    if compress not in PNG_COMPRESS:
        raise _lib.FrcnnError("%s: compress=%r (one of %s)" % (what, compress, ", ".join(PNG_COMPRESS)))
    return PNG_COMPRESS[compress]


def png_bound(h, w, compress="runs"):
    """The largest PNG file, in bytes, that ``png_encode_u8`` can make of an (h, w, 3) frame (frcnn_png_bound / frcnn_png_huff_bound: the
    stored form of every band plus the framing).  A pure host call: needs the built library, no GPU."""
    h, w = int(h), int(w)
    bound = getattr(_lib.load(), _png_entry(compress, "png_bound") + "bound")
    n = int(bound(h, w)) if 1 <= h < 2 ** 31 and 1 <= w < 2 ** 31 else 0
    if n == 0:
        raise _lib.FrcnnError(f"png_bound: frame {h}x{w} unsupported (both sides >= 1, h * (1 + 3w) below 2 GiB)")
    return n


def png_workspace_bytes(h, w, compress="runs"):
    """Bytes of device workspace ``png_encode_u8`` needs for an (h, w, 3) frame (frcnn_png_workspace_bytes / frcnn_png_huff_...)."""
    png_bound(h, w, compress)
    return int(getattr(_lib.load(), _png_entry(compress, "png_workspace_bytes") + "workspace_bytes")(int(h), int(w)))


def png_encode_u8(frame, bgr=False, out=None, out_len=None, workspace=None, compress="runs"):
    """Encode ``frame`` -- an (h, w, 3) uint8 device tensor, R,G,B per pixel or (``bgr``) B,G,R -- as an 8-bit RGB PNG file on the device
    (frcnn_png_encode_u8; ``compress`` = "huffman": frcnn_png_huff_encode_u8, adaptive row filters and a dynamic Huffman code per band of
    PNG_HUFF_BAND_ROWS rows).  -> (out, out_len): ``out`` uint8 [>= png_bound(h, w, compress)] holds the file, ``out_len`` int32 [1] its
    length; what is not passed (``workspace`` included) is allocated.  Never synchronises; reads nothing on the host per frame, so the call
    can be captured in a graph with fixed ``out`` / ``out_len`` / ``workspace``.  Bad arguments raise FrcnnError before anything is launched."""
    prefix = _png_entry(compress, "png_encode_u8")
    _require_gpu()
    if not (isinstance(frame, torch.Tensor) and frame.is_cuda and frame.dtype == torch.uint8 and frame.dim() == 3
            and frame.shape[2] == 3 and frame.is_contiguous()):
        raise _lib.FrcnnError("png_encode_u8: frame must be a contiguous (h, w, 3) uint8 device tensor, got %s"
                              % (tuple(frame.shape) if isinstance(frame, torch.Tensor) else type(frame).__name__,))
    h, w = int(frame.shape[0]), int(frame.shape[1])
    lib = _lib.load()
    bound, need = int(getattr(lib, prefix + "bound")(h, w)), int(getattr(lib, prefix + "workspace_bytes")(h, w))
    if out is None and bound:
        out = torch.empty(bound, dtype=torch.uint8, device="cuda")
    if out_len is None:
        out_len = torch.zeros(1, dtype=torch.int32, device="cuda")
    if workspace is None and need:
        workspace = _ws(need)
    for name, t, dt in (("out", out, torch.uint8), ("out_len", out_len, torch.int32), ("workspace", workspace, torch.uint8)):
        if t is not None and not (t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise _lib.FrcnnError(f"png_encode_u8: {name} must be a contiguous {dt} device tensor")
    if workspace is not None and workspace.numel() < need:
        raise _lib.FrcnnError(f"png_encode_u8: workspace of {workspace.numel()} bytes, {need} needed")
    _lib.call(prefix + "encode_u8", _p(frame) if frame.numel() else None, h, w, 1 if bgr else 0, _p(out), out.numel() if out is not None else 0,
              _p(out_len), _p(workspace), _stream())
    return out, out_len


def png_bytes(frame, bgr=False, compress="runs"):
    """``png_encode_u8`` and the file as ``bytes``: the eager convenience (one synchronisation, one copy of the encoded length)."""
    out, out_len = png_encode_u8(frame, bgr=bgr, compress=compress)
    n = int(out_len.item())
    if not 0 < n <= out.numel():
        raise _lib.FrcnnError(f"png_bytes: encoded length {n} outside (0, {out.numel()}]")
    return out[:n].cpu().numpy().tobytes()

JPEG_RESTART_MCUS = 16   # MCUs per restart interval of the device JPEG encoder (frcnn_jpeg_restart_mcus(); tests/test_jpeg_cpu.py)


def _jpeg_mode(what, subsampling, huffman):
    """-> (default mode?, the C ABI's huffman value): (444, "standard") takes frcnn_jpeg_* (revision 1 of the encoder), every other pair
    frcnn_jpeg_opt_* (include/ext/frcnn_hip_jpeg_opt.h)."""
    if isinstance(subsampling, bool) or subsampling not in _lib.JPEG_OPT_SUBSAMPLINGS:
        raise _lib.FrcnnError("%s: subsampling=%r (444 or 420)" % (what, subsampling))
    if not isinstance(huffman, str) or huffman not in _lib.JPEG_OPT_HUFFMANS:
        raise _lib.FrcnnError("%s: huffman=%r (\"standard\" or \"optimized\")" % (what, huffman))
    return (subsampling == 444 and huffman == "standard"), _lib.JPEG_OPT_HUFFMANS[huffman]


def jpeg_restart_mcus(subsampling=444):
    """MCUs per restart interval: 16 at 4:4:4, 8 at 4:2:0 (48 blocks either way)."""
    _jpeg_mode("jpeg_restart_mcus", subsampling, "standard")
    return int(_lib.load().frcnn_jpeg_opt_restart_mcus(int(subsampling)))


def jpeg_bound(h, w, subsampling=444, huffman="standard"):
    """The largest JPEG file, in bytes, that ``jpeg_encode_u8`` can make of an (h, w, 3) frame in this mode (frcnn_jpeg_bound /
    frcnn_jpeg_opt_bound: every block at its longest, every byte stuffed; the same for both ``huffman`` modes).  A pure host call: needs
    the built library, no GPU."""
    default, _ = _jpeg_mode("jpeg_bound", subsampling, huffman)
    h, w = int(h), int(w)
    lib = _lib.load()
    n = 0
    if 1 <= h < 2 ** 31 and 1 <= w < 2 ** 31:
        n = int(lib.frcnn_jpeg_bound(h, w)) if default else int(lib.frcnn_jpeg_opt_bound(h, w, int(subsampling)))
    if n == 0:
        raise _lib.FrcnnError(f"jpeg_bound: frame {h}x{w} unsupported (both sides in 1..65535, the bound below 2 GiB)")
    return n


def jpeg_header_bytes():
    """Bytes in front of a file's entropy-coded data, SOI .. SOS: the same for every frame with the standard tables, the most with
    optimised ones (frcnn_jpeg_header_bytes)."""
    return int(_lib.load().frcnn_jpeg_header_bytes())


def jpeg_workspace_bytes(h, w, subsampling=444, huffman="standard"):
    """Bytes of device workspace ``jpeg_encode_u8`` needs for an (h, w, 3) frame in this mode (frcnn_jpeg_workspace_bytes /
    frcnn_jpeg_opt_workspace_bytes)."""
    default, huff = _jpeg_mode("jpeg_workspace_bytes", subsampling, huffman)
    jpeg_bound(h, w, subsampling, huffman)
    if default:
        return int(_lib.load().frcnn_jpeg_workspace_bytes(int(h), int(w)))
    return int(_lib.load().frcnn_jpeg_opt_workspace_bytes(int(h), int(w), int(subsampling), huff))


def jpeg_encode_u8(frame, quality=90, bgr=False, out=None, out_len=None, workspace=None, subsampling=444, huffman="standard"):
    """Encode ``frame`` -- an (h, w, 3) uint8 device tensor, R,G,B per pixel or (``bgr``) B,G,R -- as a baseline JFIF file (the
    Annex K quantisation tables at IJG ``quality`` 1..100, restart intervals of jpeg_restart_mcus(subsampling) MCUs) on the device.
    ``subsampling`` 444 or 420 (chroma halved both ways), ``huffman`` "standard" (Annex K.3) or "optimized" (four tables built on the
    device from the frame's own symbol counts, libjpeg's construction).  The defaults take frcnn_jpeg_encode_u8 as before, every other
    pair frcnn_jpeg_opt_encode_u8.
    -> (out, out_len): ``out`` uint8 [>= jpeg_bound(h, w, subsampling)] holds the file, ``out_len`` int32 [1] its length; what is not
    passed (``workspace`` included) is allocated.  Never synchronises; reads nothing on the host per frame, so the call can be captured in
    a graph with fixed ``out`` / ``out_len`` / ``workspace``.  Bad arguments raise FrcnnError before anything is launched."""
    _require_gpu()
    default, huff = _jpeg_mode("jpeg_encode_u8", subsampling, huffman)
    if not (isinstance(frame, torch.Tensor) and frame.is_cuda and frame.dtype == torch.uint8 and frame.dim() == 3
            and frame.shape[2] == 3 and frame.is_contiguous()):
        raise _lib.FrcnnError("jpeg_encode_u8: frame must be a contiguous (h, w, 3) uint8 device tensor, got %s"
                              % (tuple(frame.shape) if isinstance(frame, torch.Tensor) else type(frame).__name__,))
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
        raise _lib.FrcnnError("jpeg_encode_u8: quality=%r (an integer in 1..100)" % (quality,))
    h, w = int(frame.shape[0]), int(frame.shape[1])
    lib = _lib.load()
    if default:
        bound, need = int(lib.frcnn_jpeg_bound(h, w)), int(lib.frcnn_jpeg_workspace_bytes(h, w))
    else:
        bound = int(lib.frcnn_jpeg_opt_bound(h, w, int(subsampling)))
        need = int(lib.frcnn_jpeg_opt_workspace_bytes(h, w, int(subsampling), huff))
    if out is None and bound:
        out = torch.empty(bound, dtype=torch.uint8, device="cuda")
    if out_len is None:
        out_len = torch.zeros(1, dtype=torch.int32, device="cuda")
    if workspace is None and need:
        workspace = _ws(need)
    for name, t, dt in (("out", out, torch.uint8), ("out_len", out_len, torch.int32), ("workspace", workspace, torch.uint8)):
        if t is not None and not (t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise _lib.FrcnnError(f"jpeg_encode_u8: {name} must be a contiguous {dt} device tensor")
    if workspace is not None and workspace.numel() < need:
        raise _lib.FrcnnError(f"jpeg_encode_u8: workspace of {workspace.numel()} bytes, {need} needed")
    if default:
        _lib.call("frcnn_jpeg_encode_u8", _p(frame) if frame.numel() else None, h, w, 1 if bgr else 0, int(quality), _p(out),
                  out.numel() if out is not None else 0, _p(out_len), _p(workspace), _stream())
    else:
        _lib.call("frcnn_jpeg_opt_encode_u8", _p(frame) if frame.numel() else None, h, w, 1 if bgr else 0, int(quality), int(subsampling),
                  huff, _p(out), out.numel() if out is not None else 0, _p(out_len), _p(workspace), _stream())
    return out, out_len


def jpeg_bytes(frame, quality=90, bgr=False, subsampling=444, huffman="standard"):
    """``jpeg_encode_u8`` and the file as ``bytes``: the eager convenience (one synchronisation, one copy of the encoded length)."""
    out, out_len = jpeg_encode_u8(frame, quality=quality, bgr=bgr, subsampling=subsampling, huffman=huffman)
    n = int(out_len.item())
    if not 0 < n <= out.numel():
        raise _lib.FrcnnError(f"jpeg_bytes: encoded length {n} outside (0, {out.numel()}]")
    return out[:n].cpu().numpy().tobytes()


def jpeg_build_tables(hist, out=None):
    """The optimised encoder's table kernel alone (frcnn_jpeg_opt_build_tables): ``hist`` four histograms of 256 counts (an int32
    device tensor [4][256] whose bits are read as uint32, or anything numpy makes into [4][256] counts below 2^32) -> a uint8 device
    tensor [4][276]: four ``_lib.JpegOptTable`` records (BITS[16], HUFFVAL[256], count), table k from histogram k by libjpeg's
    jpeg_gen_optimal_table.  ``jpeg_tables_from_records`` unpacks them on the host."""
    _require_gpu()
    if not isinstance(hist, torch.Tensor):
        a = np.asarray(hist)
        if a.shape != (4, 256) or a.min() < 0 or a.max() >= 2 ** 32:
            raise _lib.FrcnnError("jpeg_build_tables: hist must be [4][256] counts in 0..2^32-1")
        hist = torch.from_numpy(a.astype(np.uint32).view(np.int32).copy()).cuda()
    if not (hist.is_cuda and hist.dtype == torch.int32 and tuple(hist.shape) == (4, 256) and hist.is_contiguous()):
        raise _lib.FrcnnError("jpeg_build_tables: hist must be a contiguous int32 device tensor [4][256]")
    size = ctypes.sizeof(_lib.JpegOptTable)
    if out is None:
        out = torch.zeros((4, size), dtype=torch.uint8, device="cuda")
    if not (out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (4, size) and out.is_contiguous()):
        raise _lib.FrcnnError(f"jpeg_build_tables: out must be a contiguous uint8 device tensor [4][{size}]")
    _lib.call("frcnn_jpeg_opt_build_tables", _p(hist), _p(out), _stream())
    return out


def jpeg_tables_from_records(records):
    """``jpeg_build_tables``'s result -> [(BITS: 16 ints, HUFFVAL: the table's symbols)] x 4 on the host (one synchronising copy)."""
    raw = records.cpu().numpy().tobytes()
    size = ctypes.sizeof(_lib.JpegOptTable)
    out = []
    for k in range(4):
        rec = _lib.JpegOptTable.from_buffer_copy(raw[k * size:(k + 1) * size])
        out.append((list(rec.bits), list(rec.huffval)[:rec.count]))
    return out


class JpegUnsupported(_lib.FrcnnError):
    """``jpeg_dec_plan``: the file lies outside the device decoder's supported set; the message names the reason."""


class PngUnsupported(_lib.FrcnnError):
    """``png_dec_plan``: the file lies outside the device decoder's supported set; the message names the reason."""


PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
PNG_DEC_WINDOW_BYTES = _lib.PNG_DEC_WINDOW_BYTES    # compressed bytes per window of the inflate kernel (a larger block carries its tables over)
PNG_DEC_FULL_PLTE_BYTES = _lib.PNG_DEC_FULL_PLTE_BYTES


@dataclasses.dataclass(frozen=True)
class DeviceDecoder:
    """One device decoder of file-backed frames: what its C entry points are called and take, and every operation on them ONCE.  The
    public functions below (``jpeg_dec_plan`` ... ``png_decode_full_u8``) are bindings of these methods to one of the four records.
    ``stem`` / ``decode_stem`` / ``items_name``: the names "frcnn_" + name are the C symbols of and the messages speak of
    (<stem>_plan, <stem>_spans, <stem>_workspace_bytes, <stem>_batch_layout; <decode_stem>_batch_u8, <decode_stem>_u8); ``setting``: the
    value of a decoder setting (feed.py, entry.py) that selects it; ``palette``: its items carry ``plte_off``; ``whole_file``: what it
    stages of a file is the whole file (the JPEG records), not a stream gathered from it."""
    label: str
    setting: str
    stem: str
    decode_stem: str
    items_name: str
    plan_type: type
    item_type: type
    batch_max: int
    unsupported: type
    palette: bool = False
    whole_file: bool = False
    stateless: bool = False         # its kernels need no workspace and report no status (no <stem>_workspace_bytes / _batch_layout)
    planner: object = None          # a Python planner (the y4m header is text: y4m.parse_header) instead of frcnn_<stem>_plan

    def plan(self, data):
        if self.planner is not None:
            return self.planner(data)
        who = self.stem + "_plan"
        if not isinstance(data, (bytes, bytearray, memoryview)):
            raise _lib.FrcnnError("%s: the file's bytes, got %s" % (who, type(data).__name__))
        data = bytes(data)
        plan = self.plan_type()
        lib = _lib.load()
        code = getattr(lib, "frcnn_" + who)(data, len(data), ctypes.byref(plan))
        if code == _lib.E_UNSUPPORTED:
            raise self.unsupported((lib.frcnn_last_error() or b"").decode())
        _lib.check(code, "frcnn_" + who)
        return plan

    def workspace_bytes(self, plan):
        if self.stateless:
            return 0
        who = self.stem + "_workspace_bytes"
        n = int(getattr(_lib.load(), "frcnn_" + who)(ctypes.byref(plan)))
        if n == 0:
            raise _lib.FrcnnError("%s: not a plan that %s_plan made" % (who, self.stem))
        return n

    def layout(self, plans):
        who, n = self.stem + "_batch_layout", len(plans)
        if not 1 <= n <= self.batch_max:
            raise _lib.FrcnnError(f"{who}: {n} plans, 1..{self.batch_max} go into one batch")
        if self.stateless:
            return [0] * n, 0
        arr = (self.plan_type * n)(*plans)
        offs = (ctypes.c_uint64 * n)()
        total = int(getattr(_lib.load(), "frcnn_" + who)(arr, n, offs))
        if total == 0:
            raise _lib.FrcnnError("%s: not plans that %s_plan made" % (who, self.stem))
        return [int(o) for o in offs], total

    def items(self, plans, file_off, out_off, ws_off, plte_off=None):
        """The item table of a batch; a palette lies behind its stream in the file's staged bytes (``stage``) unless ``plte_off`` says
        where else."""
        items = (self.item_type * len(plans))()
        for it, p, f, o, w in zip(items, plans, file_off, out_off, ws_off):
            it.plan, it.file_off, it.out_off, it.ws_off = p, int(f), int(o), int(w)
        if self.palette:
            for it, q in zip(items, plte_off if plte_off is not None else [int(f) + int(p.stream_len) for f, p in zip(file_off, plans)]):
                it.plte_off = int(q)
        return items

    def decode(self, files, items, out, bgr=False, status=None, workspace=None, items_dev=None):
        _require_gpu()
        who, n = self.decode_stem + "_batch_u8", len(items)
        if not isinstance(items, ctypes.Array) or items._type_ is not self.item_type:
            raise _lib.FrcnnError("%s: items must be a table made by %s" % (who, self.items_name))
        if items_dev is None:
            items_dev = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).cuda()
        if status is None and not self.stateless:
            status = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
        if self.stateless:
            workspace = None
        elif workspace is None:
            workspace = _ws(max((int(it.ws_off) + self.workspace_bytes(it.plan) for it in items), default=0))
        for name, t, dt in (("files", files, torch.uint8), ("out", out, torch.uint8), ("status", status, torch.int32),
                            ("workspace", workspace, torch.uint8), ("items_dev", items_dev, torch.uint8)):
            if t is None and self.stateless and name in ("workspace", "status"):
                continue
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt and t.is_contiguous()):
                raise _lib.FrcnnError(f"{who}: {name} must be a contiguous {dt} device tensor")
        if items_dev.numel() < ctypes.sizeof(items) or (status is not None and status.numel() < n):
            raise _lib.FrcnnError(f"{who}: items_dev of {items_dev.numel()} bytes / status of {status.numel()} words for {n} items")
        _lib.call("frcnn_" + who, ctypes.addressof(items), _p(items_dev), n, _p(files), files.numel(), 1 if bgr else 0,
                  _p(out), out.numel(), _p(status) if status is not None else None, _p(workspace) if workspace is not None else None,
                  workspace.numel() if workspace is not None else 0, _stream())
        return status

    # ---- the PNG records only: a .png file's zlib stream is gathered on the host
    def spans(self, data, plan):
        data = bytes(data)
        n = int(plan.idat_count)
        spans = (ctypes.c_uint32 * (2 * max(n, 1)))()
        _lib.call("frcnn_%s_spans" % self.stem, data, len(data), ctypes.byref(plan), spans, n)
        return [(int(spans[2 * k]), int(spans[2 * k + 1])) for k in range(n)]

    def stream(self, data, plan):
        data = bytes(data)
        spans = self.spans(data, plan)
        return data[spans[0][0]:spans[0][0] + spans[0][1]] if len(spans) == 1 else b"".join(data[o:o + n] for o, n in spans)

    def palette_of(self, data, plan):
        """The PLTE entries zero-padded to PNG_DEC_FULL_PLTE_BYTES for a colour-type-3 file under a decoder with palettes, else b""."""
        if not self.palette or int(plan.colour_type) != 3:
            return b""
        palette = bytes(data)[int(plan.plte_off):int(plan.plte_off) + 3 * int(plan.plte_entries)]
        return palette + bytes(PNG_DEC_FULL_PLTE_BYTES - len(palette))

    def stage(self, data, plan):
        """What goes to the device for one file: the file itself (``whole_file``), or its zlib stream, behind it its staged palette where
        it has one."""
        if self.whole_file:
            return bytes(data)
        return self.stream(data, plan) + self.palette_of(data, plan)

    def decode_one(self, file_bytes, bgr=False):
        _require_gpu()
        data = bytes(file_bytes)
        plan = self.plan(data)
        files = torch.frombuffer(bytearray(self.stage(data, plan)), dtype=torch.uint8).cuda()
        out = torch.empty((int(plan.h), int(plan.w), 3), dtype=torch.uint8, device="cuda")
        status = self.decode(files, self.items([plan], [0], [0], [0]), out.view(-1), bgr=bgr)
        word = int(status.cpu()[0])
        if word:
            raise_damaged(self, word, who=self.decode_stem + "_u8")
        return out


JPEG_DECODER = DeviceDecoder("JPEG", "device", "jpeg_dec", "jpeg_decode", "jpeg_batch_items", _lib.JpegDecPlan, _lib.JpegDecBatchItem,
                             _lib.JPEG_DEC_BATCH_MAX, JpegUnsupported, whole_file=True)
# progressive files (include/ext/frcnn_hip_jpeg_dec_full.h): the decoder the JPEG setting "device_full" adds BEHIND the baseline one
JPEG_FULL_DECODER = DeviceDecoder("JPEG", "device_full", "jpeg_dec_full", "jpeg_decode_full", "jpeg_full_batch_items", _lib.JpegDecFullPlan,
                                  _lib.JpegDecFullBatchItem, _lib.JPEG_DEC_BATCH_MAX, JpegUnsupported, whole_file=True)
# by the value of a PNG decoder setting (feed.PNG_DECODERS but "host")
PNG_DECODERS = {
    "device": DeviceDecoder("PNG", "device", "png_dec", "png_decode", "png_batch_items", _lib.PngDecPlan, _lib.PngDecBatchItem,
                            _lib.PNG_DEC_BATCH_MAX, PngUnsupported),
    "device_full": DeviceDecoder("PNG", "device_full", "png_dec_full", "png_decode_full", "png_full_batch_items", _lib.PngDecFullPlan,
                                 _lib.PngDecFullBatchItem, _lib.PNG_DEC_BATCH_MAX, PngUnsupported, palette=True),
}
_PNG1, _PNGF = PNG_DECODERS["device"], PNG_DECODERS["device_full"]


# ``y4m_parse_header``: a stream outside the supported set (10/12/16-bit samples, interlaced frames, C420paldv, C411, C444alpha); a
# FrcnnError whose message names the reason (the class y4m.Y4mReader raises too)
Y4mUnsupported = _y4m.Y4mUnsupported


def y4m_parse_header(data):
    """The header of a YUV4MPEG2 stream (``data``: bytes that hold at least its first line) -> a ``_lib.Y4mPlan``: h, w, chroma, range,
    frame_bytes (the C fields: what a batch item carries), ``chroma_name`` / ``range_name``, and as attributes ``tags`` -- the F / A / I
    values verbatim -- and ``header_len``.  ``Y4mUnsupported`` (a FrcnnError) with the reason for a stream outside the supported set,
    ``FrcnnError`` for a broken header.  Pure host work, no library needed."""
    return _y4m.parse_header(data)


# YUV4MPEG2 frames (include/ext/frcnn_hip_y4m.h): what it stages of a frame is the frame; stateless, a Python planner
Y4M_DECODER = DeviceDecoder("Y4M", "device", "y4m", "y4m_decode", "y4m_batch_items", _lib.Y4mPlan, _lib.Y4mBatchItem, _lib.Y4M_BATCH_MAX,
                            Y4mUnsupported, whole_file=True, stateless=True, planner=y4m_parse_header)
_DECODER_OF = {d.plan_type: d for d in (JPEG_DECODER, JPEG_FULL_DECODER, _PNG1, _PNGF, Y4M_DECODER)}


def decoder_of(plan):
    """The ``DeviceDecoder`` whose planner made ``plan``."""
    return _DECODER_OF[type(plan)]


def raise_damaged(dec, word, name=None, who=None):
    """The FrcnnError for a file whose device decode (by ``dec``) left the status word ``word``: about the file ``name``, or in the words
    of the eager function ``who``."""
    what = "(status %d: FRCNN_%s_DEC_* in include/ext/frcnn_hip_%s_dec.h)" % (word, dec.label, dec.label.lower())
    if name is None:
        raise _lib.FrcnnError("%s: the file is damaged %s" % (who, what))
    raise _lib.FrcnnError("device %s decoder: %s is damaged %s; decode it on the host or repair the file" % (dec.label, name, what))


def jpeg_dec_plan(data):
    """The host-side marker parse of a .jpg file's bytes (frcnn_jpeg_dec_plan) -> a ``_lib.JpegDecPlan``: size, components, sampling,
    where the tables and the entropy-coded segment lie, into how many subsequences it is cut.  ``JpegUnsupported`` (a FrcnnError) with
    the reason for a file outside the supported set (include/ext/frcnn_hip_jpeg_dec.h): the caller decodes it on the host.  A pure host
    call: needs the built library, no GPU."""
    return JPEG_DECODER.plan(data)


def jpeg_dec_workspace_bytes(plan):
    """Bytes of device workspace ``jpeg_decode_u8`` needs for ``plan`` (frcnn_jpeg_dec_workspace_bytes)."""
    return JPEG_DECODER.workspace_bytes(plan)


def jpeg_decode_u8(file, plan=None, bgr=False, out=None, status=None, workspace=None):
    """Decode a baseline .jpg file on the device (frcnn_jpeg_decode_u8): ``file`` is its bytes, or a uint8 device tensor that holds them
    (then ``plan`` = jpeg_dec_plan(bytes) is required) -> (out, status): ``out`` an (h, w, 3) uint8 device tensor, R,G,B per pixel or
    (``bgr``) B,G,R, the pixels libjpeg's default decoder gives; ``status`` int32 [1], 0 for a sound file, _lib.JPEG_DEC_* bits ORed in
    otherwise (sticky: a status tensor passed in is not cleared; ``out`` is undefined then).  What is not passed (``workspace`` included) is
    allocated.  The device-tensor form never synchronises: the caller reads ``status`` where it synchronises anyway.  The bytes form is a
    convenience: its upload is a pageable copy, which blocks the host.  ``JpegUnsupported`` for a file outside the supported set."""
    _require_gpu()
    if isinstance(file, (bytes, bytearray, memoryview)):
        data = bytes(file)
        if plan is None:
            plan = jpeg_dec_plan(data)
        file = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    if not (isinstance(file, torch.Tensor) and file.is_cuda and file.dtype == torch.uint8 and file.dim() == 1 and file.is_contiguous()):
        raise _lib.FrcnnError("jpeg_decode_u8: file must be bytes or a contiguous 1-d uint8 device tensor")
    if not isinstance(plan, _lib.JpegDecPlan):
        raise _lib.FrcnnError("jpeg_decode_u8: a device tensor needs the plan of its bytes (jpeg_dec_plan)")
    if file.numel() < plan.file_len:
        raise _lib.FrcnnError(f"jpeg_decode_u8: file of {file.numel()} bytes, the plan was made of {plan.file_len}")
    need = jpeg_dec_workspace_bytes(plan)
    h, w = int(plan.h), int(plan.w)
    if out is None:
        out = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
    if workspace is None:
        workspace = _ws(need)
    for name, t, dt in (("out", out, torch.uint8), ("status", status, torch.int32), ("workspace", workspace, torch.uint8)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise _lib.FrcnnError(f"jpeg_decode_u8: {name} must be a contiguous {dt} device tensor")
    if workspace.numel() < need:
        raise _lib.FrcnnError(f"jpeg_decode_u8: workspace of {workspace.numel()} bytes, {need} needed")
    _lib.call("frcnn_jpeg_decode_u8", _p(file), ctypes.byref(plan), 1 if bgr else 0, _p(out), out.numel(), _p(status), _p(workspace),
              _stream())
    return out, status


def jpeg_dec_batch_layout(plans):
    """Workspace regions for a batch of plans laid back to back (frcnn_jpeg_dec_batch_layout) -> (ws_off, total): the byte offset of
    every plan's region (16-byte aligned, each ``jpeg_dec_workspace_bytes(plan)`` long) and the bytes of workspace the batch needs.  A
    pure host call."""
    return JPEG_DECODER.layout(plans)


def jpeg_batch_items(plans, file_off, out_off, ws_off):
    """The item table of a batch (``_lib.JpegDecBatchItem`` x n, a ctypes array: ``bytes(table)`` is what goes to the device)."""
    return JPEG_DECODER.items(plans, file_off, out_off, ws_off)


def jpeg_decode_batch_u8(files, items, out, bgr=False, status=None, workspace=None, items_dev=None):
    """Decode the baseline .jpg files of a batch on the device in ONE set of four launches (frcnn_jpeg_decode_batch_u8): ``files`` a 1-d
    uint8 device tensor that holds every file's bytes, ``items`` the table (``jpeg_batch_items``: per file its plan, where its bytes lie
    in ``files``, where its (h, w, 3) frame goes in ``out`` and where its region lies in ``workspace``), ``out`` a 1-d uint8 device
    tensor -> status: int32 [n], per file 0 or _lib.JPEG_DEC_* bits ORed in (sticky: a tensor passed in is not cleared).  ``items_dev``:
    a device tensor that already holds ``bytes(items)`` (uploaded by the caller on the current stream); None: uploaded here, a pageable
    copy, which blocks the host.  ``status`` and ``workspace`` are allocated when not passed.  Never synchronises otherwise."""
    return JPEG_DECODER.decode(files, items, out, bgr, status, workspace, items_dev)


# ---- the progressive JPEG decoder (include/ext/frcnn_hip_jpeg_dec_full.h, csrc/jpeg_dec_full.hip)
def jpeg_dec_full_plan(data):
    """``jpeg_dec_plan`` for a PROGRESSIVE .jpg file (frcnn_jpeg_dec_full_plan) -> a ``_lib.JpegDecFullPlan``: the frame fields of the
    baseline plan (``plan.frame``) and the scan table.  ``JpegUnsupported`` with the reason for a file outside ITS supported set: a
    baseline file (``jpeg_dec_plan``'s), an illegal or incomplete scan script, arithmetic coding, a cut file, ...  A pure host call."""
    return JPEG_FULL_DECODER.plan(data)


def jpeg_dec_full_workspace_bytes(plan):
    """Bytes of device workspace a file of ``plan`` needs (frcnn_jpeg_dec_full_workspace_bytes)."""
    return JPEG_FULL_DECODER.workspace_bytes(plan)


def jpeg_dec_full_batch_layout(plans):
    """Workspace regions for a batch of plans laid back to back (frcnn_jpeg_dec_full_batch_layout) -> (ws_off, total).  A pure host call."""
    return JPEG_FULL_DECODER.layout(plans)


def jpeg_full_batch_items(plans, file_off, out_off, ws_off):
    """The item table of a batch (``_lib.JpegDecFullBatchItem`` x n, a ctypes array: ``bytes(table)`` is what goes to the device);
    ``file_off``: where each WHOLE file lies."""
    return JPEG_FULL_DECODER.items(plans, file_off, out_off, ws_off)


def jpeg_decode_full_batch_u8(files, items, out, bgr=False, status=None, workspace=None, items_dev=None):
    """``jpeg_decode_batch_u8`` for progressive files, FOUR launches whatever the files' scan scripts are
    (frcnn_jpeg_decode_full_batch_u8): ``items`` the table (``jpeg_full_batch_items``) -> status: int32 [n], per file 0 or
    _lib.JPEG_DEC_FULL_* bits ORed in (sticky).  ``items_dev``, ``status`` and ``workspace`` as there."""
    return JPEG_FULL_DECODER.decode(files, items, out, bgr, status, workspace, items_dev)


def jpeg_decode_full_u8(file_bytes, bgr=False):
    """One progressive .jpg file's bytes decoded on the device: the eager convenience (a batch of one; pageable uploads, one
    synchronisation) -> an (h, w, 3) uint8 device tensor, numpy.asarray(PIL.Image.open(f).convert("RGB")) byte for byte, or its channel
    reverse with ``bgr``.  ``JpegUnsupported`` for a file outside the supported set, ``FrcnnError`` with the status word for a damaged
    one."""
    return JPEG_FULL_DECODER.decode_one(file_bytes, bgr)


# ---- YUV4MPEG2 frames (include/ext/frcnn_hip_y4m.h, csrc/y4m.hip)
def y4m_frame_bytes(h, w, chroma="420jpeg"):
    """Bytes of one frame's planes [Y | Cb | Cr] in chroma mode ``chroma`` ("420jpeg", "420mpeg2", "422", "444", "mono")."""
    return _y4m.frame_bytes(h, w, chroma)


def y4m_plan(h, w, chroma="420jpeg", range="limited", tags=None):       # noqa: A002 -- the format's own word
    """A ``_lib.Y4mPlan`` without a header: frames of (h, w) in ``chroma`` and ``range`` ("limited" / "full")."""
    return _y4m.make_plan(h, w, chroma, range, tags)


def y4m_batch_items(plans, file_off, out_off):
    """The item table of a batch (``_lib.Y4mBatchItem`` x n, a ctypes array: ``bytes(table)`` is what goes to the device)."""
    return Y4M_DECODER.items(plans, file_off, out_off, [0] * len(plans))


def y4m_decode_batch_u8(files, items, out, bgr=False, items_dev=None):
    """Up to 64 y4m frames, of any mix of sizes, chroma modes and ranges, to interleaved RGB in ONE launch
    (frcnn_y4m_decode_batch_u8): ``files`` a 1-d uint8 device tensor that holds the frames' planes, ``items`` the table
    (``y4m_batch_items``: per frame its plan, where its bytes lie in ``files`` and where its (h, w, 3) frame goes in ``out``), ``out``
    a 1-d uint8 device tensor.  ``items_dev``: a device tensor that already holds ``bytes(items)``; None: uploaded here (a pageable
    copy, which blocks the host).  Never synchronises otherwise; there is no status: a frame cannot be damaged."""
    Y4M_DECODER.decode(files, items, out, bgr, None, None, items_dev)
    return out


def y4m_decode_u8(frame_bytes_dev, plan, out=None, bgr=False):
    """One y4m frame on the device (frcnn_y4m_decode_u8, the batch of one): ``frame_bytes_dev`` a 1-d uint8 device tensor that holds
    the frame's planes (or ``bytes``: uploaded here), ``plan`` a ``_lib.Y4mPlan`` (``y4m_parse_header`` / ``y4m_plan``) -> ``out``, an
    (h, w, 3) uint8 device tensor, R,G,B per pixel or (``bgr``) B,G,R.  Never synchronises."""
    _require_gpu()
    if isinstance(frame_bytes_dev, (bytes, bytearray, memoryview)):
        frame_bytes_dev = torch.frombuffer(bytearray(frame_bytes_dev), dtype=torch.uint8).cuda()
    t = frame_bytes_dev
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 1 and t.is_contiguous()):
        raise _lib.FrcnnError("y4m_decode_u8: the frame must be bytes or a contiguous 1-d uint8 device tensor")
    if not isinstance(plan, _lib.Y4mPlan):
        raise _lib.FrcnnError("y4m_decode_u8: plan must be a Y4mPlan (y4m_parse_header, y4m_plan)")
    h, w = int(plan.h), int(plan.w)
    if out is None:
        out = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()):
        raise _lib.FrcnnError("y4m_decode_u8: out must be a contiguous uint8 device tensor")
    _lib.call("frcnn_y4m_decode_u8", _p(t) if t.numel() else None, t.numel(), ctypes.byref(plan), 1 if bgr else 0, _p(out), out.numel(),
              _stream())
    return out


def y4m_encode_frames_u8(frames, frame_stride, n, h, w, chroma="420jpeg", range="limited", bgr=False, out=None):     # noqa: A002
    """``n`` interleaved (h, w, 3) frames that lie ``frame_stride`` bytes apart in the uint8 device tensor ``frames`` -> ``out``, a
    uint8 device tensor [n][>= y4m_frame_bytes(h, w, chroma)]: per frame the record [Y | Cb | Cr], in ONE launch
    (frcnn_y4m_encode_u8).  ``chroma`` "420jpeg" or "444".  Never synchronises: capturable with fixed buffers."""
    _require_gpu()
    if chroma not in _lib.Y4M_OUT_CHROMAS or range not in _lib.Y4M_RANGES:
        raise _lib.FrcnnError("y4m_encode_u8: chroma=%r (%s), range=%r (%s)" % (chroma, ", ".join(_lib.Y4M_OUT_CHROMAS), range,
                                                                               ", ".join(_lib.Y4M_RANGES)))
    n, h, w = int(n), int(h), int(w)
    record = _y4m.frame_bytes(h, w, chroma)
    if out is None:
        out = torch.empty((n, record), dtype=torch.uint8, device="cuda")
    for name, t in (("frames", frames), ("out", out)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
            raise _lib.FrcnnError(f"y4m_encode_u8: {name} must be a contiguous uint8 device tensor")
    if out.dim() != 2 or out.shape[0] < n or n < 1 or frames.numel() < (n - 1) * int(frame_stride) + h * w * 3:
        raise _lib.FrcnnError("y4m_encode_u8: %d frames of stride %d in %d bytes, out %s" % (n, frame_stride, frames.numel(), tuple(out.shape)))
    _lib.call("frcnn_y4m_encode_u8", _p(frames), int(frame_stride), n, h, w, 1 if bgr else 0, _lib.Y4M_CHROMAS[chroma],
              _lib.Y4M_RANGES[range], _p(out), int(out.shape[1]), out.numel(), _stream())
    return out


def y4m_encode_u8(frame_dev, chroma="420jpeg", range="limited", bgr=False, out=None):       # noqa: A002
    """An (h, w, 3) uint8 device frame, R,G,B per pixel or (``bgr``) B,G,R -> its y4m record [Y | Cb | Cr] as a 1-d uint8 device tensor
    of y4m_frame_bytes(h, w, chroma) bytes; an (n, h, w, 3) tensor -> [n][record], all frames in one launch."""
    if not (isinstance(frame_dev, torch.Tensor) and frame_dev.dim() in (3, 4) and frame_dev.shape[-1] == 3):
        raise _lib.FrcnnError("y4m_encode_u8: frame must be an (h, w, 3) or (n, h, w, 3) uint8 device tensor")
    single = frame_dev.dim() == 3
    n = 1 if single else int(frame_dev.shape[0])
    h, w = int(frame_dev.shape[-3]), int(frame_dev.shape[-2])
    res = y4m_encode_frames_u8(frame_dev, h * w * 3, n, h, w, chroma, range, bgr, out if out is None or out.dim() == 2 else out.view(1, -1))
    return res[0] if single else res


def png_dec_plan(data):
    """The host-side chunk parse of a .png file's bytes (frcnn_png_dec_plan) -> a ``_lib.PngDecPlan``: size, channels, where the IDATs
    lie, the bytes of the zlib stream and of what it inflates to; the CRC-32 of IHDR and of every IDAT is verified.  ``PngUnsupported``
    (a FrcnnError) with the reason for a file outside the supported set (include/ext/frcnn_hip_png_dec.h): the caller decodes it on the
    host.  A pure host call: needs the built library, no GPU."""
    return _PNG1.plan(data)


def png_dec_spans(data, plan):
    """[(offset, length)] of the IDAT payloads of the file ``plan`` was made of (frcnn_png_dec_spans), in file order."""
    return _PNG1.spans(data, plan)


def png_dec_stream(data, plan):
    """What goes to the device: the file's zlib stream, its IDAT payloads back to back (``plan.stream_len`` bytes)."""
    return _PNG1.stream(data, plan)


def png_dec_workspace_bytes(plan):
    """Bytes of device workspace a file of ``plan`` needs (frcnn_png_dec_workspace_bytes): its inflated bytes."""
    return _PNG1.workspace_bytes(plan)


def png_dec_batch_layout(plans):
    """Workspace regions for a batch of plans laid back to back (frcnn_png_dec_batch_layout) -> (ws_off, total).  A pure host call."""
    return _PNG1.layout(plans)


def png_batch_items(plans, file_off, out_off, ws_off):
    """The item table of a batch (``_lib.PngDecBatchItem`` x n, a ctypes array: ``bytes(table)`` is what goes to the device);
    ``file_off``: where each file's staged zlib stream (``png_dec_stream``) lies."""
    return _PNG1.items(plans, file_off, out_off, ws_off)


def png_decode_batch_u8(files, items, out, bgr=False, status=None, workspace=None, items_dev=None):
    """Decode the .png files of a batch on the device in TWO launches (frcnn_png_decode_batch_u8): ``files`` a 1-d uint8 device tensor
    that holds every file's zlib stream, ``items`` the table (``png_batch_items``), ``out`` a 1-d uint8 device tensor -> status: int32
    [n], per file 0 or _lib.PNG_DEC_* bits ORed in (sticky: a tensor passed in is not cleared).  ``items_dev``: a device tensor that
    already holds ``bytes(items)``; None: uploaded here, a pageable copy, which blocks the host.  ``status`` and ``workspace`` are
    allocated when not passed.  Never synchronises otherwise."""
    return _PNG1.decode(files, items, out, bgr, status, workspace, items_dev)


def png_decode_u8(file_bytes, bgr=False):
    """One .png file's bytes decoded on the device: the eager convenience (a batch of one; pageable uploads, one synchronisation) -> an
    (h, w, 3) uint8 device tensor, numpy.asarray(PIL.Image.open(f).convert("RGB")) byte for byte, or its channel reverse with ``bgr``.
    ``PngUnsupported`` for a file outside the supported set, ``FrcnnError`` with the status word for a damaged one."""
    return _PNG1.decode_one(file_bytes, bgr)


# ---- the full-format PNG decoder (include/ext/frcnn_hip_png_dec_full.h, csrc/png_dec_full.hip): palette, 1/2/4/16-bit, grey + alpha, Adam7
def png_dec_full_plan(data):
    """``png_dec_plan`` for the full-format decoder (frcnn_png_dec_full_plan) -> a ``_lib.PngDecFullPlan``: size, colour type, bit depth,
    interlace, where the IDATs and the PLTE lie, the bytes of the zlib stream and of what it inflates to.  ``PngUnsupported`` with the
    reason for a file outside ITS supported set (16-bit grey, a palette file without a usable PLTE, a damaged container, ...).  A pure
    host call."""
    return _PNGF.plan(data)


def png_dec_full_spans(data, plan):
    """[(offset, length)] of the IDAT payloads of the file ``plan`` was made of (frcnn_png_dec_full_spans), in file order."""
    return _PNGF.spans(data, plan)


def png_dec_full_stream(data, plan):
    """What goes to the device -> (the file's zlib stream: its IDAT payloads back to back, ``plan.stream_len`` bytes; its palette: the
    PLTE entries zero-padded to PNG_DEC_FULL_PLTE_BYTES = 768 bytes for a colour-type-3 file, b"" for any other)."""
    return _PNGF.stream(data, plan), _PNGF.palette_of(data, plan)


def png_dec_full_of(plan):
    """The ``PngDecFullPlan`` that says what a revision-1 ``PngDecPlan`` says: depth 8, no interlace, no palette."""
    full = _lib.PngDecFullPlan()
    full.h, full.w, full.colour_type, full.bit_depth, full.interlace = plan.h, plan.w, {1: 0, 3: 2, 4: 6}[int(plan.channels)], 8, 0
    full.file_len, full.idat_off, full.idat_count = plan.file_len, plan.idat_off, plan.idat_count
    full.stream_len, full.inflated_len = plan.stream_len, plan.inflated_len
    return full


def png_dec_full_workspace_bytes(plan):
    """Bytes of device workspace a file of ``plan`` needs (frcnn_png_dec_full_workspace_bytes): its inflated bytes."""
    return _PNGF.workspace_bytes(plan)


def png_dec_full_batch_layout(plans):
    """Workspace regions for a batch of plans laid back to back (frcnn_png_dec_full_batch_layout) -> (ws_off, total).  A pure host call."""
    return _PNGF.layout(plans)


def png_full_batch_items(plans, file_off, out_off, ws_off, plte_off):
    """The item table of a batch (``_lib.PngDecFullBatchItem`` x n, a ctypes array: ``bytes(table)`` is what goes to the device);
    ``file_off`` / ``plte_off``: where each file's staged zlib stream and its 768 palette bytes (``png_dec_full_stream``) lie; the
    ``plte_off`` of a file that is not colour type 3 is not looked at."""
    return _PNGF.items(plans, file_off, out_off, ws_off, plte_off)


def png_decode_full_batch_u8(files, items, out, bgr=False, status=None, workspace=None, items_dev=None):
    """``png_decode_batch_u8`` for the full-format decoder, THREE launches (frcnn_png_decode_full_batch_u8): ``files`` holds every file's
    zlib stream and every palette file's 768 palette bytes, ``items`` the table (``png_full_batch_items``) -> status: int32 [n], per file
    0 or _lib.PNG_DEC_* bits ORed in (sticky).  ``items_dev``, ``status`` and ``workspace`` as there."""
    return _PNGF.decode(files, items, out, bgr, status, workspace, items_dev)


def png_decode_full_u8(file_bytes, bgr=False):
    """``png_decode_u8`` through the full-format decoder: palette, 1/2/4/16-bit, grey + alpha and Adam7 files too."""
    return _PNGF.decode_one(file_bytes, bgr)


def split_detections(packed, rows=None):
    """Views (n_dets, det_bbox, det_cls, det_prob, det_roi) into a `det_packed` buffer (device tensor or its host copy)."""
    rows = (packed.numel() - 4) // 7 if rows is None else rows
    return (packed[0:1], packed[4:4 + 4 * rows].view(rows, 4), packed[4 + 4 * rows:4 + 5 * rows],
            packed[4 + 5 * rows:4 + 6 * rows].view(torch.float32), packed[4 + 6 * rows:4 + 7 * rows])


# ----------------------------------------------------------------------------- conv backward
_DESC_CACHE = {}


def _conv_desc(x_shape, kh, kw, cout, stride, padding, act=0, layout=0, tile=0):
    """frcnn_conv_desc of a launch.  Descriptors are CACHED by their defining tuple and shared between calls (a training step
    builds ~90 of them from the same few dozen shapes; constructing the 17-field ctypes structure and asking the library for
    its workspace size cost ~4 us per launch of a host path that bounds the mixed-precision step): callers must not write
    to the returned object.  ``d._ws`` memoises the workspace-size queries made with it."""
    key = (x_shape, kh, kw, cout, stride, padding, act, layout, tile)
    d = _DESC_CACHE.get(key)
    if d is not None:
        return d
    if layout:
        h, w, n, cin = x_shape
    else:
        n, h, w, cin = x_shape
    if padding == "same":
        ho, pt = same_pad(h, kh, stride)
        wo, pl = same_pad(w, kw, stride)
    else:
        ho, wo, pt, pl = valid_out(h, kh, stride), valid_out(w, kw, stride), 0, 0
    d = _lib.ConvDesc(n=n, h=h, w=w, cin=cin, cout=cout, kh=kh, kw=kw, stride=stride, pad_top=pt, pad_left=pl,
                      ho=ho, wo=wo, act=act, ldy=0, ldres=0, tile=tile, layout=layout)
    d._ws = {}
    if len(_DESC_CACHE) > 4096:
        _DESC_CACHE.clear()
    _DESC_CACHE[key] = d
    return d


def _ws_need(d, query):
    """Workspace bytes of descriptor ``d`` under the library query ``query`` (memoised on cached descriptors)."""
    memo = getattr(d, "_ws", None)
    if memo is None:
        return getattr(_lib.load(), query)(ctypes.byref(d))
    need = memo.get(query)
    if need is None:
        need = memo[query] = getattr(_lib.load(), query)(ctypes.byref(d))
    return need


class PackedDgrad:
    """Filter of the input-gradient convolution of a stride-1 layer (transposed, flipped, with the
    forward epilogue scale folded in).  w_hwio: device or host (kh,kw,cin,cout); scale: (cout,) or None."""

    def __init__(self, w_hwio, scale=None):
        _require_gpu()
        w = _dev(w_hwio, torch.float32)
        self.kh, self.kw, cin, cout = (int(v) for v in w.shape)
        self.cin, self.cout = cout, cin                      # geometry of the dgrad convolution
        kp = _lib.load().frcnn_conv_packed_k(self.kh, self.kw, cout)
        self.w = torch.empty((cin, kp), dtype=torch.float32, device="cuda")
        sc = None if scale is None else _dev(scale, torch.float32)
        _lib.call("frcnn_pack_conv_weights_dgrad", _p(w), _p(sc), self.kh, self.kw, cin, cout, _p(self.w), _stream())
        self.scale = self.shift = None
        self._h3_spread_log2 = _channel_spread_log2(w if sc is None else w * sc, 3)   # (the transposed convolution reduces over the forward OUTPUT channels)

    x6_planes = PackedConv.x6_planes                         # the same [rows][packed k] f32 layout: the same three-plane form
    h3_planes = PackedConv.h3_planes                         # ... and the same header + two fp16 planes


def conv2d_dgrad(gy, pd, padding="valid", residual=None, mask=None, out=None):
    """Gradient w.r.t. the input of a stride-1 conv.  gy: (n,ho,wo,cout_fwd) gradient w.r.t. the layer's
    post-BN pre-activation output; residual: gradient arriving over an identity shortcut; mask: forward
    activation (n,h,w,cin_fwd) whose ReLU sits in front of this layer's input (None = no ReLU)."""
    _require_gpu()
    n, ho, wo, _ = gy.shape
    # forward 'same' (stride 1, odd kernel) pads (k-1)/2 on both sides -> so does the transposed conv
    pt = (pd.kh - 1) // 2 if padding == "same" else 0
    pl = (pd.kw - 1) // 2 if padding == "same" else 0
    assert padding == "same" or (pd.kh == 1 and pd.kw == 1), "dgrad supports 1x1 valid and odd 'same' kernels"
    if out is None:
        out = torch.empty((n, ho, wo, pd.cout), dtype=torch.float32, device="cuda")
    d = _conv_desc((n, ho, wo, pd.cin), pd.kh, pd.kw, pd.cout, 1, padding, 0, 0, 0)      # (see conv2d_dgrad_bf16)
    assert (d.pad_top, d.pad_left, d.ho, d.wo) == (pt, pl, ho, wo)
    gy = gy.contiguous()
    eng = _split_engine(d, pd, 0)                               # the split engines' policy, as for a forward launch of this geometry
    if eng == "x6":
        ws = _split_k_ws(_ws_need(d, "frcnn_conv2d_x6_workspace_bytes"))
        _lib.call("frcnn_conv2d_fwd_x6", ctypes.byref(d), _p(gy), _p(pd.x6_planes()), None, None, _p(residual), _p(mask), _p(out),
                  _p(ws), ws.numel() if ws is not None else 0, _stream())
        return out
    if eng == "h3":                                             # the gradient's magnitude record: its producer's (the dgrad launch behind it) or measured
        ws = _split_k_ws(_ws_need(d, "frcnn_conv2d_h3_workspace_bytes"))
        ya, ga = _amax_new(), amax_of(gy)
        _lib.call("frcnn_conv2d_fwd_h3", ctypes.byref(d), _p(gy), _p(ga), _p(pd.h3_planes()), None, None, _p(residual), _p(mask), _p(out), _p(ya),
                  _p(ws), ws.numel() if ws is not None else 0, _stream())
        out._amax = ya                                          # (residual and mask are applied before the epilogue takes the maximum)
        return out
    ya = _amax_new(optional=True) if (_tracking() and pd.cout >= 32) else None
    _conv_launch(d, gy, pd.w, None, None, residual, mask, out, ya)
    if ya is not None or getattr(out, "_amax", None) is not None:
        out._amax = ya
    return out


# Weight gradients of f32 layers: "native" = v_mfma_f32_32x32x2_f32; "bf16x6" = both operands split exactly into three bf16 pieces
# inside the kernel, six partial products on the bf16 matrix cores (conv_wgrad.hip wgrad_body_x6_big; layers with cin, cout >= 128,
# the others stay native).  Same slabs and fixed-order reduction: runs are bitwise reproducible either way, the two engines agree
# to f32 rounding.  The library default stays "native"; train.py opts in.
WGRAD_ENGINE = os.environ.get("FRCNN_WGRAD_ENGINE", "native")


def _wgrad_tile(dtype):
    return 71 if WGRAD_ENGINE == "bf16x6" and dtype == torch.float32 else 0


def conv2d_wgrad(x, g, kh, kw, stride=1, padding="valid", scale=None, dw=None, dbias=None, want_bias=True):
    """-> (dw (kh,kw,cin,cout), dbias (cout,) or None); g: (n,ho,wo,cout)."""
    _require_gpu()
    cout = g.shape[-1]
    d = _conv_desc(tuple(x.shape), kh, kw, cout, stride, padding, tile=_wgrad_tile(x.dtype))
    assert (d.ho, d.wo) == (g.shape[1], g.shape[2])
    if dw is None:
        dw = torch.empty((kh, kw, x.shape[-1], cout), dtype=torch.float32, device="cuda")
    if dbias is None and want_bias:
        dbias = torch.empty(cout, dtype=torch.float32, device="cuda")
    ws = _ws(_lib.load().frcnn_conv2d_wgrad_workspace_bytes(ctypes.byref(d)))
    _lib.call("frcnn_conv2d_wgrad", ctypes.byref(d), _p(x.contiguous()), _p(g.contiguous()), _p(scale), _p(dw), _p(dbias if want_bias else None),
              _p(ws), ws.numel(), _stream())
    return dw, (dbias if want_bias else None)


def conv2d_wgrad_batch(jobs):
    """Weight gradients of many layers in one go (frcnn_conv2d_wgrad_batch).  jobs: list of
    (x, g, kh, kw, stride, padding, scale or None, dw) -- x / g both f32 or both bf16, dw an f32 (kh,kw,cin,cout) tensor the
    result is written into.  Bit-identical to conv2d_wgrad / conv2d_wgrad_bf16 per layer (without the bias gradient)."""
    _require_gpu()
    if not jobs:
        return
    arr = (_lib.WgradJob * len(jobs))()
    keep = []
    for j, (x, g, kh, kw, stride, padding, scale, dw) in zip(arr, jobs):
        assert x.dtype == g.dtype and x.dtype in (torch.float32, torch.bfloat16) and dw.dtype == torch.float32 and dw.is_contiguous()
        x, g = x.contiguous(), g.contiguous()
        keep.append((x, g))
        d = _conv_desc(tuple(x.shape), kh, kw, g.shape[-1], stride, padding, tile=_wgrad_tile(x.dtype))
        assert (d.ho, d.wo) == (g.shape[1], g.shape[2]) and tuple(dw.shape[-4:]) == (kh, kw, x.shape[-1], g.shape[-1])
        j.d = d
        j.x, j.g, j.dw = x.data_ptr(), g.data_ptr(), dw.data_ptr()
        j.scale = None if scale is None else scale.data_ptr()
        j.in_bf16 = 1 if x.dtype == torch.bfloat16 else 0
    ws = _ws(_lib.load().frcnn_conv2d_wgrad_batch_workspace_bytes(arr, len(jobs)))
    _lib.call("frcnn_conv2d_wgrad_batch", arr, len(jobs), _p(ws), ws.numel(), _stream())
    return ws, keep                                              # (a capturing caller keeps the launch's buffers from being recycled)


# ----------------------------------------------------------------------------- bf16 conv path
class PackedConvBf16:
    """bf16-packed filter + f32 epilogue scale/shift (configs[3]: bf16 conv)."""

    def __init__(self, w_hwio, scale=None, shift=None):
        _require_gpu()
        w = _dev(w_hwio, torch.float32)
        self.kh, self.kw, self.cin, self.cout = (int(v) for v in w.shape)
        self.w = torch.empty((self.cout, self.kh * self.kw * self.cin), dtype=torch.bfloat16, device="cuda")
        _lib.call("frcnn_pack_conv_weights_bf16", _p(w), self.kh, self.kw, self.cin, self.cout, _p(self.w), _stream())
        self.scale = None if scale is None else _dev(scale, torch.float32)
        self.shift = None if shift is None else _dev(shift, torch.float32)


class PackedDgradBf16:
    """bf16 filter of the input-gradient convolution of a stride-1 layer (PackedDgrad's bf16 twin; cout % 64 == 0).
    Filled by frcnn_refresh_packed_bf16."""

    def __init__(self, w_hwio, scale=None):
        _require_gpu()
        w = _dev(w_hwio, torch.float32)
        self.kh, self.kw, cin, cout = (int(v) for v in w.shape)
        self.cin, self.cout = cout, cin                      # geometry of the dgrad convolution
        self.w = torch.empty((cin, self.kh * self.kw * cout), dtype=torch.bfloat16, device="cuda")
        self.scale = self.shift = None
        sc = None if scale is None else _dev(scale, torch.float32)
        job = _lib.PackJob(w_hwio=w.data_ptr(), packed=None, packed_dgrad=self.w.data_ptr(), bias=None,
                           scale=None if sc is None else sc.data_ptr(), shift_const=None, shift=None,
                           kh=self.kh, kw=self.kw, cin=cin, cout=cout)
        _lib.call("frcnn_refresh_packed_bf16", ctypes.byref(job), 1, _stream())
        torch.cuda.current_stream().synchronize()            # w / sc may be temporaries


def conv2d_dgrad_bf16(gy, pd, padding="valid", residual=None, mask=None):
    """bf16 twin of conv2d_dgrad: gy (n,ho,wo,cout_fwd) bf16 -> gradient w.r.t. the layer input, bf16."""
    _require_gpu()
    assert gy.dtype == torch.bfloat16
    n, ho, wo, _ = gy.shape
    pt = (pd.kh - 1) // 2 if padding == "same" else 0
    pl = (pd.kw - 1) // 2 if padding == "same" else 0
    assert padding == "same" or (pd.kh == 1 and pd.kw == 1), "dgrad supports 1x1 valid and odd 'same' kernels"
    out = torch.empty((n, ho, wo, pd.cout), dtype=torch.bfloat16, device="cuda")
    # (stride 1 with 'same' padding of an odd kernel, or 1x1 'valid': the forward descriptor of that geometry IS the dgrad one)
    d = _conv_desc((n, ho, wo, pd.cin), pd.kh, pd.kw, pd.cout, 1, padding, 0, 0, AUTO_TILE)
    assert (d.pad_top, d.pad_left, d.ho, d.wo) == (pt, pl, ho, wo)
    ws = _split_k_ws(_ws_need(d, "frcnn_conv2d_workspace_bytes_bf16"))
    _lib.call("frcnn_conv2d_fwd_bf16_masked", ctypes.byref(d), _p(gy.contiguous()), _p(pd.w), None, None, _p(residual), _p(mask), _p(out), 0,
              _p(ws), ws.numel() if ws is not None else 0, _stream())
    return out


def conv2d_wgrad_bf16(x, g, kh, kw, stride=1, padding="valid", scale=None, dw=None, dbias=None, want_bias=True):
    """bf16 activations x (n,h,w,cin) and gradients g (n,ho,wo,cout) -> f32 (dw (kh,kw,cin,cout), dbias or None)."""
    _require_gpu()
    assert x.dtype == torch.bfloat16 and g.dtype == torch.bfloat16
    cout = g.shape[-1]
    d = _conv_desc(tuple(x.shape), kh, kw, cout, stride, padding)
    assert (d.ho, d.wo) == (g.shape[1], g.shape[2])
    if dw is None:
        dw = torch.empty((kh, kw, x.shape[-1], cout), dtype=torch.float32, device="cuda")
    if dbias is None and want_bias:
        dbias = torch.empty(cout, dtype=torch.float32, device="cuda")
    ws = _ws(_lib.load().frcnn_conv2d_wgrad_workspace_bytes(ctypes.byref(d)))
    _lib.call("frcnn_conv2d_wgrad_bf16", ctypes.byref(d), _p(x.contiguous()), _p(g.contiguous()), _p(scale), _p(dw), _p(dbias if want_bias else None),
              _p(ws), ws.numel(), _stream())
    return dw, (dbias if want_bias else None)


def cast_f32(x):
    """bf16 device tensor -> f32."""
    _require_gpu()
    assert x.dtype == torch.bfloat16
    out = torch.empty(x.shape, dtype=torch.float32, device="cuda")
    _lib.call("frcnn_cast_bf16_to_f32", _p(x.contiguous()), x.numel(), _p(out), _stream())
    return out


def roi_crop_resize_bwd_bf16(dout, rois, rows, cols):
    _require_gpu()
    n, pool, _, C = dout.shape
    dfeat = torch.empty((rows, cols, C), dtype=torch.float32, device="cuda")
    _lib.call("frcnn_roi_crop_resize_bwd_bf16", _p(dout.contiguous()), rows, cols, C, _p(rois.reshape(-1, 4).contiguous()), n, pool, _p(dfeat), _stream())
    return dfeat


def conv2d_bf16(x, pc, stride=1, padding="valid", act=None, residual=None, out_f32=False, tile=0, layout=0):
    """x: (n,h,w,cin) bf16 NHWC -> (n,ho,wo,cout) bf16 (or f32 when out_f32); layout=1: (h,w,n,cin) -> (ho,wo,n,cout)."""
    _require_gpu()
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and x.shape[-1] == pc.cin
    d = _conv_desc(tuple(x.shape), pc.kh, pc.kw, pc.cout, stride, padding, ACT[act], layout, tile or AUTO_TILE)
    oshape = (d.ho, d.wo, d.n, pc.cout) if layout else (d.n, d.ho, d.wo, pc.cout)
    out = torch.empty(oshape, dtype=torch.float32 if out_f32 else torch.bfloat16, device="cuda")
    if residual is not None:
        assert residual.dtype == torch.bfloat16 and residual.shape == out.shape and residual.is_contiguous()
    ws = _split_k_ws(_ws_need(d, "frcnn_conv2d_workspace_bytes_bf16"))
    args = (ctypes.byref(d), _p(x), _p(pc.w), _p(pc.scale), _p(pc.shift), _p(residual), _p(out), 1 if out_f32 else 0,
            _p(ws), ws.numel() if ws is not None else 0)
    _lib.call("frcnn_conv2d_fwd_bf16_ws", *args, _stream())
    _record_launch(lambda: "k_conv_igemm_bf16", _gemm_shape(d, pc, stride), "frcnn_conv2d_fwd_bf16_ws", args, (d, x, pc, residual, out, ws))
    return out


def cast_bf16(x):
    _require_gpu()
    out = torch.empty(x.shape, dtype=torch.bfloat16, device="cuda")
    _lib.call("frcnn_cast_f32_to_bf16", _p(x.contiguous()), x.numel(), _p(out), _stream())
    return out


def avgpool_bf16(x, k, layout=0):
    """(n,k,k,c) bf16 (or (k,k,n,c) with layout=1) -> (n,c) f32."""
    _require_gpu()
    n, c = (x.shape[2] if layout else x.shape[0]), x.shape[3]
    out = torch.empty((n, c), dtype=torch.float32, device="cuda")
    _lib.call("frcnn_avgpool_bf16_to_f32_ex", _p(x.contiguous()), n, k, c, layout, _p(out), _stream())
    return out


def roi_crop_resize_bf16(feat, rois, pool, fill=None, relu=False, layout=0):
    _require_gpu()
    feat = feat.reshape(feat.shape[-3], feat.shape[-2], feat.shape[-1]).contiguous()
    rows, cols, C = feat.shape
    rois = rois.reshape(-1, 4).to(torch.float32).contiguous()
    n = rois.shape[0]
    out = torch.empty((pool, pool, n, C) if layout else (n, pool, pool, C), dtype=torch.bfloat16, device="cuda")
    _lib.call("frcnn_roi_crop_resize_fwd_bf16_ex", _p(feat), rows, cols, C, _p(rois), n, pool, _p(fill), 1 if relu else 0, layout, _p(out), _stream())
    return out


def roi_crop_resize_bf16_batch(feat, rois, n_per_img, pool, fill=None, relu=False, layout=0):
    """RoiResizeConv for the RoIs of several images in one launch: feat (B,R,C,Cf) bf16, rois (B*n_per_img,4) f32 (image =
    row // n_per_img) -> (B*n,pool,pool,Cf) bf16, or (pool,pool,B*n,Cf) with layout=1."""
    _require_gpu()
    assert feat.dtype == torch.bfloat16 and feat.dim() == 4 and feat.is_contiguous()
    B, rows, cols, C = feat.shape
    rois = rois.reshape(-1, 4).to(torch.float32).contiguous()
    n = rois.shape[0]
    assert n == B * n_per_img
    out = torch.empty((pool, pool, n, C) if layout else (n, pool, pool, C), dtype=torch.bfloat16, device="cuda")
    _lib.call("frcnn_roi_crop_resize_fwd_bf16_batch", _p(feat), B, rows, cols, C, _p(rois), n_per_img, pool, _p(fill), 1 if relu else 0, layout, _p(out), _stream())
    return out


class PackedStemBf16:
    """The fused bf16 stem's parameters (frcnn_stem_bf16_fwd): conv1's 7x7x3x64 filter packed to bf16 [64][176] and the
    folded f32 scale / shift of bias + BatchNorm (+ Scale)."""

    def __init__(self, w_hwio, scale, shift):
        _require_gpu()
        w = _dev(w_hwio, torch.float32)
        assert tuple(w.shape) == (7, 7, 3, 64), "the fused stem is conv1 of the ResNets: 7x7x3 -> 64"
        self.w = torch.empty(_lib.load().frcnn_stem_bf16_packed_elems(), dtype=torch.bfloat16, device="cuda")
        _lib.call("frcnn_pack_stem_weights_bf16", _p(w), _p(self.w), _stream())
        self.scale, self.shift = _dev(scale, torch.float32), _dev(shift, torch.float32)
        torch.cuda.current_stream().synchronize()            # w may be a temporary


def stem_bf16(x, ps):
    """(n,H,W,3) f32 preprocessed images -> (n,Hp,Wp,64) bf16: conv1 + BN (+Scale) + ReLU + 3x3/2 max-pool, one launch."""
    _require_gpu()
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4 and x.shape[-1] == 3
    n, h, w, _ = x.shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    out = torch.empty((n, (ho - 3) // 2 + 1, (wo - 3) // 2 + 1, 64), dtype=torch.bfloat16, device="cuda")
    _lib.call("frcnn_stem_bf16_fwd", _p(x), n, h, w, _p(ps.w), _p(ps.scale), _p(ps.shift), _p(out), _stream())
    return out


class PackedStemH3:
    """The fused f32 stem's parameters (frcnn_stem_h3_fwd): conv1's 7x7x3x64 filter as a header + two fp16 planes [2][64][176] and the
    folded f32 scale / shift of bias + BatchNorm (+ Scale)."""

    def __init__(self, w_hwio, scale, shift):
        _require_gpu()
        w = _dev(w_hwio, torch.float32)
        assert tuple(w.shape) == (7, 7, 3, 64), "the fused stem is conv1 of the ResNets: 7x7x3 -> 64"
        self.w = torch.empty(_lib.load().frcnn_stem_h3_packed_bytes(), dtype=torch.uint8, device="cuda")
        _lib.call("frcnn_pack_stem_weights_h3", _p(w), _p(self.w), _stream())
        self.scale, self.shift = _dev(scale, torch.float32), _dev(shift, torch.float32)
        torch.cuda.current_stream().synchronize()            # w may be a temporary


def stem_h3(x, ps):
    """(n,H,W,3) f32 preprocessed images -> (n,Hp,Wp,64) f32: conv1 + BN (+Scale) + ReLU + 3x3/2 max-pool in ONE f16x3 launch; the
    result carries its magnitude record."""
    _require_gpu()
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4 and x.shape[-1] == 3
    n, h, w, _ = x.shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    out = torch.empty((n, (ho - 3) // 2 + 1, (wo - 3) // 2 + 1, 64), dtype=torch.float32, device="cuda")
    ya, xa = _amax_new(), amax_of(x)
    args = (_p(x), _p(xa), n, h, w, _p(ps.w), _p(ps.scale), _p(ps.shift), _p(out), _p(ya))
    _lib.call("frcnn_stem_h3_fwd", *args, _stream())
    out._amax = ya
    _record_launch(lambda: "k_stem_h3", (n * ho * wo, 64, 147, 2), "frcnn_stem_h3_fwd", args, (x, ps, out, ya, xa))
    return out


class PackedVggConv1Bf16:
    """block1_conv1's parameters for frcnn_vgg_conv1_bf16_fwd (vgg.py:96-97): the 3x3x3x64 filter packed to bf16 as the four matrix
    fragments the kernel keeps in registers, and the f32 bias."""

    def __init__(self, w_hwio, bias):
        _require_gpu()
        w = _dev(w_hwio, torch.float32)
        assert tuple(w.shape) == (3, 3, 3, 64), "the conv1 kernel is block1_conv1 of VGG16: 3x3x3 -> 64"
        self.w = torch.empty(_lib.load().frcnn_vgg_conv1_bf16_packed_elems(), dtype=torch.bfloat16, device="cuda")
        _lib.call("frcnn_pack_vgg_conv1_weights_bf16", _p(w), _p(self.w), _stream())
        self.bias = _dev(bias, torch.float32)
        torch.cuda.current_stream().synchronize()            # w may be a temporary


def vgg_conv1_bf16(x, packed):
    """(n,H,W,3) f32 preprocessed images -> (n,H,W,64) bf16: block1_conv1 + bias + ReLU (SAME padding), one launch."""
    _require_gpu()
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4 and x.shape[-1] == 3
    n, h, w, _ = x.shape
    out = torch.empty((n, h, w, 64), dtype=torch.bfloat16, device="cuda")
    args = (_p(x), n, h, w, _p(packed.w), _p(packed.bias), _p(out))
    _lib.call("frcnn_vgg_conv1_bf16_fwd", *args, _stream())
    _record_launch(lambda: "k_vgg_conv1_bf16", (n * h * w, 64, 27, 1), "frcnn_vgg_conv1_bf16_fwd", args, (x, packed, out))
    return out


def pool2d_bf16(x, k, stride):
    """MaxPooling2D((k,k), strides=(stride,stride)), VALID, on a bf16 NHWC map (the library serves k = stride = 2, c % 8 == 0)."""
    _require_gpu()
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and x.dim() == 4
    n, h, w, c = x.shape
    out = torch.empty((n, valid_out(h, k, stride), valid_out(w, k, stride), c), dtype=torch.bfloat16, device="cuda")
    args = (_p(x), n, h, w, c, k, stride, _p(out))
    _lib.call("frcnn_pool2d_fwd_bf16", *args, _stream())
    _record_launch(lambda: "k_pool2_bf16", (out.numel() // c, c, k * k, 1), "frcnn_pool2d_fwd_bf16", args, (x, out))
    return out


def vgg_conv1_bf16_extents(x, packed, true_hw):
    """``vgg_conv1_bf16`` on canvases (frcnn_vgg_conv1_bf16_fwd_extents): x (n,hc,wc,3) f32, true_hw = device int32 (n,2), image i's true
    (rows, cols).  Inside the extent the map of the true-size image bit for bit, zero everywhere else."""
    _require_gpu()
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4 and x.shape[-1] == 3
    assert true_hw.dtype == torch.int32 and true_hw.is_cuda and true_hw.numel() >= 2 * x.shape[0]
    n, h, w, _ = x.shape
    out = torch.empty((n, h, w, 64), dtype=torch.bfloat16, device="cuda")
    args = (_p(x), n, h, w, _p(packed.w), _p(packed.bias), _p(true_hw), _p(out))
    _lib.call("frcnn_vgg_conv1_bf16_fwd_extents", *args, _stream())
    _record_launch(lambda: "k_vgg_conv1_bf16", (n * h * w, 64, 27, 1), "frcnn_vgg_conv1_bf16_fwd_extents", args, (x, packed, out, true_hw))
    return out


def pool2d_bf16_extents(x, true_hw):
    """``pool2d_bf16(x, 2, 2)`` on the bf16 tensors of a canvas pass (frcnn_pool2d_fwd_bf16_extents): see ``pool2d_extents``."""
    _require_gpu()
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and x.dim() == 4
    assert true_hw.dtype == torch.int32 and true_hw.is_cuda and true_hw.numel() >= 2 * x.shape[0]
    n, h, w, c = (int(v) for v in x.shape)
    out = torch.empty((n, h // 2, w // 2, c), dtype=torch.bfloat16, device="cuda")
    args = (_p(x), n, h, w, c, _p(true_hw), _p(out))
    _lib.call("frcnn_pool2d_fwd_bf16_extents", *args, _stream())
    _record_launch(lambda: "k_pool2_extents", (out.numel() // c, c, 4, 1), "frcnn_pool2d_fwd_bf16_extents", args, (x, out, true_hw))
    return out
