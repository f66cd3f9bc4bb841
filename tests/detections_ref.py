"""Plain numpy reference of the detection post-process as this build defines it (frcnn_detections / frcnn_detections_dyn,
csrc/detect.hip): the loops of the reference's voc_dets.get_dets (voc_dets.py:51-88) restated row by row, no torch, no GPU.

What it adds to ``oracle.np_ref.detections`` (docs/DETECTIONS_PARITY.md):
  * the NMS visits a class's boxes by descending score and, on equal scores, ascending row index;
  * the scored row index of every detection is returned (``det_roi``);
  * the rows that are scored follow from ``n_live``, ``roi_batch`` and ``max_rows`` as the two entry points count them;
  * ``nms_thresh``, ``stride`` and ``bg_idx`` are arguments.
The dtype flow is the oracle's: ``transform_legacy``, the f64 threshold comparison, ``int(round(v / ratio))``."""
import numpy as np

from oracle.np_ref import BBREG_MULTIPLIERS, transform_legacy

DET_MAX = 512


def n_scored(n_live, roi_batch, max_rows):
    """Rows the post-process scores: the live rows, rounded up to whole batches when ``roi_batch`` > 0 (the reference's padded last
    batch, voc_dets.py:42-46), never more than the buffers hold.  ``roi_batch`` 0 is also the static entry."""
    n = int(n_live)
    if roi_batch > 0 and n > 0:
        n = -(-n // roi_batch) * roi_batch
    return max(0, min(n, int(max_rows), DET_MAX))


def _rows(rois, out_cls, out_reg, ns, bg_idx, det_threshold, stride):
    """voc_dets.py:51-70 over the scored rows -> [(row, class, f32 score, f64 box, box moved by an exp)] in row order."""
    C = out_cls.shape[1]
    out = []
    for r in range(ns):
        c = int(np.argmax(out_cls[r]))                       # first maximum
        conf = out_cls[r, c]
        if c == bg_idx or float(conf) < float(det_threshold):        # np.float32 against a Python float: f64 under numpy 1.13
            continue
        if c >= C - 1:
            # out_reg has C - 1 classes: the reference's slice is empty there and its unpacking raises
            raise ValueError("row %d: class %d wins and has no regression columns" % (r, c))
        t = out_reg[r, 4 * c:4 * c + 4] / BBREG_MULTIPLIERS
        p = transform_legacy(rois[r], t)
        box = [float(stride) * p[0], float(stride) * p[1], float(stride) * p[2], float(stride) * p[3]]
        out.append((r, c, conf, box, bool(np.float32(t[2]) != 0 or np.float32(t[3]) != 0)))
    return out


def _nms(boxes, probs, thresh):
    """det_util.py:209-256 with the build's order: greedy, +1 pixel convention, keep overlap <= thresh.  -> pick list."""
    x1, y1, x2, y2 = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
    area = (x2 - x1 + 1) * (y2 - y1 + 1)
    remaining = np.argsort(-probs, kind="stable")            # best first, lower row first among equals
    pick = []
    while len(remaining):
        i, rest = remaining[0], remaining[1:]
        pick.append(int(i))
        w = np.maximum(0, np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]) + 1)
        h = np.maximum(0, np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]) + 1)
        inter = w * h
        overlap = inter / (area[i] + area[rest] - inter)
        remaining = rest[overlap <= thresh]
    return pick


def detections(rois, out_cls, out_reg, n_live, bg_idx, resize_ratio, det_threshold=0.0, stride=16.0, nms_thresh=0.5,
               roi_batch=0, max_rows=None):
    """-> (cls int32[nd], prob float32[nd], bbox int64[nd, 4], roi int32[nd], n_scored).

    ``rois`` / ``out_cls`` / ``out_reg`` are the buffers as the device holds them (padded rows included, as frcnn_gather_rois lays
    them out); rows at and past ``n_scored`` are never read."""
    rois = np.asarray(rois, np.float32)
    out_cls = np.asarray(out_cls, np.float32)
    out_reg = np.asarray(out_reg, np.float32)
    ns = n_scored(n_live, roi_batch, len(out_cls) if max_rows is None else max_rows)
    by_cls = {}                                              # insertion order = first-seen order
    for r, c, conf, box, _ in _rows(rois, out_cls, out_reg, ns, bg_idx, det_threshold, stride):
        bb, pp, rr = by_cls.setdefault(c, ([], [], []))
        bb.append(box)
        pp.append(conf)
        rr.append(r)
    cls, prob, bbox, roi = [], [], [], []
    for c, (bb, pp, rr) in by_cls.items():
        bb = np.array(bb, np.float64)
        pp = np.array(pp, np.float32)
        for i in _nms(bb, pp, float(nms_thresh)):
            cls.append(c)
            prob.append(pp[i])
            bbox.append([int(round(v / float(resize_ratio))) for v in bb[i]])
            roi.append(rr[i])
    return (np.array(cls, np.int32), np.array(prob, np.float32), np.array(bbox, np.int64).reshape(-1, 4), np.array(roi, np.int32), ns)


def run(case, roi_batch=None):
    """``detections`` on a case of tests/detections_cases.py; ``roi_batch`` overrides the case's (0 = the static entry)."""
    return detections(case["rois"], case["cls"], case["reg"], case["n_live"], case["bg"], case["ratio"], case["thr"], case["stride"],
                      case["nms"], case["roi_batch"] if roi_batch is None else roi_batch, len(case["cls"]))


def has_ties(case, roi_batch=None):
    """True if two scored valid rows of one class share a score: ``np.argsort(probs)[::-1]`` of the oracle is undefined there."""
    batch = case["roi_batch"] if roi_batch is None else roi_batch
    ns = n_scored(case["n_live"], batch, len(case["cls"]))
    seen = set()
    for r, c, conf, _, _ in _rows(case["rois"], case["cls"], case["reg"], ns, case["bg"], case["thr"], case["stride"]):
        key = (c, np.float32(conf).tobytes())
        if key in seen:
            return True
        seen.add(key)
    return False


def unstable(case, roi_batch=None):
    """Decisions of a case that a one-ulp difference in ``exp`` could flip, as a list (empty = every output is determined):
      ("round", row, k)   coordinate k of a box decoded with a non-zero tw or th whose v / ratio lies within 1e-9 of x.5;
      ("iou", row, row)   two boxes of one class, at least one of them decoded with a non-zero tw or th, whose IoU lies
                          within 1e-12 of the NMS threshold.
    Boxes decoded from all-zero tw / th never pass through a transcendental: they are exact and are not listed."""
    batch = case["roi_batch"] if roi_batch is None else roi_batch
    ns = n_scored(case["n_live"], batch, len(case["cls"]))
    rows = _rows(np.asarray(case["rois"], np.float32), case["cls"], case["reg"], ns, case["bg"], case["thr"], case["stride"])
    found = []
    per_cls = {}
    for r, c, _, box, moved in rows:
        per_cls.setdefault(c, []).append((r, box, moved))
        if moved:
            for k, v in enumerate(box):
                q = v / float(case["ratio"])
                if abs(q - np.floor(q) - 0.5) < 1e-9:
                    found.append(("round", r, k))
    for c, items in per_cls.items():
        b = np.array([it[1] for it in items], np.float64)
        mv = np.array([it[2] for it in items])
        if not mv.any():
            continue
        area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
        w = np.maximum(0, np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]) + 1)
        h = np.maximum(0, np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]) + 1)
        inter = w * h
        iou = inter / (area[:, None] + area[None, :] - inter)
        near = (np.abs(iou - float(case["nms"])) < 1e-12) & (mv[:, None] | mv[None, :])
        for i, j in zip(*np.nonzero(np.triu(near, 1))):
            found.append(("iou", items[i][0], items[j][0]))
    return found
