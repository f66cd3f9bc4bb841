"""Plain numpy / Python-loop reference of the post-process rule (DESIGN §8 "Post-process rule", include/ext/frcnn_hip_detect_post.h,
csrc/detect_post.hip): soft-NMS and box voting behind the rows of tests/detections_ref.py.  No torch, no GPU.

The rows scored, the arg-max, the threshold, the f64 decode and the class order are ``detections_ref``'s (``_rows``, ``n_scored``); a class
is then worked on alone over its valid rows in ranked order (score descending, row ascending) with their original f64 boxes.  Every sum
is a sequential Python loop over Python floats (IEEE f64), so the linear mode and the voting are exact sequences."""
import numpy as np

from tests import detections_ref as R

MODES = ("hard", "soft_linear", "soft_gaussian")
DEFAULT = ("hard", 0.5, 0.5, None, None)                     # mode, nms_thresh, sigma, min_score, vote_iou


def option(post):
    """(mode, nms_thresh, sigma, min_score, vote_iou) with the defaults filled in; a tuple (missing tail = defaults), a dict or None."""
    if post is None:
        post = ()
    if isinstance(post, dict):
        post = tuple(post.get(k) for k in ("mode", "nms_thresh", "sigma", "min_score", "vote_iou"))
    post = tuple(post) + (None,) * (5 - len(post))
    mode, nt, sigma = (DEFAULT[i] if post[i] is None else post[i] for i in range(3))
    assert mode in MODES
    return mode, float(nt), float(sigma), None if post[3] is None else float(post[3]), None if post[4] is None else float(post[4])


def iou(a, b):
    """det_suppresses' expression (csrc/detect.hip), +1 pixel convention, in f64."""
    area_a = (a[2] - a[0] + 1.0) * (a[3] - a[1] + 1.0)
    area_b = (b[2] - b[0] + 1.0) * (b[3] - b[1] + 1.0)
    w = max(0.0, min(a[2], b[2]) - max(a[0], b[0]) + 1.0)
    h = max(0.0, min(a[3], b[3]) - max(a[1], b[1]) + 1.0)
    inter = w * h
    return inter / (area_a + area_b - inter)


def _near(a, b, rel):
    return abs(a - b) <= rel * max(abs(a), abs(b))


def post_class(items, post, det_threshold, resize_ratio, found=None):
    """One class.  ``items``: [(row, f32 score, f64 box, moved)] in RANKED order -> [(row, f32 det_prob, [4 ints])] in pick order.
    ``found`` (a list) collects the decisions a one-ulp ``exp`` could flip (``unstable_post`` kinds b and c)."""
    mode, nt, sigma, min_score, vote = option(post)
    min_score = float(det_threshold) if min_score is None else min_score
    n = len(items)
    box = [[float(v) for v in it[2]] for it in items]
    s0 = [float(it[1]) for it in items]
    moved = [bool(it[3]) for it in items]
    any_moved = any(moved)
    s = list(s0)
    E = [0.0] * n
    left = list(range(n))                                     # not yet picked (hard: nor dropped), ascending rank
    picks = []
    while left:
        k = left[0]
        for j in left[1:]:
            if s[j] > s[k]:                                   # strict: the lower rank among equals
                k = j
        if found is not None and mode != "hard" and (mode == "soft_gaussian" or any_moved):
            others = [s[j] for j in left if j != k]
            if others:
                ru = max(others)
                if ru != s[k] and _near(ru, s[k], 1e-12):
                    found.append(("pick", items[k][0], s[k], ru))
            if s[k] != min_score and _near(s[k], min_score, 1e-12):
                found.append(("min_score", items[k][0], s[k]))
        if mode != "hard" and s[k] < min_score:
            break
        picks.append((k, np.float32(s[k]) if mode != "hard" else np.float32(items[k][1])))
        left.remove(k)
        keep = []
        for j in left:
            o = iou(box[k], box[j])
            if mode == "hard":
                if not (o <= nt):
                    continue
            elif mode == "soft_linear":
                if not (o <= nt):
                    s[j] = s[j] * (1.0 - o)
            else:
                E[j] = E[j] + o * o
                s[j] = s0[j] * float(np.exp(-(E[j] / sigma)))
            keep.append(j)
        left = keep
    out = []
    for k, prob in picks:
        b = box[k]
        if vote is not None:
            acc = [0.0, 0.0, 0.0, 0.0]
            ws = 0.0
            members_moved = False
            for j in range(n):                                # ranked order, every valid row of the class
                o = iou(box[k], box[j])
                if found is not None and (moved[k] or moved[j]) and abs(o - vote) < 1e-12:
                    found.append(("vote_iou", items[k][0], items[j][0]))
                if o >= vote:
                    for c in range(4):
                        acc[c] = acc[c] + s0[j] * box[j][c]
                    ws = ws + s0[j]
                    members_moved = members_moved or moved[j]
            if ws > 0.0:
                b = [acc[c] / ws for c in range(4)]
                if found is not None and members_moved:
                    for c in range(4):
                        q = b[c] / float(resize_ratio)
                        if abs(q - np.floor(q) - 0.5) < 1e-9:
                            found.append(("vote_round", items[k][0], c))
        out.append((items[k][0], prob, [int(round(v / float(resize_ratio))) for v in b]))
    return out


def _classes(case, roi_batch):
    batch = case["roi_batch"] if roi_batch is None else roi_batch
    ns = R.n_scored(case["n_live"], batch, len(case["cls"]))
    rows = R._rows(np.asarray(case["rois"], np.float32), np.asarray(case["cls"], np.float32), np.asarray(case["reg"], np.float32), ns,
                   case["bg"], case["thr"], case["stride"])
    by_cls = {}                                               # insertion order = first valid row
    for r, c, conf, box, moved in rows:
        by_cls.setdefault(c, []).append((r, conf, box, moved))
    for c in by_cls:
        by_cls[c].sort(key=lambda it: (-float(it[1]), it[0]))  # score descending, row ascending
    return by_cls, ns


def run(case, post=None, roi_batch=None, found=None):
    """A case of tests/detections_cases.py under ``post`` -> (cls int32[nd], prob float32[nd], bbox int64[nd, 4], roi int32[nd], n_scored),
    the shape of ``detections_ref.run``.  The case's own ``nms`` is NOT used: the threshold is the option's."""
    by_cls, ns = _classes(case, roi_batch)
    cls, prob, bbox, roi = [], [], [], []
    for c, items in by_cls.items():
        for r, p, b in post_class(items, post, case["thr"], case["ratio"], found):
            cls.append(c)
            prob.append(p)
            bbox.append(b)
            roi.append(r)
    return (np.array(cls, np.int32), np.array(prob, np.float32), np.array(bbox, np.int64).reshape(-1, 4), np.array(roi, np.int32), ns)


def unstable_post(case, post, roi_batch=None):
    """Decisions of a case under ``post`` that a one-ulp difference in ``exp`` could flip, as a list (empty = the outputs are determined,
    det_prob of the soft modes to the last f32 bit but one):
      (a) ``detections_ref.unstable``'s two kinds, with the option's nms_thresh as the threshold;
      (b) soft modes (the linear one: classes with a box decoded with non-zero tw / th only; the gaussian one: all): a pick whose
          runner-up score is not bitwise equal to it yet within relative 1e-12 of it, or a score within 1e-12 relative of min_score;
      (c) voting: a membership IoU within 1e-12 of vote_iou where either box was decoded with non-zero tw / th, and a voted coordinate
          whose v / ratio lies within 1e-9 of x.5 where any member was so decoded."""
    mode, nt, _, _, _ = option(post)
    found = list(R.unstable(dict(case, nms=nt), roi_batch))
    run(case, post, roi_batch, found)
    return found


# the parameter sets the GPU parity test runs on every case (tests/test_detections_post_gpu.py); tests/test_detections_post_ref_cpu.py
# holds the condition that none of them leaves an undetermined decision in any case
GPU_POSTS = {
    "hard": ("hard", 0.5, 0.5, None, None),
    "soft_linear": ("soft_linear", 0.3, 0.5, None, None),
    "soft_gaussian": ("soft_gaussian", 0.5, 0.5, None, None),
    "hard_vote": ("hard", 0.5, 0.5, None, 0.5),
    "soft_linear_vote": ("soft_linear", 0.3, 0.5, None, 0.5),
    # (a set of its own, not a replacement: no set above trips the condition; this one is here because every set above leaves min_score
    # to the threshold, and the explicit value takes another path through the bindings and the kernel's argument.  0.05: above most
    # cases' threshold of 0, so that it ends classes early, and under their scores' bulk, so that rows remain)
    "soft_linear_vote_min": ("soft_linear", 0.3, 0.5, 0.05, 0.5),
}


def gpu_post(name, case):
    """The parameter set ``name`` for a case: the plain hard set runs at the case's own NMS threshold, as the existing entry points do."""
    post = GPU_POSTS[name]
    return ("hard", case["nms"]) + post[2:] if name == "hard" else post
