"""Generated inputs of the detection post-process tests, shared by tests/test_detections_ref_cpu.py (which checks the
reference and the inputs) and tests/test_detections_gpu.py (which runs csrc/detect.hip on them).  numpy only, every case
from a fixed seed.

A case is a dict: ``rois`` f32 (rows, 4), ``cls`` f32 (rows, C), ``reg`` f32 (rows, 4 (C - 1)) as the device holds them,
``n_live``, ``roi_batch`` (0 = live rows only), ``bg``, ``thr`` (f64), ``ratio``, ``stride``, ``nms``, and ``name`` /
``phase`` (the part of k_detections the case is aimed at).  max_rows is ``len(cls)``: the bindings pass the buffers' rows.

Class C - 1 never wins a row unless it is the background: ``reg`` has no columns for it (the reference raises there)."""
import numpy as np

SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 320, 448, 511, 512)
DYN_LIVE = (0, 1, 63, 64, 65, 300, 449, 512)
ROUND_RATIOS = (2.0, 0.4)
NMS_EDGE_THRESHOLDS = (0.5, 0.3, 0.7)


def case(name, phase, rois, cls, reg, bg, thr=0.0, ratio=1.0, stride=1.0, nms=0.5, n_live=None, roi_batch=0):
    rois = np.ascontiguousarray(rois, np.float32).reshape(-1, 4)
    cls = np.ascontiguousarray(cls, np.float32)
    C = cls.shape[1]
    reg = np.zeros((len(cls), 4 * (C - 1)), np.float32) if reg is None else np.ascontiguousarray(reg, np.float32)
    assert len(rois) == len(cls) == len(reg) and reg.shape[1] == 4 * (C - 1) and 0 < len(cls) <= 512
    return {"name": name, "phase": phase, "rois": rois, "cls": cls, "reg": reg, "bg": int(bg), "thr": float(thr), "ratio": float(ratio),
            "stride": float(stride), "nms": float(nms), "n_live": len(cls) if n_live is None else int(n_live), "roi_batch": int(roi_batch)}


def onehot(classes, scores, C, low=0.0):
    """Row r: ``scores[r]`` at ``classes[r]``, ``low`` elsewhere."""
    out = np.full((len(classes), C), low, np.float32)
    out[np.arange(len(classes)), np.asarray(classes)] = np.asarray(scores, np.float32)
    return out


def descending(n, hi=0.99, lo=0.01):
    """n distinct f32 scores, strictly falling with the index."""
    s = np.linspace(hi, lo, n).astype(np.float32)
    assert n == 1 or (np.diff(s) < 0).all()
    return s


def random_rois(rs, n, span=60, frac=False):
    """The fuzz tool's RoIs: integer corners in [0, span), x2 > x1, y2 > y1; ``frac`` adds f32 fractions."""
    r = np.sort(rs.randint(0, span, (n, 2, 2)), axis=1).reshape(n, 4).astype(np.float32)       # (x1, y1, x2, y2)
    r[:, 2:] = np.maximum(r[:, 2:], r[:, :2] + 1)
    if frac:
        r += rs.rand(n, 4).astype(np.float32) * np.float32(0.75)
        r[:, 2:] = np.maximum(r[:, 2:], r[:, :2] + np.float32(0.25))
    return r


def random_probs(rs, n, C, never=()):
    """Softmax rows; the classes of ``never`` cannot win a row: their logit lies 0.5 to 2.5 under the row's best other one (so a row
    still has a score of its own where a single class is left to win)."""
    logits = (rs.randn(n, C) * 3).astype(np.float32)
    never = list(never)
    best = np.delete(logits, never, axis=1).max(1)
    for c in never:
        logits[:, c] = best - np.float32(0.5) - (rs.rand(n) * 2).astype(np.float32)
    p = np.exp(logits - logits.max(1, keepdims=True))
    return (p / p.sum(1, keepdims=True)).astype(np.float32)


def random_case(name, phase, seed, n, C, bg, reg_scale=0.5, frac=False, rows=None, **kw):
    """n random rows (boxes, deltas, classes); the background never wins, nor does class C - 1."""
    rs = np.random.RandomState(seed)
    rows = n if rows is None else rows
    never = sorted({bg, C - 1})
    if len(never) == C:                                       # C = 2 with background 0: nothing but the background can win
        never = [C - 1]
    return case(name, phase, random_rois(rs, rows, frac=frac), random_probs(rs, rows, C, never),
                rs.randn(rows, 4 * (C - 1)) * reg_scale, bg, **kw)


# ------------------------------------------------------------------ sizes: scan words, vmask, the cnt == 64 arm
def size_cases():
    out = []
    for i, n in enumerate(SIZES):
        out.append(random_case("size_%d_c21" % n, "scan words / vmask: nv = %d over 20 classes" % n, 100 + i, n, 21, 20,
                               stride=16.0, ratio=(1.6, 0.625)[i % 2]))
        # one class fills every word it reaches: the suppression matrix and the carried `removed` words are dense
        out.append(random_case("size_%d_c2" % n, "scan words / vmask: nv = %d in ONE class" % n, 200 + i, n, 2, 1,
                               stride=16.0, ratio=(0.625, 1.6)[i % 2]))
    return out


# ------------------------------------------------------------------ cross-word suppression (mask build + scan carry)
def chain_boxes(n):
    """10 x 10 pixel boxes stepping 2 along x: IoU(i, i + 1) = 8 / 12, IoU(i, i + 2) = 6 / 14."""
    i = np.arange(n, dtype=np.float32)
    return np.stack([2 * i, 0 * i, 2 * i + 9, 0 * i + 9], 1)


def disjoint_boxes(n):
    """10 x 10 pixel boxes on a 12-pixel grid right of x = 2000: no two overlap."""
    i = np.arange(n)
    x, y = 2000 + 12 * (i % 32), 12 * (i // 32)
    return np.stack([x, y, x + 9, y + 9], 1).astype(np.float32)


LONG_RANGE_COPIES = (63, 64, 65, 447, 448, 511)
KILLER_RANKS = tuple(64 * k + 5 for k in range(7))            # one kept row in each of words 0..6


def killer_victims(k):
    """Ranks of the copies of killer k: one in every later word, at a lane that moves with k."""
    return [64 * w + 10 + k for w in range(k + 1, 8)]


def cross_word_cases():
    n = 512
    one = onehot(np.zeros(n, int), descending(n), 2)
    out = [case("chain", "scan: a suppressed row must not suppress; `removed` carried through all 8 words", chain_boxes(n), one, None, 1)]
    b = disjoint_boxes(n)
    b[0] = (0, 0, 99, 99)
    for r in LONG_RANGE_COPIES:
        b[r] = b[0]
    out.append(case("long_range", "mask build + scan: rank 0 (word 0) suppresses copies in words 0, 1, 6 and 7", b, one, None, 1))
    b = disjoint_boxes(n)
    for k, r in enumerate(KILLER_RANKS):
        b[r] = (0, 200 * (k + 1), 99, 200 * (k + 1) + 99)
        for v in killer_victims(k):
            b[v] = b[r]
    out.append(case("late_killers", "scan: a row kept in word k sets `removed` bits in every later word, k = 0..6", b, one, None, 1))
    two = onehot(np.arange(n) % 2, descending(n), 3)
    out.append(case("interleaved", "mask build: suppression is class-restricted (the chain, classes alternating)", chain_boxes(n), two, None, 2))
    return out


# ------------------------------------------------------------------ NMS threshold edge (det_suppresses)
def nms_edge_boxes(t):
    """Pairs (stronger row first), each in its own 100-pixel column.  t is the threshold in tenths."""
    pairs = [([0, 0, 9, 9], [0, 0, 9, t - 1]),                # IoU = t / 10 exactly: kept
             ([0, 0, 9, 9], [0, 0, 9, t]),                    # one pixel row more: dropped
             ([0, 0, 9, 9], [0, 0, 9, 9]),                    # identical: IoU 1
             ([5, 5, 5, 9], [5, 5, 5, 9]),                    # zero width, identical: area 5 by the +1 rule
             ([3, 3, 3, 3], [3, 3, 4, 3]),                    # zero width and height: area 1 inside area 2, IoU 0.5
             ([7, 7, 7, 7], [7, 7, 7, 7]),                    # two points
             ([0, 20, 9, 29], [0, 30, 9, 39])]                # touching rows share no pixel: IoU 0
    boxes = []
    for i, (a, b) in enumerate(pairs):
        for q in (a, b):
            boxes.append([q[0] + 100 * i, q[1], q[2] + 100 * i, q[3]])
    return np.array(boxes, np.float32)


def nms_edge_cases():
    out = []
    for thr in NMS_EDGE_THRESHOLDS:
        b = nms_edge_boxes(int(round(thr * 10)))
        out.append(case("nms_edge_%g" % thr, "det_suppresses: IoU on / one pixel past the threshold %g, zero-extent RoIs" % thr,
                        b, onehot(np.zeros(len(b), int), descending(len(b)), 2), None, 1, nms=thr))
    return out


# ------------------------------------------------------------------ ranking ties (phase 2)
def tie_cases():
    out = []
    # groups of three overlapping, different boxes with one score; groups far apart; later groups score HIGHER, so a rule that
    # prefers the higher row index changes boxes and RoI indices, not only their order
    g = 20
    b = np.zeros((3 * g, 4), np.float32)
    s = np.zeros(3 * g, np.float32)
    for i in range(g):
        for j in range(3):
            b[3 * i + j] = (100 * i + j, j, 100 * i + 11 + j, 11 + j)    # IoU(j, j + 1) = 121 / 167, IoU(j, j + 2) = 100 / 188
        s[3 * i:3 * i + 3] = np.float32(0.2) + np.float32(0.03) * np.float32(i)
    out.append(case("tie_in_class", "ranking: equal scores in a class, the lower row wins (det_roi, det_bbox decide)", b,
                    onehot(np.zeros(3 * g, int), s, 2), None, 1))
    out.append(case("tie_all_512", "ranking: 512 rows with ONE score rank by row index", chain_boxes(512),
                    onehot(np.zeros(512, int), np.full(512, 0.5, np.float32), 2), None, 1))
    cls = np.tile([0, 1], 3 * g // 2)
    out.append(case("tie_two_classes", "ranking: equal scores across two classes", b, onehot(cls, np.repeat(s[::3], 3), 3), None, 2))
    # a real row and its padded duplicates: identical RoI, class row and regression row (frcnn_gather_rois + a deterministic head)
    rs = np.random.RandomState(7)
    n_live, rows = 100, 128
    rois = random_rois(rs, rows)
    p = random_probs(rs, rows, 21, (20,))
    reg = (rs.randn(rows, 80) * 0.5).astype(np.float32)
    rois[n_live:], p[n_live:], reg[n_live:] = rois[64], p[64], reg[64]
    out.append(case("tie_padded", "ranking: a live row ties with its padded duplicates and wins", rois, p, reg, 20, stride=16.0, ratio=1.6,
                    n_live=n_live, roi_batch=64))
    return out


# ------------------------------------------------------------------ arg-max and classes (phases 1 and 5)
def class_cases():
    out = []
    seed = 300
    for C in (2, 3, 21, 128):
        for bg in sorted({C - 1, 0, C // 2}):
            seed += 1
            out.append(random_case("argmax_c%d_bg%d" % (C, bg), "arg-max: C = %d, background at %d" % (C, bg), seed, 200, C, bg,
                                   stride=16.0, ratio=1.6))
    # the background ties with the best class: np.argmax takes the FIRST maximum
    n, C = 40, 5
    for bg, name in ((0, "lo"), (4, "hi")):
        rs = np.random.RandomState(320 + bg)
        other = 1 + rs.randint(0, 3, n)                       # classes 1..3
        p = onehot(other, descending(n, 0.9, 0.5), C, low=0.01)
        tied = np.arange(n) % 2 == 0
        p[tied, bg] = p[tied, other[tied]]
        out.append(case("argmax_bg_tie_" + name, "arg-max: background == best class; background %s index %s" %
                        (("lower", "wins, row dropped") if bg == 0 else ("higher", "loses, row stays")),
                        random_rois(rs, n), p, rs.randn(n, 16) * 0.5, bg, stride=16.0))
    rs = np.random.RandomState(330)
    p = onehot(np.full(n, 1), descending(n, 0.45, 0.2), C, low=0.01)
    p[:, 3] = p[:, 1]                                          # classes 1 and 3 tie for the maximum: 1 wins and ITS deltas decode
    out.append(case("argmax_two_tied", "arg-max: two classes tie, the first wins", random_rois(rs, n), p, rs.randn(n, 16) * 0.5, 4, stride=16.0))
    # 127 classes, every one present, first seen in a shuffled order
    rs = np.random.RandomState(340)
    n, C = 300, 128
    cls = np.concatenate([rs.permutation(C - 1), rs.randint(0, C - 1, n - (C - 1))])
    out.append(case("classes_128_shuffled", "emission: 127 classes in a shuffled first-seen order", random_rois(rs, n),
                    onehot(cls, rs.permutation(descending(n)), C), rs.randn(n, 4 * (C - 1)) * 0.5, C - 1, stride=16.0, ratio=1.6))
    # class 5 is first seen at row 0, which row 2 (same class, higher score, same place) suppresses: 5 still comes before 2
    b = np.array([[0, 0, 9, 9], [50, 0, 59, 9], [1, 0, 10, 9], [51, 0, 60, 9], [100, 0, 109, 9]], np.float32)
    out.append(case("first_seen_suppressed", "emission: a class keeps the place of its first valid row though that row is suppressed",
                    b, onehot([5, 2, 5, 2, 7], [0.3, 0.9, 0.8, 0.2, 0.6], 9), None, 8))
    rs = np.random.RandomState(350)
    out.append(case("all_background", "arg-max: every row is background", random_rois(rs, 100), onehot(np.full(100, 20), descending(100), 21, low=0.001),
                    rs.randn(100, 80), 20, stride=16.0))
    return out


# ------------------------------------------------------------------ score threshold (phase 1)
def threshold_cases():
    out = []
    rs = np.random.RandomState(400)
    n = 60
    rois = random_rois(rs, n)
    s = rs.permutation(descending(n, 0.95, 0.3))
    s[17] = np.float32(0.7)
    p = onehot(rs.randint(0, 20, n), s, 21, low=0.001)
    reg = rs.randn(n, 80) * 0.5
    at = float(np.float32(0.7))                               # the exact f64 of the f32 score
    out.append(case("thr_equal", "threshold: score == threshold in f64 is kept", rois, p, reg, 20, thr=at, stride=16.0))
    out.append(case("thr_one_step_above", "threshold: one f64 step above the f32 score drops the row (an f32 comparison would keep it)",
                    rois, p, reg, 20, thr=float(np.nextafter(at, 2.0)), stride=16.0))
    out.append(case("thr_python_0.7", "threshold: the Python float 0.7 lies above np.float32(0.7)", rois, p, reg, 20, thr=0.7, stride=16.0))
    out.append(case("thr_above_all", "threshold above every score: no detection, every output row empty", rois, p, reg, 20, thr=0.96, stride=16.0))
    b = np.array([[0, 0, 9, 9], [50, 0, 59, 9], [100, 0, 109, 9], [150, 0, 159, 9]], np.float32)
    out.append(case("thr_first_seen", "emission: first-seen counts rows that pass the threshold only",
                    b, onehot([2, 5, 2, 5], [0.1, 0.9, 0.8, 0.7], 9), None, 8, thr=0.5))
    return out


# ------------------------------------------------------------------ rounding of the emitted boxes (phase 5)
def rounding_cases():
    out = []
    n = 48
    i = np.arange(n)
    # integer corners 0..~110 of every parity, zero deltas, stride 1; nms 1.0 keeps every row (IoU <= 1)
    rois = np.stack([i, 2 * i + 1, i + 50 + i % 3, 2 * i + 1 + 13 + i % 2], 1).astype(np.float32)
    cls = onehot(i % 20, descending(n), 21)
    # rows that reach NEGATIVE halves through tx / ty alone: wa = ha = 8, tx in {-0.5, -0.25, -0.75} (reg / 10 exact), tw = th = 0
    neg = np.tile(np.array([[1, 1, 9, 9]], np.float32), (6, 1))
    reg = np.zeros((n + 6, 80), np.float32)
    for j, (rx, ry) in enumerate([(-5, -2.5), (-2.5, -5), (-7.5, -7.5), (-5, 0), (0, -7.5), (-10, -2.5)]):
        c = j % 20
        reg[n + j, 4 * c:4 * c + 2] = (rx, ry)
    allr = np.concatenate([rois, neg])
    allc = np.concatenate([cls, onehot(np.arange(6) % 20, descending(6, 0.009, 0.002), 21)])
    for ratio in ROUND_RATIOS:
        out.append(case("round_half_%g" % ratio, "box output: v / %g on x.5, even and odd x, both signs (half to even)" % ratio,
                        allr, allc, reg, 20, ratio=ratio, nms=1.0))
    return out


# ------------------------------------------------------------------ decode (phase 1)
def decode_cases():
    out = [random_case("decode_fuzz_s16", "decode: deltas at the fuzz tool's scale, stride 16", 500, 300, 21, 20, stride=16.0, ratio=1.6),
           random_case("decode_fuzz_s8", "decode: stride 8", 501, 300, 21, 20, stride=8.0, ratio=0.625),
           random_case("decode_frac_rois", "decode: RoIs with fractional f32 corners", 502, 300, 21, 20, frac=True, stride=16.0, ratio=1.6)]
    c = random_case("decode_big_tw", "decode: tw / th up to +-4", 503, 300, 21, 20, stride=16.0, ratio=1.6)
    rs = np.random.RandomState(504)
    c["reg"].reshape(300, 20, 4)[:, :, 2:] = (rs.rand(300, 20, 2) * 40 - 20).astype(np.float32)        # / 5 -> [-4, 4)
    out.append(c)
    return out


# ------------------------------------------------------------------ frcnn_detections_dyn: counts and clamps
def poison(c, first):
    """Rows at and past ``first`` are never scored: they hold a winning score for class 0 and NaN regressions."""
    c["cls"][first:] = 0
    c["cls"][first:, 0] = 1.0
    c["reg"][first:] = np.nan
    return c


def dyn_case(name, phase, seed, rows, n_live, batch):
    c = random_case(name, phase, seed, rows, 21, 20, rows=rows, stride=16.0, ratio=1.6, n_live=n_live, roi_batch=batch)
    scored = min(-(-n_live // batch) * batch if batch and n_live > 0 else n_live, rows)
    first = n_live // batch * batch if batch else 0
    if scored > n_live:
        c["rois"][n_live:scored] = c["rois"][first]          # frcnn_gather_rois: copies of the last batch's first RoI
    return poison(c, scored)


def dyn_cases():
    out = [dyn_case("dyn_live_%d" % n, "n_scored: %d live rows in batches of 64, poison behind" % n, 600 + i, 512, n, 64)
           for i, n in enumerate(DYN_LIVE)]
    out.append(dyn_case("dyn_clamp_300", "n_scored: 300 live rows pad to 320, max_rows 300 clamps", 620, 300, 300, 64))
    out.append(dyn_case("dyn_clamp_600", "n_scored: 600 live rows, max_rows 512 clamps; counts[1] stays 600", 621, 512, 600, 64))
    out.append(dyn_case("static_fewer_live", "n_scored: the static entry with n_rois < rows, poison behind", 622, 320, 200, 0))
    return out


FAMILIES = (("sizes", size_cases), ("cross_word", cross_word_cases), ("nms_edge", nms_edge_cases), ("ties", tie_cases),
            ("classes", class_cases), ("threshold", threshold_cases), ("rounding", rounding_cases), ("decode", decode_cases),
            ("dyn", dyn_cases))
_CACHE = {}


def all_cases():
    """name -> case, every family, built once."""
    if not _CACHE:
        for family, build in FAMILIES:
            for c in build():
                assert c["name"] not in _CACHE
                c["family"] = family
                _CACHE[c["name"]] = c
    return _CACHE


def names(family=None):
    return [k for k, c in all_cases().items() if family is None or c["family"] == family]
