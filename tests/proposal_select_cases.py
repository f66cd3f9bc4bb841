"""Inputs and numpy restatements for the proposal-selection kernels (csrc/sort_nms.hip): the banded NMS and the top-K's
histogram form.  tests/test_proposal_select_cpu.py checks the restatements and the cases' intent against the oracle,
tests/test_proposal_select_gpu.py runs the same cases through the library."""
import os
import re

import numpy as np

from oracle import np_ref

# csrc/sort_nms.hip: nms_band_begin, TOPK_DIRECT_N, TOPK_RANK_SLACK (test_proposal_select_cpu.py holds them to the source)
NMS_BAND_BEGIN = (0, 16, 32, 64)                # first row block (64 candidates each) of every band
TOPK_DIRECT_N = 16384                           # at or below this many scores no histogram runs
TOPK_RANK_SLACK = 1024
B = NMS_BAND_BEGIN[1] * 64                      # candidates in the first band

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "faster_rcnn_amd", "csrc", "sort_nms.hip")


def source_constants():
    src = open(SOURCE).read()
    begins = re.search(r"nms_band_begin\(int b\) \{ return b == 0 \? (\d+) : b == 1 \? (\d+) : b == 2 \? (\d+) : (\d+); \}", src)
    return {"bands": tuple(int(v) for v in begins.groups()),
            "direct_n": int(re.search(r"constexpr int TOPK_DIRECT_N = (\d+);", src).group(1)),
            "rank_slack": int(re.search(r"constexpr int TOPK_RANK_SLACK = (\d+);", src).group(1))}


# ------------------------------------------------------------------------------------------------ NMS inputs
def _cells(count, frac):
    """`count` pairwise disjoint 10x10 boxes (11x11 under the +1 convention) on a 64-wide grid of pitch 12."""
    k = np.arange(count)
    x, y = (k % 64) * 12, (k // 64) * 12
    return np.stack([x, y, x + 10, y + 10], axis=1).astype(np.float64) + frac


def chain_boxes(kept_flags, dtype, seed):
    """Box i is a fresh disjoint cell where kept_flags[i], else a copy of an earlier kept cell moved by at most one pixel in x
    (overlap 110/132 > 0.7: suppressed).  Greedy NMS keeps exactly the flagged boxes, in order."""
    rs = np.random.RandomState(seed)
    kept_flags = np.asarray(kept_flags, bool)
    assert kept_flags[0]
    cells = _cells(int(kept_flags.sum()), 0.0 if dtype == np.int16 else 0.25)
    upto = np.cumsum(kept_flags)                                    # kept cells among boxes 0..i
    src = np.where(kept_flags, upto - 1, rs.randint(0, 1 << 30, len(kept_flags)) % np.maximum(upto, 1))
    boxes = cells[src]
    boxes[:, [0, 2]] += np.where(kept_flags, 0, rs.randint(0, 2, len(kept_flags)))[:, None]
    return boxes.astype(dtype)


def stop_at(K, stop, max_boxes, dtype, seed):
    """K boxes of which exactly max_boxes are kept among the first stop + 1, box `stop` being the last of them."""
    rs = np.random.RandomState(seed)
    flags = np.zeros(K, bool)
    flags[0] = flags[stop] = True
    flags[1 + rs.choice(stop - 1, max_boxes - 2, replace=False)] = True
    flags[stop + 1:] = rs.rand(K - stop - 1) < 0.3
    return chain_boxes(flags, dtype, seed + 1)


def random_boxes(K, dtype, seed):
    """Overlapping boxes in a small field (the areas stay far inside int16, as numpy computes them there)."""
    rs = np.random.RandomState(seed)
    xy = rs.randint(0, 80, (K, 2))
    wh = rs.randint(1, 40, (K, 2))
    b = np.concatenate([xy, xy + wh], axis=1)
    return b.astype(np.int16) if dtype == np.int16 else b + rs.rand(K, 4) * 0.5


def nms_cases(dtype):
    """name -> (boxes [K][4] in descending score order, n live rows, max_boxes, thresh, index of the last kept box, None
    when max_boxes is never reached, -1 when the case does not say)."""
    cases = {}
    for K in (1, 63, 64, 65, 130, B - 1, B, B + 1, B + 64):
        cases["random_K%d" % K] = (random_boxes(K, dtype, 100 + K), K, 300, 0.7, -1)
        cases["random_K%d_short" % K] = (random_boxes(K, dtype, 200 + K), K - 1 - K // 7, 300, 0.5, -1)
    K = 2 * B + 152                                                 # three bands, the last one a part chunk
    cases["stop_inside_band0"] = (stop_at(K, 500, 300, dtype, 1), K, 300, 0.7, 500)
    cases["stop_last_row_of_band0"] = (stop_at(K, B - 1, 300, dtype, 2), K, 300, 0.7, B - 1)
    cases["stop_first_row_of_band1"] = (stop_at(K, B, 300, dtype, 3), K, 300, 0.7, B)
    cases["stop_last_row_of_band1"] = (stop_at(K, 2 * B - 1, 300, dtype, 4), K, 300, 0.7, 2 * B - 1)
    cases["stop_first_row_of_band2"] = (stop_at(K, 2 * B, 300, dtype, 5), K - 3, 300, 0.7, 2 * B)
    cases["all_identical"] = (np.repeat(_cells(1, 0.0), K, axis=0).astype(dtype), K, 300, 0.7, None)
    cases["all_disjoint"] = (_cells(K, 0.0 if dtype == np.int16 else 0.25).astype(dtype), K - 5, K + 100, 0.7, None)
    cases["bench_shape"] = (stop_at(8000, B + 476, 300, dtype, 6), 8000, 300, 0.7, B + 476)
    return cases


def oracle_keep(boxes, n, max_boxes, thresh):
    """np_ref.nms on the live rows; scores strictly descending with the position, so its argsort has no ties to break."""
    if n == 0:
        return np.zeros(0, np.int64)
    return np.asarray(np_ref.nms(boxes[:n], -np.arange(n, dtype=np.float64), thresh, max_boxes)[2], dtype=np.int64)


# ------------------------------------------------------------------------------------------------ NMS restatement
def _mask_rows(boxes, lo, hi, n, thresh):
    """suppresses(i, j) for rows lo..hi-1 against every live column, evaluated like the reference does for the boxes' dtype."""
    b = boxes[:n]
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    area = (x2 - x1 + 1) * (y2 - y1 + 1)
    r = slice(lo, hi)
    w = np.maximum(0, np.minimum(x2[r, None], x2[None]) - np.maximum(x1[r, None], x1[None]) + 1)
    h = np.maximum(0, np.minimum(y2[r, None], y2[None]) - np.maximum(y1[r, None], y1[None]) + 1)
    inter = w * h
    return ~(inter / (area[r, None] + area[None] - inter) <= thresh)


def banded_nms(boxes, n, max_boxes, thresh, bands=NMS_BAND_BEGIN):
    """The library's schedule in numpy: per band a mask launch (only that band's rows) and a scan launch that walks the band's
    64-candidate chunks, the state (removed bitmap, total, done) handed from band to band.
    -> keep [max_boxes] (-1 tail), n_keep, the bands whose launches did not return at once."""
    K = len(boxes)
    W = (K + 63) // 64
    n = min(n, K)
    chunks = (n + 63) // 64
    keep = np.full(max_boxes, -2, np.int64)                         # -2: a slot no launch wrote
    state = {"done": None, "total": None, "removed": None}          # band 0 reads none of it
    n_keep, ran = None, []
    begins = [r for r in bands if r < W]
    for b, r0 in enumerate(begins):
        r1 = begins[b + 1] if b + 1 < len(begins) else W
        if b and state["done"]:
            continue
        ran.append(b)
        rows = _mask_rows(boxes, r0 * 64, min(r1 * 64, n), n, thresh) if r0 * 64 < n else np.zeros((0, n), bool)
        removed = state["removed"].copy() if b else np.zeros(n, bool)
        total = state["total"] if b else 0
        cend = min(r1, chunks)
        c = r0
        while c < cend and total < max_boxes:
            for i in range(c * 64, min(c * 64 + 64, n)):
                if removed[i] or total >= max_boxes:
                    continue
                keep[total] = i
                total += 1
                removed[i + 1:] |= rows[i - r0 * 64, i + 1:]
            c += 1
        if total < max_boxes and cend < chunks:
            state = {"done": 0, "total": total, "removed": removed}
            continue
        keep[total:] = -1
        n_keep = total
        state["done"] = 1
    return keep, n_keep, ran


# ------------------------------------------------------------------------------------------------ top-K inputs
def topk_cases():
    """name -> (scores f32 [N], valid bool [N] or None, K)."""
    S = TOPK_DIRECT_N
    rs = np.random.RandomState(77)
    cases = {}
    for N in (S - 1, S, S + 1):
        cases["switch_N%d" % N] = (rs.rand(N).astype(np.float32), None, 1000)
        cases["switch_valid_N%d" % N] = (rs.rand(N).astype(np.float32), rs.rand(N) < 0.8, 1000)
    N = S + 1500
    cases["k_above_valid"] = (rs.rand(N).astype(np.float32), rs.rand(N) < 0.25, N // 2)      # short output on the histogram form
    cases["valid_mask"] = (rs.rand(N).astype(np.float32), rs.rand(N) < 0.5, 1500)
    cases["ties"] = ((rs.randint(0, 16, N) / 16.0 + 0.03125).astype(np.float32), rs.rand(N) < 0.9, 1500)
    cases["all_equal_small_k"] = (np.full(N, 0.5, np.float32), None, 300)        # C = N, far above the rank grid's K + slack rows
    cases["all_equal_bench_n"] = (np.full(21546, 0.25, np.float32), rs.rand(21546) < 0.95, 8000)
    wide = (np.where(rs.rand(N) < 0.5, -1.0, 1.0) * 10.0 ** rs.uniform(-30, 30, N)).astype(np.float32)
    cases["wide_spread"] = (wide, None, 2000)                       # > 4096 bins inside every workgroup: global-atomics fallback
    logits = rs.randn(21546) * 0.6 - 2.5
    cases["bench_shape"] = ((1.0 / (1.0 + np.exp(-logits))).astype(np.float32), rs.rand(21546) < 0.9, 8000)
    return cases


def oracle_order(scores, valid, K):
    idx = np.arange(len(scores)) if valid is None else np.flatnonzero(valid)
    return idx[np_ref.score_order(scores[idx].astype(np.float64), K)]


# ------------------------------------------------------------------------------------------------ top-K restatement
def mono_f32(scores):
    u = np.asarray(scores, np.float32).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def hist_topk(scores, valid, K):
    """The histogram form: bin of the K-th key by the keys' top 16 bits, candidates at or above it, rank by counting among them.
    -> order [K] (-1 tail), n, the candidate count C, the bins one 256-score workgroup spans at most."""
    N = len(scores)
    live = np.ones(N, bool) if valid is None else np.asarray(valid, bool)
    mono = mono_f32(scores)
    bins = (mono >> 16).astype(np.int64)
    hist = np.bincount(bins[live], minlength=65536)
    need = min(int(live.sum()), K)
    order = np.full(K, -1, np.int64)
    span = max(int(np.ptp(bins[i:i + 256][live[i:i + 256]])) if live[i:i + 256].any() else 0 for i in range(0, N, 256))
    if need == 0:
        return order, 0, 0, span
    above = np.cumsum(hist[::-1])                                   # keys in the top t + 1 bins
    thr = 65535 - int(np.searchsorted(above, need))
    cand = np.flatnonzero(live & (bins >= thr))
    keys = (mono[cand].astype(np.uint64) << np.uint64(32)) | (~cand.astype(np.uint32)).astype(np.uint64)
    rank = np.empty(len(cand), np.int64)
    rank[np.argsort(keys)[::-1]] = np.arange(len(cand))             # keys are unique: = the number of larger keys
    sel = rank < K
    order[rank[sel]] = cand[sel]
    return order, need, len(cand), span
