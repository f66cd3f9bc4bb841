"""tests/detections_ref.py against the oracle (oracle.np_ref.detections), against answers worked out by hand, and the
condition on the generated inputs that tests/test_detections_gpu.py relies on: no case holds a decision that one ulp of
``exp`` could flip.  No GPU."""
import os

import numpy as np
import pytest

from oracle import np_ref
from tests import detections_cases as K
from tests import detections_ref as R

CASES = K.all_cases()
TIED = {"tie_in_class", "tie_all_512", "tie_two_classes", "tie_padded"}        # the only cases the oracle's argsort leaves open


def forms(c):
    """The roi_batch values the GPU file runs a case with."""
    return (0, c["roi_batch"]) if c["roi_batch"] else (0,)


def oracle(c, batch):
    ns = R.n_scored(c["n_live"], batch, len(c["cls"]))
    return np_ref.detections(c["rois"][:ns], c["cls"][:ns], c["reg"][:ns], c["bg"], c["ratio"], stride=c["stride"], det_threshold=c["thr"],
                             num_rois=max(batch, 1), nms_thresh=c["nms"])


def same_as_oracle(got, want):
    cls, prob, bbox = got[:3]
    assert len(cls) == len(want)
    assert np.array_equal(cls, np.array([d[0] for d in want], np.int32))
    assert prob.tobytes() == np.array([d[1] for d in want], np.float32).tobytes()
    assert np.array_equal(bbox, np.array([d[2] for d in want], np.int64).reshape(-1, 4))


@pytest.mark.parametrize("tag", ["t0", "t5", "t0r", "tb"])
@pytest.mark.parametrize("rows", [300, 320])
def test_equals_the_oracle_and_the_recorded_reference_on_the_fixture(tag, rows):
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "dets_legacy.npz"))
    rois = g["rois"].astype(np.float32)
    thr, ratio = (float(v) for v in g[tag + "_args"])
    r = np.concatenate([rois, np.tile(rois[256], (rows - len(rois), 1))])
    got = R.detections(r, g["out_cls"][:rows], g["out_reg"][:rows], rows, 20, ratio, thr, 16.0)
    same_as_oracle(got, np_ref.detections(rois, g["out_cls"][:rows], g["out_reg"][:rows], 20, ratio, det_threshold=thr))
    assert np.array_equal(got[0], g[tag + "_cls"]) and np.array_equal(got[1], g[tag + "_prob"]) and np.array_equal(got[2], g[tag + "_bbox"])
    assert got[4] == rows and (got[3] < rows).all()
    # the padded form counted from the live rows is the same call; a duplicate never beats the live row it copies
    assert all(np.array_equal(a, b) for a, b in zip(got[:4], R.detections(r, g["out_cls"], g["out_reg"], 300, 20, ratio, thr, 16.0, roi_batch=64, max_rows=rows)[:4]))
    assert (got[3] < 300).all()


@pytest.mark.parametrize("name", list(CASES))
def test_generated_case_is_stable_and_equals_the_oracle_where_it_is_defined(name):
    c = CASES[name]
    for batch in forms(c):
        assert R.unstable(c, batch) == []
        tied = R.has_ties(c, batch)
        assert tied == (name in TIED and (name != "tie_padded" or batch == 64)), "the oracle comparison must not be skipped by accident"
        got = R.run(c, batch)
        assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[2].dtype == np.int64 and got[3].dtype == np.int32
        if not tied:
            same_as_oracle(got, oracle(c, batch))


def test_families_reach_what_they_are_aimed_at():
    """Conditions on the inputs that the case builders promise."""
    for n in K.SIZES:
        for tag in ("c21", "c2"):
            c = CASES["size_%d_%s" % (n, tag)]
            valid = sum(1 for _ in R._rows(c["rois"], c["cls"], c["reg"], n, c["bg"], c["thr"], c["stride"]))
            assert valid == n == len(c["cls"])                                   # nv = rows: no background winner, threshold 0
    assert len(set(R.run(CASES["classes_128_shuffled"])[0].tolist())) == 127
    assert len(R.run(CASES["size_512_c2"])[0]) < 512 and len(R.run(CASES["size_512_c21"])[0]) < 512      # the NMS has work to do
    for ratio in K.ROUND_RATIOS:                                                 # halves of both signs and both parities are hit
        c = CASES["round_half_%g" % ratio]
        q = np.array([[v / ratio for v in row[3]] for row in R._rows(c["rois"], c["cls"], c["reg"], len(c["cls"]), 20, 0.0, 1.0)])
        half = q[np.abs(q - np.floor(q) - 0.5) == 0]
        assert (half < 0).any() and (np.floor(half[half > 0]) % 2 == 0).any() and (np.floor(half[half > 0]) % 2 == 1).any()
    for n in K.DYN_LIVE:
        c = CASES["dyn_live_%d" % n]
        ns = R.n_scored(n, 64, 512)
        assert ns == -(-n // 64) * 64 and np.isnan(c["reg"][ns:]).all() and not np.isnan(c["reg"][:ns]).any()
        assert (c["rois"][n:ns] == c["rois"][n // 64 * 64 if ns > n else 0]).all()
    assert R.n_scored(300, 64, 300) == 300 and R.n_scored(600, 64, 512) == 512 and R.n_scored(200, 0, 320) == 200
    assert R.n_scored(0, 64, 512) == 0 and R.n_scored(513, 0, 600) == 512


# ------------------------------------------------------------------ answers worked out by hand
def test_kat_chain_keeps_every_even_row():
    cls, prob, bbox, roi, ns = R.run(CASES["chain"])
    assert ns == 512 and roi.tolist() == list(range(0, 512, 2)) and not cls.any()
    assert bbox.tolist() == [[4 * k, 0, 4 * k + 9, 9] for k in range(256)]
    assert prob.tobytes() == CASES["chain"]["cls"][::2, 0].tobytes()


def test_kat_cross_word_cases():
    assert R.run(CASES["long_range"])[3].tolist() == [r for r in range(512) if r not in (63, 64, 65, 447, 448, 511)]
    victims = {74, 138, 202, 266, 330, 394, 458, 139, 203, 267, 331, 395, 459, 204, 268, 332, 396, 460, 269, 333, 397, 461, 334, 398, 462,
               399, 463, 464}
    assert victims == {v for k in range(7) for v in K.killer_victims(k)}
    assert R.run(CASES["late_killers"])[3].tolist() == [r for r in range(512) if r not in victims]
    cls, _, _, roi, _ = R.run(CASES["interleaved"])
    assert roi.tolist() == list(range(0, 512, 2)) + list(range(1, 512, 2)) and cls.tolist() == [0] * 256 + [1] * 256


def test_kat_iou_on_the_threshold_is_kept():
    """Pairs of nms_edge_boxes, rows (2 i, 2 i + 1).  +1 convention: [0,0,9,9] holds 100 pixels, [0,0,9,4] 50 of them: IoU 0.5."""
    a = R.detections([[0, 0, 9, 9], [0, 0, 9, 4]], [[0.9, 0], [0.8, 0]], np.zeros((2, 4)), 2, 1, 1.0, stride=1.0)
    assert a[3].tolist() == [0, 1] and a[2].tolist() == [[0, 0, 9, 9], [0, 0, 9, 4]]
    a = R.detections([[0, 0, 9, 9], [0, 0, 9, 5]], [[0.9, 0], [0.8, 0]], np.zeros((2, 4)), 2, 1, 1.0, stride=1.0)
    assert a[3].tolist() == [0]
    assert R.run(CASES["nms_edge_0.5"])[3].tolist() == [0, 1, 2, 4, 6, 8, 9, 10, 12, 13]
    assert R.run(CASES["nms_edge_0.3"])[3].tolist() == [0, 1, 2, 4, 6, 8, 10, 12, 13]          # 30 / 100 is kept, the 1-in-2 pixel pair is not
    assert R.run(CASES["nms_edge_0.7"])[3].tolist() == [0, 1, 2, 4, 6, 8, 9, 10, 12, 13]


def test_kat_round_half_to_even():
    # zero deltas, stride 1, ratio 2: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4
    a = R.detections([[1, 3, 5, 7]], [[0.9, 0]], np.zeros((1, 4)), 1, 1, 2.0, stride=1.0)
    assert a[2].tolist() == [[0, 2, 2, 4]]
    # wa = ha = 8, centre (5, 5), tx = -5 / 10, ty = -2.5 / 10: the box is (-3, -1, 5, 7) -> -1.5, -0.5, 2.5, 3.5
    a = R.detections([[1, 1, 9, 9]], [[0.9, 0]], [[-5, -2.5, 0, 0]], 1, 1, 2.0, stride=1.0)
    assert a[2].tolist() == [[-2, 0, 2, 4]]
    a = R.detections([[1, 1, 9, 9]], [[0.9, 0]], [[-7.5, -7.5, 0, 0]], 1, 1, 2.0, stride=1.0)      # (-5, -5, 3, 3) -> -2.5, 1.5
    assert a[2].tolist() == [[-2, -2, 2, 2]]
    # 0.4 is no binary fraction, but the f64 quotients 1, 3, 5, 7 / 0.4 still round to 2.5, 7.5, 12.5, 17.5 exactly: to even
    a = R.detections([[1, 3, 5, 7]], [[0.9, 0]], np.zeros((1, 4)), 1, 1, 0.4, stride=1.0)
    assert a[2].tolist() == [[2, 8, 12, 18]]


def test_kat_first_seen_order():
    cls, prob, bbox, roi, _ = R.run(CASES["first_seen_suppressed"])
    assert cls.tolist() == [5, 2, 7] and roi.tolist() == [2, 1, 4]
    assert bbox.tolist() == [[1, 0, 10, 9], [50, 0, 59, 9], [100, 0, 109, 9]]
    cls, _, _, roi, _ = R.run(CASES["thr_first_seen"])
    assert cls.tolist() == [5, 5, 2] and roi.tolist() == [1, 3, 2]           # row 0 (class 2) is under the threshold: 5 is seen first


def test_kat_tie_rule():
    # two overlapping boxes, one score: the lower row is visited first and removes the other
    a = R.detections([[0, 0, 9, 9], [1, 0, 10, 9]], [[0.5, 0], [0.5, 0]], np.zeros((2, 4)), 2, 1, 1.0, stride=1.0)
    assert a[3].tolist() == [0] and a[2].tolist() == [[0, 0, 9, 9]]
    assert R.run(CASES["tie_in_class"])[3].tolist() == [3 * i for i in range(19, -1, -1)]
    assert R.run(CASES["tie_all_512"])[3].tolist() == list(range(0, 512, 2))
    cls, _, _, roi, _ = R.run(CASES["tie_two_classes"])
    # groups (0, 1, 0), (1, 0, 1), ...: the outer rows share a class and overlap, the lower one stays
    want0 = [r for i in range(19, -1, -1) for r in ([3 * i] if i % 2 == 0 else [3 * i + 1])]
    want1 = [r for i in range(19, -1, -1) for r in ([3 * i + 1] if i % 2 == 0 else [3 * i])]
    assert roi.tolist() == want0 + want1 and cls.tolist() == [0] * 20 + [1] * 20
    roi = R.run(CASES["tie_padded"])[3]
    assert 64 in roi and (roi < 100).all()                                   # the duplicates of row 64 all lose to it


def test_kat_background_and_threshold():
    assert len(R.run(CASES["all_background"])[0]) == 0 and len(R.run(CASES["thr_above_all"])[0]) == 0
    lo, hi = R.run(CASES["argmax_bg_tie_lo"]), R.run(CASES["argmax_bg_tie_hi"])
    assert sorted(lo[3].tolist()) == list(range(1, 40, 2))                    # even rows tie with background 0 and are dropped
    assert set(range(0, 40, 2)) & set(hi[3].tolist())                         # ... and stay when the background sits behind them
    assert set(R.run(CASES["argmax_two_tied"])[0].tolist()) == {1}
    assert 17 in R.run(CASES["thr_equal"])[3] and 17 not in R.run(CASES["thr_one_step_above"])[3] and 17 not in R.run(CASES["thr_python_0.7"])[3]
    assert len(R.run(CASES["thr_equal"])[0]) == len(R.run(CASES["thr_one_step_above"])[0]) + 1
    with pytest.raises(ValueError):                                           # class C - 1 has no regression columns
        R.detections([[0, 0, 9, 9]], [[0.1, 0.2, 0.7]], np.zeros((1, 8)), 1, 0, 1.0)
