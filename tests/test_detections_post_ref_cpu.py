"""The post-process rule's reference (tests/detections_post_ref.py) without a GPU: it is ``detections_ref`` in the hard mode without
voting, it gives the hand-worked answers, the option normaliser refuses what it should, and -- the condition the GPU parity test rests on
-- no case of tests/detections_cases.py holds a decision that a one-ulp ``exp`` could flip under any parameter set that test uses."""
import numpy as np
import pytest

from tests import detections_cases as K
from tests import detections_post_ref as P
from tests import detections_ref as R

CASES = K.all_cases()


def two_class_scores(scores):
    """Rows of class 0 with the given scores; class 1 is the background and loses every row."""
    return K.onehot([0] * len(scores), scores, 3)


def test_hard_without_vote_is_the_existing_reference():
    assert len(CASES) == 74
    for name, c in CASES.items():
        for batch in ((0, None) if c["roi_batch"] else (0,)):
            want = R.run(c, batch)
            got = P.run(c, ("hard", c["nms"]), batch)
            assert got[4] == want[4], name
            assert got[1].tobytes() == want[1].tobytes(), name
            for a, b in zip(got[:4], want[:4]):
                assert a.dtype == b.dtype and np.array_equal(a, b), name


def test_linear_keeps_both_of_two_overlapping_boxes():
    # A 10 x 10, B its upper 10 x 6: inter 60, IoU 60 / (100 + 60 - 60) = 0.6
    c = K.case("two", "post", [[0, 0, 9, 9], [0, 0, 9, 5]], two_class_scores([0.9, 0.8]), None, bg=1)
    assert P.iou([0, 0, 9, 9], [0, 0, 9, 5]) == 0.6
    cls, prob, bbox, roi, _ = P.run(c, ("soft_linear", 0.3))
    assert roi.tolist() == [0, 1] and cls.tolist() == [0, 0] and bbox.tolist() == [[0, 0, 9, 9], [0, 0, 9, 5]]
    assert prob[0] == np.float32(0.9) and prob[1] == np.float32(float(np.float32(0.8)) * (1.0 - 0.6))
    assert P.run(c, ("hard", 0.5))[3].tolist() == [0]                       # the hard rule deletes B
    assert P.run(c, ("soft_linear", 0.6))[1][1] == np.float32(0.8)          # o <= Nt: untouched


def test_min_score_equal_to_a_decayed_score_keeps_it():
    c = K.case("two", "post", [[0, 0, 9, 9], [0, 0, 9, 5]], two_class_scores([0.9, 0.8]), None, bg=1)
    s = float(np.float32(0.8)) * (1.0 - 0.6)
    assert P.run(c, ("soft_linear", 0.3, 0.5, s))[3].tolist() == [0, 1]
    assert P.run(c, ("soft_linear", 0.3, 0.5, float(np.nextafter(s, 1.0))))[3].tolist() == [0]
    # None = the image's threshold: the f64 the threshold comparison uses
    c_thr = dict(c, thr=s)
    assert P.run(c_thr, ("soft_linear", 0.3))[3].tolist() == [0, 1]
    assert P.run(dict(c, thr=float(np.nextafter(s, 1.0))), ("soft_linear", 0.3))[3].tolist() == [0]


@pytest.mark.parametrize("swap", (False, True))
def test_gaussian_symmetric_history_ties_exactly(swap):
    """X takes overlap a from P and b from Q, Y takes b from P and a from Q (P and Q apart): one exp of the summed exponent a a + b b
    = b b + a a gives both the same score to the last bit, and the lower row goes first.  A product of two exps need not."""
    p, q, x, y = [0, 0, 9, 9], [20, 0, 29, 9], [3, 0, 22, 9], [7, 0, 26, 9]
    a, b = P.iou(p, x), P.iou(q, x)
    assert a == P.iou(q, y) and b == P.iou(p, y) and a != b and a > 0 and b > 0 and P.iou(p, q) == 0.0
    rois = [p, q, y, x] if swap else [p, q, x, y]
    c = K.case("sym", "post", rois, two_class_scores([0.9, 0.8, 0.5, 0.5]), None, bg=1)
    cls, prob, bbox, roi, _ = P.run(c, ("soft_gaussian", 0.5, 0.5))
    assert roi.tolist() == [0, 1, 2, 3]
    assert prob[1] == np.float32(0.8)                                       # exp(-0) = 1: Q is not touched by P
    assert prob[2] == np.float32(0.5 * float(np.exp(-((0.0 + a * a + b * b) / 0.5))))
    assert prob[3] < prob[2]                                                # the first of the pair then decays the second
    assert P.unstable_post(c, ("soft_gaussian", 0.5, 0.5)) == []            # a bitwise tie is determined


def test_voting_over_three_boxes():
    # A 0.5 and B 0.25 overlap at 80 / 120, C 0.25 stands apart: A's voted x1 = (0.5 * 0 + 0.25 * 2) / 0.75, x2 = (4.5 + 2.75) / 0.75
    c = K.case("vote", "post", [[0, 0, 9, 9], [2, 0, 11, 9], [40, 40, 49, 49]], two_class_scores([0.5, 0.25, 0.25]), None, bg=1)
    cls, prob, bbox, roi, _ = P.run(c, ("hard", 0.5, 0.5, None, 0.5))
    assert roi.tolist() == [0, 2] and prob.tolist() == [0.5, 0.25]          # B is suppressed, and still votes
    assert bbox.tolist() == [[1, 0, 10, 9], [40, 40, 49, 49]]
    assert P.run(c, ("hard", 0.5, 0.5, None, 0.7))[2].tolist() == [[0, 0, 9, 9], [40, 40, 49, 49]]     # 2 / 3 < 0.7: A alone
    # the soft modes pick B too; its vote has the same members, and scores never see a voted box
    cls, prob, bbox, roi, _ = P.run(c, ("soft_linear", 0.3, 0.5, None, 0.5))
    assert roi.tolist() == [0, 2, 1] and bbox.tolist() == [[1, 0, 10, 9], [40, 40, 49, 49], [1, 0, 10, 9]]
    assert prob[2] == np.float32(0.25 * (1.0 - 80.0 / 120.0))
    # the resize ratio divides the voted coordinate
    assert P.run(dict(c, ratio=2.0), ("hard", 0.5, 0.5, None, 0.5))[2].tolist()[0] == [0, 0, 5, 4]


def test_unstable_post_finds_what_it_should():
    c = K.case("two", "post", [[0, 0, 9, 9], [0, 0, 9, 5]], two_class_scores([0.9, 0.8]), None, bg=1)
    assert P.unstable_post(c, ("soft_gaussian", 0.5, 0.5)) == []
    s = float(np.float32(0.8)) * float(np.exp(-((0.6 * 0.6) / 0.5)))
    near = P.unstable_post(c, ("soft_gaussian", 0.5, 0.5, s * (1 + 1e-13)))
    assert [u[0] for u in near] == ["min_score"]
    # a moved box whose IoU with another sits on the voting threshold
    reg = np.zeros((2, 8), np.float32)
    reg[1, 2] = 1e-30                                                        # tw != 0, exp(tw) == 1: the box itself does not move
    moved = K.case("edge", "post", [[0, 0, 9, 9], [0, 0, 9, 5]], two_class_scores([0.9, 0.8]), reg, bg=1)
    assert ("vote_iou", 0, 1) in P.unstable_post(moved, ("hard", 0.7, 0.5, None, 0.6))
    assert P.unstable_post(c, ("hard", 0.7, 0.5, None, 0.6)) == []           # exact boxes are not listed


@pytest.mark.parametrize("name", sorted(P.GPU_POSTS))
def test_condition_no_case_is_unstable_under_the_gpu_parameter_sets(name):
    """THE CONDITION of tests/test_detections_post_gpu.py: all 74 cases, none left out, both ways of counting the scored rows."""
    for cname, c in CASES.items():
        for batch in ((0, None) if c["roi_batch"] else (0,)):
            assert P.unstable_post(c, P.gpu_post(name, c), batch) == [], (name, cname, batch)


def test_option_normaliser():
    from faster_rcnn_amd import ops
    assert ops.det_post_option(None) == ("hard", 0.5, 0.5, None, None) == ops.det_post_option(()) == ops.det_post_option({})
    assert ops.det_post_option("soft_linear") == ("soft_linear", 0.5, 0.5, None, None)
    assert ops.det_post_option(("soft_gaussian", None, 0.25, 0, 1)) == ("soft_gaussian", 0.5, 0.25, 0.0, 1.0)
    assert ops.det_post_option({"vote_iou": 0.5, "mode": "soft_gaussian"}) == ("soft_gaussian", 0.5, 0.5, None, 0.5)
    assert ops.det_post_option(ops.det_post_option(("soft_linear", 0.3, 0.5, 0.05, 0.5))) == ("soft_linear", 0.3, 0.5, 0.05, 0.5)
    for bad, word in ((("soft",), "mode"), (("hard", 1.5), "nms_thresh"), (("hard", -0.1), "nms_thresh"), (("hard", None, 0.0), "sigma"),
                      (("hard", None, -1.0), "sigma"), (("hard", None, float("inf")), "sigma"), (("hard", None, None, 1.5), "min_score"),
                      (("hard", None, None, -0.5), "min_score"), (("hard", None, None, None, 0.0), "vote_iou"),
                      (("hard", None, None, None, 1.5), "vote_iou"), (("hard", None, float("nan")), "sigma"),
                      (("hard", True), "nms_thresh"), (("hard", "0.5"), "nms_thresh"), ({"iou": 0.5}, "iou"),
                      (("hard", 0.5, 0.5, None, None, 1), "tuple"), (5, "tuple")):
        with pytest.raises(ValueError) as e:
            ops.det_post_option(bad)
        assert word in str(e.value), (bad, str(e.value))
