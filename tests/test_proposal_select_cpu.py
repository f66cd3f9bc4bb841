"""CPU restatement of the proposal selection's schedule (csrc/sort_nms.hip): the NMS built and scanned in bands of row blocks
with its state handed from band to band, and the top-K's histogram form.  Both must give what oracle/np_ref gives, and every
case of tests/proposal_select_cases.py must exercise what its name says (tests/test_proposal_select_gpu.py runs the same cases
on the device)."""
import numpy as np
import pytest

from tests import proposal_select_cases as psc


def test_constants_match_the_source():
    c = psc.source_constants()
    assert c["bands"] == psc.NMS_BAND_BEGIN and c["direct_n"] == psc.TOPK_DIRECT_N and c["rank_slack"] == psc.TOPK_RANK_SLACK


@pytest.fixture(scope="module", params=[np.int16, np.float64], ids=["i16", "f64"])
def nms_cases(request):
    return psc.nms_cases(request.param)


def test_banded_nms_equals_the_oracle(nms_cases):
    for name, (boxes, n, max_boxes, thresh, stop) in nms_cases.items():
        want = psc.oracle_keep(boxes, n, max_boxes, thresh)
        keep, n_keep, ran = psc.banded_nms(boxes, n, max_boxes, thresh)
        assert n_keep == len(want), name
        assert np.array_equal(keep[:n_keep], want) and (keep[n_keep:] == -1).all(), name


def test_nms_cases_stop_where_they_say(nms_cases):
    B = psc.B
    bands_of = lambda K: sum(1 for r in psc.NMS_BAND_BEGIN if r < (K + 63) // 64)
    ran_bands = {}
    for name, (boxes, n, max_boxes, thresh, stop) in nms_cases.items():
        want = psc.oracle_keep(boxes, n, max_boxes, thresh)
        ran_bands[name] = psc.banded_nms(boxes, n, max_boxes, thresh)[2]
        if stop == -1:                                  # random boxes: wherever the scan ends
            continue
        if stop is not None:
            assert len(want) == max_boxes and want[-1] == stop, name
        else:
            assert len(want) < max_boxes, name
            assert len(ran_bands[name]) == sum(1 for r in psc.NMS_BAND_BEGIN if r * 64 < max(n, 1)), name     # every band with live rows
    assert ran_bands["stop_inside_band0"] == [0] and ran_bands["stop_last_row_of_band0"] == [0]
    assert ran_bands["stop_first_row_of_band1"] == [0, 1] and ran_bands["stop_last_row_of_band1"] == [0, 1]
    assert ran_bands["stop_first_row_of_band2"] == [0, 1, 2]
    assert ran_bands["bench_shape"] == [0, 1] and bands_of(8000) == 4
    assert len(nms_cases["all_identical"][0]) > 2 * B and ran_bands["all_identical"] == [0, 1, 2]
    assert ran_bands["all_disjoint"] == [0, 1, 2] and nms_cases["all_disjoint"][1] < nms_cases["all_disjoint"][2]
    assert len(psc.oracle_keep(*[nms_cases["all_identical"][i] for i in (0, 1, 2, 3)])) == 1


def test_hist_topk_equals_the_oracle():
    S, slack = psc.TOPK_DIRECT_N, psc.TOPK_RANK_SLACK
    seen = {}
    for name, (scores, valid, K) in psc.topk_cases().items():
        want = psc.oracle_order(scores, valid, K)
        order, n, C, span = psc.hist_topk(scores, valid, K)
        assert n == len(want) and np.array_equal(order[:n], want) and (order[n:] == -1).all(), name
        seen[name] = (len(scores), K, n, C, span)
    # ... and the cases are what their names say
    assert [seen["switch_N%d" % N][0] for N in (S - 1, S, S + 1)] == [S - 1, S, S + 1]
    N, K, n, C, _ = seen["k_above_valid"]
    assert N > S and K < N and n < K
    for name in ("all_equal_small_k", "all_equal_bench_n"):
        N, K, n, C, _ = seen[name]
        assert N > S and K < N and C > K + slack + 256 and C >= 0.9 * N, name        # more candidates than the rank grid has rows for
    N, K, n, C, span = seen["wide_spread"]
    assert N > S and K < N and span >= 4096
    N, K, n, C, span = seen["bench_shape"]
    assert (N, K, n) == (21546, 8000, 8000) and K <= C <= K + slack and span < 4096
    N, K, n, C, _ = seen["ties"]
    assert len(np.unique(psc.topk_cases()["ties"][0])) == 16 and C > K
