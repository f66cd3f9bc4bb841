"""GPU parity of the proposal selection (csrc/sort_nms.hip) where its launches changed shape: the NMS mask built and scanned in
bands of row blocks with the scan's state handed on in the workspace, and the top-K's histogram form with a rank grid sized for
about K candidates.  Every comparison is exact, against oracle/np_ref on the cases of tests/proposal_select_cases.py (which
tests/test_proposal_select_cpu.py holds to what their names say), and against the library's own one-band / no-histogram form."""
import numpy as np
import pytest

from tests import proposal_select_cases as psc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ops():
    from faster_rcnn_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dirty(*nbytes):
    """Stale non-zero bytes in the caching allocator's free blocks of these sizes: the calls define every output slot themselves."""
    keep = [torch.full((max(int(n), 1),), 0x5A, dtype=torch.uint8, device="cuda") for n in nbytes]
    torch.cuda.synchronize()
    del keep


# ------------------------------------------------------------------------------------------------ NMS
_NMS = {}


def nms_case(dtype, name):
    """(boxes, n, max_boxes, thresh, stop, the oracle's keep): built once per dtype, shared and left unchanged."""
    if dtype not in _NMS:
        _NMS[dtype] = {k: v + (psc.oracle_keep(*v[:4]),) for k, v in psc.nms_cases(dtype).items()}
    return _NMS[dtype][name]


NMS_NAMES = sorted(psc.nms_cases(np.int16))


@pytest.mark.parametrize("dtype", [np.int16, np.float64], ids=["i16", "f64"])
@pytest.mark.parametrize("name", NMS_NAMES)
def test_banded_nms(ops, dtype, name):
    boxes, n, max_boxes, thresh, stop, want = nms_case(dtype, name)
    K = len(boxes)
    dirty(max_boxes * 4, 4, ops._lib.load().frcnn_nms_workspace_bytes(K))
    keep, n_keep = ops.nms_sorted(dev(boxes), dev(np.array([n], np.int32)), thresh, max_boxes)
    keep, nk = keep.cpu().numpy(), int(n_keep.item())
    assert nk == len(want)
    assert np.array_equal(keep[:nk], want)
    assert (keep[nk:] == -1).all()
    if K > psc.B:
        # the one-band form (K <= the first band: the launches the library always had) on the leading candidates keeps the same ones
        head, n_head = ops.nms_sorted(dev(boxes[:psc.B]), dev(np.array([min(n, psc.B)], np.int32)), thresh, max_boxes)
        head = head.cpu().numpy()[:int(n_head.item())]
        assert np.array_equal(head, keep[:nk][keep[:nk] < psc.B])


@pytest.mark.parametrize("dtype", [np.int16, np.float64], ids=["i16", "f64"])
def test_banded_nms_shares_a_workspace_in_a_replayed_graph(ops, dtype):
    """Two different inputs through ONE workspace back to back inside a captured graph, replayed twice: the first stops inside
    band 1 (done set early, a bitmap handed on once), the second runs every band.  A `done` word or bitmap left over from the
    call or the replay before would change what either keeps."""
    from faster_rcnn_amd import _lib
    a = nms_case(dtype, "stop_first_row_of_band1")
    b = nms_case(dtype, "all_disjoint")
    K = len(a[0])
    assert len(b[0]) == K
    name = {np.int16: "frcnn_nms_i16", np.float64: "frcnn_nms_f64"}[dtype]
    ws = torch.empty(_lib.load().frcnn_nms_workspace_bytes(K), dtype=torch.uint8, device="cuda")
    ins = [(dev(c[0]), dev(np.array([c[1]], np.int32)), c[3], c[2]) for c in (a, b)]
    outs = [(torch.empty(c[2], dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")) for c in (a, b)]

    def both():
        for (boxes, n, thresh, max_boxes), (keep, n_keep) in zip(ins, outs):
            _lib.call(name, boxes.data_ptr(), n.data_ptr(), K, float(thresh), int(max_boxes), keep.data_ptr(), n_keep.data_ptr(),
                      ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        both()
    for _ in range(2):
        for keep, n_keep in outs:
            keep.fill_(0x5A5A5A5A)
            n_keep.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        for c, (keep, n_keep) in zip((a, b), outs):
            want = c[5]
            keep, nk = keep.cpu().numpy(), int(n_keep.item())
            assert nk == len(want) and np.array_equal(keep[:nk], want) and (keep[nk:] == -1).all()


# ------------------------------------------------------------------------------------------------ top-K
_TOPK = {}


def topk_case(name):
    if not _TOPK:
        _TOPK.update({k: v + (psc.oracle_order(*v),) for k, v in psc.topk_cases().items()})
    return _TOPK[name]


@pytest.mark.parametrize("name", sorted(psc.topk_cases()))
def test_topk_histogram_form(ops, name):
    scores, valid, K, want = topk_case(name)
    N = len(scores)
    s, v = dev(scores), None if valid is None else dev(valid.astype(np.uint8))
    dirty(K * 4, 4, ops._lib.load().frcnn_topk_workspace_bytes(N))
    order, n = ops.topk_order(s, v, K)
    order, n = order.cpu().numpy(), int(n.item())
    assert n == len(want)
    assert np.array_equal(order[:n], want)
    assert (order[n:] == -1).all()
    # K = N makes every valid score a candidate with no histogram in front (the form small inputs always took): same leading entries
    full, n_full = ops.topk_order(s, v, N)
    assert int(n_full.item()) == (N if valid is None else int(valid.sum()))
    assert np.array_equal(full.cpu().numpy()[:n], order[:n])
