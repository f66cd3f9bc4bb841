"""GPU parity of the post-process extension (k_detections_post, csrc/detect_post.hip; include/ext/frcnn_hip_detect_post.h) through both C
entry points against tests/detections_post_ref.py, on all 74 cases of tests/detections_cases.py under the six parameter sets of
``detections_post_ref.GPU_POSTS`` (tests/test_detections_post_ref_cpu.py holds the condition that none of them leaves a decision open).

Classes, integer boxes, RoI indices, counts, order and the empty rows are compared exactly.  det_prob is exact in the hard mode, and in
the linear mode on the cases whose scored ``reg`` rows are all zero (no transcendental anywhere); elsewhere in the soft modes it lies
within one f32 ulp: a box that feeds an IoU, or the gaussian weight itself, may differ from numpy's in the last f64 bit through ``exp``.
The hard mode without voting equals frcnn_detections / frcnn_detections_dyn on the same buffers, whole packed buffer."""
import numpy as np
import pytest

from tests import detections_cases as K
from tests import detections_post_ref as P
from tests import detections_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = K.all_cases()
FILL = 0x7f7f7f7f
E_ARG = -1                                                    # FRCNN_E_ARG (include/frcnn_hip.h)
_WANT = {}


@pytest.fixture(scope="module")
def ops():
    from faster_rcnn_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def upload(c):
    return {"rois": dev(c["rois"]), "cls": dev(c["cls"]), "reg": dev(c["reg"]), "n": dev(np.array([c["n_live"]], np.int32)),
            "dyn": dev(np.array([c["ratio"], c["thr"]], np.float64))}


def want_for(pname, c, batch):
    key = (pname, c["name"], batch)
    if key not in _WANT:
        _WANT[key] = P.run(c, P.gpu_post(pname, c), batch)
    return _WANT[key]


def extra(ops, post):
    mode, nt, sigma, min_score, vote = ops.det_post_option(post)
    return nt, [ops.DET_POST_MODES.index(mode), sigma, -1.0 if min_score is None else min_score, 0.0 if vote is None else vote]


def raw(ops, c, d, form, post, batch=0, fn_post=True):
    """The C entry itself on an output buffer pre-filled with 0x7f bytes -> the packed words on the host."""
    from faster_rcnn_amd import _lib
    rows, C = c["cls"].shape
    packed = torch.full((4 + 7 * rows,), FILL, dtype=torch.int32, device="cuda")
    n_dets, bbox, cls, prob, roi = ops.split_detections(packed, rows)
    p = lambda t: t.data_ptr()
    nt, ex = extra(ops, post)
    ex = ex if fn_post else []
    suffix = "_post" if fn_post else ""
    if form == "static":
        _lib.call("frcnn_detections" + suffix, p(d["rois"]), p(d["n"]), rows, p(d["cls"]), p(d["reg"]), C, c["bg"], c["thr"], c["stride"],
                  c["ratio"], nt, p(cls), p(prob), p(bbox), p(roi), p(n_dets), *ex, ops._stream())
    else:
        _lib.call("frcnn_detections%s_dyn" % suffix, p(d["rois"]), p(d["n"]), batch, rows, p(d["cls"]), p(d["reg"]), C, c["bg"], c["stride"],
                  nt, p(d["dyn"]), p(cls), p(prob), p(bbox), p(roi), p(packed), *ex, ops._stream())
    return packed.cpu()


def check_packed(ops, packed, want, c, form, what, exact_prob):
    w_cls, w_prob, w_bbox, w_roi, _ = want
    rows = len(c["cls"])
    n_dets, bbox, cls, prob, roi = (t.numpy() for t in ops.split_detections(packed, rows))
    nd = int(n_dets[0])
    head = packed[:4].tolist()
    assert nd == len(w_cls), (what, nd, len(w_cls))
    if form == "static":
        assert head[1:] == [FILL] * 3, what
    elif form == "dyn":
        assert head[1:] == [c["n_live"], FILL, FILL], what
    assert np.array_equal(cls[:nd], w_cls), what
    assert np.array_equal(roi[:nd], w_roi), what                              # the rows and their order
    assert np.array_equal(bbox[:nd], w_bbox), what
    if exact_prob:
        assert prob[:nd].tobytes() == w_prob.tobytes(), what
    else:
        ulps = np.abs(prob[:nd].view(np.int32).astype(np.int64) - w_prob.view(np.int32).astype(np.int64))
        print(what, "max det_prob ulps", int(ulps.max()) if nd else 0)
        assert (ulps <= 1).all() and (np.sign(prob[:nd]) == np.sign(w_prob)).all(), (what, int(ulps.max()))
    assert (cls[nd:] == -1).all() and (roi[nd:] == -1).all() and not bbox[nd:].any(), what
    assert prob[nd:].tobytes() == bytes(4 * (rows - nd)), what                # +0.0, not -0.0


def check_case(ops, pname, c):
    post = P.gpu_post(pname, c)
    d = upload(c)
    rows = len(c["cls"])
    mode = post[0]
    batches = (0, c["roi_batch"]) if c["roi_batch"] else (0,)
    for batch in batches:
        ns = R.n_scored(c["n_live"], batch, rows)
        exact = mode == "hard" or (mode == "soft_linear" and not np.asarray(c["reg"])[:ns].any())
        want = want_for(pname, c, batch)
        dy = raw(ops, c, d, "dyn", post, batch)
        check_packed(ops, dy, want, c, "dyn", "%s %s dyn batch %d" % (pname, c["name"], batch), exact)
        o = ops.detections_post_dyn(d["rois"], d["n"], d["cls"], d["reg"], batch, c["bg"], c["stride"], d["dyn"], post)
        got = o["det_packed"].cpu()
        assert torch.equal(got[:2], dy[:2]) and torch.equal(got[4:], dy[4:])
        if batch == 0:
            st = raw(ops, c, d, "static", post)
            check_packed(ops, st, want, c, "static", "%s %s static" % (pname, c["name"]), exact)
            assert torch.equal(dy[4:], st[4:]) and dy[0] == st[0]
            o = ops.detections_post(d["rois"], d["n"], d["cls"], d["reg"], 64, c["bg"], c["thr"], c["stride"], c["ratio"], post)
            got = o["det_packed"].cpu()
            assert got[0] == st[0] and torch.equal(got[4:], st[4:])
            for k, v in zip(("n_dets", "det_bbox", "det_cls", "det_prob", "det_roi"), ops.split_detections(o["det_packed"], rows)):
                assert o[k].data_ptr() == v.data_ptr() and o[k].shape == v.shape
        if pname == "hard":                                                   # the existing entry points, byte for byte
            old = raw(ops, c, d, "dyn", post, batch, fn_post=False)
            assert torch.equal(old, dy), c["name"]
            if batch == 0:
                assert torch.equal(raw(ops, c, d, "static", post, fn_post=False), st), c["name"]
                b1 = ops.detections(d["rois"], d["n"], d["cls"], d["reg"], 64, c["bg"], c["thr"], c["stride"], c["ratio"], c["nms"])
                assert b1["det_packed"][0].item() == st[0] and torch.equal(b1["det_packed"].cpu()[4:], st[4:])
            b2 = ops.detections_dyn(d["rois"], d["n"], d["cls"], d["reg"], batch, c["bg"], c["stride"], d["dyn"], c["nms"])
            assert torch.equal(b2["det_packed"].cpu()[:2], dy[:2]) and torch.equal(b2["det_packed"].cpu()[4:], dy[4:])


@pytest.mark.parametrize("name", K.names())
@pytest.mark.parametrize("pname", list(P.GPU_POSTS))
def test_parity(ops, pname, name):
    check_case(ops, pname, CASES[name])


def test_every_case_runs():
    assert len(K.names()) == 74 and {"size_512_c2", "chain", "tie_all_512", "late_killers"} <= set(K.names())
    assert any(c["cls"].shape[1] == 128 for c in CASES.values())


def test_modes_differ(ops):
    """The parameter sets are not one answer five times: on a crowded case the soft modes emit more rows than the hard one, and voting
    moves boxes."""
    c = CASES["size_320_c21"]
    d = upload(c)
    out = {}
    for pname in P.GPU_POSTS:
        o = ops.detections_post_dyn(d["rois"], d["n"], d["cls"], d["reg"], 0, c["bg"], c["stride"], d["dyn"], P.gpu_post(pname, c))
        out[pname] = (int(o["n_dets"].item()), o["det_bbox"].cpu())
    assert out["soft_gaussian"][0] > out["hard"][0] and out["soft_linear"][0] > out["hard"][0]
    assert out["hard_vote"][0] == out["hard"][0] and not torch.equal(out["hard_vote"][1], out["hard"][1])


def test_graph_replay(ops):
    """One captured frcnn_detections_post_dyn replayed after dyn, n_live and the inputs were rewritten in place: no allocation, no host
    read, min_score taken from dyn[1] on the device."""
    post = P.GPU_POSTS["soft_linear_vote"]
    a, b = CASES["dyn_live_300"], CASES["dyn_live_65"]
    c = dict(a)
    d = upload(c)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.detections_post_dyn(d["rois"], d["n"], d["cls"], d["reg"], 64, c["bg"], c["stride"], d["dyn"], post)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        out = ops.detections_post_dyn(d["rois"], d["n"], d["cls"], d["reg"], 64, c["bg"], c["stride"], d["dyn"], post)
    for src, ratio, thr, n_live in [(a, 1.6, 0.0, 300), (b, 0.625, 0.3, 65), (a, 2.0, 0.6, 0)]:
        c = dict(src, ratio=ratio, thr=thr, n_live=n_live, roi_batch=64)
        assert P.unstable_post(c, post) == []
        d["rois"].copy_(dev(c["rois"])); d["cls"].copy_(dev(c["cls"])); d["reg"].copy_(dev(c["reg"]))
        d["n"].copy_(dev(np.array([n_live], np.int32))); d["dyn"].copy_(dev(np.array([ratio, thr], np.float64)))
        out["det_packed"].fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        check_packed(ops, out["det_packed"].cpu(), P.run(c, post), c, "dyn", "replay n_live %d" % n_live, False)


def test_refusals(ops):
    """Every argument check returns FRCNN_E_ARG before anything is launched: the pre-filled outputs keep their bytes."""
    from faster_rcnn_amd import _lib
    lib = _lib.load()
    c = CASES["size_64_c21"]
    d = upload(c)
    rows, C = c["cls"].shape
    packed = torch.full((4 + 7 * rows,), FILL, dtype=torch.int32, device="cuda")
    n_dets, bbox, cls, prob, roi = ops.split_detections(packed, rows)
    p = lambda t: t.data_ptr()
    tail = [2, 0.5, -1.0, 0.5, ops._stream()]
    good_s = [p(d["rois"]), p(d["n"]), rows, p(d["cls"]), p(d["reg"]), C, c["bg"], c["thr"], c["stride"], c["ratio"], c["nms"],
              p(cls), p(prob), p(bbox), p(roi), p(n_dets)] + tail
    good_d = [p(d["rois"]), p(d["n"]), 64, rows, p(d["cls"]), p(d["reg"]), C, c["bg"], c["stride"], c["nms"], p(d["dyn"]),
              p(cls), p(prob), p(bbox), p(roi), p(packed)] + tail
    bad = []
    for fn, good, i_rows, i_C, i_nt, ptrs in (("frcnn_detections_post", good_s, 2, 5, 10, (0, 1, 3, 4, 11, 12, 13, 14, 15)),
                                              ("frcnn_detections_post_dyn", good_d, 3, 6, 9, (0, 1, 4, 5, 10, 11, 12, 13, 14, 15))):
        changes = [(i_rows, 0), (i_rows, 513), (i_C, 1), (i_C, 129), (i_nt, -0.1), (i_nt, 1.5), (i_nt, float("nan"))]
        changes += [(16, -1), (16, 3), (17, 0.0), (17, -0.5), (17, float("inf")), (17, float("nan")), (18, 1.5), (18, float("nan")),
                    (19, 1.5), (19, -0.5), (19, float("nan"))]
        for i, v in changes + [(i, None) for i in ptrs]:
            bad.append((fn, good[:i] + [v] + good[i + 1:], "arg %d = %r" % (i, v)))
    bad.append(("frcnn_detections_post_dyn", good_d[:2] + [-1] + good_d[3:], "roi_batch -1"))
    bad.append(("frcnn_detections_post_dyn", good_d[:10] + [p(d["dyn"]) + 4] + good_d[11:], "dyn 4 bytes off"))
    for fn, args, what in bad:
        assert getattr(lib, fn)(*args) == E_ARG, (fn, what)
        with pytest.raises(_lib.FrcnnError):
            _lib.call(fn, *args)
    torch.cuda.synchronize()
    assert (packed.cpu() == FILL).all()
    for bad_post in (("soft",), ("hard", None, 0.0), ("hard", None, None, None, 1.5)):
        with pytest.raises(ValueError):
            ops.detections_post(d["rois"], d["n"], d["cls"], d["reg"], 64, c["bg"], c["thr"], c["stride"], c["ratio"], bad_post)
    assert (packed.cpu() == FILL).all()
    assert getattr(lib, "frcnn_detections_post")(*good_s) == 0 and getattr(lib, "frcnn_detections_post_dyn")(*good_d) == 0
    torch.cuda.synchronize()
    assert int(packed[0].item()) == len(P.run(c, ("soft_gaussian", c["nms"], 0.5, None, 0.5), 64)[0])
