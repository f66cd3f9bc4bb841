"""GPU parity of the detection post-process (k_detections, csrc/detect.hip) through both C entry points against the plain
reference of tests/detections_ref.py, on the generated cases of tests/detections_cases.py (docs/DETECTIONS_PARITY.md).
Everything is compared exactly: classes, f32 score bits, integer boxes, RoI indices, counts and the empty rows."""
import numpy as np
import pytest

from tests import detections_cases as K
from tests import detections_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = K.all_cases()
FILL = 0x7f7f7f7f
E_ARG = -1                                                    # FRCNN_E_ARG (include/frcnn_hip.h)


@pytest.fixture(scope="module")
def ops():
    from faster_rcnn_amd import ops as o
    return o


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def upload(c):
    return {"rois": dev(c["rois"]), "cls": dev(c["cls"]), "reg": dev(c["reg"]), "n": dev(np.array([c["n_live"]], np.int32)),
            "dyn": dev(np.array([c["ratio"], c["thr"]], np.float64))}


def raw(ops, c, d, form, batch=0):
    """The C entry itself on an output buffer pre-filled with 0x7f bytes -> the packed words on the host."""
    from faster_rcnn_amd import _lib
    rows, C = c["cls"].shape
    packed = torch.full((4 + 7 * rows,), FILL, dtype=torch.int32, device="cuda")
    n_dets, bbox, cls, prob, roi = ops.split_detections(packed, rows)
    p = lambda t: t.data_ptr()
    if form == "static":
        _lib.call("frcnn_detections", p(d["rois"]), p(d["n"]), rows, p(d["cls"]), p(d["reg"]), C, c["bg"], c["thr"], c["stride"], c["ratio"],
                  c["nms"], p(cls), p(prob), p(bbox), p(roi), p(n_dets), ops._stream())
    else:
        _lib.call("frcnn_detections_dyn", p(d["rois"]), p(d["n"]), batch, rows, p(d["cls"]), p(d["reg"]), C, c["bg"], c["stride"], c["nms"],
                  p(d["dyn"]), p(cls), p(prob), p(bbox), p(roi), p(packed), ops._stream())
    return packed.cpu()


def check_packed(ops, packed, want, c, form, what):
    """One packed buffer against the reference: the count words, the nd detections, and every row at and past nd empty."""
    w_cls, w_prob, w_bbox, w_roi, _ = want
    rows = len(c["cls"])
    n_dets, bbox, cls, prob, roi = (t.numpy() for t in ops.split_detections(packed, rows))
    nd = int(n_dets[0])
    head = packed[:4].tolist()
    assert nd == len(w_cls), (what, nd, len(w_cls))
    if form == "static":
        assert head[1:] == [FILL] * 3, what                   # the three pad words are not the kernel's
    elif form == "dyn":
        assert head[1:] == [c["n_live"], FILL, FILL], what    # counts[1]: the live rows, whatever was scored
    assert np.array_equal(cls[:nd], w_cls), what
    assert prob[:nd].tobytes() == w_prob.tobytes(), what
    assert np.array_equal(bbox[:nd], w_bbox), what
    assert np.array_equal(roi[:nd], w_roi), what
    assert (cls[nd:] == -1).all() and (roi[nd:] == -1).all() and not bbox[nd:].any(), what
    assert prob[nd:].tobytes() == bytes(4 * (rows - nd)), what                # +0.0, not -0.0


def check_case(ops, c):
    d = upload(c)
    rows = len(c["cls"])
    want = R.run(c, 0)
    st = raw(ops, c, d, "static")
    check_packed(ops, st, want, c, "static", c["name"] + " static")
    dy = raw(ops, c, d, "dyn", 0)
    check_packed(ops, dy, want, c, "dyn", c["name"] + " dyn batch 0")
    assert torch.equal(dy[4:], st[4:]) and dy[0] == st[0]
    # the bindings (torch.empty outputs) give the same words
    o1 = ops.detections(d["rois"], d["n"], d["cls"], d["reg"], 64, c["bg"], c["thr"], c["stride"], c["ratio"], c["nms"])
    o2 = ops.detections_dyn(d["rois"], d["n"], d["cls"], d["reg"], 0, c["bg"], c["stride"], d["dyn"], c["nms"])
    for o in (o1, o2):
        got = o["det_packed"].cpu()
        assert torch.equal(got[4:], st[4:]) and got[0] == st[0], c["name"]
        for k, v in zip(("n_dets", "det_bbox", "det_cls", "det_prob", "det_roi"), ops.split_detections(o["det_packed"], rows)):
            assert o[k].data_ptr() == v.data_ptr() and o[k].shape == v.shape
    assert o2["det_packed"][1].item() == c["n_live"]
    if c["roi_batch"]:
        want_b = R.run(c)
        db = raw(ops, c, d, "dyn", c["roi_batch"])
        check_packed(ops, db, want_b, c, "dyn", c["name"] + " dyn batch %d" % c["roi_batch"])
        o3 = ops.detections_dyn(d["rois"], d["n"], d["cls"], d["reg"], c["roi_batch"], c["bg"], c["stride"], d["dyn"], c["nms"])
        assert torch.equal(o3["det_packed"].cpu()[:2], db[:2]) and torch.equal(o3["det_packed"].cpu()[4:], db[4:])
    return st


@pytest.mark.parametrize("name", K.names("sizes"))
def test_sizes(ops, name):
    check_case(ops, CASES[name])


@pytest.mark.parametrize("name", K.names("cross_word"))
def test_cross_word_suppression(ops, name):
    check_case(ops, CASES[name])


@pytest.mark.parametrize("name", K.names("nms_edge"))
def test_nms_threshold_edge(ops, name):
    check_case(ops, CASES[name])


@pytest.mark.parametrize("name", K.names("ties"))
def test_ranking_ties(ops, name):
    check_case(ops, CASES[name])


@pytest.mark.parametrize("name", K.names("classes"))
def test_argmax_and_classes(ops, name):
    check_case(ops, CASES[name])


@pytest.mark.parametrize("name", K.names("threshold"))
def test_score_threshold(ops, name):
    st = check_case(ops, CASES[name])
    if name == "thr_above_all":
        assert st[0] == 0 and (st[4 + 4 * 60:4 + 5 * 60] == -1).all()


@pytest.mark.parametrize("name", K.names("rounding"))
def test_rounding(ops, name):
    check_case(ops, CASES[name])


@pytest.mark.parametrize("name", K.names("decode"))
def test_decode(ops, name):
    check_case(ops, CASES[name])


@pytest.mark.parametrize("name", K.names("dyn"))
def test_dyn_counts_and_clamps(ops, name):
    """check_case runs the case's own roi_batch beside batch 0 and the static entry (which scores min(n_live, rows) rows); the rows
    behind what is scored hold a winning score and NaN deltas."""
    check_case(ops, CASES[name])


def test_values_from_device_memory(ops):
    """One dyn tensor rewritten in place between calls: each call reads the pair that is there when it runs."""
    c = dict(CASES["decode_fuzz_s16"])
    d = upload(c)
    seen = set()
    for ratio, thr in ((1.0, 0.0), (1.6, 0.5), (0.625, float(np.float32(0.9)))):
        d["dyn"].copy_(dev(np.array([ratio, thr], np.float64)))
        c["ratio"], c["thr"] = ratio, thr
        assert R.unstable(c) == []
        got = ops.detections_dyn(d["rois"], d["n"], d["cls"], d["reg"], 0, c["bg"], c["stride"], d["dyn"], c["nms"])
        st = ops.detections(d["rois"], d["n"], d["cls"], d["reg"], 64, c["bg"], thr, c["stride"], ratio, c["nms"])
        assert torch.equal(got["det_packed"][4:], st["det_packed"][4:]) and torch.equal(got["n_dets"], st["n_dets"])
        check_packed(ops, got["det_packed"].cpu(), R.run(c), c, "any", "dyn values %g %g" % (ratio, thr))
        seen.add(int(got["n_dets"].item()))
    assert len(seen) == 3                                     # the three pairs really give three answers


def test_graph_replay(ops):
    """One captured frcnn_detections_dyn (a single stream, one kernel node) replayed after dyn, n_live and the inputs were rewritten in
    place: every replay equals the eager call and the reference."""
    a, b = CASES["dyn_live_300"], CASES["dyn_live_65"]
    c = dict(a)
    d = upload(c)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.detections_dyn(d["rois"], d["n"], d["cls"], d["reg"], 64, c["bg"], c["stride"], d["dyn"], c["nms"])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        out = ops.detections_dyn(d["rois"], d["n"], d["cls"], d["reg"], 64, c["bg"], c["stride"], d["dyn"], c["nms"])
    # (inputs, ratio, threshold, n_live): live counts at or under the inputs' own, so the poison stays behind what is scored
    steps = [(a, 1.6, 0.0, 300), (b, 0.625, 0.3, 65), (b, 1.0, 0.3, 1), (a, 1.6, 0.0, 256), (a, 2.0, 0.6, 0)]
    for src, ratio, thr, n_live in steps:
        c = dict(src, ratio=ratio, thr=thr, n_live=n_live)
        assert R.unstable(c) == [] and not np.isnan(c["reg"][:R.n_scored(n_live, 64, 512)]).any()
        d["rois"].copy_(dev(c["rois"])); d["cls"].copy_(dev(c["cls"])); d["reg"].copy_(dev(c["reg"]))
        d["n"].copy_(dev(np.array([n_live], np.int32))); d["dyn"].copy_(dev(np.array([ratio, thr], np.float64)))
        out["det_packed"].fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        replayed = out["det_packed"].cpu()
        eager = ops.detections_dyn(d["rois"], d["n"], d["cls"], d["reg"], 64, c["bg"], c["stride"], d["dyn"], c["nms"])["det_packed"].cpu()
        assert torch.equal(replayed[:2], eager[:2]) and torch.equal(replayed[4:], eager[4:])
        check_packed(ops, replayed, R.run(c), c, "dyn", "replay n_live %d" % n_live)


def test_deterministic(ops):
    c = CASES["size_512_c21"]
    d = upload(c)
    first = raw(ops, c, d, "dyn", 0)
    again = raw(ops, c, d, "dyn", 0)
    assert first[0] == again[0] and torch.equal(first[4:], again[4:])


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
    # frcnn_detections(rois, n_rois, max_rows, out_cls, out_reg, C, bg, thr, stride, ratio, nms, cls, prob, bbox, roi, n_dets, stream)
    good_s = [p(d["rois"]), p(d["n"]), rows, p(d["cls"]), p(d["reg"]), C, c["bg"], c["thr"], c["stride"], c["ratio"], c["nms"],
              p(cls), p(prob), p(bbox), p(roi), p(n_dets), ops._stream()]
    # frcnn_detections_dyn(rois, n_rois, roi_batch, max_rows, out_cls, out_reg, C, bg, stride, nms, dyn, cls, prob, bbox, roi, counts, stream)
    good_d = [p(d["rois"]), p(d["n"]), 64, rows, p(d["cls"]), p(d["reg"]), C, c["bg"], c["stride"], c["nms"], p(d["dyn"]),
              p(cls), p(prob), p(bbox), p(roi), p(packed), ops._stream()]
    bad = []
    for fn, good, i_rows, i_C, ptrs in (("frcnn_detections", good_s, 2, 5, (0, 1, 3, 4, 11, 12, 13, 14, 15)),
                                        ("frcnn_detections_dyn", good_d, 3, 6, (0, 1, 4, 5, 10, 11, 12, 13, 14, 15))):
        for i, v in [(i_rows, 0), (i_rows, 513), (i_rows, -1), (i_C, 1), (i_C, 129)] + [(i, None) for i in ptrs]:
            bad.append((fn, good[:i] + [v] + good[i + 1:], "arg %d = %r" % (i, v)))
    bad.append(("frcnn_detections_dyn", good_d[:2] + [-1] + good_d[3:], "roi_batch -1"))
    bad.append(("frcnn_detections_dyn", good_d[:10] + [p(d["dyn"]) + 4] + good_d[11:], "dyn 4 bytes off"))
    for fn, args, what in bad:
        assert getattr(lib, fn)(*args) == E_ARG, (fn, what)
        with pytest.raises(_lib.FrcnnError):
            _lib.call(fn, *args)
    torch.cuda.synchronize()
    assert (packed.cpu() == FILL).all()
    # the accepted neighbours then run: max_rows 1 and 512 are inside the range, as are 2 and 128 classes (test_argmax_and_classes)
    assert getattr(lib, "frcnn_detections")(*good_s) == 0 and getattr(lib, "frcnn_detections_dyn")(*good_d) == 0
    torch.cuda.synchronize()
    assert int(packed[0].item()) == len(R.run(c, 64)[0])
