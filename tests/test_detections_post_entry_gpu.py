"""The post-process option through the detection entry and voc_dets: an engine built with ``post=`` returns, through a plain batched
pass, an annotating pass and voc_dets' eager path, the detections tests/detections_post_ref.py computes from THAT pass's own rois, cls and
reg; the engine without the option stands beside it as a table entry of its own and returns what it always did."""
import numpy as np
import pytest

from tests import detections_post_ref as P
from tests import detections_ref as R
from tests.test_redact_entry_gpu import RESIZE, engine, f32_models, quiet, staged      # noqa: F401  (the synthetic ResNet-50 pair)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POST = ("soft_gaussian", 0.5, 0.5, None, 0.5)
THR = 0.05


@pytest.fixture(scope="module")
def post_engine(f32_models, engine):
    from faster_rcnn_amd import entry
    mgr, det, _ = f32_models
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight("f32"), post=POST)
    assert eng is not engine and eng.post == POST and engine.post is None
    return eng


def case_of(rois, cls, reg, n_live, mapping, ratio, thr, roi_batch):
    return {"name": "pass", "rois": rois.cpu().numpy(), "cls": cls.cpu().numpy(), "reg": reg.cpu().numpy(), "n_live": int(n_live),
            "roi_batch": roi_batch, "bg": mapping["bg"], "thr": float(thr), "ratio": float(ratio), "stride": 16.0, "nms": 0.5}


def check_dets(dets, case, mapping, post, what):
    names = dict((v, k) for k, v in mapping.items())
    if post is None:
        w_cls, w_prob, w_bbox, _, _ = R.run(case)
        assert R.unstable(case) == [], what
    else:
        assert P.unstable_post(case, post) == [], what
        w_cls, w_prob, w_bbox, _, _ = P.run(case, post)
    assert len(dets) == len(w_cls) and len(dets) > 0, (what, len(dets), len(w_cls))
    assert [d["cls_name"] for d in dets] == [names[int(c)] for c in w_cls], what
    assert np.array_equal(np.array([d["bbox"] for d in dets]).reshape(-1, 4), w_bbox), what
    got = np.array([d["prob"] for d in dets], np.float32)
    ulps = np.abs(got.view(np.int32).astype(np.int64) - w_prob.view(np.int32).astype(np.int64))
    assert (ulps <= (0 if post is None or post[0] == "hard" else 1)).all(), (what, int(ulps.max()))


def pass_cases(eng, ticket, B, mapping, ratios, thr):
    from faster_rcnn_amd import entry
    out = ticket.slot.out
    batch = eng.num_rois if entry.PAD_TO_BATCH else 0
    if B == 1 and not isinstance(out["n_rois"], (list, tuple)):
        return [case_of(out["rois"], out["cls"], out["reg"], out["n_rois"].item(), mapping, ratios[0], thr, batch)]
    return [case_of(out["rois"][i], out["cls"][i], out["reg"][i], out["n_rois"][i].item(), mapping, ratios[i], thr, batch) for i in range(B)]


def test_three_paths_and_the_engine_beside(post_engine, engine, f32_models, staged, monkeypatch):
    from faster_rcnn_amd import ops, voc_dets
    mgr, det, _ = f32_models
    mapping = mgr.class_mapping
    srcs, resized, ratios, pixels = staged
    assert len(mgr._entries) >= 2 and sum(e is post_engine or e is engine for e in mgr._entries.values()) == 2
    assert post_engine.stats()["post"] == dict(zip(ops.DET_POST_FIELDS, POST)) and "post" not in engine.stats()
    soft_counts = []
    # 1. a plain batched pass
    t = post_engine.submit_batch(resized[:4], ratios[:4], THR, pixels[:4], batch=4)
    res = post_engine.collect_batch(t)
    for i, (c, r) in enumerate(zip(pass_cases(post_engine, t, 4, mapping, ratios, THR), res)):
        check_dets(r[1], c, mapping, POST, "batched %d" % i)
        soft_counts.append(len(r[1]))
    # 2. an annotating pass
    t = post_engine.submit_batch(resized[:1], ratios[:1], THR, pixels[:1], batch=1, annotate=True)
    res = post_engine.collect_batch(t)
    check_dets(res[0][1], pass_cases(post_engine, t, 1, mapping, ratios, THR)[0], mapping, POST, "annotating")
    assert res[0][2].shape == srcs[0].shape and (res[0][2] != srcs[0]).any()
    # 3. voc_dets' eager path, on the inputs it hands to the op
    seen = []
    real = ops.detections_post

    def recording(rois, n_rois, out_cls, out_reg, roi_batch, bg_idx, det_threshold, stride, resize_ratio, post=None):
        seen.append((rois, n_rois, out_cls, out_reg, roi_batch, det_threshold, resize_ratio, post))
        return real(rois, n_rois, out_cls, out_reg, roi_batch, bg_idx, det_threshold, stride, resize_ratio, post)

    monkeypatch.setattr(ops, "detections_post", recording)
    dets, _ = quiet(voc_dets._get_dets_eager, mgr, det, resized[0], ratios[0], 64, 16, THR, POST)
    assert len(seen) == 1 and seen[0][7] == POST
    rois, n_rois, out_cls, out_reg, _, thr, ratio, _ = seen[0]
    check_dets(dets, case_of(rois, out_cls, out_reg, n_rois.item(), mapping, ratio, thr, 0), mapping, POST, "eager")
    monkeypatch.setattr(ops, "detections_post", real)
    # the engine without the option: the reference's rule on its own pass, as before, and fewer rows than the soft mode keeps
    t = engine.submit_batch(resized[:4], ratios[:4], THR, pixels[:4], batch=4)
    res = engine.collect_batch(t)
    hard_counts = []
    for i, (c, r) in enumerate(zip(pass_cases(engine, t, 4, mapping, ratios, THR), res)):
        check_dets(r[1], c, mapping, None, "plain %d" % i)
        hard_counts.append(len(r[1]))
    assert sum(soft_counts) > sum(hard_counts)
    assert not any("post" in str(k) for k in engine.cache.keys())
