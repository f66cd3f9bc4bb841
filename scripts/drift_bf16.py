#!/usr/bin/env python3
"""BASELINE's "box mAP delta vs ref" for the bf16 configs over MANY frames: the plain fp32 oracle end to end
against the bf16 device end to end on N synthetic frames (default 32; bench.py's own leg uses the 4-8 its cpu_baseline budget
allows and reads 0.09-0.21 from sample to sample), the pair's mAP delta with a bootstrap over frames (resampled with replacement):
mean, standard deviation and the 2.5 / 97.5 percentiles.  Rank 0 prints ONE JSON object; profiles/round5_drift_bf16_*.json are
its outputs, and bench.DRIFT_MAP_BARS / tests/test_configs_full_size_gpu.py take their bound from them.

    python scripts/drift_bf16.py [--config c4|c2] [--frames 32] [--boot 200]
    python scripts/drift_bf16.py --network vgg16 [--frames 4]      # configs[0]'s network: the statistic of bench.e2e_drift_bf16 (no bootstrap)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench


def vgg16(frames):
    """bf16 VGG16 (600x1000, head as drawn) against the plain fp32 oracle end to end on ``frames`` synthetic frames: the share of
    detections paired by class and IoU >= 0.5 and the mean score difference of the pairs (what bench.e2e_drift_bf16 computes for the
    ResNets, held there to bench.DRIFT_BARS_AS_DRAWN), and -- the statistic that is never empty -- the drift of the class probabilities
    and regressions of the proposals both sides kept."""
    from oracle import e2e, np_ref
    from oracle.keras_ref import KerasGraphs
    from faster_rcnn_amd import util, vgg
    from faster_rcnn_amd.pipeline import InferencePipeline
    from faster_rcnn_amd.weights import synthetic_vgg16
    anchors = util.get_anchors([128, 256, 512])
    w = synthetic_vgg16(anchors_per_loc=9, num_classes=21, seed=1)
    rpn = vgg.vgg16_rpn(vgg.vgg16_base(weights=w, dtype="bf16"), include_conv=True, anchors_per_loc=9)
    pipe = InferencePipeline(rpn, vgg.vgg16_classifier(64, 21, weights=w, dtype="bf16"), anchors, max_proposals=300)
    graphs = KerasGraphs(w, torch.float32)
    matched = total = 0
    diffs, cls_d, reg_d, shared = [], [], [], []
    t0 = time.perf_counter()
    for i in range(frames):
        x = vgg.preprocess(np.random.RandomState(1000 + i).randint(0, 256, (1, 600, 1000, 3)))
        with torch.no_grad():
            feat = graphs.vgg_base(x.astype(np.float32))
            cls, reg = graphs.rpn(feat)
            kept = np_ref.proposals(reg.numpy(), cls.numpy(), anchors, 16, 8000, 300)[0]
            o_cls, o_reg = graphs.vgg_classifier(feat, kept.astype(np.float32), 21)
        o_dets = np_ref.detections(kept, o_cls.numpy(), o_reg.numpy(), 20, 1.0)
        out = pipe.forward_dev(torch.from_numpy(x.astype(np.float32)).cuda(), 1.0)
        torch.cuda.synchronize()
        n, nd = int(out["n_rois"].item()), int(out["n_dets"].item())
        d_dets = [(int(c), np.float32(p), b.astype(np.int64)) for c, p, b in zip(out["det_cls"].cpu().numpy()[:nd], out["det_prob"].cpu().numpy()[:nd],
                                                                                 out["det_bbox"].cpu().numpy()[:nd])]
        pairs = e2e.match_detections(o_dets, d_dets, 0.5)
        matched += len(pairs)
        total += max(len(o_dets), len(d_dets))
        diffs += [abs(a - b) for a, b, _ in pairs]
        # the proposals both kept (same box): how far their class probabilities and regressions are apart
        rows = {tuple(r): j for j, r in enumerate(np.asarray(kept, np.float32).tolist())}
        d_rois, d_cls, d_reg = out["rois"].cpu().numpy()[:n], out["cls"].cpu().numpy()[:n], out["reg"].cpu().numpy()[:n]
        both = [(rows[tuple(r)], j) for j, r in enumerate(d_rois.tolist()) if tuple(r) in rows]
        shared.append((len(both), max(len(kept), n)))
        if both:
            oi, di = (np.array(v) for v in zip(*both))
            cls_d.append(np.abs(o_cls.numpy()[oi] - d_cls[di]))
            reg_d.append(np.abs(o_reg.numpy()[oi] - d_reg[di]) / max(float(np.abs(o_reg.numpy()).max()), 1e-30))
    cat = lambda v: np.concatenate([a.ravel() for a in v]) if v else np.zeros(1)
    return {"what": "fp32 oracle end to end vs bf16 device end to end, %d synthetic 600x1000 frames, VGG16, head as drawn" % frames,
            "detections_matched_iou50": "%d/%d" % (matched, total), "matched_frac": round(matched / max(total, 1), 4),
            "matched_score_diff_mean": float("%.3g" % (np.mean(diffs) if diffs else 0.0)), "matched_score_diff_max": float("%.3g" % (max(diffs) if diffs else 0.0)),
            "proposals_identical": "%d/%d" % (sum(a for a, _ in shared), sum(b for _, b in shared)),
            "shared_proposals_class_prob_abs_diff": {"mean": float("%.3g" % cat(cls_d).mean()), "max": float("%.3g" % cat(cls_d).max())},
            "shared_proposals_regression_diff_rel_to_max": {"mean": float("%.3g" % cat(reg_d).mean()), "max": float("%.3g" % cat(reg_d).max())},
            "bars_as_drawn": list(bench.DRIFT_BARS_AS_DRAWN), "wall_s": round(time.perf_counter() - t0, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--network", choices=("resnet", "vgg16"), default="resnet", help="vgg16: configs[0]'s network on the bf16 path (--config is not used)")
    ap.add_argument("--config", choices=("c4", "c2"), default="c4", help="c4: configs[3] (ResNet-101 600x1500 bf16); c2: configs[1] shapes on the bf16 engine")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--boot", type=int, default=200)
    args = ap.parse_args()
    json_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    if args.network == "vgg16":
        json_out.write(json.dumps(vgg16(min(args.frames, 8) if args.frames != 32 else 4)) + "\n")
        json_out.flush()
        return
    bench.select_config(args.config)
    bench.DTYPE = "bf16"
    from oracle import e2e
    from faster_rcnn_amd.data.voc_data_helpers import KITTI_CLASS_MAPPING, VOC_CLASS_MAPPING
    from faster_rcnn_amd.pipeline import InferencePipeline
    pipe, weights, anchors = bench.build_pipeline()
    mapping = VOC_CLASS_MAPPING if bench.NUM_CLASSES == len(VOC_CLASS_MAPPING) else KITTI_CLASS_MAPPING
    runs = []
    t0 = time.perf_counter()
    cpu = bench.cpu_baseline(weights, anchors, budget_s=0.0, runs=runs, min_images=args.frames, alt_dense_class=getattr(pipe, "raw_dense_class", None))
    oracle_s = time.perf_counter() - t0
    one = InferencePipeline(pipe.rpn, pipe.det, anchors, max_proposals=bench.PROPOSALS)
    raw, _ = bench.raw_head_pipeline(pipe, weights, anchors)
    out = {"what": "fp32 oracle end to end vs bf16 device end to end, %d synthetic %dx%d frames, ResNet-%d; bootstrap over frames (%d resamples)"
                   % (len(runs), bench.HEIGHT, bench.WIDTH, bench.DEPTH, args.boot),
           "oracle": cpu, "oracle_wall_s": round(oracle_s, 1)}
    rs = np.random.RandomState(0)
    for tag, p, col in (("head_calibrated", one, 2), ("head_as_drawn", raw, 3)):
        if p is None or any(len(r) <= col for r in runs):
            continue
        items = [{"name": "synth%03d" % r[0], "size": (bench.WIDTH, bench.HEIGHT), "oracle": (r[1], r[col]), "device": e2e.device_detect(p, bench.synth_image(r[0]))}
                 for r in runs]
        full = e2e.compare(items, mapping)
        m, t = (int(v) for v in full["detections_matched_iou50"].split("/"))
        deltas, per_frame = [], []
        for it in items:                                        # frame by frame: how far one frame's pair is apart on the same metric
            per_frame.append(e2e.compare([it], mapping)["map_pair_delta"])
        for _ in range(args.boot):
            pick = rs.randint(0, len(items), len(items))
            sub = [dict(items[i], name="%s_%02d" % (items[i]["name"], k)) for k, i in enumerate(pick)]       # (duplicates need distinct file names)
            deltas.append(e2e.compare(sub, mapping)["map_pair_delta"])
        d = np.asarray(deltas)
        out[tag] = {"map_pair_delta_all_frames": full["map_pair_delta"], "map_pseudo_gt": full.get("map_pseudo_gt"),
                    "matched_frac": round(m / max(t, 1), 4), "matched_score_diff": full["matched_score_diff"], "proposals_identical": full["proposals_identical"],
                    "bootstrap": {"mean": round(float(d.mean()), 4), "std": round(float(d.std()), 4),
                                  "p2.5": round(float(np.percentile(d, 2.5)), 4), "p97.5": round(float(np.percentile(d, 97.5)), 4), "max": round(float(d.max()), 4)},
                    "single_frame_deltas": {"mean": round(float(np.mean(per_frame)), 4), "max": round(float(np.max(per_frame)), 4)}}
    json_out.write(json.dumps(out) + "\n")
    json_out.flush()


if __name__ == "__main__":
    main()
