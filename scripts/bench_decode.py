"""Host-decode against device-decode legs of voc_dets.get_dets_by_cls from JPEG files, alternating within each repetition.

    python scripts/bench_decode.py [--images 64] [--reps 5] [--file tests/golden/VOC_test/JPEGImages/000005.jpg]
    python scripts/bench_decode.py --op-only [--iters 200]      # only ops.jpeg_decode_u8 in a loop: the target of
    rocprofv3 --kernel-trace --stats -- python scripts/bench_decode.py --op-only      # (counters, if any, in a run of their own)

The list is ``--images`` Image objects over ONE file (one geometry: the captured, batched path), so the two legs differ in who decodes
and in what crosses the link (the file's bytes against the decoded frame).  The models are the small synthetic ResNet-50 of the tests:
the figure is a ratio of the two legs on the same passes, not a headline rate.  Prints one JSON line."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def models():
    import numpy as np
    import torch
    from faster_rcnn_amd import resnet, util
    from faster_rcnn_amd.data.voc_data_helpers import VOC_CLASS_MAPPING
    from faster_rcnn_amd.det_util import DetTrainingManager
    from faster_rcnn_amd.pipeline import InferencePipeline
    from faster_rcnn_amd.weights import calibrate_classifier, synthetic_resnet
    anchors = util.get_anchors([128, 256, 512])
    w = synthetic_resnet(50, anchors_per_loc=9, num_classes=21, seed=1)
    rpn = resnet.resnet50_rpn(resnet.resnet50_base(weights=w), include_conv=True, anchors_per_loc=9)
    det = resnet.resnet50_classifier(64, 21, weights=w)
    x = resnet.preprocess(np.random.RandomState(99).randint(0, 256, (320, 480, 3)).astype(np.uint8))[None].astype(np.float32)
    out = InferencePipeline(rpn, det, anchors).forward_dev(torch.from_numpy(x).cuda())
    n = int(out["n_rois"].item())
    det.get_layer("dense_class_21").set_weights(calibrate_classifier(w, 21, out["cls"][:n].cpu().numpy()))
    mgr = DetTrainingManager(rpn_model=rpn, class_mapping=VOC_CLASS_MAPPING, preprocess_func=resnet.preprocess, anchor_dims=anchors)
    return mgr, det


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--file", default=os.path.join(ROOT, "tests", "golden", "VOC_test", "JPEGImages", "000005.jpg"))
    p.add_argument("--images", type=int, default=64)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--op-only", dest="op_only", action="store_true")
    p.add_argument("--iters", type=int, default=200)
    args = p.parse_args()
    import torch
    from faster_rcnn_amd import entry, ops, shapes, util, voc_dets
    data = open(args.file, "rb").read()
    plan = ops.jpeg_dec_plan(data)
    if args.op_only:
        file_dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        ws = torch.empty(ops.jpeg_dec_workspace_bytes(plan), dtype=torch.uint8, device="cuda")
        out = torch.empty((plan.h, plan.w, 3), dtype=torch.uint8, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        for _ in range(10):
            ops.jpeg_decode_u8(file_dev, plan, out=out, status=status, workspace=ws)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            ops.jpeg_decode_u8(file_dev, plan, out=out, status=status, workspace=ws)
        torch.cuda.synchronize()
        print(json.dumps({"op": "jpeg_decode_u8", "file_bytes": len(data), "h": plan.h, "w": plan.w, "iters": args.iters,
                          "ms_per_file": round(1e3 * (time.perf_counter() - t0) / args.iters, 4), "status": int(status.item())}))
        return
    mgr, det = models()
    images = [shapes.Image(shapes.Metadata("i%d" % i, plan.w, plan.h, [], args.file)) for i in range(args.images)]
    resized, ratios = util.resize_imgs(images, min_size=600, max_size=1000)
    legs = {"host": [], "device": []}

    def run(decoder):
        entry.set_jpeg_decoder(decoder)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            voc_dets.get_dets_by_cls(mgr, det, ratios, resized, det_threshold=0.1)
        torch.cuda.synchronize()
        return len(images) / (time.perf_counter() - t0)

    for decoder in legs:                                    # captures and warm-up: not timed
        run(decoder)
    for _ in range(args.reps):
        for decoder in legs:
            legs[decoder].append(round(run(decoder), 1))
    entry.set_jpeg_decoder(None)
    med = lambda v: sorted(v)[len(v) // 2]
    print(json.dumps({"workload": "get_dets_by_cls from files, small synthetic ResNet-50", "images": args.images, "reps": args.reps,
                      "img_per_s": legs, "median": {k: med(v) for k, v in legs.items()},
                      "device_over_host": round(med(legs["device"]) / med(legs["host"]), 3)}))


if __name__ == "__main__":
    main()
