"""Three legs of voc_dets.get_dets_by_cls from JPEG files, alternating within each repetition: the host decoder, the device decoder one
file at a time (FRCNN_ENTRY_JPEG_BATCH=0) and the device decoder batched (one ops.jpeg_decode_batch_u8 per pass).

    python scripts/bench_decode.py [--images 64] [--reps 5] [--file tests/golden/VOC_test/JPEGImages/000005.jpg] [--mixed]
    python scripts/bench_decode.py --op-only [--iters 200] [--batch 8]   # only the decode ops in a loop: the target of
    rocprofv3 --kernel-trace --stats -- python scripts/bench_decode.py --op-only      # (counters, if any, in a run of their own)

The list is ``--images`` Image objects over ONE file (one geometry: the captured, batched path), so the legs differ in who decodes, in
what crosses the link (the file's bytes against the decoded frame) and in how many launches stand in front of a replay.  ``--mixed``:
the list cycles over several sizes cut from the photograph and saved as baseline JPEG at mixed subsampling, so that canvas passes form
(the VOC case).  ``--op-only --batch N``: N copies of the file through ops.jpeg_decode_u8 one after another against one
ops.jpeg_decode_batch_u8.  The models are the small synthetic ResNet-50 of the tests: the figures are ratios of legs on the same
passes, not a headline rate.  ``--progressive``: the same legs on a PROGRESSIVE re-save of the input (quality 90), decoded under the JPEG
decoder setting "device_full" (csrc/jpeg_dec_full.hip); the per-file leg is the batched one there (progressive files are always
decoded as a batch), and ``--op-only`` times one ops.jpeg_decode_full_batch_u8 of max(1, --batch) copies.  Prints one JSON line."""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
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


# (rows, columns) cut off the photograph for --mixed: more sizes than entry.CANVAS_MIN_GEOMETRIES
MIXED_CUTS = ((0, 0), (8, 0), (0, 12), (16, 20), (24, 4), (4, 28), (32, 32), (12, 40))


def op_batch(args, data, plan):
    """--op-only --batch N: N copies of the file per iteration, decoded by N ops.jpeg_decode_u8 and by one ops.jpeg_decode_batch_u8."""
    import numpy as np
    import torch
    from faster_rcnn_amd import ops
    n, frame = args.batch, plan.h * plan.w * 3
    files = torch.from_numpy(np.frombuffer(data * n, dtype=np.uint8).copy()).cuda()
    ws_off, total = ops.jpeg_dec_batch_layout([plan] * n)
    ws = torch.empty(total, dtype=torch.uint8, device="cuda")
    out = torch.empty(n * frame, dtype=torch.uint8, device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    items = ops.jpeg_batch_items([plan] * n, [i * len(data) for i in range(n)], [i * frame for i in range(n)], ws_off)
    items_dev = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).cuda()

    def per_file():
        for i in range(n):
            ops.jpeg_decode_u8(files[i * len(data):(i + 1) * len(data)], plan, out=out[i * frame:(i + 1) * frame].view(plan.h, plan.w, 3),
                               status=status[i:i + 1], workspace=ws)

    def batched():
        ops.jpeg_decode_batch_u8(files, items, out, status=status, workspace=ws, items_dev=items_dev)

    ms = {}
    for name, fn in (("per_file", per_file), ("batched", batched), ("per_file_again", per_file), ("batched_again", batched)):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        ms[name] = round(1e3 * (time.perf_counter() - t0) / args.iters, 4)
    print(json.dumps({"op": "jpeg_decode_batch_u8", "batch": n, "file_bytes": len(data), "h": plan.h, "w": plan.w, "iters": args.iters,
                      "ms_per_batch": ms, "per_file_over_batched": round(ms["per_file_again"] / ms["batched_again"], 2),
                      "status": int(status.abs().max().item())}))


def op_progressive(args, data):
    """--progressive --op-only: max(1, --batch) copies of the progressive file through one ops.jpeg_decode_full_batch_u8 per iteration."""
    import numpy as np
    import torch
    from faster_rcnn_amd import ops
    plan = ops.jpeg_dec_full_plan(data)
    n, frame = max(1, args.batch), plan.h * plan.w * 3
    files = torch.from_numpy(np.frombuffer(data * n, dtype=np.uint8).copy()).cuda()
    ws_off, total = ops.jpeg_dec_full_batch_layout([plan] * n)
    ws = torch.empty(total, dtype=torch.uint8, device="cuda")
    out = torch.empty(n * frame, dtype=torch.uint8, device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    items = ops.jpeg_full_batch_items([plan] * n, [i * len(data) for i in range(n)], [i * frame for i in range(n)], ws_off)
    items_dev = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).cuda()
    for _ in range(5):
        ops.jpeg_decode_full_batch_u8(files, items, out, status=status, workspace=ws, items_dev=items_dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        ops.jpeg_decode_full_batch_u8(files, items, out, status=status, workspace=ws, items_dev=items_dev)
    torch.cuda.synchronize()
    print(json.dumps({"op": "jpeg_decode_full_batch_u8", "batch": n, "file_bytes": len(data), "h": plan.h, "w": plan.w, "scans": int(plan.scans),
                      "iters": args.iters, "ms_per_batch": round(1e3 * (time.perf_counter() - t0) / args.iters, 4),
                      "status": int(status.abs().max().item())}))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--file", default=os.path.join(ROOT, "tests", "golden", "VOC_test", "JPEGImages", "000005.jpg"))
    p.add_argument("--images", type=int, default=64)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--op-only", dest="op_only", action="store_true")
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--batch", type=int, default=0, help="--op-only: N copies of the file per iteration, per-file loop against one batched call")
    p.add_argument("--mixed", action="store_true", help="several sizes cut from the file, so that canvas passes form")
    p.add_argument("--progressive", action="store_true", help="the legs on a progressive re-save of the file, the device legs under device_full")
    args = p.parse_args()
    import torch
    from faster_rcnn_amd import entry, ops, shapes, util, voc_dets
    keep = tempfile.TemporaryDirectory()
    if args.progressive:
        from PIL import Image as PilImage
        with PilImage.open(args.file) as im:
            args.file = os.path.join(keep.name, "progressive.jpg")
            im.convert("RGB").save(args.file, "JPEG", quality=90, progressive=True)
    data = open(args.file, "rb").read()
    if args.progressive and args.op_only:
        return op_progressive(args, data)
    plan = ops.jpeg_dec_full_plan(data).frame if args.progressive else ops.jpeg_dec_plan(data)
    if args.op_only and args.batch > 0:
        return op_batch(args, data, plan)
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
    tmp = tempfile.TemporaryDirectory()
    if args.mixed:
        from PIL import Image as PilImage
        paths = []
        with PilImage.open(args.file) as im:
            im = im.convert("RGB")
            for k, (dh, dw) in enumerate(MIXED_CUTS):
                path = os.path.join(tmp.name, "cut%d.jpg" % k)
                im.crop((0, 0, plan.w - dw, plan.h - dh)).save(path, "JPEG", quality=90, subsampling=k % 3, progressive=args.progressive)
                paths.append((path, plan.h - dh, plan.w - dw))
        images = [shapes.Image(shapes.Metadata("i%d" % i, paths[i % len(paths)][2], paths[i % len(paths)][1], [], paths[i % len(paths)][0]))
                  for i in range(args.images)]
    else:
        images = [shapes.Image(shapes.Metadata("i%d" % i, plan.w, plan.h, [], args.file)) for i in range(args.images)]
    resized, ratios = util.resize_imgs(images, min_size=600, max_size=1000)
    legs = {"host": [], "device_per_file": [], "device_batched": []}

    def run(leg):
        entry.set_jpeg_decoder("host" if leg == "host" else ("device_full" if args.progressive else "device"))
        os.environ["FRCNN_ENTRY_JPEG_BATCH"] = "0" if leg == "device_per_file" else "1"
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            voc_dets.get_dets_by_cls(mgr, det, ratios, resized, det_threshold=0.1)
        torch.cuda.synchronize()
        return len(images) / (time.perf_counter() - t0)

    for leg in legs:                                        # captures and warm-up: not timed
        run(leg)
    for _ in range(args.reps):
        for leg in legs:
            legs[leg].append(round(run(leg), 1))
    entry.set_jpeg_decoder(None)
    os.environ.pop("FRCNN_ENTRY_JPEG_BATCH", None)
    med = lambda v: sorted(v)[len(v) // 2]
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight("f32"))
    print(json.dumps({"workload": "get_dets_by_cls from files, small synthetic ResNet-50", "images": args.images, "reps": args.reps,
                      "mixed": bool(args.mixed), "progressive": bool(args.progressive), "canvas_passes": sum(k[0] == "canvas" for k in eng.cache.keys()), "batch": eng.batch,
                      "img_per_s": legs, "median": {k: med(v) for k, v in legs.items()},
                      "spread": {k: round((max(v) - min(v)) / med(v), 3) for k, v in legs.items()},
                      "batched_over_per_file": round(med(legs["device_batched"]) / med(legs["device_per_file"]), 3),
                      "batched_over_host": round(med(legs["device_batched"]) / med(legs["host"]), 3)}))
    tmp.cleanup()


if __name__ == "__main__":
    main()
