"""configs[0]: VGG16 at 600x1000.  RPN-only forward (default) or, with --detector, the full detection pass (RPN + proposals +
detector head + post-process) through captured passes; img/s and the per-launch table.

    python scripts/bench_vgg.py                               # f32, eager RPN-only forward on the ambient engine (as before)
    python scripts/bench_vgg.py --captured --engine f16x3     # ... replayed from a hipGraph on the f16x3 engine (the README's line)
    python scripts/bench_vgg.py --captured --dtype bf16
    python scripts/bench_vgg.py --detector --engine f16x3     # f32 detector, one image per pass
    python scripts/bench_vgg.py --detector --dtype bf16 --batch 8
    python scripts/bench_vgg.py --mixed --dtype bf16          # a shuffled list of mixed sizes through voc_dets.get_dets_by_cls (canvas passes)
    python scripts/bench_vgg.py --mixed --dtype bf16 --canvas 0     # ... through exact-geometry passes (what a VGG16 list got before canvases)
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from faster_rcnn_amd import ops, util, vgg
from faster_rcnn_amd.weights import synthetic_vgg16

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32")
ap.add_argument("--detector", action="store_true", help="the full RPN + detector pass through captured passes (300 proposals)")
ap.add_argument("--batch", type=int, default=1, help="images per captured pass (--detector; more than one needs --dtype bf16)")
ap.add_argument("--captured", action="store_true", help="RPN-only: replay the forward from a captured graph")
ap.add_argument("--engine", choices=("native", "bf16x6", "f16x3"), default=None, help="matrix path of the f32 launches (default: ambient)")
ap.add_argument("--streams", type=int, default=1, help="captured passes in flight, each on its own stream (captured modes)")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--runs", type=int, default=1, help="timed runs of --steps replays each")
ap.add_argument("--no-table", action="store_true")
ap.add_argument("--mixed", action="store_true", help="256 frames over the geometries of bench.py's mixed_sizes leg through voc_dets.get_dets_by_cls")
ap.add_argument("--canvas", type=int, default=1, help="--mixed: 0 = exact-geometry passes (FRCNN_ENTRY_CANVAS=0's policy)")
args = ap.parse_args()
engine = args.engine or ops.F32_ENGINE

anchors = util.get_anchors([128, 256, 512])
w = synthetic_vgg16(anchors_per_loc=9, seed=1, with_classifier=args.detector or args.mixed)
base = vgg.vgg16_base(weights=w, dtype=args.dtype)
rpn = vgg.vgg16_rpn(base, include_conv=True, anchors_per_loc=9)
rs = np.random.RandomState(0)
B = args.batch if args.detector else 1
S = max(1, args.streams) if (args.detector or args.captured) else 1
shared = S > 1 or B > 1                               # tiles for a shared chip, no split-K (as bench.py and entry.DetectionEntry choose)
x = torch.from_numpy((rs.randint(0, 256, (B, 600, 1000, 3)).astype(np.float32) - 110.0)).cuda()
tag = "VGG16 %s %s 600x1000" % (args.dtype, "RPN + detector, %d image(s) per pass" % B if args.detector else "RPN forward")


def timed(step):
    rates = []
    for _ in range(args.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        rates.append(B * S * args.steps / (time.perf_counter() - t0))
    return rates


def table(forward):
    """Every distinct launch of one forward re-issued back to back between one HIP-event pair."""
    ops.CONV_PROFILE = []
    forward()
    torch.cuda.synchronize()
    prof, ops.CONV_PROFILE = ops.CONV_PROFILE, None
    for p in prof:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        p["relaunch"](); e0.record()
        for _ in range(5): p["relaunch"]()
        e1.record(); torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / 5 * 1e3
        print("  %-34s M=%7d N=%4d K=%5d  %7.1f us  %6.1f TF" % (p["kernel"], p["shape"][0], p["shape"][1], p["shape"][2], us, p["flops"] / us / 1e6))
    return prof


def mixed_leg(n_images=256, seed=77):
    """bench.py's mixed_sizes list (same histogram, seed and construction: 36 geometries after the resize within 600 / 1000) with the
    VGG16 pair: the first call in a warm process (one frame of another size has been through the entry point), the same call again,
    captures, eager images and the bytes the captured passes hold."""
    import contextlib
    import io
    import json
    from bench import MIXED_SIZES
    from faster_rcnn_amd import entry, shapes, voc_dets
    from faster_rcnn_amd.data.voc_data_helpers import VOC_CLASS_MAPPING
    from faster_rcnn_amd.det_util import DetTrainingManager
    det = vgg.vgg16_classifier(64, 21, weights=w, dtype=args.dtype)
    mgr = DetTrainingManager(rpn_model=rpn, class_mapping=VOC_CLASS_MAPPING, preprocess_func=vgg.preprocess, anchor_dims=anchors)
    rs = np.random.RandomState(seed)
    sizes = []
    for (wd, h), share in MIXED_SIZES:
        sizes += [(wd, h)] * int(round(share * n_images))
    while len(sizes) < n_images:
        sizes.append((500, int(rs.randint(250, 500))))
    sizes = sizes[:n_images]
    rs.shuffle(sizes)
    pool, raw = {}, []
    for i, (wd, h) in enumerate(sizes):
        if (wd, h) not in pool:
            pool[(wd, h)] = rs.randint(0, 256, (h, wd, 3)).astype(np.uint8)
        raw.append(shapes.Image(shapes.Metadata("mixed%03d" % i, wd, h, [], "none"), pool[(wd, h)]))
    images, ratios = util.resize_imgs(raw, min_size=600, max_size=1000)
    os.environ["FRCNN_ENTRY_CANVAS"] = "1" if args.canvas else "0"     # (VGG16 canvases are opt-in)
    eng = entry.for_models(mgr, det, 64, 16, entry.default_in_flight(args.dtype))
    eager = [0]
    real = voc_dets._get_dets_eager
    voc_dets._get_dets_eager = lambda *a, **k: (eager.__setitem__(0, eager[0] + 1), real(*a, **k))[1]

    def run(imgs, rts):
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.perf_counter()
            voc_dets.get_dets_by_cls(mgr, det, rts, imgs)
            return time.perf_counter() - t0
    warm = shapes.Image(shapes.Metadata("warm", 480, 320, [], "none"), rs.randint(0, 256, (320, 480, 3)).astype(np.uint8))
    run([warm], [1.0])                                           # the process is warm: library loaded, filters packed, allocator primed
    eng.cache.clear()
    eager[0] = 0
    before = eng.stats()
    t1 = run(images, ratios)
    mid, e1 = eng.stats(), eager[0]
    t2 = run(images, ratios)
    after = eng.stats()
    print(json.dumps({"leg": "VGG16 %s mixed sizes, %s" % (args.dtype, "canvas passes" if eng.canvas_capable else "exact-geometry passes"),
                      "images": n_images, "geometries": len({(im.height, im.width) for im in images}),
                      "first_call_img_s": round(n_images / t1, 1), "second_call_img_s": round(n_images / t2, 1),
                      "captures_first": mid["captures"] - before["captures"], "captures_second": after["captures"] - mid["captures"],
                      "eager_images_first": e1, "eager_images_second": eager[0] - e1, "bytes_held": after["bytes"], "graphs": after["graphs"],
                      "canvas_classes": sorted({k[1:3] for k in eng.cache.keys() if k[:1] == ("canvas",)}),
                      "images_per_pass": eng.batch, "in_flight": eng.in_flight, "f32_engine": eng.f32_engine,
                      "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "4")}))
    eng.cache.clear()


if args.mixed:
    mixed_leg()
elif args.detector:
    from faster_rcnn_amd.pipeline import BatchedInferencePipeline, InferencePipeline
    det = vgg.vgg16_classifier(64, 21, weights=w, dtype=args.dtype)
    make = (lambda: BatchedInferencePipeline(rpn, det, anchors, B, max_proposals=300)) if B > 1 else (lambda: InferencePipeline(rpn, det, anchors, max_proposals=300))
    # (fp32 passes keep split-K beside other passes, bf16 ones drop it: entry.DetectionEntry's choice)
    pipes = [make().capture(600, 1000, split_k=(not shared) or (args.dtype == "f32" and B == 1), throughput=shared, f32_engine=engine) for _ in range(S)]
    streams = [torch.cuda.Stream() for _ in range(S)]
    for pl in pipes:
        pl.replay(x)

    def step():
        for pl, st in zip(pipes, streams):
            with torch.cuda.stream(st):
                pl._graph.replay()
    rates = timed(step)
    print("%s, %d captured pass(es) in flight (f32 launches on %s): %s img/s" % (tag, S, engine, " / ".join("%.1f" % r for r in rates)))
    if not args.no_table:
        pipe = pipes[0]
        with ops.f32_engine(engine), ops.conv_workspace(pipe._conv_ws), ops.tile_policy(shared), ops.amax_arena(pipe._amax):
            table(lambda: pipe.forward_dev(x))
    for pl in pipes:
        pl.close()
elif args.captured:
    from faster_rcnn_amd.pipeline import no_gc

    class Pass:
        """One captured RPN-only forward with its own split-K workspace and magnitude records."""

        def __init__(self):
            self.arena = ops.AmaxArena() if engine == "f16x3" else None
            self.ws = ops.NO_SPLIT_K if shared else ops.ConvWorkspace()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), self.scope():
                for _ in range(2):
                    self.forward()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with no_gc(), torch.cuda.graph(self.graph, capture_error_mode="thread_local"), self.scope():
                self.out = self.forward()

        def scope(self):
            import contextlib
            st = contextlib.ExitStack()
            for c in (ops.conv_workspace(self.ws), ops.tile_policy(shared), ops.f32_engine(engine), ops.amax_arena(self.arena)):
                st.enter_context(c)
            return st

        def forward(self):
            ops.amax_begin()
            return rpn.forward_dev(x)

    passes = [Pass() for _ in range(S)]
    streams = [torch.cuda.Stream() for _ in range(S)]

    def step():
        for ps, st in zip(passes, streams):
            with torch.cuda.stream(st):
                ps.graph.replay()
    rates = timed(step)
    print("%s, %d captured pass(es) in flight (f32 launches on %s): %s img/s" % (tag, S, engine, " / ".join("%.1f" % r for r in rates)))
    if not args.no_table:
        with passes[0].scope():
            table(passes[0].forward)
else:
    with ops.f32_engine(engine):
        for _ in range(3):
            out = rpn.forward_dev(x)
        torch.cuda.synchronize()
        rates = timed(lambda: rpn.forward_dev(x))
        dt = 1.0 / rates[-1]
        print("%s: %.2f ms/img, %s img/s" % (tag, dt * 1e3, " / ".join("%.1f" % r for r in rates)))
        if not args.no_table:
            prof = table(lambda: rpn.forward_dev(x))
            print("  %.1f GFLOP in the table's launches -> %.1f TF/s over the forward" % (sum(p["flops"] for p in prof) / 1e9, sum(p["flops"] for p in prof) / dt / 1e12))
