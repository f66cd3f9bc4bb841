"""Times of the detection post-process kernels on cases of tests/detections_cases.py: k_detections (frcnn_detections_dyn) beside
k_detections_post (frcnn_detections_post_dyn) in its modes.  DESIGN §8 "Post-process rule" quotes the figures.

    python scripts/profile_detect_post.py [--cases size_512_c2,size_320_c21,chain,tie_all_512] [--iters 50] [--only MODE] [--lib PATH]
    python scripts/profile_detect_post.py --build_variant PATH.so --wg_rows N    (host only: needs hipcc and a built csrc/_obj)

Every (case, mode) is launched ``--iters`` times back to back between two events after a warm-up; the figure is microseconds per launch,
launch gaps included (one workgroup: the kernel is latency, the gap is the floor that ``empty`` -- nothing scored, n_live 0 -- shows).
``--only MODE`` launches one mode alone, for a run under a kernel tracer whose statistics go by kernel name.
``--build_variant`` links a second library whose detect_post.hip is compiled with -DDP_WG_ROWS=N: 0 = every class by all eight waves
with a workgroup barrier per pick, 512 = every class by one wave (the two pure forms the library's mix, classes of more than 256 rows
by the workgroup, was chosen from); ``--lib`` then times that library's kernel."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {"k_detections": None, "hard": ("hard", None), "soft_linear": ("soft_linear", 0.3), "soft_gaussian": ("soft_gaussian", 0.5, 0.5),
         "soft_gaussian_vote": ("soft_gaussian", 0.5, 0.5, None, 0.5), "hard_vote": ("hard", 0.5, 0.5, None, 0.5)}


def build_variant(out, wg_rows):
    from faster_rcnn_amd import build
    src = os.path.join(build.CSRC, "detect_post.hip")
    obj = os.path.splitext(out)[0] + "_detect_post.o"
    subprocess.check_call([build._hipcc(), "-c", src, "-o", obj, "-DDP_WG_ROWS=%d" % wg_rows] + build.COMMON + build.SOURCES["detect_post.hip"])
    objs = [os.path.join(build.OBJ, f.replace(".hip", ".o")) for f in build._sources() if f != "detect_post.hip"]
    subprocess.check_call([build._hipcc(), "-shared", "-fPIC", "--offload-arch=%s" % build.ARCH, "-Wl,-z,defs", "-o", out, obj] + objs)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="size_512_c2,size_320_c21,chain,tie_all_512")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only", choices=sorted(MODES), default=None)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--build_variant", default=None, metavar="PATH.so")
    ap.add_argument("--wg_rows", type=int, default=0)
    args = ap.parse_args()
    if args.build_variant:
        print(build_variant(os.path.abspath(args.build_variant), args.wg_rows))
        return
    import numpy as np
    import torch
    from faster_rcnn_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    from faster_rcnn_amd import ops
    from tests import detections_cases as K
    cases = K.all_cases()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = {"lib": os.path.basename(_lib.LIB_PATH), "iters": args.iters, "unit": "us per launch"}
    for name in args.cases.split(","):
        c = cases[name]
        d = {"rois": dev(c["rois"]), "cls": dev(c["cls"]), "reg": dev(c["reg"]), "dyn": dev(np.array([c["ratio"], c["thr"]], np.float64))}
        res = {"rows": len(c["cls"]), "classes": int(c["cls"].shape[1])}
        for live, tag in ((c["n_live"], ""), (0, "empty_")):
            n = dev(np.array([live], np.int32))
            for mode, post in MODES.items():
                if (args.only and mode != args.only) or (tag and mode not in ("k_detections", "soft_gaussian")):
                    continue
                if post is None:
                    fn = lambda: ops.detections_dyn(d["rois"], n, d["cls"], d["reg"], 0, c["bg"], c["stride"], d["dyn"], c["nms"])
                else:
                    fn = lambda: ops.detections_post_dyn(d["rois"], n, d["cls"], d["reg"], 0, c["bg"], c["stride"], d["dyn"], post)
                for _ in range(5):
                    r = fn()
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.iters):
                    r = fn()
                t1.record()
                torch.cuda.synchronize()
                res[tag + mode] = round(1e3 * t0.elapsed_time(t1) / args.iters, 1)
                if not tag:
                    res[mode + "_n_dets"] = int(r["n_dets"].item())
        out[name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
