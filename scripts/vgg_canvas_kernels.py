"""The two kernels of a VGG16 canvas pass beside the unmasked ones at 8 x 600 x 1000 (bf16 block 1): each launched ``--reps`` times, for a
`rocprofv3 --kernel-trace --stats -- python scripts/vgg_canvas_kernels.py` run (per-kernel time) -- and, without the profiler, timed here
between HIP events.  The masked forms are launched at FULL extent (every cell inside: the same bytes as the unmasked kernels move) and
at the extents of bench.py's mixed list on its largest canvas class (600 x 1000 canvases holding 600 x 800 .. 562 x 1000 images)."""
import argparse
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from faster_rcnn_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()
rs = np.random.RandomState(6)
n, H, W = 8, 600, 1000
x = torch.from_numpy((rs.randint(0, 256, (n, H, W, 3)).astype(np.float32) - 110.0)).cuda()
pk = ops.PackedVggConv1Bf16((rs.randn(3, 3, 3, 64) * np.sqrt(2.0 / 27) / 70.0).astype(np.float32), (rs.randn(64) * 0.1).astype(np.float32))
full = torch.tensor([[H, W]] * n, dtype=torch.int32, device="cuda")
mixed = torch.tensor([[600, 800], [600, 901], [562, 1000], [600, 899], [600, 898], [600, 750], [600, 840], [600, 798]], dtype=torch.int32, device="cuda")
y = ops.vgg_conv1_bf16(x, pk)
y32 = y[:2].float().contiguous()


def timed(name, fn):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    print("%-64s %8.1f us per launch" % (name, e0.elapsed_time(e1) / args.reps * 1e3))


timed("k_vgg_conv1_bf16<false>  8 x 600 x 1000", lambda: ops.vgg_conv1_bf16(x, pk))
timed("k_vgg_conv1_bf16<true>   8 x 600 x 1000, full extent", lambda: ops.vgg_conv1_bf16_extents(x, pk, full))
timed("k_vgg_conv1_bf16<true>   8 x 600 x 1000, mixed extents", lambda: ops.vgg_conv1_bf16_extents(x, pk, mixed))
timed("k_pool2_bf16             8 x 600 x 1000 x 64", lambda: ops.pool2d_bf16(y, 2, 2))
timed("k_pool2_extents<bf16>    8 x 600 x 1000 x 64, full extent", lambda: ops.pool2d_bf16_extents(y, full))
timed("k_pool2_extents<bf16>    8 x 600 x 1000 x 64, mixed extents", lambda: ops.pool2d_bf16_extents(y, mixed))
timed("k_pool<true> (f32)       2 x 600 x 1000 x 64", lambda: ops.pool2d(y32, 2, 2, True))
timed("k_pool2_extents<f32>     2 x 600 x 1000 x 64, full extent", lambda: ops.pool2d_extents(y32, full))
