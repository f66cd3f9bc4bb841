"""res5a's RoI-resampled shortcut gathered inside the closing 1x1 convolution's epilogue (include/ext/frcnn_hip_roi_res.h;
csrc/conv_f32_common.h x6_epilogue_vec<.., GRES>, csrc/roi.hip k_roi_tap_table) against the unfused path -- frcnn_roi_crop_resize_fwd_batch
/ _fwd_ex, then the same convolution with ``residual=`` -- BIT FOR BIT, both sides on the f16x3 engine's tile code 86.

Two images on the 9 x 13 map of tests/test_roi_kernels_gpu.py; eleven RoIs of its shared list (the whole map, 1x1 boxes in two corners,
fractional corners, corners in (-1, 0), and one rejected box per clause of the validity predicate), six per image: M = 539 rows = two full
256-row tiles and a ragged one, both images inside the second tile; Cin = 64 (two chunks), Cout = 256 (two column tiles: the second reads
the map and the fill vector at a column offset).  The fill vector has negative entries and the launch ends in a ReLU.

Mutation seen during development (nothing of the kind is left in the suite): an epilogue that used tx where ty belongs failed
test_gathered_residual_equals_the_unfused_path on 31 004 of 137 984 elements -- every accepted row whose two fractions differ.  An epilogue
that yields zeros instead of the fill piece for a rejected RoI (six of the eleven) failed all eight cases of that test and
test_one_map_without_n_per_img (profiles/roi_res_epilogue_ab.txt)."""
import ctypes

import numpy as np
import pytest

from tests import roi_ref as R
from tests.test_roi_kernels_gpu import COLS, ROWS, roi_list

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POOL, CIN, COUT, N_PER_IMG, TILE = 7, 64, 256, 6, 86
PICK = [0, 3, 1, 8, 9, 15, 5, 19, 10, 20, -1]       # accepted and rejected boxes alternate; image 0 takes the first six


def rois_np():
    rois = roi_list(POOL)[PICK]
    ok = [R.accepted(r, ROWS, COLS) for r in rois]
    assert len(rois) == 11 and sum(ok) == 5 and ok[0] and ok[6]          # both images have accepted and rejected boxes
    return rois


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.fixture(scope="module")
def data():
    from faster_rcnn_amd import ops
    rs = np.random.RandomState(77)
    fmap = torch.from_numpy(rs.randn(2, ROWS, COLS, COUT).astype(np.float32)).cuda()
    fill = torch.from_numpy(rs.randn(COUT).astype(np.float32)).cuda()      # (negative entries: the ReLU bites on rejected rows)
    assert (fill < 0).any() and (fill > 0).any()
    wt = (rs.randn(1, 1, CIN, COUT) * np.sqrt(2.0 / CIN)).astype(np.float32)
    pc = ops.PackedConv(wt, (1 + 0.1 * rs.randn(COUT)).astype(np.float32), (0.1 * rs.randn(COUT)).astype(np.float32))
    pc0 = ops.PackedConv((rs.randn(1, 1, CIN, CIN) * np.sqrt(2.0 / CIN)).astype(np.float32))
    x = rs.randn(11, POOL, POOL, CIN).astype(np.float32)
    return {"fmap": fmap, "fill": fill, "pc": pc, "pc0": pc0, "x": x, "rois": torch.from_numpy(rois_np()).cuda()}


def conv_input(ops, data, layout, planes_in):
    x = data["x"].transpose(1, 2, 0, 3) if layout else data["x"]
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    if not planes_in:
        return xd
    xp = ops.conv2d(xd, data["pc0"], 1, "valid", "relu", tile=TILE, layout=layout, planes_out=True)
    assert isinstance(xp, ops.PlaneTensor)
    return xp


@pytest.mark.parametrize("planes_out", [False, True])
@pytest.mark.parametrize("planes_in", [False, True])
@pytest.mark.parametrize("layout", [0, 1])
def test_gathered_residual_equals_the_unfused_path(data, layout, planes_in, planes_out):
    from faster_rcnn_amd import ops
    with ops.f32_engine("f16x3"):
        fmap = data["fmap"]
        fmap._amax = ops.amax_of(fmap)
        x = conv_input(ops, data, layout, planes_in)
        s = ops.roi_crop_resize(fmap, data["rois"], POOL, fill=data["fill"], layout=layout, n_per_img=N_PER_IMG)
        want = ops.conv2d(x, data["pc"], 1, "valid", "relu", residual=s, tile=TILE, layout=layout, planes_out=planes_out)
        assert ops.conv_takes_roi_res(x, data["pc"], 1, "valid", "relu", layout, TILE)
        g = ops.roi_shortcut(fmap, data["rois"], POOL, x, data["pc"], fill=data["fill"], layout=layout, n_per_img=N_PER_IMG, act="relu", tile=TILE)
        assert isinstance(g, ops.RoiResidual) and tuple(g.shape) == tuple(s.shape)
        got = ops.conv2d(x, data["pc"], 1, "valid", "relu", residual=g, tile=TILE, layout=layout, planes_out=planes_out)
        torch.cuda.synchronize()
    assert isinstance(got, ops.PlaneTensor) == isinstance(want, ops.PlaneTensor) == planes_out
    if planes_out:
        assert int(got.exponent.item()) == int(want.exponent.item())
        assert torch.equal(bits(got.planes), bits(want.planes))
        assert bool((want.planes[0] == 0).any()) and bool((want.planes[0] > 0).any())        # the ReLU bit, and not everywhere
    else:
        assert torch.equal(bits(got), bits(want))
        assert bool((want == 0).any()) and bool((want > 0).any())
    # the output's magnitude record, status word (word 1) included
    assert torch.equal(bits(got._amax), bits(want._amax))
    assert int(bits(got._amax)[1].item()) == 0


def test_one_map_without_n_per_img(data):
    """frcnn_roi_crop_resize_fwd_ex's form (one map, the one-image pass): the second image's RoIs read the same map."""
    from faster_rcnn_amd import ops
    with ops.f32_engine("f16x3"):
        fmap = data["fmap"][1:2].contiguous()
        x = conv_input(ops, data, 1, True)
        s = ops.roi_crop_resize(fmap, data["rois"], POOL, fill=data["fill"], layout=1)
        want = ops.conv2d(x, data["pc"], 1, "valid", "relu", residual=s, tile=TILE, layout=1)
        g = ops.roi_shortcut(fmap, data["rois"], POOL, x, data["pc"], fill=data["fill"], layout=1, act="relu", tile=TILE)
        assert isinstance(g, ops.RoiResidual)
        got = ops.conv2d(x, data["pc"], 1, "valid", "relu", residual=g, tile=TILE, layout=1)
    assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("layout", [0, 1])
def test_tap_table_against_the_reference_taps(data, layout):
    from faster_rcnn_amd import ops
    rois = rois_np()
    g = ops.RoiResidual(data["fmap"], data["rois"], POOL, fill=data["fill"], layout=layout, n_per_img=N_PER_IMG)
    torch.cuda.synchronize()
    tab = g.taps.cpu().numpy()
    n = len(rois)
    assert tab.shape == (n * POOL * POOL, 8) and tab.dtype == np.int32
    want = np.zeros_like(tab)
    for r, roi in enumerate(rois):
        tp = R.taps(roi, POOL, ROWS, COLS)
        for py in range(POOL):
            for px in range(POOL):
                m = (py * POOL + px) * n + r if layout else (r * POOL + py) * POOL + px
                if tp is None:
                    continue                                           # rejected: offsets 0, fractions 0, ok 0
                y_lo, y_hi, ty, x_lo, x_hi, tx = tp
                base = (r // N_PER_IMG) * ROWS * COLS
                want[m, :4] = [(base + y * COLS + xx) * COUT for y, xx in ((y_lo[py], x_lo[px]), (y_lo[py], x_hi[px]), (y_hi[py], x_lo[px]), (y_hi[py], x_hi[px]))]
                want[m, 4] = np.float32(tx[px]).view(np.int32)
                want[m, 5] = np.float32(ty[py]).view(np.int32)
                want[m, 6] = 1
    assert np.array_equal(tab, want)                                   # integers exact, tx / ty bit-equal


@pytest.mark.parametrize("tile", [81, 83, 84, 87, 184, 181, "native"])
def test_other_tiles_and_engines_fall_back(data, tile):
    """Only the 256x128 form on sixteen waves has the mode: the query says so for every other code and for the native engine, and
    ops.roi_shortcut then hands the resampled tensor on -- the result still equals the reference path's."""
    from faster_rcnn_amd import _lib, ops
    code = 0 if tile == "native" else tile
    xd = conv_input(ops, data, 0, False)
    d = ops._conv_desc(tuple(xd.shape), 1, 1, COUT, 1, "valid", 1, 0, code)
    lib = _lib.load()
    assert lib.frcnn_conv2d_roi_res_available(ctypes.byref(d), 0 if tile == "native" else 2, 0) == 0
    assert lib.frcnn_conv2d_roi_res_available(ctypes.byref(d), 0 if tile == "native" else 2, 1) == 0
    assert not ops.conv_takes_roi_res(xd, data["pc"], 1, "valid", "relu", 0, code)
    fmap = data["fmap"]
    fmap._amax = None
    s = ops.roi_crop_resize(fmap, data["rois"], POOL, fill=data["fill"], n_per_img=N_PER_IMG)
    want = ops.conv2d(xd, data["pc"], 1, "valid", "relu", residual=s, tile=code)
    g = ops.roi_shortcut(fmap, data["rois"], POOL, xd, data["pc"], fill=data["fill"], n_per_img=N_PER_IMG, act="relu", tile=code)
    assert isinstance(g, torch.Tensor) and torch.equal(bits(g), bits(s))
    got = ops.conv2d(xd, data["pc"], 1, "valid", "relu", residual=g, tile=code)
    assert torch.equal(bits(got), bits(want))
    with pytest.raises(_lib.FrcnnError):                                # a RoiResidual handed to such a launch is refused, not resampled behind the caller's back
        ops.conv2d(xd, data["pc"], 1, "valid", "relu", residual=ops.RoiResidual(fmap, data["rois"], POOL, fill=data["fill"], n_per_img=N_PER_IMG), tile=code)


def test_plane_output_over_a_map_without_a_record(data):
    """A map nobody left a magnitude record on (or whose record belongs to an earlier pass): the bound is measured, as for a resampled
    tensor without a record, and merged with max|fill|; the planes then hold the f32 result to their 22 bits under a clean status."""
    from faster_rcnn_amd import ops
    with ops.f32_engine("f16x3"):
        fmap = data["fmap"]
        fmap._amax = None
        x = conv_input(ops, data, 0, True)
        g = ops.RoiResidual(fmap, data["rois"], POOL, fill=data["fill"], n_per_img=N_PER_IMG)
        assert g._amax is None
        got = ops.conv2d(x, data["pc"], 1, "valid", "relu", residual=g, tile=TILE, planes_out=True)
        want = ops.conv2d(x, data["pc"], 1, "valid", "relu", residual=ops.RoiResidual(fmap, data["rois"], POOL, fill=data["fill"], n_per_img=N_PER_IMG), tile=TILE)
        torch.cuda.synchronize()
    assert isinstance(got, ops.PlaneTensor) and int(bits(got._amax)[1].item()) == 0
    bound = float(max(fmap.abs().max().item(), data["fill"].abs().max().item()))
    assert float(g._amax.max()) == bound                               # max(|map|, |fill|), measured
    assert float((got.float() - want).abs().max()) <= 2.0 ** -21 * float(want.abs().max()) * 2
