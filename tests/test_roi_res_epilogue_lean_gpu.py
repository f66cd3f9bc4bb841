"""The gathered-residual epilogue with the tile's tap records staged in LDS (csrc/conv_f32_common.h x6_epilogue_vec<.., GRES>): a workgroup
loads the 256 records of its row tile once -- one 16-byte word per thread on its first 512 threads, rows past M through the descriptor's
out-of-range path -- and every wave-row reads its records back from LDS.  Each case compares the gathered launch BIT FOR BIT against the
unfused path (``ops.roi_crop_resize`` into an f32 tensor, then the same convolution with ``residual=``), as
tests/test_roi_res_epilogue_gpu.py does, at the shapes where the staging can go wrong:

  rows     3 RoIs x 49 = 147: less than one tile, the record load over-covers (109 rows past M);  6 RoIs = 294: the second tile holds
           38 rows, its last three wave-rows lie wholly past M;  11 RoIs = 539: three tiles, the last one ragged.
  columns  Cout = 128 (one column tile) and 384 (three: the map pieces and the fill piece are read at n0 > 0).
  depth    Cin = 32 (the smallest the form accepts: one chunk), 64 and 512.
  RoIs     the shared list of tests/test_roi_kernels_gpu.py in the order of tests/test_roi_res_epilogue_gpu.py: accepted and rejected
           boxes alternate, so the fill branch is taken in the first, a middle and the last tile and in different wave-rows; two images.

Both crop layouts, f32 and plane activations (the two gathered instantiations), f32 and plane outputs (the two epilogues inside each), with
and without a fill vector.  Every gathered launch runs twice into buffers of its own and both results must equal the reference: records
left in LDS by another tile, or read before the staging barrier, would differ between a workgroup's first and later tiles."""
import numpy as np
import pytest

from tests import roi_ref as R
from tests.test_roi_kernels_gpu import COLS, ROWS, roi_list
from tests.test_roi_res_epilogue_gpu import PICK, bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POOL, TILE = 7, 86
N_ROIS = [3, 6, 11]
REJECTED = {3: [1], 6: [1, 3, 5], 11: [1, 3, 5, 7, 9, 10]}             # positions of the rejected boxes among the first n of PICK


def test_the_rejected_boxes_sit_where_the_cases_need_them():
    rois = roi_list(POOL)[PICK]
    for n, want in REJECTED.items():
        assert [i for i in range(n) if not R.accepted(rois[i], ROWS, COLS)] == want
    # [roi][7][7] rows: RoI 1 lies in the first tile, RoI 5 ends the second tile of 294 rows and spans the first two of 539,
    # RoI 10 fills the ragged last tile (rows 490 .. 538)
    assert 1 * 49 < 256 and 5 * 49 < 256 < 6 * 49 and 10 * 49 < 512 < 11 * 49


@pytest.fixture(scope="module")
def data():
    from faster_rcnn_amd import ops
    rs = np.random.RandomState(91)
    d = {"rois": roi_list(POOL)[PICK], "fmap": {}, "fill": {}, "pc": {}, "pc0": {}, "x": {}}
    for cout in (128, 384):
        d["fmap"][cout] = torch.from_numpy(rs.randn(2, ROWS, COLS, cout).astype(np.float32)).cuda()
        d["fill"][cout] = torch.from_numpy(rs.randn(cout).astype(np.float32)).cuda()
        assert (d["fill"][cout] < 0).any() and (d["fill"][cout] > 0).any()
    for cin in (32, 64, 512):
        d["x"][cin] = rs.randn(11, POOL, POOL, cin).astype(np.float32)
        d["pc0"][cin] = ops.PackedConv((rs.randn(1, 1, cin, cin) * np.sqrt(2.0 / cin)).astype(np.float32))
        for cout in (128, 384):
            wt = (rs.randn(1, 1, cin, cout) * np.sqrt(2.0 / cin)).astype(np.float32)
            d["pc"][cin, cout] = ops.PackedConv(wt, (1 + 0.1 * rs.randn(cout)).astype(np.float32), (0.1 * rs.randn(cout)).astype(np.float32))
    return d


def check(data, n, cout, cin, layout, planes_in, planes_out=False, with_fill=True):
    from faster_rcnn_amd import ops
    pc, fmap, fill = data["pc"][cin, cout], data["fmap"][cout], data["fill"][cout] if with_fill else None
    rois = torch.from_numpy(data["rois"][:n]).cuda()
    n_per_img = (n + 1) // 2                                           # two images, the second one short by one RoI when n is odd
    xh = data["x"][cin][:n]
    xd = torch.from_numpy(np.ascontiguousarray(xh.transpose(1, 2, 0, 3) if layout else xh)).cuda()
    with ops.f32_engine("f16x3"):
        fmap._amax = ops.amax_of(fmap)
        x = ops.conv2d(xd, data["pc0"][cin], 1, "valid", "relu", tile=TILE, layout=layout, planes_out=True) if planes_in else xd
        assert isinstance(x, ops.PlaneTensor) == planes_in
        s = ops.roi_crop_resize(fmap, rois, POOL, fill=fill, layout=layout, n_per_img=n_per_img)
        want = ops.conv2d(x, pc, 1, "valid", "relu", residual=s, tile=TILE, layout=layout, planes_out=planes_out)
        assert ops.conv_takes_roi_res(x, pc, 1, "valid", "relu", layout, TILE)
        g = ops.roi_shortcut(fmap, rois, POOL, x, pc, fill=fill, layout=layout, n_per_img=n_per_img, act="relu", tile=TILE)
        assert isinstance(g, ops.RoiResidual) and tuple(g.shape) == tuple(s.shape) and s.numel() == n * POOL * POOL * cout
        gots = [ops.conv2d(x, pc, 1, "valid", "relu", residual=g, tile=TILE, layout=layout, planes_out=planes_out) for _ in range(2)]
        torch.cuda.synchronize()
    for got in gots:
        assert isinstance(got, ops.PlaneTensor) == isinstance(want, ops.PlaneTensor) == planes_out
        if planes_out:
            assert got.planes.data_ptr() != want.planes.data_ptr()
            assert int(got.exponent.item()) == int(want.exponent.item())
            assert torch.equal(bits(got.planes), bits(want.planes))
        else:
            assert got.data_ptr() != want.data_ptr()
            assert torch.equal(bits(got), bits(want))
        assert torch.equal(bits(got._amax), bits(want._amax)) and int(bits(got._amax)[1].item()) == 0
    if planes_out:
        assert gots[0].planes.data_ptr() != gots[1].planes.data_ptr()
        assert bool((want.planes[0] == 0).any()) and bool((want.planes[0] > 0).any())
    else:
        assert gots[0].data_ptr() != gots[1].data_ptr()
        assert bool((want == 0).any()) and bool((want > 0).any())      # the ReLU bit, and not everywhere


@pytest.mark.parametrize("planes_in", [False, True])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("cin", [64, 512])
@pytest.mark.parametrize("cout", [128, 384])
@pytest.mark.parametrize("n", N_ROIS)
def test_staged_records_equal_the_unfused_path(data, n, cout, cin, layout, planes_in):
    check(data, n, cout, cin, layout, planes_in)


@pytest.mark.parametrize("planes_in", [False, True])
@pytest.mark.parametrize("n,layout", [(3, 1), (6, 0), (11, 1)])
def test_plane_output(data, n, layout, planes_in):
    check(data, n, 384, 64, layout, planes_in, planes_out=True)


@pytest.mark.parametrize("planes_in", [False, True])
@pytest.mark.parametrize("n,layout", [(3, 0), (11, 1)])
def test_one_chunk_of_reduction(data, n, layout, planes_in):
    """Cin = 32: the main loop is a single chunk, the epilogue starts right behind the first barrier of the launch."""
    check(data, n, 384, 32, layout, planes_in)


@pytest.mark.parametrize("planes_in", [False, True])
@pytest.mark.parametrize("n,layout", [(6, 0), (11, 1)])
def test_without_a_fill_vector(data, n, layout, planes_in):
    """res_fill = NULL: a rejected RoI yields zeros, as the resampling kernel does without a fill vector."""
    check(data, n, 384, 64, layout, planes_in, with_fill=False)
