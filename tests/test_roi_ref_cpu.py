"""The references of tests/roi_ref.py against the oracle (oracle.keras_ref.roi_resize / roi_resize_torch) and against each other.
No GPU: what tests/test_roi_kernels_gpu.py holds the kernels to is itself checked here."""
import numpy as np
import pytest

from oracle import keras_ref
from tests import roi_ref as R

torch = pytest.importorskip("torch")

ROWS, COLS = 9, 13
# accepted boxes only (the oracle has no rejection rule): whole map, 1x1 corners, strips, fractional and (-1, 0) corners, edges
VALID = np.array([[0, 0, 13, 9], [0, 0, 1, 1], [12, 8, 13, 9], [4, 0, 5, 9], [0, 3, 13, 4], [2, 1, 8, 7], [2, 1, 9, 8], [1, 0, 9, 8],
                  [0, 0, 13, 7], [3.2, 1.9, 8.5, 5.9], [-0.7, -0.7, 5.9, 3.2], [6, 2, 13.9, 9.9], [2, 1, 8, 7]], np.float32)


@pytest.mark.parametrize("pool", [1, 2, 7, 14])
def test_fwd_f32_is_the_oracle_bit_for_bit(pool):
    rs = np.random.RandomState(pool)
    feat = rs.randn(ROWS, COLS, 12).astype(np.float32)
    got = R.fwd_f32(feat, VALID, pool)
    want = keras_ref.roi_resize(feat, VALID, pool)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    # position-major is the transpose; ReLU clamps; a batch of maps reads image r // n_per_img
    assert np.array_equal(R.fwd_f32(feat, VALID, pool, relu=True, layout=1), np.maximum(want, 0).transpose(1, 2, 0, 3))
    maps = np.stack([feat, feat[::-1].copy(), -feat])
    b = R.fwd_f32(maps, VALID, pool, n_per_img=5)
    for i in range(3):
        assert np.array_equal(b[5 * i:5 * i + 5], keras_ref.roi_resize(maps[i], VALID[5 * i:5 * i + 5], pool))


@pytest.mark.parametrize("pool", [1, 2, 7, 14])
def test_fwd_f64_is_the_torch_oracle_in_float64(pool):
    """Both lerp in f64 from the same f32 fractions: they differ by f64 roundings only, and the f32 reference stays inside its own
    derived bar of the f64 one."""
    rs = np.random.RandomState(10 + pool)
    feat = rs.randn(ROWS, COLS, 12).astype(np.float32)
    val, mag, err = R.fwd_f64(feat, VALID, pool)
    want = keras_ref.roi_resize_torch(torch.from_numpy(feat).double(), VALID, pool).numpy()
    assert np.abs(val - want).max() <= 2.0 ** -48 * np.abs(feat).max()
    assert (mag >= np.abs(val) * (1 - 2.0 ** -40)).all()
    d = np.abs(R.fwd_f32(feat, VALID, pool).astype(np.float64) - val)
    print("fwd_f32 vs fwd_f64, pool %d: max err/bound %.3f" % (pool, (d / np.maximum(err, 1e-300)).max()))
    assert (d <= err).all()


def test_fill_relu_and_rejected_rois():
    rs = np.random.RandomState(3)
    feat = rs.randn(ROWS, COLS, 4).astype(np.float32)
    fill = np.array([-1.5, 2.0, 0.0, -0.25], np.float32)
    rois = np.array([[2, 1, 8, 7], [5, 5, 5, 8], [0, 0, 14, 9]], np.float32)          # accepted, w = 0, x2 = cols + 1
    out = R.fwd_f32(feat, rois, 3, fill=fill)
    assert np.array_equal(out[0], keras_ref.roi_resize(feat, rois[:1], 3)[0])
    assert (out[1] == fill).all() and (out[2] == fill).all()
    assert (R.fwd_f32(feat, rois, 3)[1:] == 0).all()
    assert (R.fwd_f32(feat, rois, 3, fill=fill, relu=True)[1:] == np.maximum(fill, 0)).all()
    val, mag, err = R.fwd_f64(feat, rois, 3, fill=fill, relu=True, layout=1)
    assert val.shape == (3, 3, 3, 4) and (val[:, :, 1] == np.maximum(fill, 0)).all() and (err[:, :, 1:] == 0).all()


# (roi, accepted, truncated corners) on the 9 x 13 map -- written out by hand
PREDICATE = [
    ([2, 1, 8, 7], True, (2, 1, 8, 7)),
    ([5.9, 3.2, 8.5, 6.99], True, (5, 3, 8, 6)),                # fractions truncate
    ([-0.7, -0.99, 3, 3], True, (0, 0, 3, 3)),                  # (-1, 0) truncates to 0: accepted where a floor (-1) would reject
    ([0, 0, 13, 9], True, (0, 0, 13, 9)),                       # x2 == cols, y2 == rows
    ([0, 0, 13.9, 9.9], True, (0, 0, 13, 9)),                   # cols + 0.9 still truncates to cols
    ([12, 8, 13, 9], True, (12, 8, 13, 9)),
    ([3, 4, 9, 4], False, (3, 4, 9, 4)),                        # h = 0
    ([3, 4, 3.9, 8], False, (3, 4, 3, 8)),                      # w = 0 after truncation
    ([8, 7, 2, 1], False, (8, 7, 2, 1)),                        # inverted
    ([-1, 0, 5, 5], False, (-1, 0, 5, 5)),                      # x1 = -1
    ([0, -1.5, 5, 5], False, (0, -1, 5, 5)),                    # y1 = -1.5 -> -1
    ([0, 0, 14, 9], False, (0, 0, 14, 9)),                      # x2 = cols + 1
    ([0, 0, 13, 10], False, (0, 0, 13, 10)),                    # y2 = rows + 1
    ([0, 0, 0.9, 0.9], False, (0, 0, 0, 0)),                    # empty after truncation
]


@pytest.mark.parametrize("roi,ok,corners", PREDICATE)
def test_predicate_table(roi, ok, corners):
    assert R.trunc_corners(roi) == corners
    assert R.accepted(roi, ROWS, COLS) is ok
    tp = R.taps(roi, 7, ROWS, COLS)
    assert (tp is not None) is ok
    if ok:
        y_lo, y_hi, ty, x_lo, x_hi, tx = tp
        x1, y1, x2, y2 = corners
        assert y_lo.min() >= y1 and y_hi.max() <= y2 - 1 and x_lo.min() >= x1 and x_hi.max() <= x2 - 1
        assert (y_hi - y_lo <= 1).all() and (x_hi - x_lo <= 1).all() and ty.dtype == np.float32
        assert (0 <= ty).all() and (ty < 1).all() and (0 <= tx).all() and (tx < 1).all()


def test_taps_known_values():
    """h = 3 over pool 2: scale 1.5, sources 0 and 1.5; w = 1: every source on the one column, fraction irrelevant (lo == hi)."""
    y_lo, y_hi, ty, x_lo, x_hi, tx = R.taps([4, 2, 5, 5], 2, ROWS, COLS)
    assert y_lo.tolist() == [2, 3] and y_hi.tolist() == [3, 4] and ty.tolist() == [0.0, 0.5]
    assert x_lo.tolist() == [4, 4] and x_hi.tolist() == [4, 4] and tx.tolist() == [0.0, 0.5]
    # extent 2 * pool: integer sources, every fraction 0
    y_lo, y_hi, ty, _, _, _ = R.taps([0, 0, 13, 8], 4, ROWS, COLS)
    assert y_lo.tolist() == [0, 2, 4, 6] and y_hi.tolist() == [1, 3, 5, 7] and not ty.any()


@pytest.mark.parametrize("pool", [1, 2, 7, 14])
def test_bwd_f64_is_float64_autograd_and_bwd_seq_f32_stays_in_its_bar(pool):
    rs = np.random.RandomState(20 + pool)
    C = 5
    rois = np.concatenate([VALID, [[3, 4, 3.9, 8], [0, 0, 14, 9]]]).astype(np.float32)      # two rejected ones at the end: no gradient
    dout = rs.randn(len(rois), pool, pool, C).astype(np.float32)
    val, cnt, mag = R.bwd_f64(dout, rois, ROWS, COLS, pool)
    x = torch.zeros(ROWS, COLS, C, dtype=torch.float64, requires_grad=True)
    y = keras_ref.roi_resize_torch(x, VALID, pool)
    y.backward(torch.from_numpy(dout[:len(VALID)]).double())
    want = x.grad.numpy()
    # the reference's weights are the f32 fl(1 - t), autograd's the exact 1 - t: two weights per tap, U each
    assert (np.abs(val - want) <= (2 * R.U + 2.0 ** -45) * mag + 1e-300).all()
    assert cnt.sum() == 4 * pool * pool * len(VALID) and (mag[cnt == 0] == 0).all()
    seq = R.bwd_seq_f32(dout, rois, ROWS, COLS, pool)
    assert seq.dtype == np.float32 and not seq[cnt == 0].any()
    d, bar = np.abs(seq.astype(np.float64) - val), R.bwd_bar(cnt, mag)
    print("bwd_seq_f32 vs bwd_f64, pool %d: max err/bound %.3f" % (pool, (d[bar > 0] / bar[bar > 0]).max()))
    assert (d <= bar).all()


def test_bf16_helpers():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -2.5, 0.0], np.float32)
    bits = R.bf16_bits_rne(x)
    assert bits.tolist() == [0x3F80, 0x3F80, 0x3F82, 0xC020, 0x0000]               # ties go to the even pattern
    y = np.random.RandomState(0).randn(4096).astype(np.float32)
    assert np.array_equal(R.bf16_bits_rne(y).view(np.int16), torch.from_numpy(y).bfloat16().view(torch.int16).numpy())
    assert R.bf16_bits_to_f32(bits)[3] == -2.5
    assert R.bf16_half_ulp(np.array([1.0, 1.5, 2.0, 0.0])).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 0.0]
