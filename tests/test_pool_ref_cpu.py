"""The numpy pooling references of tests/pool_ref.py against oracle.keras_ref.pool2d and against each other, and the conditions on the
inputs that tests/test_pool_kernels_gpu.py relies on (no GPU needed)."""
import numpy as np
import pytest
import torch

from oracle import keras_ref
from tests import pool_ref as R


def tag(case):
    return "n%d %dx%d c%d %d/%d" % case


@pytest.mark.parametrize("case", R.SMALL, ids=tag)
def test_max_and_mean_equal_the_oracle(case):
    k, s = case[4:]
    x = R.position_coded(case).astype(np.float64)
    want_max = keras_ref.pool2d(torch.from_numpy(x), k, s, True).numpy()
    got_max = R.pool_max(x, k, s)
    assert got_max.shape == want_max.shape and got_max.tobytes() == want_max.tobytes()
    want_avg = keras_ref.pool2d(torch.from_numpy(x), k, s, False).numpy()
    mean, mag = R.pool_avg64(x, k, s)
    # two float64 summations of the same k^2 terms in different orders: each within k^2 2^-53 sum|x| / k^2 of the exact mean
    assert mean.shape == want_avg.shape and (np.abs(mean - want_avg) <= 2 * k * k * 2.0 ** -53 * mag).all()
    assert (mag >= np.abs(mean)).all()


@pytest.mark.parametrize("case", R.CASES, ids=tag)
def test_sequential_f32_mean_within_its_bar(case):
    k, s = case[4:]
    x = R.position_coded(case)
    mean, mag = R.pool_avg64(x, k, s)
    seq = R.pool_avg32_seq(x, k, s)
    assert seq.dtype == np.float32 and seq.shape == mean.shape
    assert (np.abs(seq.astype(np.float64) - mean) <= R.avg_bound(mag, k)).all()
    if k == 1:
        assert seq.tobytes() == np.ascontiguousarray(x[:, ::s, ::s]).tobytes()


def test_sequential_mean_starts_from_plus_zero_and_divides_once():
    x = np.array([-0.0, -0.0, -0.0, -0.0], np.float32).reshape(1, 2, 2, 1)
    assert not np.signbit(R.pool_avg32_seq(x, 2, 2)).any()                   # +0.0 + -0.0 = +0.0
    x = np.array([1, 1, 1, 2 ** -24, 0, 0, 0, 0, 0], np.float32).reshape(1, 3, 3, 1)
    assert R.pool_avg32_seq(x, 3, 3)[0, 0, 0, 0] == np.float32(3.0) / np.float32(9.0)     # 3 + 2^-24 rounds to 3: raster order, f32 partial sums
    back = np.ascontiguousarray(x[:, ::-1, ::-1])                              # the small term first: 2^-24 + 1 rounds to 1 all the same ...
    assert R.pool_avg32_seq(back, 3, 3)[0, 0, 0, 0] == np.float32(3.0) / np.float32(9.0)
    x = np.array([2 ** -24, 2 ** -24, 1, 0, 0, 0, 0, 0, 0], np.float32).reshape(1, 3, 3, 1)     # ... but two small terms first add up to one ulp of 1
    assert R.pool_avg32_seq(x, 3, 3)[0, 0, 0, 0] == np.float32(np.float32(1.0 + 2.0 ** -23) / np.float32(9.0))
    assert R.pool_avg32_seq(np.ascontiguousarray(x[:, ::-1, ::-1]), 3, 3)[0, 0, 0, 0] == np.float32(1.0) / np.float32(9.0)
    x = np.full((1, 3, 3, 1), 0.1, np.float32)
    acc = np.float32(0)
    for _ in range(9):
        acc = np.float32(acc + np.float32(0.1))
    assert R.pool_avg32_seq(x, 3, 3)[0, 0, 0, 0] == np.float32(acc / np.float32(9))


def test_windows_drop_what_no_window_covers():
    x = np.zeros((1, 15, 20, 4), np.float32)
    x[:, 14:, :, :] = 9.0                                                      # row 14 and columns 14.. lie outside every 7/7 window
    x[:, :, 14:, :] = 9.0
    assert R.pool_max(x, 7, 7).shape == (1, 2, 2, 4) and not R.pool_max(x, 7, 7).any()
    x = np.zeros((1, 8, 11, 4), np.float32)                                    # 2/3: columns 2, 5, 8 and rows 2, 5 fall in the holes
    x[:, [2, 5], :, :] = 9.0
    x[:, :, [2, 5, 8], :] = 9.0
    assert R.pool_max(x, 2, 3).shape == (1, 3, 4, 4) and not R.pool_max(x, 2, 3).any()


@pytest.mark.parametrize("case", R.PLANE_CASES, ids=tag)
def test_planes_model_and_the_share_left_out_of_the_bit_comparison(case):
    k, s = case[4:]
    x = R.position_coded(case)
    e = R.plane_exponent(np.abs(x).max())
    assert 2.0 ** 14 <= float(np.abs(x).max()) * 2.0 ** e < 2.0 ** 15
    for v in (R.pool_max(x, k, s), R.pool_avg32_seq(x, k, s)):
        hi, lo, back = R.planes_model(v, e)
        assert np.isfinite(hi).all() and np.isfinite(lo).all() and R.status_bits(hi) == 0
        assert (np.abs(back - v.astype(np.float64)) <= R.plane_bound(v)).all()
        # the GPU test leaves these out of the hi plane's bit comparison: a condition on the inputs, so that it cannot hide a failure
        assert R.below_f16_normal(v, e).mean() <= 1e-3


def test_status_rule():
    f = lambda bits: R.status_bits(np.array([0x3C00, bits], np.uint16).view(np.float16))
    assert [f(b) for b in (0x0000, 0x77FF, 0x7800, 0x7BFE, 0x7BFF, 0x7C00, 0x7E00)] == [0, 0, 1, 1, 3, 7, 7]
    assert [f(b | 0x8000) for b in (0x77FF, 0x7800, 0x7BFF, 0x7C00)] == [0, 1, 3, 7]            # the sign does not count


@pytest.mark.parametrize("case", R.STATUS_CASES, ids=tag)
def test_status_inputs_keep_everything_but_the_peak_quiet(case):
    x, peak = R.status_input(case)
    e = R.plane_exponent(peak)
    assert peak * 2.0 ** e == 2.0 ** 14 and float(np.abs(x).max()) * 2.0 ** (e + 3) <= 2.0 ** 14
    one = np.array([peak, -peak], np.float32)
    assert R.status_bits(R.planes_model(one, e)[0]) == 0
    assert R.planes_model(one, e + 1)[0].view(np.uint16).tolist() == [0x7800, 0xF800] and R.status_bits(R.planes_model(one, e + 1)[0]) == 1
    near = np.array([65472.0 / 2.0 ** (e + 1)], np.float32)                    # 0x7bfe after scaling: the largest pattern that is only H3_UNDER
    assert R.planes_model(near, e + 1)[0].view(np.uint16).tolist() == [0x7BFE] and float(near[0]) * 2.0 ** e < 2.0 ** 15
