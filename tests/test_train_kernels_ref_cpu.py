"""The references of tests/train_kernels_ref.py checked against each other and against torch, so that a wrong reference cannot
pass a wrong kernel in tests/test_train_kernels_gpu.py."""
import numpy as np
import torch

from oracle import keras_train_ref as ktr
from tests import train_kernels_ref as R


def test_maxpool_bwd_first_vs_torch_autograd_tie_free():
    rs = np.random.RandomState(0)
    for (n, H, W, C), k in (((2, 6, 8, 3), 2), ((1, 7, 9, 5), 2), ((1, 9, 10, 4), 3)):
        x = rs.permutation(n * H * W * C).reshape(n, H, W, C).astype(np.float32)          # all distinct: no ties
        gy = rs.randn(n, H // k, W // k, C).astype(np.float32)
        xt = torch.from_numpy(x).permute(0, 3, 1, 2).double().requires_grad_(True)
        y = torch.nn.functional.max_pool2d(xt, k, k)
        y.backward(torch.from_numpy(gy).permute(0, 3, 1, 2).double())
        assert np.array_equal(R.maxpool_bwd_first(x, gy, k), xt.grad.permute(0, 2, 3, 1).numpy().astype(np.float32))


def test_maxpool_bwd_first_vs_literal_loop_with_ties():
    rs = np.random.RandomState(1)
    for (n, H, W, C), k in (((2, 5, 7, 3), 2), ((1, 7, 6, 2), 3)):
        x = np.maximum(rs.randn(n, H, W, C), 0).astype(np.float32)                          # post-ReLU: most windows tie at 0
        x[0, :k, :k, 0] = 0.0
        x[0, 0, 0, 0] = -0.0                                                                # -0.0 == +0.0: the first one wins
        x[0, 2:4, 2:4, 1] = 3.0                                                             # a window of one repeated value
        gy = rs.randn(n, H // k, W // k, C).astype(np.float32)
        a, b = R.maxpool_bwd_first(x, gy, k), R.maxpool_bwd_loops(x, gy, k)
        assert np.array_equal(a, b)
        assert a[0, 0, 0, 0] == gy[0, 0, 0, 0] and a[0, 0, 1, 0] == 0
        assert np.count_nonzero(a) <= gy.size and not a[:, (H // k) * k:].any() and not a[:, :, (W // k) * k:].any()


def test_bf16_rne_vs_torch():
    rs = np.random.RandomState(2)
    bits = rs.randint(0, 2 ** 32, size=1 << 20, dtype=np.uint64).astype(np.uint32)
    edge = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0, 0x80000000,
                     1, 0x007FFFFF, 0x00008000, 0x00018000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32)
    x = np.concatenate([edge, bits]).view(np.float32)
    got = R.bf16_bits_rne(x)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], want[~nan])
    assert R.bf16_is_nan(got[nan]).all() and R.bf16_is_nan(want[nan]).all()
    assert got[0] == 0x3F80 and got[1] == 0x3F82 and got[4] == 0x7F80                      # ties to even both ways; FLT_MAX -> inf
    # half a bf16 ulp: reached exactly by the ties, 2^-8 of 1 + 2^-8 (so no flat 2^-9 |x| bound can hold), never exceeded
    fin = np.isfinite(x) & (np.abs(x) > 2.0 ** -120) & (np.abs(x) < 3e38)
    err = np.abs(R.bf16_bits_to_f32(got[fin]).astype(np.float64) - x[fin].astype(np.float64))
    assert (err <= R.bf16_half_ulp(x[fin])).all() and err[0] == 2.0 ** -8 == R.bf16_half_ulp(x[0])
    assert (err > 2.0 ** -9 * np.abs(x[fin].astype(np.float64))).any()
    allb = np.arange(65536, dtype=np.uint16)
    back = torch.from_numpy(allb.view(np.int16).copy()).view(torch.bfloat16).float().numpy()
    assert np.array_equal(R.bf16_bits_to_f32(allb).view(np.uint32), back.view(np.uint32))


def _rpn_case(rs, cells, A):
    yc = np.concatenate([rs.rand(cells, A) < 0.5, rs.rand(cells, A) < 0.3], axis=1).astype(np.float32)
    p = rs.rand(cells, A).astype(np.float32)
    flat = p.reshape(-1)
    special = [0.0, 1.0, 5e-8, 1 - 2.0 ** -24, R.CLIP_LO, R.CLIP_HI]
    flat[:min(len(special), flat.size)] = special[:flat.size]
    yr = np.concatenate([np.repeat(rs.rand(cells, A) < 0.3, 4, axis=1), rs.randn(cells, 4 * A) * 2], axis=1).astype(np.float32)
    pr = rs.randn(cells, 4 * A).astype(np.float32)
    return yc, p, yr, pr


def test_loss_closed_forms_vs_autograd():
    rs = np.random.RandomState(3)
    for cells, A in ((1, 1), (7, 9), (40, 15)):
        yc, p, yr, pr = _rpn_case(rs, cells, A)
        for i in range(min(6, cells * A)):
            yc[i // A, i % A] = 1                                      # the special probabilities are selected anchors
        l, g = R.rpn_cls_autograd(yc, p, A)
        lc, gc, bl, bg = R.rpn_cls_closed(yc, p, A)
        assert abs(l - lc) <= 1e-12 * max(1.0, abs(l)) and np.abs(g - gc).max() <= 1e-9 / 256
        flat = g.reshape(-1)
        assert flat[0] == 0 and (cells * A < 4 or (flat[1] == 0 and flat[2] == 0 and flat[3] == 0))     # clipped: exactly 0
        assert cells * A < 6 or (flat[4] != 0 and flat[5] != 0)                                        # ON a bound: not clipped
        l, g = R.rpn_reg_autograd(yr, pr, A)
        lc, gc, _, _ = R.rpn_reg_closed(yr, pr, A)
        assert abs(l - lc) <= 1e-12 * max(1.0, abs(l)) and np.abs(g - gc).max() <= 1e-15
    # an f64 clip at 1 - 1e-7 is NOT what f32 Keras does: the f32 upper bound is 1 - 2^-23
    assert float(R.CLIP_HI) == 1 - 2.0 ** -23 and float(R.CLIP_LO) > 1e-7
    for n, C in ((1, 2), (5, 21), (64, 81)):
        x = rs.randn(n, C)
        p = torch.softmax(torch.from_numpy(x), dim=1).numpy().astype(np.float32)
        y = np.eye(C, dtype=np.float32)[rs.randint(0, C, n)]
        if n >= 5:
            p[1] = 1.0 / (C - 1); p[1, y[1].argmax()] = 0.0               # true class at 0: clipped
            p[2] = 0.0; p[2, y[2].argmax()] = 1.0                         # true class at 1: clipped
        l, g = R.det_cls_autograd(y, p, x)
        lc, gc, bl, bg = R.det_cls_closed(y, p)
        assert abs(l - lc) <= 1e-12 * max(1.0, abs(l))
        assert (np.abs(g - gc) <= bg).all() and (n < 5 or (not g[1].any() and not g[2].any()))
        K = C - 1
        yr = np.concatenate([np.repeat(y[:, :K], 4, axis=1), rs.randn(n, 4 * K)], axis=1).astype(np.float32)
        pr = rs.randn(n, 4 * K).astype(np.float32)
        l, g = R.det_reg_autograd(yr, pr, K)
        m, t = R.f64(yr[:, :4 * K]), R.f64(yr[:, 4 * K:])
        v, s = R._smooth_l1(t - R.f64(pr))
        assert abs(l - (m * v).sum() / (1e-4 + m).sum()) <= 1e-12 and np.abs(g + m * s / (1e-4 + m).sum()).max() <= 1e-15


def test_smooth_l1_seam_same_from_both_sides():
    d = np.array([1.0, -1.0, 0.0])
    v, s = R._smooth_l1(d)
    assert np.array_equal(v, [0.5, 0.5, 0.0]) and np.array_equal(s, [1.0, -1.0, 0.0])
    assert np.array_equal(np.abs(d) - 0.5, [0.5, 0.5, -0.5])              # the other branch agrees at |d| = 1


def test_optimiser_refs_vs_oracle_optim():
    """oracle.keras_train_ref.Optim from the same f32 state.  Optim hard-codes beta1 = 0.9, beta2 = 0.999, eps = 1e-8 in f64 where the
    kernels receive their f32 roundings (1 - 0.999f is 1.3e-5 away from 0.001), so the Adam reference is asked for the f64 scalars
    here (as_f32=False): then only f64 rounding separates the two."""
    rs = np.random.RandomState(4)
    w0, g, s1, s2 = (rs.randn(37).astype(np.float32) for _ in range(4))
    s2 = np.abs(s2)
    T = lambda a: torch.from_numpy(R.f64(a))
    lr = float(np.float32(1e-3))
    for slot in (np.zeros(37, np.float32), s1):                          # the first step after compile(), and a later one
        opt = ktr.Optim("sgd", lr, 0.5)
        opt.slots["w"] = T(slot)
        want = opt.step({"w": T(w0)}, {"w": T(g)})["w"].numpy()
        wn, vn, _, _ = R.sgd_momentum(w0, g, slot, lr, 0.5, 0.0, 1.0)
        assert np.abs(want - wn).max() <= 1e-15 and np.abs(opt.slots["w"].numpy() - vn).max() <= 1e-15
    for t, m0, v0 in ((1, np.zeros(37, np.float32), np.zeros(37, np.float32)), (2, s1, s2), (1000, s1, s2)):
        opt = ktr.Optim("adam", lr)
        opt.t, opt.slots["w"] = t - 1, (T(m0), T(v0))
        want = opt.step({"w": T(w0)}, {"w": T(g)})["w"].numpy()
        wn, mn, vn = R.adam(w0, g, m0, v0, lr, 0.9, 0.999, 1e-8, t, 0.0, 1.0, as_f32=False)[:3]
        assert np.abs(want - wn).max() <= 1e-15
        assert np.abs(opt.slots["w"][0].numpy() - mn).max() <= 1e-15 and np.abs(opt.slots["w"][1].numpy() - vn).max() <= 1e-15
        assert abs(R.adam_lr_t(lr, 0.9, 0.999, t) / R.adam_lr_t(lr, 0.9, 0.999, t, as_f32=False) - 1) < 1e-5
    # L2 and the gradient scale enter as g*gs + 2 l2 w
    wn, vn, bw, bv = R.sgd_momentum(w0, g, s1, 0.25, 0.5, 0.125, 0.125)
    want = 0.5 * R.f64(s1) - 0.25 * (R.f64(g) * 0.125 + 0.25 * R.f64(w0))
    assert np.abs(vn - want).max() <= 1e-15 and np.abs(wn - (R.f64(w0) + want)).max() <= 1e-15 and (bw > 0).all()
    wn, mn, vn = R.adam(w0, g, s1, s2, lr, 0.5, 0.5, 0.0, 1, 0.125, 0.125)[:3]
    gi = R.f64(g) * 0.125 + 0.25 * R.f64(w0)
    assert np.abs(mn - (0.5 * R.f64(s1) + 0.5 * gi)).max() <= 1e-15 and np.abs(vn - (0.5 * R.f64(s2) + 0.5 * gi * gi)).max() <= 1e-15
    z = np.zeros(5, np.float32)
    wn, mn, vn, bw, bm, bv = R.adam(w0[:5], z, z, z, lr, 0.9, 0.999, 1e-8, 1, 0.0, 1.0)
    assert np.array_equal(wn, R.f64(w0[:5])) and not mn.any() and not vn.any() and np.isfinite(bw).all()


def test_softmax_and_pool_refs():
    rs = np.random.RandomState(5)
    x = (rs.randn(9, 33) * 10).astype(np.float32)
    x[3] = 2.5; x[4, ::2], x[4, 1::2] = 1e4, -1e4
    y, b = R.softmax_rows(x)
    assert np.abs(y - torch.softmax(torch.from_numpy(x).double(), dim=1).numpy()).max() <= 1e-15
    assert np.allclose(y[3], 1 / 33, rtol=1e-15) and (b > 0).all() and (b < 1e-4).all()
    v, b = R.avgpool_mean(rs.randn(4, 3, 8), 0)
    assert v.shape == (3, 8) and (b > 0).all()
    s, b = R.sumsq(np.array([3.0, 4.0], np.float32))
    assert s == 25.0 and 0 < b < 1e-5
    g = R.relu_bwd(np.array([1.0, 2.0, 3.0, 4.0], np.float32), np.array([-0.0, 0.0, 1e-45, -1.0], np.float32))
    assert np.array_equal(g, [0, 0, 3, 0])
