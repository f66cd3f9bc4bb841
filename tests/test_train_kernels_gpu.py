"""Per-kernel parity of the small kernels between the conv engines on the training path and at the detector head: the four losses
(csrc/train.hip), ReLU / max-pool / average-pool backward, SGD-momentum, Adam, sum of squares, the bias fold, the dense-head split and
the position-major average pool (csrc/pool.hip), the bf16 helpers (csrc/conv_bf16.hip, csrc/roi.hip).

Each kernel is called through the C ABI (or the ops wrapper the product uses) and compared over the WHOLE tensor with the references of
tests/train_kernels_ref.py: bit for bit where the source claims it, elsewhere within a bound counted from the kernel's own roundings
(U = 2^-24 per f32 operation, 4 ulp ASSUMED for logf / expf / log1pf, half a bf16 ulp for a bf16 result; the count stands next to each reference).
Every comparison prints `name: max |err| / bound` (pytest -s) so the margin is on record; a bound of 0 means equality.
Sizes above 4096 * 256 elements take a second trip round the grid-stride loops (ew_grid caps the grid at 4096 workgroups)."""
import ctypes

import numpy as np
import pytest

from tests import train_kernels_ref as R

pytestmark = pytest.mark.gpu

TRIP = 4096 * 256                            # elements one trip of a capped elementwise grid covers


@pytest.fixture(scope="module")
def G():
    import torch
    from faster_rcnn_amd import _lib, ops

    class _G:
        pass
    g = _G()
    g.torch, g.lib, g.ops = torch, _lib, ops
    g.dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    g.call = lambda name, *a: _lib.call(name, *a, ops._stream())
    g.ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off) if t is not None else None
    return g


def within(name, got, want, bound):
    """|got - want| <= bound everywhere (bound 0: equal), printing the largest share of the bound any element uses."""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(want))
    assert got.shape == want.shape and np.isfinite(got).all(), name
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    print("%-44s max|err| %.3e  max err/bound %.3f" % (name, err.max() if err.size else 0.0, share.max() if share.size else 0.0))
    assert (err <= bound).all(), "%s: %d of %d outside the bound, worst err/bound %.3f" % (name, int((err > bound).sum()), err.size, share.max())


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint8).tobytes()


def bf16_dev(G, bits16):
    return G.dev(np.asarray(bits16, np.uint16).view(np.int16)).view(G.torch.bfloat16)


# ----------------------------------------------------------------------------- losses
def _loss(G, name, yt, yp, a, b, grad=True, ldg=None, gbuf=None, goff=0):
    """One loss call.  Returns (loss f32 scalar as numpy, gradient array or None)."""
    t = G.torch
    ytd, ypd = G.dev(np.asarray(yt, np.float32)), G.dev(np.asarray(yp, np.float32))
    loss = t.full((1,), -7.0, dtype=t.float32, device="cuda")
    g = None
    if grad:
        g = gbuf if gbuf is not None else t.full(ypd.shape, -7.0, dtype=t.float32, device="cuda")
    args = [G.ptr(ytd), G.ptr(ypd), a, b, G.ptr(loss), G.ptr(g, 4 * goff) if g is not None else None]
    if "_det_" in name:
        args.append(ldg if ldg is not None else ypd.shape[1])
    if name.endswith("_ws"):
        ws = t.zeros(G.lib.load().frcnn_loss_workspace_bytes(), dtype=t.uint8, device="cuda")
        args.append(G.ptr(ws))
    G.call(name, *args)
    return loss.cpu().numpy()[0], (g.cpu().numpy() if g is not None else None)


RPN_SHAPES = [(1, 1), (5, 1), (7, 9), (1000, 9), (2394, 9), (2394, 15), (9500, 15)]
P_SPECIAL = [0.0, 1.0, 5e-8, 1 - 2.0 ** -24, R.CLIP_LO, R.CLIP_HI]       # four clipped (gradient exactly 0), two ON the bounds (not clipped)


def _rpn_inputs(cells, A, mask):
    rs = np.random.RandomState(cells * 31 + A)
    n = cells * A
    sel = {"rand": rs.rand(cells, A) < 0.5, "zero": np.zeros((cells, A), bool), "one": np.ones((cells, A), bool)}[mask]
    z = rs.rand(cells, A) < 0.3
    p = (0.01 + 0.98 * rs.rand(cells, A)).astype(np.float32)                # clear of both clip bounds
    for rep in range(2):                                                    # the special probabilities, each under z = 0 and z = 1 ...
        for j, v in enumerate(P_SPECIAL):
            i = rep * len(P_SPECIAL) + j
            if i < n:
                p[i // A, i % A], z[i // A, i % A] = v, bool(rep)
                if mask == "rand":
                    sel[i // A, i % A] = True
    if mask == "rand" and n > 30:                                           # ... and on unselected anchors (rpn_cls: gradient exactly 0)
        for j, v in enumerate(P_SPECIAL):
            i = n - 1 - j
            p[i // A, i % A], sel[i // A, i % A] = v, False
    yc = np.concatenate([sel, z], axis=1).astype(np.float32)
    m4 = {"rand": np.repeat(rs.rand(cells, A) < 0.3, 4, axis=1), "zero": np.zeros((cells, 4 * A), bool), "one": np.ones((cells, 4 * A), bool)}[mask]
    pred = rs.randn(cells, 4 * A).astype(np.float32)
    tgt = (pred + 2 * rs.randn(cells, 4 * A)).astype(np.float32)
    for i, d in enumerate((1.0, -1.0, 0.0)):                               # the smooth-L1 seam and its centre, exactly
        if i < 4 * n:
            pred[i // (4 * A), i % (4 * A)] = 0.5
            tgt[i // (4 * A), i % (4 * A)] = 0.5 + d
    yr = np.concatenate([m4, tgt], axis=1).astype(np.float32)
    return yc, p, yr, pred


@pytest.mark.parametrize("cells,A", RPN_SHAPES)
@pytest.mark.parametrize("mask", ["rand", "zero", "one"])
def test_rpn_losses(G, cells, A, mask):
    yc, p, yr, pred = _rpn_inputs(cells, A, mask)
    tag = "%dx%d/%s" % (cells, A, mask)
    for name, yt, yp, auto, closed in (("frcnn_loss_rpn_cls", yc, p, R.rpn_cls_autograd, R.rpn_cls_closed),
                                       ("frcnn_loss_rpn_reg", yr, pred, R.rpn_reg_autograd, R.rpn_reg_closed)):
        l_ref, g_ref = auto(yt, yp, A)
        l_cf, g_cf, bl, bg = closed(yt, yp, A)
        l1, g1 = _loss(G, name, yt, yp, cells, A)
        l0, _ = _loss(G, name, yt, yp, cells, A, grad=False)
        lw, gw = _loss(G, name + "_ws", yt, yp, cells, A)
        lw2, gw2 = _loss(G, name + "_ws", yt, yp, cells, A)
        lw0, _ = _loss(G, name + "_ws", yt, yp, cells, A, grad=False)
        assert l0.tobytes() == l1.tobytes() and lw0.tobytes() == lw.tobytes(), "a null gradient pointer changed the loss"
        assert (lw.tobytes(), gw.tobytes()) == (lw2.tobytes(), gw2.tobytes()), "the _ws form is not reproducible"
        assert g1.tobytes() == gw.tobytes(), "the _ws gradient differs from the one-workgroup form's"
        # bars: R.rpn_cls_closed (per term U (2 + 8 |x|) through logf, 32 U on the softplus, 2 U bce; + U loss; gradient 2 U |g|),
        # R.rpn_reg_closed (3 U per term + one cast = 4 U loss; gradient 3 U |g|)
        within("%s %s loss" % (name[11:], tag), l1, l_ref, bl)
        within("%s_ws %s loss" % (name[11:], tag), lw, l_ref, bl)
        within("%s %s grad vs autograd" % (name[11:], tag), g1, g_ref, bg)
        within("%s_ws %s grad vs closed form" % (name[11:], tag), gw, g_cf, bg)
    # what must be exactly zero, and what must not
    _, g = _loss(G, "frcnn_loss_rpn_cls", yc, p, cells, A)
    sel, pf = yc[:, :A] != 0, p
    clipped = (pf < R.CLIP_LO) | (pf > R.CLIP_HI)
    assert not g[~sel].any() and not g[clipped].any()
    assert (g[sel & ~clipped & (pf != yc[:, A:])] != 0).all()
    _, gr = _loss(G, "frcnn_loss_rpn_reg", yr, pred, cells, A)
    d = yr[:, 4 * A:].astype(np.float64) - pred.astype(np.float64)
    if not yr[:, :4 * A].any():
        assert not gr.any()                                                  # mean(mask) = 0: the whole loss is 0
    else:
        assert (gr[d != 0] != 0).all()                                       # the mask is OUTSIDE the sum: unselected anchors have a gradient


DET_N, DET_C = [1, 4, 64, 300, 2400], [2, 21, 81]


def _det_inputs(n, C, mask):
    rs = np.random.RandomState(n * 131 + C)
    K4 = 4 * (C - 1)
    x = rs.randn(n, C)                                                     # sigma 1: every share stays above 1e-6, clear of the clip bounds
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    cls = rs.randint(0, C, n)
    y = np.eye(C, dtype=np.float32)[cls]
    if n >= 4:
        p[1] = 1.0 / (C - 1); p[1, cls[1]] = 0.0                            # the true class at 0: clipped low, the row's gradient is 0
        p[2] = 0.0; p[2, cls[2]] = 1.0                                      # ... at 1: clipped high
    m = {"rand": np.repeat(y[:, :C - 1], 4, axis=1), "zero": np.zeros((n, K4), np.float32), "one": np.ones((n, K4), np.float32)}[mask]
    pred = rs.randn(n, K4).astype(np.float32)
    tgt = (pred + 2 * rs.randn(n, K4)).astype(np.float32)
    for i, d in enumerate((1.0, -1.0, 0.0)):
        pred[0, i], tgt[0, i] = 0.5, 0.5 + d
    if mask == "rand":
        m[0, :4] = 1.0                                                       # keep the seam under the mask
    return x, p, y, np.concatenate([m, tgt], axis=1).astype(np.float32), pred


@pytest.mark.parametrize("C", DET_C)
@pytest.mark.parametrize("n", DET_N)
def test_det_losses(G, n, C):
    t = G.torch
    K4 = 4 * (C - 1)
    for mask in ("rand", "zero", "one"):
        x, p, y, yr, pred = _det_inputs(n, C, mask)
        tag = "%dx%d/%s" % (n, C, mask)
        q = (p.astype(np.float64) / p.astype(np.float64).sum(axis=1, keepdims=True) * y).sum(axis=1)
        special = np.zeros(n, bool)
        special[1:3] = n >= 4
        assert ((q[~special] > 1e-6) & (q[~special] < 1 - 1e-6)).all(), "an ordinary row sits too close to a clip bound"
        lc_ref, gc_ref = R.det_cls_autograd(y, p, x)
        _, gc_cf, blc, bgc = R.det_cls_closed(y, p)
        lr_ref, gr_ref = R.det_reg_autograd(yr, pred, C - 1)
        blr, bgr = R.det_reg_bounds(lr_ref, gr_ref)
        # ldg = the row width
        lc, gc = _loss(G, "frcnn_loss_det_cls", y, p, n, C)
        lr, gr = _loss(G, "frcnn_loss_det_reg", yr, pred, n, C - 1)
        assert lc.tobytes() == _loss(G, "frcnn_loss_det_cls", y, p, n, C, grad=False)[0].tobytes()
        assert lr.tobytes() == _loss(G, "frcnn_loss_det_reg", yr, pred, n, C - 1, grad=False)[0].tobytes()
        # bars: R.det_cls_closed (loss mean(C U + 8 U |l_r|) + U |loss|; gradient (3 U |p - y| + U p) / n, 0 in clipped rows),
        # R.det_reg_bounds (loss 6 U |loss|; gradient 5 U |g|)
        within("det_cls %s loss" % tag, lc, lc_ref, blc)
        within("det_cls %s grad vs autograd" % tag, gc, gc_ref, bgc)
        within("det_cls %s grad vs closed form" % tag, gc, gc_cf, bgc)
        within("det_reg %s loss" % tag, lr, lr_ref, blr)
        within("det_reg %s grad" % tag, gr, gr_ref, bgr)
        if n >= 4:
            assert not gc[1].any() and not gc[2].any()
        if mask == "zero":
            assert lr == 0 and not gr.any()
        # the fused [d logits | d reg] buffer of the training step: each kernel writes its own columns and no others
        fused = t.full((n, C + K4), 12345.0, dtype=t.float32, device="cuda")
        lc2, f1 = _loss(G, "frcnn_loss_det_cls", y, p, n, C, ldg=C + K4, gbuf=fused)
        assert lc2.tobytes() == lc.tobytes() and f1[:, :C].tobytes() == gc.tobytes() and (f1[:, C:] == 12345.0).all()
        fused = t.full((n, C + K4), 12345.0, dtype=t.float32, device="cuda")
        lr2, f2 = _loss(G, "frcnn_loss_det_reg", yr, pred, n, C - 1, ldg=C + K4, gbuf=fused, goff=C)
        assert lr2.tobytes() == lr.tobytes() and f2[:, C:].tobytes() == gr.tobytes() and (f2[:, :C] == 12345.0).all()


# ----------------------------------------------------------------------------- max-pool backward
def _pool_fwd(G, x, k):
    """The pool output the training step would hand to the backward kernel: ops.pool2d where it applies (C % 4 == 0)."""
    if x.shape[3] % 4 == 0:
        return G.ops.pool2d(G.dev(x), k, k, True).cpu().numpy()
    n, H, W, C = x.shape
    return x[:, :H // k * k, :W // k * k].reshape(n, H // k, k, W // k, k, C).max(axis=(2, 4))


def _maxpool_check(G, x, k, tag):
    n, H, W, C = x.shape
    rs = np.random.RandomState(7)
    gy = rs.randn(n, H // k, W // k, C).astype(np.float32)
    gy[gy == 0] = 1.0
    y = _pool_fwd(G, x, k)
    gx = G.torch.full(x.shape, -7.0, dtype=G.torch.float32, device="cuda")
    xd, yd, gyd = G.dev(x), G.dev(y), G.dev(gy)
    G.call("frcnn_maxpool_bwd", G.ptr(xd), G.ptr(yd), G.ptr(gyd), n, H, W, C, k, G.ptr(gx))
    got = gx.cpu().numpy()
    want = R.maxpool_bwd_first(x, gy, k)
    assert got.tobytes() == want.tobytes(), "maxpool_bwd %s: %d elements differ from the first-maximum rule" % (tag, int((got != want).sum()))
    Ho, Wo = H // k, W // k
    per_window = (got[:, :Ho * k, :Wo * k].reshape(n, Ho, k, Wo, k, C) != 0).sum(axis=(2, 4))
    assert (per_window == 1).all() and not got[:, Ho * k:].any() and not got[:, :, Wo * k:].any()
    print("%-44s bit-equal, one element per window" % ("maxpool_bwd " + tag))


@pytest.mark.parametrize("shape,k", [((1, 37, 53, 64), 2), ((1, 37, 53, 64), 3), ((2, 14, 18, 3), 2), ((2, 14, 18, 3), 3),
                                     ((1, 130, 130, 64), 2), ((1, 129, 131, 64), 3)])
def test_maxpool_bwd(G, shape, k):
    rs = np.random.RandomState(11)
    n, H, W, C = shape
    assert n * H * W * C > TRIP or H < 100
    x = np.maximum(rs.randn(*shape), 0).astype(np.float32)                    # post-ReLU: most windows tie at 0
    x[0, 0:k, 0:k, :] = 3.0                                                   # windows of one repeated value
    x[0, 0:k, k:2 * k, :] = 0.0
    x[0, 0, k, :] = -0.0                                                      # -0.0 first, +0.0 after it
    x[0, 0:k, 2 * k:3 * k, :] = -0.0
    x[0, k - 1, 3 * k - 1, :] = 0.0                                           # +0.0 last, -0.0 before it
    for j in range(min(k * k, W // k)):                                       # a unique maximum at each window position
        x[0, k:2 * k, j * k:(j + 1) * k, :] = 0.0
        x[0, k + j // k, j * k + j % k, :] = 5.0
    _maxpool_check(G, x, k, "%s k=%d" % (shape, k))


@pytest.mark.parametrize("vals", [[0, 0, 0, 0], [2, 2, 2, 2], [-0.0, 0.0, 0.0, -0.0], [0.0, -0.0, -0.0, 0.0], [5, 1, 1, 1], [1, 5, 1, 1],
                                  [1, 1, 5, 1], [1, 1, 1, 5], [1, 5, 5, 1], [-3, -1, -1, -2]])
def test_maxpool_bwd_single_window(G, vals):
    _maxpool_check(G, np.array(vals, np.float32).reshape(1, 2, 2, 1), 2, "(1,2,2,1) %s" % vals)


# ----------------------------------------------------------------------------- ReLU backward
@pytest.mark.parametrize("n", [4, 1028, 4 * TRIP + 4])
def test_relu_bwd_inplace(G, n):
    rs = np.random.RandomState(n % 1000)
    y = rs.randn(n).astype(np.float32)
    tiny = np.array([-0.0, 0.0, 1e-45, 1.17549435e-38], np.float32)             # -0, +0, the smallest subnormal, the smallest normal
    y[:4] = tiny
    if n > 8:
        y[-4:] = tiny[::-1]
    g = rs.randn(n).astype(np.float32)
    g[g == 0] = 1.0
    gd = G.dev(g)
    yd = G.dev(y)
    G.call("frcnn_relu_bwd_inplace", G.ptr(gd), G.ptr(yd), n)
    got = gd.cpu().numpy()
    assert got.tobytes() == R.relu_bwd(g, y).tobytes(), "relu_bwd n=%d: %d differ (first four %s)" % (n, int((got != R.relu_bwd(g, y)).sum()), got[:4])
    assert got[2] == g[2] and got[3] == g[3] and got[0] == 0 and got[1] == 0    # TF's ReluGrad passes the gradient for ANY y > 0
    print("%-44s bit-equal" % ("relu_bwd_inplace n=%d" % n))


def test_relu_bwd_inplace_rejects_n_not_multiple_of_4(G):
    z = G.torch.zeros(8, dtype=G.torch.float32, device="cuda")
    for n in (1, 2, 3, 5, 7):
        with pytest.raises(G.lib.FrcnnError):
            G.call("frcnn_relu_bwd_inplace", G.ptr(z), G.ptr(z), n)


@pytest.mark.parametrize("n", [4, 1028, 1029, 4 * TRIP + 5])
def test_relu_bwd_inplace_bf16(G, n):
    rs = np.random.RandomState(n % 1000)
    yb = R.bf16_bits_rne(rs.randn(n).astype(np.float32))
    tiny = np.array([0x8000, 0x0000, 0x0001, 0x0080], np.uint16)               # -0, +0, smallest subnormal, smallest normal (bf16)
    yb[:4] = tiny
    if n > 8:
        yb[-4:] = tiny[::-1]
    gb = R.bf16_bits_rne(rs.randn(n).astype(np.float32))
    gb[(gb & 0x7FFF) == 0] = 0x3F80
    gd = bf16_dev(G, gb)
    yd = bf16_dev(G, yb)
    G.call("frcnn_relu_bwd_inplace_bf16", G.ptr(gd), G.ptr(yd), n)
    got = gd.view(G.torch.int16).cpu().numpy().view(np.uint16)
    want = np.where(R.bf16_bits_to_f32(yb) > 0, gb, np.uint16(0))
    assert np.array_equal(got, want), "relu_bwd_bf16 n=%d: %d differ (first four %s)" % (n, int((got != want).sum()), got[:4])
    assert got[2] == gb[2] and got[3] == gb[3]
    print("%-44s bit-equal" % ("relu_bwd_inplace_bf16 n=%d" % n))


# ----------------------------------------------------------------------------- average-pool backward
def _avgpool_bwd_inputs(n, k, c):
    rs = np.random.RandomState(n * 7 + c)
    y = rs.randn(n, k, k, c).astype(np.float32)                                # negatives ...
    y[rs.rand(n, k, k, c) < 0.3] = 0.0                                         # ... and zeros of both signs
    y[rs.rand(n, k, k, c) < 0.05] = -0.0
    return y, rs.randn(n, c).astype(np.float32)


@pytest.mark.parametrize("n,k,c", [(1, 7, 2048), (3, 7, 512), (64, 7, 2048), (2, 2, 4)])
def test_avgpool_bwd_masked(G, n, k, c):
    y, gp = _avgpool_bwd_inputs(n, k, c)
    gx = G.torch.full(y.shape, -7.0, dtype=G.torch.float32, device="cuda")
    gpd, yd = G.dev(gp), G.dev(y)
    G.call("frcnn_avgpool_bwd_masked", G.ptr(gpd), G.ptr(yd), n, k, c, G.ptr(gx))
    want, bound = R.avgpool_bwd_masked(gp, y, k)
    within("avgpool_bwd_masked (%d,%d,%d)" % (n, k, c), gx.cpu().numpy(), want, bound)       # 2 U |v|, zeros exact: R.avgpool_bwd_masked


@pytest.mark.parametrize("n,k,c", [(1, 7, 2048), (3, 7, 512), (64, 7, 2048), (2, 2, 4), (2, 2, 6)])
def test_avgpool_bwd_masked_bf16(G, n, k, c):
    y, gp = _avgpool_bwd_inputs(n, k, c)
    yb = R.bf16_bits_rne(y)
    gx = bf16_dev(G, np.full(y.shape, 0x4049, np.uint16))
    gpd, yd = G.dev(gp), bf16_dev(G, yb)
    G.call("frcnn_avgpool_bwd_masked_bf16", G.ptr(gpd), G.ptr(yd), n, k, c, G.ptr(gx))
    got = R.bf16_bits_to_f32(gx.view(G.torch.int16).cpu().numpy().view(np.uint16))
    want, bound = R.avgpool_bwd_masked(gp, R.bf16_bits_to_f32(yb), k)
    # the f32 product (within 2 U of the f64 value) rounded once to bf16: half a bf16 ulp at the product's magnitude
    within("avgpool_bwd_masked_bf16 (%d,%d,%d)" % (n, k, c), got, want, R.bf16_half_ulp(np.abs(want) * (1 + 2 * R.U)) + 2 * R.U * np.abs(want))


# ----------------------------------------------------------------------------- optimisers
OPT_N = [1, 3, 4, 5, 7, 1027, 4 * TRIP + 7]
COMBOS = [(0.0, 1.0), (1e-4, 1.0), (0.0, 0.125), (1e-4, 0.125)]               # (l2, grad_scale)


def _grads(rs, n):
    g = (10.0 ** rs.uniform(-12, 3, n) * rs.choice([-1.0, 1.0], n)).astype(np.float32)
    g[::5] = 0.0                                                              # gradients that are exactly 0
    return g


def _slices(G, arrs, offset):
    """Device copies of the arrays, 16-byte aligned (offset 0) or starting one float into their buffer (the scalar path)."""
    out = []
    for a in arrs:
        buf = G.torch.zeros(a.size + 4, dtype=G.torch.float32, device="cuda")
        assert buf.data_ptr() % 16 == 0
        v = buf[offset:offset + a.size]
        v.copy_(G.dev(a))
        out.append(v)
    return out


@pytest.mark.parametrize("n", OPT_N)
def test_sgd_momentum(G, n):
    rs = np.random.RandomState(n % 997)
    lr, mom = 1e-3, 0.9
    for l2, gs in (COMBOS if n < TRIP else COMBOS[::3]):
        w0, v0 = rs.randn(n).astype(np.float32), (0.01 * rs.randn(n)).astype(np.float32)
        grads = [_grads(rs, n), _grads(rs, n)]
        state = {}
        for off in (0, 1):
            w, v = _slices(G, (w0, v0), off)
            hw, hv = w0, v0
            for step, g in enumerate(grads):                                  # two consecutive steps, each against f64 from the f32 state before it
                gd, = _slices(G, (g,), off)
                G.call("frcnn_sgd_momentum", G.ptr(w), G.ptr(gd), G.ptr(v), n, lr, mom, l2, gs)
                wn, vn, bw, bv = R.sgd_momentum(hw, g, hv, lr, mom, l2, gs)
                hw, hv = w.cpu().numpy(), v.cpu().numpy()
                tag = "sgd n=%d l2=%g gs=%g %s step %d" % (n, l2, gs, ("aligned", "offset")[off], step + 1)
                within(tag + " w", hw, wn, bw)                                # U |w'| + 4 U D, D = |mom v| + lr (|g gs| + |2 l2 w|): R.sgd_momentum
                within(tag + " v", hv, vn, bv)                                # 4 U D
            state[off] = (hw.tobytes(), hv.tobytes())
        assert state[0] == state[1], "sgd_momentum n=%d: the 16-byte and the scalar path give different bits" % n


@pytest.mark.parametrize("n", OPT_N)
def test_adam(G, n):
    rs = np.random.RandomState(n % 991)
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    for t0 in ((1, 1000, 100000) if n < TRIP else (1,)):
        for l2, gs in (COMBOS if n < TRIP else COMBOS[::3]):
            w0 = rs.randn(n).astype(np.float32)
            grads = [_grads(rs, n), _grads(rs, n)]
            fresh = t0 == 1                                                   # t = 1: the moments compile() creates; later: some history
            m0 = np.zeros(n, np.float32) if fresh else (0.5 * grads[0]).astype(np.float32)
            v0 = np.zeros(n, np.float32) if fresh else (0.5 * grads[0] * grads[0]).astype(np.float32)
            state = {}
            for off in (0, 1):
                w, m, v = _slices(G, (w0, m0, v0), off)
                hw, hm, hv = w0, m0, v0
                for step, g in enumerate(grads):                              # t0 and t0 + 1
                    gd, = _slices(G, (g,), off)
                    G.call("frcnn_adam", G.ptr(w), G.ptr(gd), G.ptr(m), G.ptr(v), n, lr, b1, b2, eps, t0 + step, l2, gs)
                    wn, mn, vn, bw, bm, bv = R.adam(hw, g, hm, hv, lr, b1, b2, eps, t0 + step, l2, gs)
                    before = hw
                    hw, hm, hv = w.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()
                    tag = "adam n=%d t=%d l2=%g gs=%g %s" % (n, t0 + step, l2, gs, ("aligned", "offset")[off])
                    within(tag + " w", hw, wn, bw)                            # U |w'| + lr_t / (sqrt v + eps) (5 U M + |m| (5 U + 4 U V / v)): R.adam
                    within(tag + " m", hm, mn, bm)                            # 5 U M, M = |b1 m| + (1 - b1) G
                    within(tag + " v", hv, vn, bv)                            # 8 U V, V = b2 v + (1 - b2) G^2
                    if fresh and l2 == 0.0:                                    # g = 0 on zero moments: 0 / (0 + eps), the update is exactly 0
                        zero = g == 0
                        assert hw[zero].tobytes() == before[zero].tobytes() and not hm[zero].any() and not hv[zero].any()
                state[off] = (hw.tobytes(), hm.tobytes(), hv.tobytes())
            assert state[0] == state[1], "adam n=%d: aligned and offset buffers give different bits" % n


# ----------------------------------------------------------------------------- sum of squares, bias fold
@pytest.mark.parametrize("n", [1, 2, 3, 4, 1023, 4 * 257 + 1, 4 * 257 + 2, 4 * 257 + 3, 4 * 1024 * 256 + 5])
def test_sumsq(G, n):
    """Two buffers per n.  "span": 1e-18 .. 1e18 in one buffer, the largest term last (in the tail when n % 4 != 0); its bar, U of a sum
    of about 2e36, hides everything but the few huge terms.  "unit": |w| in [1, 2], where one element adds at least 1 to a sum of at
    most 4 n, against the same bar of U = 6e-8 of the sum (0.15 at the largest n, asserted below): a single dropped element -- let alone
    a workgroup's 256 float4s, a partial left out of the final sum or a wrong grid stride -- exceeds it, so every slot matters."""
    t = G.torch
    rs = np.random.RandomState(n % 983)
    span = rs.randn(n).astype(np.float32)
    span[0] = 1e-18
    span[n // 2] = 1e9
    span[-1] = -1e18
    if n > 8:
        span[3], span[n - 3] = 1e18, 3e17
    unit = (rs.uniform(1.0, 2.0, n) * rs.choice([-1.0, 1.0], n)).astype(np.float32)
    nbytes = G.lib.load().frcnn_sumsq_workspace_bytes()
    for kind, w in (("span", span), ("unit", unit)):
        ws = t.full((nbytes,), 0xFF, dtype=t.uint8, device="cuda")             # NaN partials: one the kernel does not write shows
        buf = t.zeros(n + 4, dtype=t.float32, device="cuda")
        buf[:n].copy_(G.dev(w))
        out = t.full((2,), -7.0, dtype=t.float32, device="cuda")
        G.call("frcnn_sumsq", G.ptr(buf), n, G.ptr(out), G.ptr(ws), nbytes)
        G.call("frcnn_sumsq", G.ptr(buf), n, G.ptr(out, 4), G.ptr(ws), nbytes)
        got = out.cpu().numpy()
        assert got[:1].tobytes() == got[1:].tobytes(), "sumsq is not reproducible"
        want, bound = R.sumsq(w)                                                 # (U + n 2^-53) sum: one cast, f64 accumulation (R.sumsq)
        assert want == float(np.sum(w.astype(np.float64) ** 2))
        if kind == "unit":
            assert (w.astype(np.float64) ** 2).min() > 2 * bound, "a single element would hide under the bar"
        within("sumsq %s n=%d" % (kind, n), got[0], want, bound)
    with pytest.raises(G.lib.FrcnnError):                                      # host-side rejections: nothing is launched
        G.call("frcnn_sumsq", G.ptr(buf, 4), n, G.ptr(out), G.ptr(ws), nbytes)
    with pytest.raises(G.lib.FrcnnError):
        G.call("frcnn_sumsq", G.ptr(buf), n, G.ptr(out), G.ptr(ws), nbytes - 1)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2048])
def test_fold_bias(G, n):
    rs = np.random.RandomState(n)
    b, s, c = (rs.randn(n).astype(np.float32) for _ in range(3))
    for drop in (None, 0, 1, 2):
        args = [None if drop == i else a for i, a in enumerate((b, s, c))]
        out = G.torch.full((n + 1,), -7.0, dtype=G.torch.float32, device="cuda")
        devs = [G.dev(a) if a is not None else None for a in args]
        G.call("frcnn_fold_bias", *[G.ptr(d) for d in devs], G.ptr(out), n)
        got = out.cpu().numpy()
        want, bound = R.fold_bias(*args, n)
        within("fold_bias n=%d null=%s" % (n, drop), got[:n], want, bound)        # 2 U (|bias scale| + |shift|): R.fold_bias
        assert got[n] == -7.0                                                  # nothing past n


# ----------------------------------------------------------------------------- the dense heads' split
@pytest.mark.parametrize("cols", [1, 2, 21, 32, 33, 64, 81])
def test_dense_heads_split(G, cols):
    t = G.torch
    rs = np.random.RandomState(cols)
    worst = 0.0
    for rows in (1, 7, 8, 9, 64, 300, 2400):
        for tail in sorted({0, 4, 4 * (cols - 1)}):
            for ldx in (cols + tail, cols + tail + 5):
                patterns = ("rand", "same", "huge") if rows == 1 else ("mixed",)
                for pat in patterns:
                    x = (rs.randn(rows, ldx) * 10).astype(np.float32)
                    same = [0] if pat == "same" else [1] if pat == "mixed" else []
                    huge = [0] if pat == "huge" else [2] if pat == "mixed" else []
                    for r in same:
                        x[r, :cols] = 2.5                                     # a row of one repeated value
                    for r in huge:
                        x[r, :cols] = np.where(np.arange(cols) % 2 == 0, 1e4, -1e4)
                    xd = G.dev(x)
                    cls = t.full((rows, cols), -7.0, dtype=t.float32, device="cuda")
                    reg = t.full((rows, tail), -7.0, dtype=t.float32, device="cuda") if tail else None
                    G.call("frcnn_dense_heads_split", G.ptr(xd), rows, cols, tail, ldx, G.ptr(cls), G.ptr(reg))
                    soft = t.full((rows, cols), -7.0, dtype=t.float32, device="cuda")
                    G.call("frcnn_softmax_rows", G.ptr(xd), rows, cols, ldx, G.ptr(soft), cols)
                    what = "dense_heads_split rows=%d cols=%d tail=%d ldx=%d %s" % (rows, cols, tail, ldx, pat)
                    assert bits(cls) == bits(soft), what + ": cls differs from frcnn_softmax_rows"
                    if tail:
                        assert reg.cpu().numpy().tobytes() == np.ascontiguousarray(x[:, cols:cols + tail]).tobytes(), what + ": reg is not the copied columns"
                    got = cls.cpu().numpy().astype(np.float64)
                    want, bound = R.softmax_rows(x[:, :cols])              # y U (|d| + max|d| + 16 + cols + 1) + 2^-126: R.softmax_rows
                    err = np.abs(got - want)
                    assert (err <= bound).all(), "%s: worst err/bound %.3f" % (what, (err / bound).max())
                    assert (np.abs(got.sum(axis=1) - 1.0) <= bound.sum(axis=1)).all(), what + ": a row does not sum to 1"
                    worst = max(worst, float((err / bound).max()))
    print("%-44s bit-equal to softmax_rows; max err/bound vs f64 %.3f" % ("dense_heads_split cols=%d" % cols, worst))


# ----------------------------------------------------------------------------- average pools of the detector head
@pytest.mark.parametrize("npos,n,c", [(49, 1, 2048), (49, 64, 2048), (49, 300, 512), (4, 3, 4)])
def test_avgpool_pos_major(G, npos, n, c):
    k = int(round(npos ** 0.5))
    rs = np.random.RandomState(n + c)
    x = rs.randn(k, k, n, c).astype(np.float32)
    xd = G.dev(x)
    got = G.ops.avgpool_pos_major(xd)
    nhwc = G.ops.pool2d(xd.permute(2, 0, 1, 3).contiguous(), k, k, False).reshape(n, c)
    assert bits(got) == bits(nhwc), "avgpool_pos_major differs from pool2d(avg) of the transposed tensor"
    want, bound = R.avgpool_mean(x.astype(np.float64), (0, 1))
    within("avgpool_pos_major (%d,%d,%d)" % (npos, n, c), got.cpu().numpy(), want, bound)      # npos U sum|x| / npos: R.avgpool_mean


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("npos,n,c", [(49, 1, 2048), (49, 64, 2048), (49, 300, 512), (4, 3, 4), (4, 3, 12), (49, 5, 12)])
def test_avgpool_bf16_to_f32_ex(G, npos, n, c, layout):
    t = G.torch
    k = int(round(npos ** 0.5))
    rs = np.random.RandomState(n + c + layout)
    shape = (k, k, n, c) if layout else (n, k, k, c)
    xb = R.bf16_bits_rne(rs.randn(*shape).astype(np.float32))
    want, bound = R.avgpool_mean(R.bf16_bits_to_f32(xb).astype(np.float64), (0, 1) if layout else (1, 2))
    res = {}
    for off in (0, 1):                                                        # 16-byte aligned (eight-wide form when c % 8 == 0) / 2 bytes off (scalar form)
        src = bf16_dev(G, np.full(xb.size + 8, 0x7FC0, np.uint16))              # NaN all round the data: a read outside it shows
        src[off:off + xb.size].copy_(bf16_dev(G, xb.reshape(-1)))
        out = t.full((n * c + 1,), -7.0, dtype=t.float32, device="cuda")
        G.call("frcnn_avgpool_bf16_to_f32_ex", G.ptr(src, 2 * off), n, k, c, layout, G.ptr(out))
        o = out.cpu().numpy()
        assert o[-1] == -7.0
        res[off] = o[:-1].reshape(n, c)
        # npos U sum|x| / npos (npos - 1 adds and a divide, on the stored bf16 values): R.avgpool_mean
        within("avgpool_bf16_to_f32_ex (%d,%d,%d) layout %d %s" % (npos, n, c, layout, ("aligned", "2 bytes off")[off]), res[off], want, bound)
    assert res[0].tobytes() == res[1].tobytes(), "the eight-wide and the scalar form give different bits"
    assert bits(G.ops.avgpool_bf16(bf16_dev(G, xb.reshape(shape)), k, layout)) == res[0].tobytes()


# ----------------------------------------------------------------------------- casts
F32_EDGES = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,        # ties: to even downwards, upwards, both signs
             0x3F807FFF, 0x3F808001, 0x7F7FFFFF, 0xFF7FFFFF,        # either side of a tie; the largest finite f32 (rounds to inf)
             0x7F7F7FFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF,       # inf, NaNs (a NaN stays a NaN)
             0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x00008000, 0x00018000, 0x80008000, 0x00800000]     # zeros, f32 subnormals


def test_cast_f32_to_bf16(G):
    rs = np.random.RandomState(5)
    n = 4 * TRIP + 4 * 1000                                                     # a second trip round the float4 loop
    b = rs.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    b[:len(F32_EDGES)] = F32_EDGES
    b[-len(F32_EDGES):] = F32_EDGES
    x = b.view(np.float32)
    got = G.ops.cast_bf16(G.dev(x)).view(G.torch.int16).cpu().numpy().view(np.uint16)
    want = R.bf16_bits_rne(x)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], want[~nan]), "%d of %d differ from round-to-nearest-even" % (int((got[~nan] != want[~nan]).sum()), int((~nan).sum()))
    assert R.bf16_is_nan(got[nan]).all() and nan.sum() > 1000
    with pytest.raises(G.lib.FrcnnError):
        x8, y8 = G.dev(x[:8]), G.torch.zeros(8, dtype=G.torch.bfloat16, device="cuda")
        G.call("frcnn_cast_f32_to_bf16", G.ptr(x8), 6, G.ptr(y8))
    print("%-44s bit-equal on %d patterns" % ("cast_f32_to_bf16", n))


def test_cast_bf16_to_f32(G):
    allb = np.arange(65536, dtype=np.uint16)
    want = R.bf16_bits_to_f32(allb)
    nan = np.isnan(want)
    got = G.ops.cast_f32(bf16_dev(G, allb)).cpu().numpy()
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]) and np.isnan(got[nan]).all()
    out = G.torch.full((65536,), -7.0, dtype=G.torch.float32, device="cuda")
    alld = bf16_dev(G, allb)
    G.call("frcnn_cast_bf16_to_f32", G.ptr(alld), 65535, G.ptr(out))                     # an odd n, and nothing past it
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32)[:65535][~nan[:65535]], want.view(np.uint32)[:65535][~nan[:65535]]) and got[65535] == -7.0
    big = np.resize(allb[~nan], TRIP + 3)                                       # a second trip round the loop
    got = G.ops.cast_f32(bf16_dev(G, big)).cpu().numpy()
    assert got.tobytes() == R.bf16_bits_to_f32(big).tobytes()
    print("%-44s bit-equal on all 65536 patterns" % "cast_bf16_to_f32")


# ----------------------------------------------------------------------------- RoI crop backward, bf16 gradient
def test_roi_crop_resize_bwd_bf16(G):
    rs = np.random.RandomState(2)
    rois = np.array([[0, 0, 62, 37], [5, 5, 6, 6], [10, 3, 17, 10], [10, 3, 24, 8], [61, 36, 62, 37], [3, 0, 5, 30],
                     [20, 20, 34, 34], [0, 0, 1, 37]], dtype=np.float32)       # the list of test_boxes_gpu.test_roi_crop_resize
    for pool in (7, 14):
        db = R.bf16_bits_rne(rs.randn(len(rois), pool, pool, 64).astype(np.float32))
        got = G.ops.roi_crop_resize_bwd_bf16(bf16_dev(G, db), G.dev(rois), 38, 63)
        want = G.ops.roi_crop_resize_bwd(G.dev(R.bf16_bits_to_f32(db)), G.dev(rois), 38, 63)
        assert bits(got) == bits(want) and got.abs().sum().item() > 0, "pool %d: the bf16 form differs from the f32 form on the widened gradient" % pool
    none = G.ops.roi_crop_resize_bwd_bf16(bf16_dev(G, np.zeros((0, 7, 7, 64), np.uint16)), G.dev(rois[:0]), 38, 63)
    assert none.shape == (38, 63, 64) and not none.any().item()                # no RoIs: zeros
    print("%-44s bit-equal to the f32 form" % "roi_crop_resize_bwd_bf16")
