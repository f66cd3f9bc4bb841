"""Per-kernel parity of the forward pooling kernels of csrc/pool.hip: frcnn_pool2d_fwd (k_pool<max / average>) and frcnn_pool2d_fwd_planes
(k_pool_planes, the two fp16 planes VGG's block<n>_conv1 multiplies, with its own copy of the f16x3 engine's status logic).

Both are called through the C ABI, as ops.pool2d calls them, and compared over the WHOLE output with the numpy references of
tests/pool_ref.py on position-coded inputs.  Output buffers are pre-filled with NaN (f32) or 0x7e00 (planes): an element the kernel does
not write fails the comparison.  The bars: bit equality; k^2 U sum|x| / k^2 for the f32 mean against float64 (k^2 - 1 additions and one
division, U = 2^-24); 2^-22 |v| + 2^-38 max|v| for the planes (the bar of tests/test_conv_h3_gpu.py); and one bound on TIME, reasoned in
test_grid_stride_loop_visits_each_piece_once, for the one fault of the grid-stride loop that no value can show.
Every comparison prints `name: max |err|  max err/bound` (pytest -s); docs/POOL_KERNEL_PARITY.md records what an MI355X printed."""
import ctypes
import functools

import numpy as np
import pytest

from tests import pool_ref as R

pytestmark = pytest.mark.gpu


def tag(case):
    return "n%d %dx%d c%d %d/%d" % case


@pytest.fixture(scope="module")
def G():
    import torch
    from faster_rcnn_amd import _lib, ops

    class _G:
        pass
    g = _G()
    g.torch, g.lib, g.ops = torch, _lib, ops
    g.dev = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()           # (a copy: the shared references are read-only)
    g.call = lambda name, *a: _lib.call(name, *a, ops._stream())
    g.ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off) if t is not None else None
    return g


@functools.lru_cache(maxsize=None)
def ref(case):
    """The input of a case and its two f32 references, computed once and read-only."""
    k, s = case[4:]
    out = {"x": R.position_coded(case)}
    out["max"], out["avg"] = R.pool_max(out["x"], k, s), R.pool_avg32_seq(out["x"], k, s)
    for a in out.values():
        a.setflags(write=False)
    return out


def within(name, got, want, bound):
    """|got - want| <= bound everywhere, printing the largest share of the bound any element uses."""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(want))
    assert got.shape == want.shape and np.isfinite(got).all(), "%s: %d elements not finite (not written?)" % (name, int((~np.isfinite(got)).sum()))
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    print("%-58s max|err| %.3e  max err/bound %.3f" % (name, err.max(), share.max()))
    assert (err <= bound).all(), "%s: %d of %d outside the bound, worst err/bound %.3f" % (name, int((err > bound).sum()), err.size, share.max())


def same_bits(name, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, name
    a, b = got.view(np.int32 if got.dtype == np.float32 else np.int16), want.view(np.int32 if want.dtype == np.float32 else np.int16)
    diff = a != b
    first = tuple(int(v) for v in np.argwhere(diff)[0]) if diff.any() else None
    print("%-58s %s" % (name, "bit-equal" if first is None else "%d of %d differ" % (int(diff.sum()), diff.size)))
    assert first is None, "%s: %d of %d elements differ, first at %s: got %r, want %r" % (name, int(diff.sum()), diff.size, first, got[first], want[first])


def run_f32(G, xd, k, s, is_max):
    n, h, w, c = xd.shape
    ho, wo = R.out_hw(h, w, k, s)
    y = G.torch.full((n, ho, wo, c), float("nan"), dtype=G.torch.float32, device="cuda")
    G.call("frcnn_pool2d_fwd", G.ptr(xd), n, h, w, c, k, s, int(is_max), G.ptr(y))
    return y


def run_planes(G, xd, k, s, is_max, e, status=True):
    """-> (planes (2,n,ho,wo,c) fp16 on the device, the status word as a device int32 tensor that started at 0, or None)."""
    t = G.torch
    n, h, w, c = xd.shape
    ho, wo = R.out_hw(h, w, k, s)
    planes = t.full((2, n, ho, wo, c), 0x7E00, dtype=t.int16, device="cuda").view(t.float16)
    ex = t.tensor([e], dtype=t.int32, device="cuda")
    st = t.zeros(1, dtype=t.int32, device="cuda") if status else None
    assert planes.data_ptr() % 16 == 0
    hp = G.lib.H3Planes(planes=planes.data_ptr(), exponent=ex.data_ptr(), status=st.data_ptr() if status else None)
    G.call("frcnn_pool2d_fwd_planes", G.ptr(xd), n, h, w, c, k, s, int(is_max), ctypes.byref(hp))
    return planes, st


# ----------------------------------------------------------------------------- frcnn_pool2d_fwd
@pytest.mark.parametrize("case", R.CASES, ids=tag)
def test_max_f32(G, case):
    k, s = case[4:]
    r = ref(case)
    got = run_f32(G, G.dev(r["x"]), k, s, True).cpu().numpy()
    same_bits("max %s == exact maximum" % tag(case), got, r["max"])


@pytest.mark.parametrize("case", R.CASES, ids=tag)
def test_avg_f32(G, case):
    k, s = case[4:]
    r = ref(case)
    got = run_f32(G, G.dev(r["x"]), k, s, False).cpu().numpy()
    mean, mag = R.pool_avg64(r["x"], k, s)
    within("avg %s vs float64" % tag(case), got, mean, R.avg_bound(mag, k))          # k^2 - 1 additions + 1 division: k^2 U sum|x| / k^2
    same_bits("avg %s == sequential f32 model" % tag(case), got, r["avg"])


def test_max_special_values(G):
    """(1,4,4,4,2,2): four windows, the special value at tap c of channel c."""
    inf = np.float32(np.inf)
    x = np.array(R.position_coded((1, 4, 4, 4, 2, 2)))
    taps = [(0, 0), (0, 1), (1, 0), (1, 1)]
    for c, (r, q) in enumerate(taps):
        x[0, r, q, c] = -inf                       # window (0,0): -inf beside finite values
        x[0, 2 + r, q, c] = inf                    # window (1,0): +inf
        x[0, 2:4, 2:4, c] = [[-1.0, -2.0], [-3.0, -0.5]]
        x[0, 2 + r, 2 + q, c] = 0.0                # window (1,1): +0.0 and -0.0 (in the next tap), the rest negative
        r2, q2 = taps[(c + 1) % 4]
        x[0, 2 + r2, 2 + q2, c] = -0.0
    x[0, 0:2, 2:4, :] = -inf                       # window (0,1): all -inf
    got = run_f32(G, G.dev(x), 2, 2, True).cpu().numpy()
    want = R.pool_max(x, 2, 2)
    assert np.isfinite(want[0, 0, 0]).all() and (want[0, 0, 1] == -inf).all() and (want[0, 1, 0] == inf).all() and (want[0, 1, 1] == 0).all()
    same_bits("max special: -inf among finite values; +inf", got[0, :, 0].copy(), want[0, :, 0].copy())
    same_bits("max special: all -inf", got[0, 0, 1], want[0, 0, 1])
    assert (got[0, 1, 1] == 0).all(), got[0, 1, 1]                               # fmaxf's choice between +0.0 and -0.0 is not specified
    print("%-58s signs of the zero chosen per channel: %s" % ("max special: +0.0 and -0.0 in one window", np.signbit(got[0, 1, 1]).tolist()))


def test_max_ignores_a_nan_among_finite_values(G):
    """The reference framework propagates a NaN; fmaxf drops it.  This pins the kernel's PRESENT behaviour (docs/POOL_KERNEL_PARITY.md):
    a NaN at any tap of a window, the first included, leaves the maximum of the other values."""
    x = np.array(R.position_coded((1, 4, 4, 4, 2, 2)))
    clean = R.pool_max(x, 2, 2)
    for c, (r, q) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        for (h0, w0) in ((0, 0), (0, 2), (2, 0)):
            x[0, h0 + r, w0 + q, c] = np.nan
    x[0, 2:4, 2:4, :] = np.nan                                                   # a window of nothing but NaN: reported, not asserted
    got = run_f32(G, G.dev(x), 2, 2, True).cpu().numpy()
    want = np.nanmax(R.windows(x, 2, 2)[0].reshape(2, 2, 4, 4)[[0, 0, 1], [0, 1, 0]], axis=2)          # (window, channel) of the three windows
    assert (want <= clean[0, [0, 0, 1], [0, 1, 0]]).all() and (want < clean[0, [0, 0, 1], [0, 1, 0]]).any()       # some NaNs replaced a window's maximum
    same_bits("max with one NaN per window == max of the rest", got[0, [0, 0, 1], [0, 1, 0]], want)
    print("%-58s %s" % ("max of a window of four NaNs (observed)", got[0, 1, 1].tolist()))
    avg = run_f32(G, G.dev(x), 2, 2, False).cpu().numpy()
    assert np.isnan(avg).all()                                                   # the mean propagates it, as the reference framework does


@pytest.mark.parametrize("shape,k", [((1, 6, 8, 4), 2), ((1, 7, 9, 4), 3)])
def test_forward_max_agrees_with_the_backward_on_ties(G, shape, k):
    """Values from {0, 1, 2}: nearly every window ties.  frcnn_maxpool_bwd pools k x k windows at stride k (it has no other form), so the
    agreement is checked on those: with a gradient of ones, each window of the input gradient has ONE non-zero cell, the input there
    equals the forward kernel's output, and it is the first such cell in scan order.  (1,7,9,4) leaves row 6 outside every window; its 3/2
    forward (overlapping windows, which the backward cannot pool) is held to the exact maximum as well."""
    t = G.torch
    n, H, W, C = shape
    x = np.random.RandomState(H * W).randint(0, 3, shape).astype(np.float32)
    Ho, Wo = H // k, W // k
    win = x[:, :Ho * k, :Wo * k].reshape(n, Ho, k, Wo, k, C).transpose(0, 1, 3, 5, 2, 4).reshape(n, Ho, Wo, C, k * k)
    ties = ((win == win.max(axis=4, keepdims=True)).sum(axis=4) > 1).mean()
    assert ties > 0.4, ties                                                     # 48 % of these windows at k = 2, 92 % at k = 3
    xd = G.dev(x)
    y = run_f32(G, xd, k, k, True)
    same_bits("max %s %d/%d, ties in %.0f %% of windows" % (shape, k, k, 100 * ties), y.cpu().numpy(), R.pool_max(x, k, k))
    if k == 3:
        same_bits("max %s 3/2 on the same tensor" % (shape,), run_f32(G, xd, 3, 2, True).cpu().numpy(), R.pool_max(x, 3, 2))
    gy = t.ones_like(y)
    gx = t.full(shape, float("nan"), dtype=t.float32, device="cuda")
    G.call("frcnn_maxpool_bwd", G.ptr(xd), G.ptr(y), G.ptr(gy), n, H, W, C, k, G.ptr(gx))
    g = gx.cpu().numpy()
    assert np.isfinite(g).all() and not g[:, Ho * k:].any() and not g[:, :, Wo * k:].any()
    gw = g[:, :Ho * k, :Wo * k].reshape(n, Ho, k, Wo, k, C).transpose(0, 1, 3, 5, 2, 4).reshape(n, Ho, Wo, C, k * k)
    assert ((gw != 0).sum(axis=4) == 1).all() and (gw.sum(axis=4) == 1).all()
    at = (gw != 0).argmax(axis=4)                                                # the cell the backward routes the gradient to
    yv = y.cpu().numpy()
    assert (np.take_along_axis(win, at[..., None], axis=4)[..., 0] == yv).all(), "the backward's cell does not hold the forward's maximum"
    assert (at == (win == yv[..., None]).argmax(axis=4)).all(), "the backward's cell is not the FIRST cell equal to the forward's maximum"
    print("%-58s one cell per window, the first that equals the forward output" % ("maxpool_bwd %s k=%d" % (shape, k)))


def test_grid_stride_loop_visits_each_piece_once(G):
    """A grid-stride loop that steps by blockDim.x alone (not gridDim.x * blockDim.x) still writes every piece, with the right value: no
    comparison of values can see it.  What it changes is the work: workgroup b then walks every piece from 256 b to the end, on average
    half the tensor, so the 8192 workgroups of the capped grid move 8192 / 2 = 4096 times the bytes.  At k = 1, stride 1 the right kernel
    reads and writes exactly what a device copy of the tensor does, so its time is held to 64 copies -- sqrt(4096), the midpoint (in
    ratio) between the right loop and the wrong one.  Best of five launches each, timed by device events."""
    t = G.torch
    case = R.GRID_STRIDE[0]
    xd = G.dev(ref(case)["x"])
    n, h, w, c = xd.shape
    y = t.empty_like(xd)

    def best(fn):
        fn()
        t.cuda.synchronize()
        out = []
        for _ in range(5):
            a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return min(out)
    for is_max in (1, 0):
        copy = best(lambda: y.copy_(xd))
        pool = best(lambda: G.call("frcnn_pool2d_fwd", G.ptr(xd), n, h, w, c, 1, 1, is_max, G.ptr(y)))
        hp_planes, _ = run_planes(G, xd, 1, 1, is_max, 0)
        ex = t.zeros(1, dtype=t.int32, device="cuda")
        hp = G.lib.H3Planes(planes=hp_planes.data_ptr(), exponent=ex.data_ptr(), status=None)
        planes = best(lambda: G.call("frcnn_pool2d_fwd_planes", G.ptr(xd), n, h, w, c, 1, 1, is_max, ctypes.byref(hp)))
        print("%-58s copy %.3f ms, f32 %.3f ms (%.1f copies), planes %.3f ms (%.1f copies); bar 64 copies"
              % ("grid-stride time %s" % ("max" if is_max else "avg"), copy, pool, pool / copy, planes, planes / copy))
        assert pool <= 64 * copy and planes <= 64 * copy


# ----------------------------------------------------------------------------- frcnn_pool2d_fwd_planes
@pytest.mark.parametrize("case", R.PLANE_CASES, ids=tag)
def test_planes(G, case):
    k, s = case[4:]
    r = ref(case)
    xd = G.dev(r["x"])
    e = R.plane_exponent(np.abs(r["x"]).max())
    assert 2.0 ** 14 <= float(np.abs(r["x"]).max()) * 2.0 ** e < 2.0 ** 15
    for is_max in (True, False):
        name = "planes %s %s" % ("max" if is_max else "avg", tag(case))
        v_ref = r["max"] if is_max else r["avg"]
        planes, st = run_planes(G, xd, k, s, is_max, e)
        p = planes.cpu().numpy()
        hi, lo = p[0], p[1]
        v_dev = run_f32(G, xd, k, s, is_max).cpu().numpy()
        skip = R.below_f16_normal(v_ref, e)                                      # at most 0.1 %: tests/test_pool_ref_cpu.py
        want_hi = R.planes_model(v_ref, e)[0]
        same_bits("%s hi == model (%d of %d below 2^-14 left out)" % (name, int(skip.sum()), skip.size),
                  np.where(skip, np.float16(0), hi), np.where(skip, np.float16(0), want_hi))
        within(name + " hi + lo / 2048 vs the f32 kernel", R.plane_values(hi, lo, e), v_dev, R.plane_bound(v_dev))      # 2^-22 |v| + 2^-38 max|v|
        assert int(st.item()) == 0, "%s: status %d on a tensor inside its bound" % (name, int(st.item()))
        again, _ = run_planes(G, xd, k, s, is_max, e, status=False)             # a null status pointer: the same planes
        assert again.cpu().numpy().tobytes() == p.tobytes(), name + ": a null status pointer changed the planes"


POSITIONS = {R.STATUS_SMALL: [("first", 0), ("lane 13", 13), ("last", 31)],
             R.STATUS_WAVE: [("first", 0), ("lane 40", 40), ("last (lane 63)", 63)],
             R.GRID_STRIDE[1]: [("first", 0), ("lane 40", 1234600), ("last (second trip, lane 63)", R.pieces(R.GRID_STRIDE[1]) - 1),
                                ("second trip, lane 50", R.GRID_CAP + 2 * 64 + 50)]}


@pytest.mark.parametrize("is_max", [True, False], ids=["max", "avg"])
@pytest.mark.parametrize("case", R.STATUS_CASES, ids=tag)
def test_planes_status(G, case, is_max):
    """k_pool_planes' own copy of the engine's status logic.  R.status_input: every value of the tensor is at most peak / 8, peak a power
    of two, so that the ONE output piece whose window is filled with +-peak decides the word (started at 0): 0 at the exponent e that puts
    the peak at 2^14; H3_UNDER at e + 1 (the peak at exactly 2^15, hi pattern 0x7800, the lowest that reports; and 0x7bfe, the highest
    that is not saturated); H3_UNDER | H3_SATURATED at e + 3 (2^17: clamped to +-65504, sign kept, everything finite); all three bits for
    one +inf in the window; for one NaN under the mean at least H3_UNDER.  The piece sits in turn at the first piece, at a lane other
    than lane 0 of its wave, at the last piece, and (grid-stride case) at a piece of the second trip: the same word every time.  (1,8,8,8,2,2) has 32 pieces, half
    a wave; (1,8,8,16,2,2), 64 pieces, is added so that lanes 32..63 -- the half the first step of the reduction brings in -- report at a
    small size too."""
    t = G.torch
    n, h, w, c, k, s = case
    ho, wo = R.out_hw(h, w, k, s)
    x, peak = R.status_input(case)
    e = R.plane_exponent(peak)
    xd = G.dev(x)
    total = R.pieces(case)
    assert total > R.GRID_CAP or total <= 64
    what = "status %s %s" % ("max" if is_max else "avg", tag(case))
    seen_nan = set()

    def check_bar(name, planes, ee):
        v = run_f32(G, xd, k, s, is_max).double()
        back = (planes[0].double() + planes[1].double() / 2048.0) * 2.0 ** -ee
        err, bound = (back - v).abs(), 2.0 ** -22 * v.abs() + 2.0 ** -38 * v.abs().max()
        assert bool(t.isfinite(back).all())
        print("%-58s max|err| %.3e  max err/bound %.3f" % (name, float(err.max()), float((err / bound).max())))
        assert bool((err <= bound).all()), name

    for j, (where, piece) in enumerate(POSITIONS[case]):
        assert 0 <= piece < total and (where == "first" or piece % 64 != 0)
        img, oh, ow, c4 = (int(v) for v in np.unravel_index(piece, (n, ho, wo, c // 4)))
        ch = 4 * c4 + (j + 1) % 4
        sign = -1.0 if j % 2 else 1.0
        cell = (img, slice(oh * s, oh * s + k), slice(ow * s, ow * s + k), ch)
        one = (img, oh * s + k - 1, ow * s + (j % k), ch)                       # one cell of that window
        saved = xd[cell].clone()
        words = []
        xd[cell] = sign * peak
        planes, st = run_planes(G, xd, k, s, is_max, e)
        words.append(int(st.item()))
        hi_at = lambda p: int(p[0].view(t.int16).reshape(-1, 4)[piece, ch % 4].item()) & 0xFFFF
        assert hi_at(planes) == (0x7400 | (0x8000 if sign < 0 else 0))           # 2^14, inside the bound
        planes, st = run_planes(G, xd, k, s, is_max, e + 1)
        words.append(int(st.item()))
        assert hi_at(planes) == (0x7800 | (0x8000 if sign < 0 else 0))
        check_bar("%s e + 1, peak at the %s piece" % (what, where), planes, e + 1)
        planes, st = run_planes(G, xd, k, s, is_max, e + 3)
        words.append(int(st.item()))
        assert hi_at(planes) == (0x7BFF | (0x8000 if sign < 0 else 0)), "the clamped value lost its sign or was not clamped: %#x" % hi_at(planes)
        assert bool(t.isfinite(planes).all())
        xd[cell] = sign * 65472.0 / 2.0 ** (e + 1)                               # 0x7bfe at e + 1
        planes, st = run_planes(G, xd, k, s, is_max, e + 1)
        words.append(int(st.item()))
        assert hi_at(planes) == (0x7BFE | (0x8000 if sign < 0 else 0))
        xd[cell] = saved
        xd[one] = float("inf")
        planes, st = run_planes(G, xd, k, s, is_max, e)
        words.append(int(st.item()))
        assert hi_at(planes) == 0x7C00
        xd[cell] = saved
        assert words == [0, R.H3_UNDER, R.H3_UNDER | R.H3_SATURATED, R.H3_UNDER, 7], "%s, the %s piece: status words %s" % (what, where, words)
        if not is_max:
            xd[one] = float("nan")
            planes, st = run_planes(G, xd, k, s, is_max, e)
            word = int(st.item())
            assert word != 0 and word & R.H3_UNDER, "%s, NaN at the %s piece: status %d" % (what, where, word)
            seen_nan.add((word, hi_at(planes)))
            xd[cell] = saved
        _, st = run_planes(G, xd, k, s, is_max, e)                               # the tensor is back as it was
        assert int(st.item()) == 0
        print("%-58s words %s" % ("%s, the %s piece" % (what, where), words))
    if not is_max:
        assert len(seen_nan) == 1, seen_nan                                      # the same word in every position
        print("%-58s status %d, hi pattern %#06x" % (what + ", one NaN under the mean (observed)", *seen_nan.pop()))


def test_ops_pool2d_planes_out(G):
    t, ops = G.torch, G.ops
    case = (2, 17, 23, 64, 3, 2)
    x = G.dev(ref(case)["x"])
    with ops.f32_engine("f16x3"):
        x._amax = ops.amax_of(x)
        p_f = ops.pool2d(x, 3, 2, False)
        p_p = ops.pool2d(x, 3, 2, False, planes_out=True)
        assert isinstance(p_p, ops.PlaneTensor) and p_p.shape == tuple(p_f.shape)
        e = int(p_p.exponent.item())
        assert 2.0 ** 14 <= float(x.abs().max()) * 2.0 ** e < 2.0 ** 15
        pl = p_p.planes.cpu().numpy()
        v = p_f.cpu().numpy()
        within("ops.pool2d(planes_out) avg %s vs ops.pool2d" % tag(case), R.plane_values(pl[0], pl[1], e), v, R.plane_bound(v))
        assert int(p_p._amax.view(t.int32)[1].item()) == 0                       # the record's status word
    same_bits("ops.pool2d avg %s == sequential f32 model" % tag(case), v, ref(case)["avg"])
