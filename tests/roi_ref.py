"""Plain numpy references for the RoI crop / bilinear-resize kernels (csrc/roi.hip, k_roi_fwd_bf16* of csrc/conv_bf16.hip), with the
rounding-error bound each comparison uses.  TEST INFRASTRUCTURE ONLY: nothing here imports the package under test.
tests/test_roi_ref_cpu.py checks these references against oracle.keras_ref; tests/test_roi_kernels_gpu.py holds the kernels to them.

The operation is custom_layers.RoiResizeConv.call (custom_layers.py:35-56): K.cast(., 'int32') of the four corners (truncation toward
zero), the crop [y1:y2, x1:x2], then TF 1.3 resize_bilinear, align_corners=False, no half-pixel centres:
    scale = in / out (f32); src = i * scale; lo = (int)src; hi = min(lo + 1, in - 1); t = src - lo
    top = tl + (tr - tl) * tx; bot = bl + (br - bl) * tx; out = top + (bot - top) * ty
The kernels add one rule of their own: a RoI is REJECTED (it yields the fill vector, default zeros, and takes no gradient) unless
    h > 0 and w > 0 and x1 >= 0 and y1 >= 0 and x2 <= cols and y2 <= rows          (after the truncation)
where the reference's strided_slice would clamp a box that sticks out of the map (docs/ROI_KERNEL_PARITY.md, "Boxes outside the map").

Bounds: U = 2^-24 per f32 add / subtract / multiply (|fl(x) - x| <= U |x|), half a bf16 ulp for a bf16 result, f64 arithmetic taken as
exact next to them (SLACK covers its 2^-53 and the second-order terms).  A fused multiply-add rounds once where the separate operations
round twice, so a bound counted for the separate operations also holds for a contracted kernel."""
import numpy as np

f32 = np.float32
U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20


# ----------------------------------------------------------------------------- bf16 (bit patterns as uint16)
def bf16_bits_rne(x):
    """f32 array -> uint16 bf16 bit patterns, round to nearest even (finite inputs)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_bits_to_f32(bits):
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_half_ulp(x):
    """Half the spacing of bf16 (8 significant bits) at |x|, normal range: 2^(floor(log2 |x|) - 8); 0 at 0."""
    a = np.abs(np.asarray(x, np.float64))
    with np.errstate(divide="ignore"):
        return np.where(a > 0, 2.0 ** (np.floor(np.log2(np.where(a > 0, a, 1.0))) - 8), 0.0)


# ----------------------------------------------------------------------------- taps
def trunc_corners(roi):
    """(x1, y1, x2, y2) as K.cast(., 'int32') gives them: truncation toward zero of the f32 values (5.9 -> 5, -0.7 -> 0, -1.5 -> -1)."""
    return tuple(int(f32(v)) for v in roi)


def accepted(roi, rows, cols):
    """The kernels' validity predicate, on the truncated corners."""
    x1, y1, x2, y2 = trunc_corners(roi)
    return (y2 - y1) > 0 and (x2 - x1) > 0 and x1 >= 0 and y1 >= 0 and x2 <= cols and y2 <= rows


def _axis(lo0, extent, pool):
    """One axis of resize_bilinear: absolute lo / hi indices and the f32 fraction of each of the ``pool`` output positions.
    Roundings: the division, the product, the subtraction -- each an f32 operation, as in the kernel."""
    scale = f32(extent) / f32(pool)
    lo, hi, t = np.empty(pool, np.int64), np.empty(pool, np.int64), np.empty(pool, np.float32)
    for i in range(pool):
        src = f32(i) * scale
        l = int(src)
        lo[i], hi[i], t[i] = lo0 + l, lo0 + min(l + 1, extent - 1), f32(src - f32(l))
    return lo, hi, t


def taps(roi, pool, rows, cols):
    """None for a rejected RoI, otherwise (y_lo, y_hi, ty, x_lo, x_hi, tx): per output row / column the two map rows / columns
    (absolute, int64 (pool,)) and the f32 fraction (pool,).  Every index lies inside the box, hence inside the map."""
    if not accepted(roi, rows, cols):
        return None
    x1, y1, x2, y2 = trunc_corners(roi)
    return _axis(y1, y2 - y1, pool) + _axis(x1, x2 - x1, pool)


def _corners(feat, tp):
    y_lo, y_hi, ty, x_lo, x_hi, tx = tp
    tl, tr = feat[y_lo][:, x_lo], feat[y_lo][:, x_hi]           # (pool, pool, C)
    bl, br = feat[y_hi][:, x_lo], feat[y_hi][:, x_hi]
    return tl, tr, bl, br, ty[:, None, None], tx[None, :, None]


def _maps(feat, n, n_per_img):
    feat = np.asarray(feat)
    if n_per_img > 0:
        assert feat.ndim == 4 and n <= feat.shape[0] * n_per_img
        return feat, (lambda r: feat[r // n_per_img])
    feat = feat.reshape(feat.shape[-3:])
    return feat, (lambda r: feat)


def _finish(out, relu, layout):
    if relu:
        out = np.maximum(out, out.dtype.type(0))
    return np.ascontiguousarray(out.transpose(1, 2, 0, 3)) if layout else out


# ----------------------------------------------------------------------------- forward
def fwd_f32(feat, rois, pool, fill=None, relu=False, layout=0, n_per_img=0):
    """The kernels' f32 result, operation by operation: for an accepted RoI the three lerps in TF's order, every operation rounded to
    f32 (numpy rounds each ufunc call; nothing is fused) -- bit for bit oracle.keras_ref.roi_resize; for a rejected RoI the fill
    vector (default zeros); max(., 0) on both when ``relu``.  feat (R,C,Cf), or (B,R,C,Cf) with n_per_img > 0 (RoI r reads image
    r // n_per_img).  -> (n,pool,pool,Cf), or (pool,pool,n,Cf) with layout=1.  No bound: the comparison is equality."""
    rois = np.asarray(rois, np.float32).reshape(-1, 4)
    feat, img = _maps(np.asarray(feat, np.float32), len(rois), n_per_img)
    rows, cols, C = feat.shape[-3:]
    out = np.zeros((len(rois), pool, pool, C), np.float32)
    for r, roi in enumerate(rois):
        tp = taps(roi, pool, rows, cols)
        if tp is None:
            if fill is not None:
                out[r] = np.asarray(fill, np.float32)
            continue
        tl, tr, bl, br, ty, tx = _corners(img(r), tp)
        top = tl + (tr - tl) * tx
        bot = bl + (br - bl) * tx
        out[r] = top + (bot - top) * ty
    return _finish(out, relu, layout)


def fwd_f64(feat, rois, pool, fill=None, relu=False, layout=0, n_per_img=0):
    """The same samples in f64 from the SAME f32 fractions -> (value, mag, err32), each shaped like fwd_f32's result.
    mag = sum_i |w_i| |v_i| over the four corners with w = (1-ty)(1-tx), (1-ty)tx, ty(1-tx), ty tx: the size of the sample as a
    weighted sum.  It does NOT bound the lerp form's rounding error (tl = 1, tr = 0, tx = 0.99: top = 0.01 = mag, yet (tr - tl) * tx
    alone rounds by up to U * 0.99), so the bar is counted on the lerp form itself, nine f32 roundings:
        top~ = fl(tl + fl(fl(tr - tl) tx)):  |top~ - top| <= E_top = U (2 |tr - tl| tx + |top|)      (subtract, multiply, add)
        bot~ likewise;  v~ = fl(top~ + fl(fl(bot~ - top~) ty)) is the exact lerp of (top~, bot~) -- which moves by at most
        (1-ty) E_top + ty E_bot -- plus its own three roundings U (2 |bot - top| ty + |v|):
        err32 = [(1-ty) E_top + ty E_bot + U (2 |bot - top| ty + |v|)] * SLACK.
    ReLU is 1-Lipschitz and the fill vector is copied: both keep the bound (err32 = 0 for a rejected RoI).
    A bf16 result adds half a bf16 ulp of the rounded value: bf16_bar()."""
    rois = np.asarray(rois, np.float32).reshape(-1, 4)
    feat, img = _maps(np.asarray(feat, np.float32), len(rois), n_per_img)
    rows, cols, C = feat.shape[-3:]
    val = np.zeros((len(rois), pool, pool, C), np.float64)
    mag, err = np.zeros_like(val), np.zeros_like(val)
    for r, roi in enumerate(rois):
        tp = taps(roi, pool, rows, cols)
        if tp is None:
            if fill is not None:
                val[r] = np.asarray(fill, np.float32).astype(np.float64)
                mag[r] = np.abs(val[r])
            continue
        tl, tr, bl, br, ty, tx = (a.astype(np.float64) for a in _corners(img(r), tp))
        top = tl + (tr - tl) * tx
        bot = bl + (br - bl) * tx
        v = top + (bot - top) * ty
        e_top = U * (2 * np.abs(tr - tl) * tx + np.abs(top))
        e_bot = U * (2 * np.abs(br - bl) * tx + np.abs(bot))
        val[r] = v
        mag[r] = (1 - ty) * ((1 - tx) * np.abs(tl) + tx * np.abs(tr)) + ty * ((1 - tx) * np.abs(bl) + tx * np.abs(br))
        err[r] = ((1 - ty) * e_top + ty * e_bot + U * (2 * np.abs(bot - top) * ty + np.abs(v))) * SLACK
    if layout:
        mag, err = (np.ascontiguousarray(a.transpose(1, 2, 0, 3)) for a in (mag, err))
    return _finish(val, relu, layout), mag, err


def bf16_bar(val, err32):
    """The bar of a bf16 result against fwd_f64: the f32 value lies within err32 of ``val``; rounding it to bf16 (nearest) adds at
    most half a bf16 ulp taken at the largest magnitude the f32 value can have."""
    return err32 + bf16_half_ulp(np.abs(val) + err32)


# ----------------------------------------------------------------------------- backward
def _samples(rois, rows, cols, pool):
    """Accepted RoIs in list order, as (r, taps)."""
    for r, roi in enumerate(np.asarray(rois, np.float32).reshape(-1, 4)):
        tp = taps(roi, pool, rows, cols)
        if tp is not None:
            yield r, tp


def bwd_seq_f32(dout, rois, rows, cols, pool):
    """Gradient w.r.t. the map as the sequential f32 scatter, in the order TF's CPU ResizeBilinearGrad walks the samples: RoI, output
    row, output column; top-left, top-right, bottom-left, bottom-right; per tap ((wy * g) * wx) with wy = fl(1 - ty) or ty, wx =
    fl(1 - tx) or tx; rejected RoIs skipped.  dout (n,pool,pool,C) f32 -> (rows,cols,C) f32.  The gather kernel sums every cell's taps
    in this order from +0, so the comparison is equality (a tap whose weight is 0 still adds its signed zero, here and there)."""
    dout = np.asarray(dout, np.float32)
    seq = np.zeros((rows, cols, dout.shape[-1]), np.float32)
    one = f32(1)
    for r, (y_lo, y_hi, ty, x_lo, x_hi, tx) in _samples(rois, rows, cols, pool):
        for py in range(pool):
            wt, wb = one - ty[py], ty[py]
            for px in range(pool):
                g = dout[r, py, px]
                dtop, dbot = wt * g, wb * g
                wl, wr = one - tx[px], tx[px]
                seq[y_lo[py], x_lo[px]] += dtop * wl
                seq[y_lo[py], x_hi[px]] += dtop * wr
                seq[y_hi[py], x_lo[px]] += dbot * wl
                seq[y_hi[py], x_hi[px]] += dbot * wr
    return seq


def bwd_f64(dout, rois, rows, cols, pool):
    """The same sum in f64 from the same f32 weights (fl(1 - t) included) -> (value (rows,cols,C), taps (rows,cols) int, mag
    (rows,cols,C) = sum |wy g wx| over the cell's taps).  The f32 sum of k taps rounds each tap twice (two products: 2 U |tap|) and adds
    them one after another from 0 (the first addition is exact; k - 1 roundings, each at most U times a partial sum <= mag):
        bar = (k + 1) U mag * SLACK                                                                          -> bwd_bar().
    Against float64 autograd through the lerp form, whose weights are the exact 1 - t, the two rounded weights add 2 U mag."""
    dout = np.asarray(dout, np.float32).astype(np.float64)
    val = np.zeros((rows, cols, dout.shape[-1]), np.float64)
    mag = np.zeros_like(val)
    cnt = np.zeros((rows, cols), np.int64)
    one = f32(1)
    for r, (y_lo, y_hi, ty, x_lo, x_hi, tx) in _samples(rois, rows, cols, pool):
        wy = np.stack([one - ty, ty]).astype(np.float64)               # (2, pool): the f32 weights, widened
        wx = np.stack([one - tx, tx]).astype(np.float64)
        ys, xs = (y_lo, y_hi), (x_lo, x_hi)
        for a in range(2):
            for b in range(2):
                t = dout[r] * wy[a][:, None, None] * wx[b][None, :, None]
                iy, ix = np.repeat(ys[a], pool), np.tile(xs[b], pool)
                np.add.at(val, (iy, ix), t.reshape(pool * pool, -1))
                np.add.at(mag, (iy, ix), np.abs(t).reshape(pool * pool, -1))
                np.add.at(cnt, (iy, ix), 1)
    return val, cnt, mag


def bwd_bar(cnt, mag):
    return (cnt[..., None] + 1) * U * mag * SLACK
