"""Plain numpy / torch-f64 references for the small training-path and detector-head kernels (csrc/train.hip, the pooling and
dense-head kernels of csrc/pool.hip, the bf16 helpers of csrc/conv_bf16.hip), with the rounding-error bound each comparison uses.
TEST INFRASTRUCTURE ONLY.  tests/test_train_kernels_ref_cpu.py checks these references against each other;
tests/test_train_kernels_gpu.py holds the kernels to them.

Every reference works in f64 on the kernel's own f32 (or bf16) inputs, so only the kernel's roundings separate the two.  The bounds
count them: U = 2^-24 per f32 add / multiply / divide / sqrtf (|fl(x) - x| <= U |x|), LIBM_ULP ulps (1 ulp <= 2 U relative) for logf /
expf / log1pf, half a bf16 ulp for a bf16 result (bf16_half_ulp: 2^(e-8) for |x| in [2^e, 2^(e+1)), i.e. between 2^-9 and 2^-8 of |x|; a flat
2^-9 |x| is NOT reachable by a correctly rounded result: 1 + 2^-8 lies 2^-8 from both its neighbours), f64 accumulation exact.  The HIP math-accuracy table is not shipped with the
ROCm install, so LIBM_ULP = 4 is an ASSUMPTION (the published figures for these three functions are 1-2 ulp)."""
import numpy as np
import torch

from oracle import keras_train_ref as ktr

U = 2.0 ** -24
LIBM_ULP = 4
F32_TINY = 2.0 ** -126                       # below this a relative bound means nothing (subnormal / flushed results)
CLIP_LO = np.float32(1e-7)                   # Keras' epsilon as f32 arithmetic sees it ...
CLIP_HI = np.float32(1) - np.float32(1e-7)   # ... and 1 - epsilon ROUNDED in f32 (0.99999988, not 0.9999999)


def f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


# ----------------------------------------------------------------------------- bf16
def bf16_bits_rne(x):
    """f32 array -> uint16 bf16 bit patterns, round to nearest even (NaN -> a quiet NaN of the same sign)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    nan = (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return np.where(nan, ((b >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16), r)


def bf16_bits_to_f32(bits):
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_half_ulp(x):
    """Half the spacing of bf16 (8 significant bits) at |x|, normal range: 2^(floor(log2 |x|) - 8); 0 at 0."""
    a = np.abs(np.asarray(x, np.float64))
    with np.errstate(divide="ignore"):
        return np.where(a > 0, 2.0 ** (np.floor(np.log2(np.where(a > 0, a, 1.0))) - 8), 0.0)


def bf16_is_nan(bits):
    return (np.asarray(bits, np.uint16) & np.uint16(0x7FFF)) > np.uint16(0x7F80)


# ----------------------------------------------------------------------------- pooling / ReLU backward
def maxpool_bwd_first(x, gy, k):
    """MaxPooling2D((k,k), strides (k,k)) backward, NHWC: each window's gradient goes to its FIRST maximum in scan order (row, then
    column), -0.0 == +0.0; rows / columns past the last whole window get 0."""
    n, H, W, C = x.shape
    Ho, Wo = H // k, W // k
    win = x[:, :Ho * k, :Wo * k].reshape(n, Ho, k, Wo, k, C).transpose(0, 1, 3, 5, 2, 4).reshape(n, Ho, Wo, C, k * k)
    first = np.argmax(win, axis=-1)                                   # numpy: the first of equal maxima
    g = np.zeros((n, Ho, Wo, C, k * k), dtype=gy.dtype)
    np.put_along_axis(g, first[..., None], gy[..., None], axis=-1)
    gx = np.zeros_like(x)
    gx[:, :Ho * k, :Wo * k] = g.reshape(n, Ho, Wo, C, k, k).transpose(0, 1, 4, 2, 5, 3).reshape(n, Ho * k, Wo * k, C)
    return gx


def maxpool_bwd_loops(x, gy, k):
    """The same rule as a literal loop (small inputs only)."""
    n, H, W, C = x.shape
    gx = np.zeros_like(x)
    for i in range(n):
        for ho in range(H // k):
            for wo in range(W // k):
                for c in range(C):
                    best, at = None, None
                    for r in range(ho * k, ho * k + k):
                        for q in range(wo * k, wo * k + k):
                            if best is None or x[i, r, q, c] > best:
                                best, at = x[i, r, q, c], (r, q)
                    gx[i, at[0], at[1], c] = gy[i, ho, wo, c]
    return gx


def relu_bwd(g, y):
    """g * (y > 0): the gradient's own bits where y > 0 (subnormals included), +0.0 elsewhere."""
    return np.where(y > 0, g, np.zeros_like(g))


def avgpool_bwd_masked(gp, y, k):
    """(value f64, bound) of (y > 0) * gp / k^2; gp (n,c), y (n,k,k,c).  The kernel rounds 1/k^2 once and multiplies once: 2 U."""
    v = np.where(f64(y) > 0, f64(gp)[:, None, None, :] / (k * k), 0.0)
    return v, 2 * U * np.abs(v)


def avgpool_mean(x, axis):
    """(mean f64, bound) of sequential f32 adds over `axis` followed by one division: (npos - 1) + 1 roundings against sum|x| / npos."""
    x = np.asarray(x, np.float64)
    npos = x.shape[axis] if isinstance(axis, int) else int(np.prod([x.shape[a] for a in axis]))
    return x.mean(axis=axis), npos * U * np.abs(x).sum(axis=axis) / npos + F32_TINY


# ----------------------------------------------------------------------------- optimisers
def sgd_momentum(w, g, v, lr, momentum, l2, gscale):
    """Keras SGD(momentum) with the L2 gradient 2 l2 w, in f64 from f32 inputs.  Returns (w', v', bound_w, bound_v).
    Kernel: gi = g*gs + (2 l2)*w  (2 mults + add: |err| <= 2 U G, G = |g gs| + |2 l2 w|);  vi = mom*v - lr*gi  (2 mults + add on
    top of lr * err(gi): |err| <= 4 U D, D = |mom v| + lr G);  w += vi  (one add: U |w'|).  bound_w = U |w'| + 4 U D, bound_v = 4 U D."""
    lr, momentum, l2, gscale = _scalars((lr, momentum, l2, gscale), True)
    w, g, v = f64(w), f64(g), f64(v)
    G = np.abs(g * gscale) + np.abs(2 * l2 * w)
    vi = momentum * v - lr * (g * gscale + 2 * l2 * w)
    D = np.abs(momentum * v) + lr * G
    return w + vi, vi, U * np.abs(w + vi) + 4 * U * D, 4 * U * D


def _scalars(vals, as_f32):
    """The kernels receive their scalar arguments as f32; as_f32=False keeps the f64 values (to compare with the oracle's Optim, which
    hard-codes 0.9 / 0.999 / 1e-8 in f64: 1 - 0.999f is 1.3e-5 away from 0.001)."""
    return tuple(float(np.float32(s)) if as_f32 else float(s) for s in vals)


def adam_lr_t(lr, b1, b2, t, as_f32=True):
    lr, b1, b2 = _scalars((lr, b1, b2), as_f32)
    return lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def adam(w, g, m, v, lr, b1, b2, eps, t, l2, gscale, as_f32=True):
    """Keras Adam in f64 from f32 inputs.  Returns (w', m', v', bound_w, bound_m, bound_v).
    gi as in sgd_momentum (2 U G).  mi = b1*m + (1-b1)*gi: subtract, 2 mults, add on top of (1-b1) err(gi): <= 5 U M,
    M = |b1 m| + (1-b1) G.  vi = b2*v + (1-b2)*gi*gi: gi^2 carries 4 U G^2, then subtract, 3 mults, add: <= 8 U V, V = b2 v + (1-b2) G^2.
    step = lr_t * mi / (sqrtf(vi) + eps): lr_t cast, mult, sqrtf, add, divide = 5 U relative, mi's 5 U M, and vi's 8 U V through the
    square root (half of it, relative to vi): bound_step = lr_t / (sqrt(vi) + eps) * (5 U M + |mi| (5 U + 4 U V / vi)); w -= step: U |w'|."""
    lr_t = adam_lr_t(lr, b1, b2, t, as_f32)
    b1, b2, eps, l2, gscale = _scalars((b1, b2, eps, l2, gscale), as_f32)
    w, g, m, v = f64(w), f64(g), f64(m), f64(v)
    gi = g * gscale + 2 * l2 * w
    G = np.abs(g * gscale) + np.abs(2 * l2 * w)
    mi = b1 * m + (1 - b1) * gi
    M = np.abs(b1 * m) + (1 - b1) * G
    vi = b2 * v + (1 - b2) * gi * gi
    V = b2 * v + (1 - b2) * G * G
    with np.errstate(divide="ignore", invalid="ignore"):
        amp = np.where(vi > 0, V / vi, 0.0)
    scale = lr_t / (np.sqrt(vi) + eps)
    wn = w - scale * mi
    bound_step = scale * (5 * U * M + np.abs(mi) * (5 * U + 4 * U * amp))
    return wn, mi, vi, U * np.abs(wn) + bound_step, 5 * U * M, 8 * U * V


def sumsq(w):
    """(sum(w^2) in f64, bound): the kernel accumulates in f64 (n 2^-53 relative at the worst) and rounds once to f32 (U)."""
    s = float(np.sum(f64(w) ** 2))
    return s, (U + np.size(w) * 2.0 ** -53) * s


def fold_bias(bias, scale, shift, n):
    """(bias*scale + shift in f64, bound): a multiply and an add (an FMA removes one): 2 U (|bias scale| + |shift|)."""
    b = f64(bias) if bias is not None else np.zeros(n)
    s = f64(scale) if scale is not None else np.ones(n)
    c = f64(shift) if shift is not None else np.zeros(n)
    return b * s + c, 2 * U * (np.abs(b * s) + np.abs(c))


# ----------------------------------------------------------------------------- softmax
def softmax_rows(x):
    """(softmax f64, bound) of f32 logits (rows, cols).  Kernel per entry: d = x - max (U |d|, which is the RELATIVE error it leaves in
    exp(d)), expf (2 LIBM_ULP U), the row sum (cols adds, and its terms' own errors: at most the largest of them), one divide:
    bound = y U (|d| + max|d| + 4 LIBM_ULP + cols + 1) + 2^-126."""
    x = f64(x)
    d = x - x.max(axis=1, keepdims=True)
    e = np.exp(d)
    y = e / e.sum(axis=1, keepdims=True)
    c = np.abs(d) + np.abs(d).max(axis=1, keepdims=True) + 4 * LIBM_ULP + x.shape[1] + 1
    return y, y * U * c + F32_TINY


# ----------------------------------------------------------------------------- losses
def _tie(value_f32, fn_of_x):
    """A tensor whose VALUE is the f32 array the kernel was given (widened) and whose derivative is fn_of_x's."""
    return fn_of_x + (torch.from_numpy(f64(value_f32)) - fn_of_x).detach()


def _clip(p):
    """Keras' clip as f32 arithmetic performs it: both bounds are f32 values, so clamping the widened value is the f32 clamp widened.
    (After it the oracle's own f64 clamp to [1e-7, 1 - 1e-7] never binds: CLIP_LO > 1e-7 and CLIP_HI < 1 - 1e-7.)"""
    return p.clamp(float(CLIP_LO), float(CLIP_HI))


def rpn_cls_autograd(y_true, p, A):
    """cls_loss_rpn and its gradient w.r.t. the logit x, p = sigmoid(x), by autograd.  (loss, grad (cells, A))."""
    p32 = np.asarray(p, np.float32)
    pc = np.clip(p32, CLIP_LO, CLIP_HI).astype(np.float64)
    x = torch.from_numpy(np.log(pc / (1 - pc))).requires_grad_(True)           # a logit whose sigmoid is p (clipped p where p is 0 or 1)
    loss = ktr.cls_loss_rpn(torch.from_numpy(f64(y_true)), _clip(_tie(p32, torch.sigmoid(x))), A)
    g, = torch.autograd.grad(loss, x)
    return float(loss.detach()), g.numpy()


def rpn_cls_closed(y_true, p, A):
    """The same in closed form, plus the bounds.  Returns (loss, grad, bound_loss, bound_grad).
    Kernel per term: x = logf(pc / (1 - pc)): a subtract and a divide leave 2 U relative in the ratio = 2 U absolute in x, logf adds
    2 LIBM_ULP U |x|: ex = U (2 + 2 LIBM_ULP |x|).  bce = max(x,0) - x z + log1pf(expf(-|x|)), z in {0,1}: the first two are exact and
    either cancel (bce = sp, the softplus term alone) or leave |x| (ex absolute); sp takes ex as a relative error through expf, then
    2 LIBM_ULP U each for expf and log1pf; two adds, U bce each.  Terms are summed in f64; /256 exact; one cast: U |loss|.
    Gradient sel (pc - z) / 256: one subtract (and this reference's own round trip through the logit, far below U): 2 U |g|."""
    yt, p32 = f64(y_true), np.asarray(p, np.float32)
    sel, z = yt[..., :A], yt[..., A:]
    pc = np.clip(p32, CLIP_LO, CLIP_HI).astype(np.float64)
    x = np.log(pc / (1 - pc))
    sp = np.log1p(np.exp(-np.abs(x)))
    lin = np.maximum(x, 0) - x * z
    bce = lin + sp
    loss = float((sel * bce).sum() / 256.0)
    clipped = (p32 < CLIP_LO) | (p32 > CLIP_HI)
    grad = np.where(clipped, 0.0, sel * (pc - z) / 256.0)
    ex = U * (2 + 2 * LIBM_ULP * np.abs(x))
    eterm = ex * (lin != 0) + sp * (ex + 4 * LIBM_ULP * U) + 2 * U * bce
    return loss, grad, float((sel * eterm).sum() / 256.0) + U * abs(loss), 2 * U * np.abs(grad)


def rpn_reg_autograd(y_true, pred, A):
    pr = torch.from_numpy(f64(pred)).requires_grad_(True)
    loss = ktr.bbreg_loss_rpn(torch.from_numpy(f64(y_true)), pr, A)
    g, = torch.autograd.grad(loss, pr)
    return float(loss.detach()), g.numpy()


def _smooth_l1(d):
    a = np.abs(d)
    return np.where(a <= 1.0, 0.5 * a * a, a - 0.5), np.where(a <= 1.0, d, np.sign(d))


def rpn_reg_closed(y_true, pred, A):
    """(loss, grad, bound_loss, bound_grad).  Kernel per term: d = t - pred (U), then 0.5 a a (one more inexact multiply: 3 U relative)
    or a - 0.5 (U a + U (a - 0.5) <= 3 U (a - 0.5) as a > 1): 3 U per term, all terms >= 0, f64 sums, one cast: 4 U loss.
    Gradient -coef * slope: coef cast once (U), slope d carries U, one multiply: 3 U |g|."""
    yt, pr = f64(y_true), f64(pred)
    mask, t = yt[..., :4 * A], yt[..., 4 * A:]
    v, s = _smooth_l1(t - pr)
    coef = mask.mean() * 10.0 / 2400.0
    loss, grad = float(coef * v.sum()), -coef * s
    return loss, grad, 4 * U * abs(loss), 3 * U * np.abs(grad)


def det_reg_autograd(y_true, pred, K):
    pr = torch.from_numpy(f64(pred)).requires_grad_(True)
    loss = ktr.bbreg_loss_det(torch.from_numpy(f64(y_true)), pr, K)
    g, = torch.autograd.grad(loss, pr)
    return float(loss.detach()), g.numpy()


def det_reg_bounds(loss, grad):
    """Kernel: numerator terms m * smooth_l1 (m in {0,1}: 3 U each, as rpn_reg_closed), denominator terms 1e-4f + m (the f32 constant
    is within U of 1e-4, the add rounds once: 2 U), quotient in f64, one cast: 6 U |loss|.  Gradient -m * inv * slope: inv = 1/Den cast
    (2 U + U), slope (U), one inexact multiply (U): 5 U |g|."""
    return 6 * U * abs(loss), 5 * U * np.abs(grad)


def det_cls_autograd(y_true, p, logits):
    """cls_loss_det and its gradient w.r.t. the pre-softmax logits (f64 array whose softmax, rounded to f32, is p except in rows set by
    hand, which must be clipped rows).  (loss, grad (n, C))."""
    x = torch.from_numpy(np.asarray(logits, np.float64)).requires_grad_(True)
    pt = _tie(p, torch.softmax(x, dim=1))
    yt = torch.from_numpy(f64(y_true))
    qt = (yt * _clip(pt / pt.sum(dim=-1, keepdim=True))).sum(dim=-1, keepdim=True)      # the true class's clipped share (f32 bounds)
    # hand the oracle a row that sums to 1 identically and holds qt at the true class: its own renormalisation and f64 clip are then
    # the identity, and it returns mean(-log qt)
    loss = ktr.cls_loss_det(yt, yt * qt + (1 - yt) * (1 - qt) / (yt.shape[1] - 1))
    g, = torch.autograd.grad(loss, x)
    return float(loss.detach()), g.numpy()


def det_cls_closed(y_true, p):
    """(loss, grad, bound_loss, bound_grad) for ONE-HOT y_true.
    Kernel per row: sum of C probabilities ((C-1) U) and a divide (U) leave C U relative in q = C U absolute in log q, logf adds
    2 LIBM_ULP U |log q|; rows summed in f64, /n, one cast: bound_loss = mean(C U + 2 LIBM_ULP U |l_r|) + U |loss|.
    Gradient (p - y) / n: a subtract and a divide, 2 U |p - y| / n; the autograd reference differentiates the f64 softmax s whose
    rounding p is (|s - p| <= U p, and the factor s_c / p_c it carries is within U of 1): another (U p + U |p - y|) / n."""
    yt, pp = f64(y_true), f64(p)
    n, C = pp.shape
    q32 = (pp / pp.sum(axis=1, keepdims=True))
    qt = (yt * q32).sum(axis=1)
    clipped = (qt < float(CLIP_LO)) | (qt > float(CLIP_HI))
    l = -np.log(np.clip(qt, float(CLIP_LO), float(CLIP_HI)))
    loss = float(l.mean())
    grad = np.where(clipped[:, None], 0.0, (pp - yt) / n)
    bl = float((C * U + 2 * LIBM_ULP * U * np.abs(l)).mean()) + U * abs(loss)
    return loss, grad, bl, np.where(clipped[:, None], 0.0, (3 * U * np.abs(pp - yt) + U * pp) / n)
