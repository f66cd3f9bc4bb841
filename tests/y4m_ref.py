"""The YUV4MPEG2 frame arithmetic restated in numpy: THE CONTRACT of csrc/y4m.hip (include/ext/frcnn_hip_y4m.h states it in words).
Integers only; ``>>`` on numpy's signed integers rounds towards minus infinity.  Written per pixel with explicit index arrays -- sample
(x, y) of the output reads these samples of the planes -- so that it shares nothing with the product's host code (faster_rcnn_amd/y4m.py:
whole-plane shifts), which tests/test_y4m_cpu.py holds against it.

Chroma modes on input: "420jpeg" (centred both ways), "420mpeg2" (co-sited horizontally, centred vertically), "422" (co-sited
horizontally), "444", "mono".  On output: "420jpeg", "444".  Ranges: "limited" (BT.601, the table below) and "full" (JFIF)."""
import numpy as np

CHROMAS = ("420jpeg", "420mpeg2", "422", "444", "mono")
OUT_CHROMAS = ("420jpeg", "444")
RANGES = ("limited", "full")

# BT.601 limited range, 16 fractional bits, each coefficient rounded ONCE from the reals (Kr = 0.299, Kb = 0.114, Kg = 0.587; luma
# excursion 219, chroma excursion 224):
#   decode  255/219, 2(1-Kr) 255/224, 2(1-Kb)Kb/Kg 255/224, 2(1-Kr)Kr/Kg 255/224, 2(1-Kb) 255/224
#   encode  K 219/255 for Y; K / (2(1-Kb)) 224/255 for Cb; K / (2(1-Kr)) 224/255 for Cr
KR, KB = 0.299, 0.114
KG = 1.0 - KR - KB
DEC_Y, DEC_RV, DEC_GU, DEC_GV, DEC_BU = 76309, 104597, 25675, 53279, 132201
ENC_Y = (16829, 33039, 6416)
ENC_CB = (-9714, -19071, 28784)
ENC_CR = (28784, -24103, -4681)


def coefficients_from_reals():
    """The table above, recomputed: round(65536 * real)."""
    r = lambda v: int(round(v * 65536.0))      # noqa: E731
    dec = (r(255 / 219), r(2 * (1 - KR) * 255 / 224), r(2 * (1 - KB) * KB / KG * 255 / 224), r(2 * (1 - KR) * KR / KG * 255 / 224),
           r(2 * (1 - KB) * 255 / 224))
    ey = tuple(r(k * 219 / 255) for k in (KR, KG, KB))
    ecb = (-r(KR / (2 * (1 - KB)) * 224 / 255), -r(KG / (2 * (1 - KB)) * 224 / 255), r(0.5 * 224 / 255))
    ecr = (r(0.5 * 224 / 255), -r(KG / (2 * (1 - KR)) * 224 / 255), -r(KB / (2 * (1 - KR)) * 224 / 255))
    return dec, ey, ecb, ecr


def chroma_size(h, w, chroma):
    if chroma == "mono":
        return 0, 0
    return (w if chroma == "444" else (w + 1) // 2), ((h + 1) // 2 if chroma.startswith("420") else h)


def frame_bytes(h, w, chroma):
    cw, ch = chroma_size(h, w, chroma)
    return h * w + 2 * cw * ch


def split(frame, h, w, chroma):
    """bytes -> (Y, Cb, Cr) int64 planes (Cb = Cr = None for mono)."""
    buf = np.frombuffer(bytes(frame), dtype=np.uint8).astype(np.int64)
    assert buf.size == frame_bytes(h, w, chroma)
    cw, ch = chroma_size(h, w, chroma)
    lum = buf[:h * w].reshape(h, w)
    if chroma == "mono":
        return lum, None, None
    return lum, buf[h * w:h * w + cw * ch].reshape(ch, cw), buf[h * w + cw * ch:].reshape(ch, cw)


# ------------------------------------------------------------------------------------------------------------------- upsampling
def upsample(c, h, w, chroma):
    """One chroma plane at full size."""
    ch, cw = c.shape
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if chroma == "444":
        return c[y, x]
    i = x >> 1
    i1 = np.minimum(i + 1, cw - 1)
    xodd = x & 1
    if chroma == "422":                                          # co-sited: the sample itself, or the rounded mean with the next
        return np.where(xodd == 1, (c[y, i] + c[y, i1] + 1) >> 1, c[y, i])
    yr, yodd = y >> 1, y & 1
    yf = np.where(yodd == 1, np.minimum(yr + 1, ch - 1), np.maximum(yr - 1, 0))     # the farther row (edges replicate)
    if chroma == "420mpeg2":                                     # vertical triangle per chroma column, then co-sited horizontally
        a = (3 * c[yr, i] + c[yf, i] + 1 + yodd) >> 2
        b = (3 * c[yr, i1] + c[yf, i1] + 1 + yodd) >> 2
        return np.where(xodd == 1, (a + b + 1) >> 1, a)
    assert chroma == "420jpeg"                                   # libjpeg's h2v2 fancy upsampling: 9-3-3-1 over 16
    ix = np.where(xodd == 1, np.minimum(i + 1, cw - 1), np.maximum(i - 1, 0))       # the farther column
    cs, co = 3 * c[yr, i] + c[yf, i], 3 * c[yr, ix] + c[yf, ix]
    return (3 * cs + co + np.where(xodd == 1, 7, 8)) >> 4


# ----------------------------------------------------------------------------------------------------------------------- colour
def ycc_to_rgb(lum, cb, cr, range_):
    """Y, Cb, Cr in 0..255 (arrays) -> R, G, B in 0..255."""
    lum, cb, cr = np.asarray(lum, np.int64), np.asarray(cb, np.int64) - 128, np.asarray(cr, np.int64) - 128
    if range_ == "full":                                         # JFIF, libjpeg's jdcolor.c
        r = lum + ((91881 * cr + 32768) >> 16)
        g = lum + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
        b = lum + ((116130 * cb + 32768) >> 16)
    else:
        base = DEC_Y * (lum - 16) + 32768
        r = (base + DEC_RV * cr) >> 16
        g = (base - DEC_GU * cb - DEC_GV * cr) >> 16
        b = (base + DEC_BU * cb) >> 16
    return tuple(np.clip(v, 0, 255) for v in (r, g, b))


def rgb_to_ycc(r, g, b, range_):
    r, g, b = (np.asarray(v, np.int64) for v in (r, g, b))
    if range_ == "full":                                         # JFIF, libjpeg's jccolor.c
        cround = (128 << 16) + 32767
        return ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16, (-11059 * r - 21709 * g + 32768 * b + cround) >> 16,
                (32768 * r - 27439 * g - 5329 * b + cround) >> 16)
    out = []
    for off, k in ((16, ENC_Y), (128, ENC_CB), (128, ENC_CR)):
        out.append(np.clip(off + ((k[0] * r + k[1] * g + k[2] * b + 32768) >> 16), 0, 255))
    return tuple(out)


# -------------------------------------------------------------------------------------------------------------- frames
def decode(frame, h, w, chroma, range_, bgr=False):
    """A frame's planes (bytes) -> (h, w, 3) uint8."""
    lum, cb, cr = split(frame, h, w, chroma)
    if chroma == "mono":
        cb = cr = np.full((h, w), 128, dtype=np.int64)
    else:
        cb, cr = upsample(cb, h, w, chroma), upsample(cr, h, w, chroma)
    r, g, b = ycc_to_rgb(lum, cb, cr, range_)
    return np.stack([b, g, r] if bgr else [r, g, b], axis=2).astype(np.uint8)


def encode(rgb, chroma, range_, bgr=False):
    """(h, w, 3) uint8 -> the frame's record [Y | Cb | Cr] as bytes; "420jpeg": the 2x2 box average of the per-pixel Cb / Cr with
    libjpeg's bias (1 at even, 2 at odd chroma columns), the last column / row repeated into a group that reaches past the frame."""
    assert chroma in OUT_CHROMAS
    rgb = np.asarray(rgb)
    h, w = rgb.shape[:2]
    px = rgb[:, :, ::-1] if bgr else rgb
    lum, cb, cr = rgb_to_ycc(px[:, :, 0], px[:, :, 1], px[:, :, 2], range_)
    if chroma == "420jpeg":
        cw, ch = chroma_size(h, w, chroma)
        yy, xx = np.meshgrid(np.arange(ch), np.arange(cw), indexing="ij")
        planes = []
        for c in (cb, cr):
            s = 0
            for dy in (0, 1):
                for dx in (0, 1):
                    s = s + c[np.minimum(2 * yy + dy, h - 1), np.minimum(2 * xx + dx, w - 1)]
            planes.append((s + 1 + (xx & 1)) >> 2)
        cb, cr = planes
    return b"".join(np.asarray(p).astype(np.uint8).tobytes() for p in (lum, cb, cr))
