"""YUV4MPEG2 (.y4m) streams on the host side: the header, a sequential reader that works on a pipe, a writer, and the frame arithmetic
in numpy for whoever wants pixels without a device (``_Y4mFrame.raw_rgb`` in annotate_video.py).  The per-pixel work of the captured
passes is csrc/y4m.hip (ops.y4m_decode_batch_u8 / ops.y4m_encode_u8); include/ext/frcnn_hip_y4m.h states the arithmetic, and
``decode_host`` here computes the same bytes.

A stream is one text line ``YUV4MPEG2 W<w> H<h> [F<n>:<d>] [I<p>] [A<n>:<d>] [C<mode>] [X...]`` and then, per frame, a line
``FRAME[ params]`` followed by the frame's planes [Y | Cb | Cr], 8 bits per sample, rows unpadded.  Taken: 8-bit progressive streams in
C420jpeg (and bare C420), C420mpeg2, C422, C444 and Cmono; limited range unless the header says XCOLORRANGE=FULL."""
import numpy as np

from . import _lib
from ._lib import FrcnnError

MAGIC = b"YUV4MPEG2"
MAX_HEADER = 4096                       # bytes of a header or FRAME line (mjpegtools' own limit is 256)
CHROMA_TAGS = {"420jpeg": "420jpeg", "420": "420jpeg", "420mpeg2": "420mpeg2", "422": "422", "444": "444", "mono": "mono"}
REFUSED_CHROMAS = {"420paldv": "C420paldv: vertically alternating chroma sites (PAL DV) are not supported",
                   "411": "C411: 4:1:1 chroma is not supported", "444alpha": "C444alpha: an alpha plane is not supported"}
DEFAULT_TAGS = {"F": "25:1", "A": "0:0", "I": "p"}


class Y4mUnsupported(FrcnnError):
    """``parse_header``: a well-formed stream outside the supported set; the message names the reason."""


def frame_bytes(h, w, chroma):
    """Bytes of one frame's planes (frcnn_y4m_frame_bytes); ``chroma`` a name of ``_lib.Y4M_CHROMAS``."""
    h, w = int(h), int(w)
    if chroma not in _lib.Y4M_CHROMAS or not (1 <= h <= _lib.Y4M_MAX_SIDE and 1 <= w <= _lib.Y4M_MAX_SIDE):
        raise FrcnnError("y4m frame_bytes: h=%r w=%r (1..%d), chroma=%r (%s)" % (h, w, _lib.Y4M_MAX_SIDE, chroma, ", ".join(_lib.Y4M_CHROMAS)))
    cw, ch = chroma_size(h, w, chroma)
    return h * w + 2 * cw * ch


def chroma_size(h, w, chroma):
    """(plane width, plane height) of a chroma plane; (0, 0) for "mono"."""
    if chroma == "mono":
        return 0, 0
    return (w if chroma == "444" else (w + 1) // 2), ((h + 1) // 2 if chroma in ("420jpeg", "420mpeg2") else h)


def make_plan(h, w, chroma="420jpeg", range="limited", tags=None):          # noqa: A002 -- the format's own word
    """A ``_lib.Y4mPlan`` for frames of (h, w) in ``chroma`` / ``range``; ``tags``: the stream's F / A / I values."""
    if range not in _lib.Y4M_RANGES:
        raise FrcnnError("y4m: range=%r (%s)" % (range, ", ".join(_lib.Y4M_RANGES)))
    plan = _lib.Y4mPlan(int(h), int(w), _lib.Y4M_CHROMAS.get(chroma, -1), _lib.Y4M_RANGES[range], frame_bytes(h, w, chroma), 0)
    plan.tags = dict(DEFAULT_TAGS, **(tags or {}))
    plan.header_len = 0
    return plan


def parse_header(data):
    """The stream header at the start of ``data`` (bytes that hold at least its first line) -> a ``_lib.Y4mPlan``: h, w, chroma, range,
    frame_bytes, and as Python attributes ``tags`` ({"F", "A", "I"}: the values verbatim, defaults where the header has none) and
    ``header_len`` (bytes up to and including the newline).  ``Y4mUnsupported`` with the reason for high bit depths, interlaced streams
    and the chroma modes not taken; ``FrcnnError`` for a broken header."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise FrcnnError("y4m_parse_header: the stream's first bytes, got %s" % type(data).__name__)
    data = bytes(data[:MAX_HEADER])
    end = data.find(b"\n")
    if not data.startswith(MAGIC + b" ") or end < 0:
        raise FrcnnError("y4m header: no 'YUV4MPEG2 ' line within the first %d bytes" % min(len(data), MAX_HEADER))
    try:
        fields = data[len(MAGIC) + 1:end].decode("ascii").split()
    except UnicodeDecodeError:
        raise FrcnnError("y4m header: not ASCII") from None
    seen = {}
    for f in fields:
        if f[0] == "X":
            seen.setdefault("X", []).append(f[1:])
        elif f[0] in seen:
            raise FrcnnError("y4m header: tag %s twice" % f[0])
        else:
            seen[f[0]] = f[1:]
    size = {}
    for k in ("W", "H"):
        v = seen.get(k, "")
        if not v.isdigit() or not 1 <= int(v) <= _lib.Y4M_MAX_SIDE:
            raise FrcnnError("y4m header: %s%s (a size in 1..%d is required)" % (k, v, _lib.Y4M_MAX_SIDE))
        size[k] = int(v)
    for k in ("F", "A"):
        v = seen.get(k)
        if v is not None and not (v.count(":") == 1 and all(p.isdigit() for p in v.split(":"))):
            raise FrcnnError("y4m header: %s%s (a ratio n:d)" % (k, v))
    inter = seen.get("I", "p")
    if inter in ("t", "b", "m"):
        raise Y4mUnsupported("I%s: interlaced streams are not supported (progressive only)" % inter)
    if inter != "p":
        raise FrcnnError("y4m header: I%s (Ip, It, Ib or Im)" % inter)
    mode = seen.get("C", "420jpeg")
    base, _, depth = mode.partition("p") if mode not in REFUSED_CHROMAS else (mode, "", "")
    if mode in REFUSED_CHROMAS:
        raise Y4mUnsupported(REFUSED_CHROMAS[mode])
    if depth.isdigit() and base in CHROMA_TAGS:
        raise Y4mUnsupported("C%s: %s bits per sample, only 8-bit streams are supported" % (mode, depth))
    if mode not in CHROMA_TAGS:
        raise Y4mUnsupported("C%s: an unknown chroma mode" % mode)
    full = any(x.upper() == "COLORRANGE=FULL" for x in seen.get("X", []))
    plan = make_plan(size["H"], size["W"], CHROMA_TAGS[mode], "full" if full else "limited",
                     {k: seen[k] for k in ("F", "A", "I") if k in seen})
    plan.header_len = end + 1
    return plan


def header_line(w, h, chroma="420jpeg", range="limited", tags=None):       # noqa: A002
    """The stream header for these settings, newline included."""
    frame_bytes(h, w, chroma)
    if range not in _lib.Y4M_RANGES:
        raise FrcnnError("y4m: range=%r (%s)" % (range, ", ".join(_lib.Y4M_RANGES)))
    t = dict(DEFAULT_TAGS, **(tags or {}))
    line = "YUV4MPEG2 W%d H%d F%s I%s A%s C%s" % (w, h, t["F"], t["I"], t["A"], chroma)
    return (line + (" XCOLORRANGE=FULL" if range == "full" else "") + "\n").encode("ascii")


def _read_exact(f, n):
    """Up to ``n`` bytes from a file object that may return short reads (a pipe)."""
    parts, got = [], 0
    while got < n:
        part = f.read(n - got)
        if not part:
            break
        parts.append(part)
        got += len(part)
    return parts[0] if len(parts) == 1 else b"".join(parts)


class Y4mReader:
    """Frames of a y4m stream, in order, from a binary file object that is only ever read forwards (a pipe will do).  ``plan``: the
    header's (``parse_header``).  Iterating yields each frame's planes as ``bytes``; FRAME parameter tags are skipped; a stream that
    ends inside a frame raises FrcnnError naming the frame's index."""

    def __init__(self, fileobj, name="<stream>"):
        self.f, self.name, self.index = fileobj, name, 0
        line = fileobj.readline(MAX_HEADER)
        self.plan = parse_header(line)

    def __iter__(self):
        return self

    def __next__(self):
        line = self.f.readline(MAX_HEADER)
        if not line:
            raise StopIteration
        if not (line.startswith(b"FRAME") and line.endswith(b"\n") and line[5:6] in (b"\n", b" ")):
            raise FrcnnError("%s: frame %d: no FRAME line (%r)" % (self.name, self.index, line[:16]))
        need = int(self.plan.frame_bytes)
        data = _read_exact(self.f, need)
        if len(data) != need:
            raise FrcnnError("%s: frame %d is cut short: %d of %d bytes" % (self.name, self.index, len(data), need))
        self.index += 1
        return data


class Y4mWriter:
    """A y4m stream written to a binary file object: the header at construction, then ``write(frame)`` per frame (its planes, exactly
    ``frame_bytes`` long)."""

    def __init__(self, fileobj, w, h, chroma="420jpeg", range="limited", tags=None):         # noqa: A002
        self.f, self.w, self.h, self.chroma, self.range = fileobj, int(w), int(h), chroma, range
        self.frame_bytes = frame_bytes(h, w, chroma)
        self.frames = 0
        fileobj.write(header_line(self.w, self.h, chroma, range, tags))

    def write(self, frame):
        if len(frame) != self.frame_bytes:
            raise FrcnnError("y4m writer: frame %d has %d bytes, a %dx%d C%s frame has %d" % (self.frames, len(frame), self.w, self.h, self.chroma, self.frame_bytes))
        self.f.write(b"FRAME\n")
        self.f.write(frame)
        self.frames += 1

    def flush(self):
        self.f.flush()


# ---------------------------------------------------------------------------------------------------------------- host arithmetic
# (include/ext/frcnn_hip_y4m.h; >> on numpy's signed integers rounds towards minus infinity, as the kernels' does)
BT601_DEC = {"y": 76309, "rv": 104597, "gu": 25675, "gv": 53279, "bu": 132201}


def _tri(a, b, odd):
    return (3 * a + b + 1 + odd) >> 2


def _up_centred(c, n, axis):
    """A plane upsampled two-fold along ``axis`` to ``n`` samples by the triangle filter (edges replicate)."""
    c = np.moveaxis(c, axis, 0)
    lo, hi = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    out = np.empty((2 * c.shape[0],) + c.shape[1:], dtype=np.int64)
    out[0::2], out[1::2] = _tri(c, lo, 0), _tri(c, hi, 1)
    return np.moveaxis(out[:n], 0, axis)


def _up_cosited(c, n, axis):
    c = np.moveaxis(c, axis, 0)
    out = np.empty((2 * c.shape[0],) + c.shape[1:], dtype=np.int64)
    out[0::2], out[1::2] = c, (c + np.concatenate([c[1:], c[-1:]]) + 1) >> 1
    return np.moveaxis(out[:n], 0, axis)


def _up_h2v2(c, h, w):
    """Both axes centred: libjpeg's h2v2 fancy upsampling, 9-3-3-1 over 16 with biases 8 (even columns) and 7 (odd columns)."""
    near = np.repeat(c, 2, axis=0)[:h]
    far = np.empty_like(near)
    up, down = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    far[0::2], far[1::2] = up[:(h + 1) // 2], down[:h // 2]
    cs = 3 * near + far
    left, right = np.concatenate([cs[:, :1], cs[:, :-1]], axis=1), np.concatenate([cs[:, 1:], cs[:, -1:]], axis=1)
    out = np.empty((h, 2 * c.shape[1]), dtype=np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * cs + left + 8) >> 4, (3 * cs + right + 7) >> 4
    return out[:, :w]


def decode_host(frame, plan, bgr=False):
    """One frame's planes (bytes) -> (h, w, 3) uint8, R,G,B per pixel (``bgr``: B,G,R): what ops.y4m_decode_u8 computes, in numpy."""
    h, w, chroma = int(plan.h), int(plan.w), plan.chroma_name
    buf = np.frombuffer(frame, dtype=np.uint8)
    if buf.size != int(plan.frame_bytes):
        raise FrcnnError("y4m decode_host: %d bytes, the plan's frames have %d" % (buf.size, int(plan.frame_bytes)))
    lum = buf[:h * w].reshape(h, w).astype(np.int64)
    if chroma == "mono":
        cb = cr = np.zeros((h, w), dtype=np.int64)
    else:
        cw, ch = chroma_size(h, w, chroma)
        planes = [buf[h * w + k * cw * ch:h * w + (k + 1) * cw * ch].reshape(ch, cw).astype(np.int64) for k in (0, 1)]
        if chroma == "420jpeg":
            planes = [_up_h2v2(c, h, w) for c in planes]
        elif chroma == "420mpeg2":
            planes = [_up_cosited(_up_centred(c, h, 0), w, 1) for c in planes]
        elif chroma == "422":
            planes = [_up_cosited(c, w, 1) for c in planes]
        cb, cr = planes[0] - 128, planes[1] - 128
    if plan.range_name == "full":
        r = lum + ((91881 * cr + 32768) >> 16)
        g = lum + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
        b = lum + ((116130 * cb + 32768) >> 16)
    else:
        k, base = BT601_DEC, BT601_DEC["y"] * (lum - 16) + 32768
        r, g, b = (base + k["rv"] * cr) >> 16, (base - k["gu"] * cb - k["gv"] * cr) >> 16, (base + k["bu"] * cb) >> 16
    return np.clip(np.stack([b, g, r] if bgr else [r, g, b], axis=2), 0, 255).astype(np.uint8)
