"""The full-format device PNG decoder restated (faster_rcnn_amd/csrc/png_dec_full.hip, include/ext/frcnn_hip_png_dec_full.h): plain numpy
and ``zlib.decompress``.  Parse the chunks, split the inflated bytes into the Adam7 passes (or the one pass of a file without interlace),
undo the row filters per pass with a filter unit of max(1, bits_per_pixel / 8) bytes, expand the samples (sub-byte MSB first, palette
lookup with black beyond the PLTE's entries, grey x 255 / 85 / 17, the high byte of a 16-bit sample, alpha dropped) and place every pixel
at (y0 + r * dy, x0 + i * dx).  tests/test_png_full_cpu.py holds this to Pillow byte for byte; the kernels are held to this."""
import struct
import zlib

import numpy as np

# (x0, y0, dx, dy) of the seven Adam7 passes
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


class BadFilter(ValueError):
    """A row whose filter byte is not 0..4."""


def parse(data):
    """The chunks of a sound file -> dict(h, w, depth, colour, interlace, plte_off, entries, palette (768 bytes or b""), stream, spans)."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, info, spans = 8, dict(plte_off=0, entries=0, palette=b""), []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if kind == b"IHDR":
            info["w"], info["h"], info["depth"], info["colour"], _, _, info["interlace"] = struct.unpack(">IIBBBBB", body)
        elif kind == b"PLTE" and info["colour"] == 3 and not spans:
            info["plte_off"], info["entries"], info["palette"] = pos + 8, n // 3, body + bytes(768 - n)
        elif kind == b"IDAT":
            spans.append((pos + 8, n))
        pos += 12 + n
    info["spans"] = spans
    info["stream"] = b"".join(data[o:o + n] for o, n in spans)
    return info


def passes(h, w, interlace):
    """[(x0, y0, dx, dy, pw, ph)] of the passes that exist, in stream order."""
    if not interlace:
        return [(0, 0, 1, 1, w, h)]
    out = []
    for x0, y0, dx, dy in ADAM7:
        pw, ph = max(0, -(-(w - x0) // dx)), max(0, -(-(h - y0) // dy))
        if pw and ph:
            out.append((x0, y0, dx, dy, pw, ph))
    return out


def row_bytes(pw, bits):
    return (pw * bits + 7) // 8


def inflated_len(h, w, bits, interlace):
    return sum(ph * (1 + row_bytes(pw, bits)) for _, _, _, _, pw, ph in passes(h, w, interlace))


def unfilter(raw, ph, rb, bpp):
    """``ph`` rows of a filter byte and ``rb`` bytes -> the reconstructed (ph, rb) uint8 rows; the row above the first is zero."""
    out = np.zeros((ph, rb), np.uint8)
    prev = bytearray(rb)
    for r in range(ph):
        at = r * (1 + rb)
        ft, cur = raw[at], bytearray(raw[at + 1:at + 1 + rb])
        if ft > 4:
            raise BadFilter("row %d: filter type %d" % (r, ft))
        if ft == 1:
            for i in range(bpp, rb):
                cur[i] = (cur[i] + cur[i - bpp]) & 255
        elif ft == 2:
            for i in range(rb):
                cur[i] = (cur[i] + prev[i]) & 255
        elif ft == 3:
            for i in range(rb):
                cur[i] = (cur[i] + (((cur[i - bpp] if i >= bpp else 0) + prev[i]) >> 1)) & 255
        elif ft == 4:
            for i in range(rb):
                a, b, c = (cur[i - bpp], prev[i], prev[i - bpp]) if i >= bpp else (0, prev[i], 0)
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                cur[i] = (cur[i] + (a if pa <= pb and pa <= pc else (b if pb <= pc else c))) & 255
        out[r] = np.frombuffer(bytes(cur), np.uint8)
        prev = cur
    return out


def expand(rows, pw, info):
    """The reconstructed (ph, rb) rows of one pass -> its (ph, pw, 3) RGB pixels."""
    ph, depth, colour = rows.shape[0], info["depth"], info["colour"]
    ch = CHANNELS[colour]
    if depth < 8:
        bits = np.unpackbits(rows, axis=1)[:, :pw * depth].reshape(ph, pw, depth).astype(np.int64)
        s = (bits << np.arange(depth - 1, -1, -1)).sum(axis=2)[:, :, None]
    elif depth == 8:
        s = rows[:, :pw * ch].reshape(ph, pw, ch).astype(np.int64)
    else:
        s = rows[:, :pw * ch * 2].reshape(ph, pw, ch, 2)[:, :, :, 0].astype(np.int64)      # the high byte
    if colour == 3:
        table = np.zeros((256, 3), np.uint8)
        table[:info["entries"]] = np.frombuffer(info["palette"], np.uint8).reshape(256, 3)[:info["entries"]]
        return table[s[:, :, 0]]
    if ch < 3:
        grey = s[:, :, 0] * ({1: 255, 2: 85, 4: 17}.get(depth, 1))
        return np.repeat(grey[:, :, None], 3, axis=2).astype(np.uint8)
    return s[:, :, :3].astype(np.uint8)


def decode(data, bgr=False):
    """A sound file's bytes -> its (h, w, 3) uint8 frame, R,G,B (or B,G,R): numpy.asarray(PIL.Image.open(f).convert("RGB"))."""
    info = parse(data)
    h, w = info["h"], info["w"]
    bits = CHANNELS[info["colour"]] * info["depth"]
    raw = zlib.decompress(info["stream"])
    assert len(raw) == inflated_len(h, w, bits, info["interlace"])
    out, at, bpp = np.zeros((h, w, 3), np.uint8), 0, max(1, bits // 8)
    for x0, y0, dx, dy, pw, ph in passes(h, w, info["interlace"]):
        rb = row_bytes(pw, bits)
        rows = unfilter(raw[at:at + ph * (1 + rb)], ph, rb, bpp)
        at += ph * (1 + rb)
        out[y0::dy, x0::dx] = expand(rows, pw, info)
    return np.ascontiguousarray(out[:, :, ::-1] if bgr else out)
