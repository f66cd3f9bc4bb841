"""The files the device PNG decoder's tests decode (faster_rcnn_amd/csrc/png_dec.hip, include/ext/frcnn_hip_png_dec.h), all made at test
time: Pillow's own files, and files from a small chunk writer with a numpy row filter and ``zlib.compressobj`` so that the filter types,
the deflate block types and the places where the IDATs are cut can be chosen.  A case is (name, file bytes, expected (h, w, 3) RGB frame);
for a written file the expected pixels are the generating frame, and tests/test_png_dec_cpu.py checks that Pillow agrees."""
import functools
import io
import os
import struct
import zlib

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
PHOTO = os.path.join(HERE, "golden", "VOC_test", "JPEGImages", "000005.jpg")
SIGNATURE = b"\x89PNG\r\n\x1a\n"
COLOUR = {1: 0, 3: 2, 4: 6}


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def png_file(w, h, channels, idats, depth=8, interlace=0, extra=b""):
    """A PNG file around the given IDAT payloads (a list: one chunk each)."""
    ihdr = struct.pack(">IIBBBBB", w, h, depth, COLOUR[channels], 0, 0, interlace)
    return SIGNATURE + chunk(b"IHDR", ihdr) + extra + b"".join(chunk(b"IDAT", d) for d in idats) + chunk(b"IEND", b"")


def filter_rows(frame, types):
    """The filtered bytes of an (h, w, c) uint8 frame: row y under filter type types[y] (PNG filter method 0)."""
    h, w, c = frame.shape
    cur = frame.reshape(h, w * c).astype(np.int32)
    up = np.vstack([np.zeros((1, w * c), np.int32), cur[:-1]])
    left = np.hstack([np.zeros((h, c), np.int32), cur[:, :-c]])
    upleft = np.hstack([np.zeros((h, c), np.int32), up[:, :-c]])
    p = left + up - upleft
    pa, pb, pc = abs(p - left), abs(p - up), abs(p - upleft)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
    pred = [np.zeros_like(cur), left, up, (left + up) >> 1, paeth]
    out = bytearray()
    for y in range(h):
        out.append(types[y])
        out += ((cur[y] - pred[types[y]][y]) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem=8):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, mem, strategy)
    return c.compress(raw) + c.flush()


def written(frame, types=None, **how):
    h, w, c = frame.shape
    return png_file(w, h, c, [deflate(filter_rows(frame, types or [0] * h), **how)])


def expected(frame):
    return np.ascontiguousarray(np.repeat(frame, 3, axis=2) if frame.shape[2] == 1 else frame[:, :, :3])


def split(stream, cuts):
    """The stream cut at the given offsets -> a list of IDAT payloads."""
    edges = [0] + list(cuts) + [len(stream)]
    return [stream[a:b] for a, b in zip(edges, edges[1:])]


def idat_payload(data):
    """(the IDAT payloads of a file back to back, [(offset, length)] of each)."""
    pos, spans = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if kind == b"IDAT":
            spans.append((pos + 8, n))
        pos += 12 + n
    return b"".join(data[o:o + n] for o, n in spans), spans


def pil_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@functools.lru_cache(maxsize=None)
def photo():
    return np.asarray(Image.open(PHOTO).convert("RGB"))


def pattern(h, w, c, seed):
    """A frame with structure (so that deflate finds matches) and noise (so that the codes are not trivial)."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = ((x * 7 + y * 13) & 255)[:, :, None] + np.arange(c)[None, None, :] * 40
    noise = rng.randint(0, 24, size=(h, w, c))
    return ((base + noise) & 255).astype(np.uint8)


def pil_file(frame, **save):
    mode = {1: "L", 3: "RGB", 4: "RGBA"}[frame.shape[2]]
    buf = io.BytesIO()
    Image.fromarray(frame[:, :, 0] if frame.shape[2] == 1 else frame, mode).save(buf, "PNG", **save)
    return buf.getvalue()


def skewed(n, seed):
    """Bytes whose Huffman code is well below 8 bits (zlib then writes a dynamic block, not a stored one) without a single match."""
    rng = np.random.RandomState(seed)
    return np.minimum(rng.geometric(0.08, size=n) - 1, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def sound_cases(window_bytes=8192):
    """[(name, file, expected RGB)]: every supported file of the set but the two photographs (``photo_cases``)."""
    cases = []
    # ---- Pillow's own files
    sizes = [(1, 1), (1, 7), (7, 1), (17, 23), (33, 65)]
    for h, w in sizes:
        for c in (3, 1, 4):
            frame = pattern(h, w, c, 100 * h + c)
            levels = (0, 1, 6, 9) if (h, w) in ((1, 1), (17, 23)) or c == 3 else (6,)
            for level in levels:
                cases.append(("pil_%dx%d_c%d_l%d" % (h, w, c, level), pil_file(frame, compress_level=level), None))
            if (h, w) in ((17, 23), (33, 65)):
                cases.append(("pil_%dx%d_c%d_opt" % (h, w, c), pil_file(frame, optimize=True), None))
    cases = [(name, data, pil_rgb(data)) for name, data, _ in cases]
    # ---- the writer's files: filter types
    for c in (3, 4):
        frame = pattern(17, 23, c, 7 + c)
        for ft in range(5):
            cases.append(("filter%d_c%d" % (ft, c), written(frame, [ft] * 17), expected(frame)))
        cases.append(("filter_mix_c%d" % c, written(frame, [(y + 1) % 5 for y in range(17)]), expected(frame)))
    grey = pattern(70, 9, 1, 3)                                 # (two strips of rows: the row kept between them, one byte per pixel)
    cases.append(("filter_mix_grey_70rows", written(grey, [(y * 3 + 4) % 5 for y in range(70)]), expected(grey)))
    tall = pattern(130, 5, 4, 4)
    cases.append(("filter_paeth_rgba_130rows", written(tall, [4 if y % 64 else 3 for y in range(130)]), expected(tall)))
    # ---- deflate strategies
    frame = pattern(17, 23, 3, 21)
    cases.append(("fixed", written(frame, [(y + 2) % 5 for y in range(17)], strategy=zlib.Z_FIXED), expected(frame)))
    cases.append(("huffman_only", written(frame, strategy=zlib.Z_HUFFMAN_ONLY), expected(frame)))
    stripes = np.zeros((40, 300, 3), np.uint8)
    stripes[10:20] = 200
    stripes[30:] = (1, 2, 3)
    cases.append(("rle_stripes", written(stripes, strategy=zlib.Z_RLE), expected(stripes)))
    rng = np.random.RandomState(5)
    far = rng.randint(0, 256, size=(64, 200, 3)).astype(np.uint8)
    far[54:64] = far[0:10]                                      # matches at distance 54 * 601 = 32 454, just under the window
    data = written(far)
    assert len(idat_payload(data)[0]) < 34000, "zlib did not take the far matches"
    cases.append(("far_matches", data, expected(far)))
    # ---- several blocks of different types in one stream
    frame = pattern(33, 65, 3, 9)
    raw = filter_rows(frame, [(y + 3) % 5 for y in range(33)])
    c = zlib.compressobj(6)
    third = len(raw) // 3
    stream = c.compress(raw[:third]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(raw[third:2 * third]) + c.flush(zlib.Z_FULL_FLUSH) + \
        c.compress(raw[2 * third:]) + c.flush()
    cases.append(("flushes", png_file(65, 33, 3, [stream]), expected(frame)))

    def segment(part, level, last):
        s = zlib.compressobj(level, zlib.DEFLATED, -15)
        return s.compress(part) + s.flush(zlib.Z_FINISH if last else zlib.Z_SYNC_FLUSH)
    stream = b"\x78\x9c" + segment(raw[:third], 6, False) + segment(raw[third:2 * third], 0, False) + segment(raw[2 * third:], 6, True) + \
        struct.pack(">I", zlib.adler32(raw))
    cases.append(("level_6_0_6", png_file(65, 33, 3, [stream]), expected(frame)))
    # ---- IDATs cut at hostile places
    frame = pattern(17, 23, 3, 11)
    stream = deflate(filter_rows(frame, [4] * 17))
    cases.append(("idat_1byte", png_file(23, 17, 3, [stream[i:i + 1] for i in range(len(stream))]), expected(frame)))
    cases.append(("idat_empty", png_file(23, 17, 3, split(stream, [100, 100])), expected(frame)))
    cases.append(("idat_header_adler", png_file(23, 17, 3, split(stream, [1, len(stream) - 2])), expected(frame)))
    text = chunk(b"tEXt", b"Comment\0skipped") + chunk(b"gAMA", struct.pack(">I", 45455))
    cases.append(("ancillary", png_file(23, 17, 3, [stream], extra=text), expected(frame)))
    # ---- one dynamic block larger than the kernel's window: the tables are carried over
    n = 64 * 200 * 3
    noisy = skewed(n, 17).reshape(64, 200, 3)
    data = written(noisy, strategy=zlib.Z_HUFFMAN_ONLY, mem=9)
    stream = idat_payload(data)[0]
    assert len(stream) > 2 * window_bytes and (stream[2] >> 1) & 3 == 2, "not a dynamic block beyond the window"
    cases.append(("block_beyond_window", data, expected(noisy)))
    # ---- exactly one row past a strip of 64 rows
    rows65 = pattern(65, 6, 3, 65)
    cases.append(("filter_mix_rgb_65rows", written(rows65, [4 if y % 64 else 3 for y in range(65)]), expected(rows65)))
    return cases


@functools.lru_cache(maxsize=None)
def photo_cases():
    """The realistic largest: the 375x500 photograph at levels 1 and 6."""
    out = []
    for level in (1, 6):
        data = pil_file(photo(), compress_level=level)
        out.append(("photo_l%d" % level, data, pil_rgb(data)))
    return out


def _patch_ihdr(data, index, value):
    ihdr = bytearray(data[16:29])
    ihdr[index] = value
    return data[:16] + bytes(ihdr) + struct.pack(">I", zlib.crc32(b"IHDR" + bytes(ihdr))) + data[33:]


@functools.lru_cache(maxsize=None)
def refusals():
    """[(name, file, a word of the planner's reason)]: one file per class the planner refuses."""
    frame = pattern(17, 23, 3, 31)
    sound = pil_file(frame, compress_level=6)
    buf = io.BytesIO()
    Image.fromarray(frame).convert("P", palette=Image.ADAPTIVE).save(buf, "PNG")
    palette = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray((frame[:, :, 0].astype(np.uint16) * 257)).save(buf, "PNG")
    deep = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(frame[:, :, :2], "LA").save(buf, "PNG")
    grey_alpha = buf.getvalue()
    bad_crc = bytearray(sound)
    _, spans = idat_payload(sound)
    bad_crc[spans[0][0] + 20] ^= 0x40
    unknown = sound[:33] + chunk(b"XYZa", b"1234") + sound[33:]
    apng = sound[:33] + chunk(b"acTL", struct.pack(">II", 1, 0)) + sound[33:]
    return [("palette", palette, "palette"), ("16bit", deep, "16-bit"), ("grey_alpha", grey_alpha, "grey + alpha"),
            ("interlaced", _patch_ihdr(sound, 12, 1), "Adam7"), ("bad_crc", bytes(bad_crc), "CRC"),
            ("truncated", sound[:len(sound) * 6 // 10], "truncated"), ("unknown_critical", unknown, "critical"), ("apng", apng, "APNG"),
            ("not_png", b"\xff\xd8\xff\xe0" + sound[4:], "signature"), ("empty", b"", "empty")]


@functools.lru_cache(maxsize=None)
def damaged():
    """(sound file, its RGB frame, a copy with 96 bytes of its IDAT payload overwritten and the chunk's CRC recomputed, a copy with one
    byte of the Adler-32 flipped): the planner accepts all three."""
    frame = photo()[100:133, 200:265]
    sound = pil_file(frame, compress_level=6)
    stream, spans = idat_payload(sound)
    assert len(spans) == 1 and len(stream) > 400
    rng = np.random.RandomState(77)
    hurt = bytearray(stream)
    hurt[200:296] = rng.randint(0, 256, size=96).astype(np.uint8).tobytes()
    flipped = bytearray(stream)
    flipped[-2] ^= 0x10
    return sound, pil_rgb(sound), png_file(65, 33, 3, [bytes(hurt)]), png_file(65, 33, 3, [bytes(flipped)])
