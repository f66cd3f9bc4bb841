"""The files the full-format device PNG decoder's tests decode (faster_rcnn_amd/csrc/png_dec_full.hip,
include/ext/frcnn_hip_png_dec_full.h), all made at test time.  Pillow cannot write Adam7, so the generator carries its own small writer:
split the samples into passes, pack the rows, prefix a filter byte per row, compress with ``zlib`` and compute the CRCs.  A case is
(name, file bytes); what it decodes to is ``expected(name)``: the restatement (tests/png_full_ref.py), computed once and shared, which
tests/test_png_full_cpu.py holds to Pillow byte for byte on every case."""
import functools
import io
import struct
import zlib

import numpy as np
from PIL import Image

from tests import png_dec_cases as R1
from tests import png_full_ref as ref

PAIRS = [(0, 1), (0, 2), (0, 4), (0, 8), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]
BPP_PAIRS = {1: (0, 8), 2: (4, 8), 3: (2, 8), 4: (6, 8), 6: (2, 16), 8: (6, 16)}      # filter unit in bytes -> a pair that has it


def pack_rows(sub, depth):
    """(ph, pw, channels) integer samples -> the (ph, row bytes) uint8 rows of a pass (sub-byte samples MSB first, 16-bit big-endian)."""
    ph = sub.shape[0]
    flat = sub.reshape(ph, -1)
    if depth == 8:
        return flat.astype(np.uint8)
    if depth == 16:
        return np.ascontiguousarray(flat.astype(">u2")).view(np.uint8).reshape(ph, -1)
    bits = ((flat[:, :, None] >> np.arange(depth - 1, -1, -1)) & 1).astype(np.uint8).reshape(ph, -1)
    return np.packbits(bits, axis=1)


def filter_bytes(rows, bpp, types):
    """The filtered bytes of (ph, rb) uint8 rows: row r under filter type types[r], with a filter unit of ``bpp`` bytes."""
    ph, rb = rows.shape
    cur = rows.astype(np.int32)
    up = np.vstack([np.zeros((1, rb), np.int32), cur[:-1]])
    left = np.hstack([np.zeros((ph, bpp), np.int32), cur[:, :-bpp]])[:, :rb]
    upleft = np.hstack([np.zeros((ph, bpp), np.int32), up[:, :-bpp]])[:, :rb]
    p = left + up - upleft
    pa, pb, pc = abs(p - left), abs(p - up), abs(p - upleft)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
    pred = [np.zeros_like(cur), left, up, (left + up) >> 1, paeth]
    out = bytearray()
    for r in range(ph):
        out.append(types[r])
        out += ((cur[r] - pred[min(types[r], 4)][r]) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def filtered(samples, colour, depth, interlace=0, types=lambda k, r: 0):
    """The bytes a file's zlib stream inflates to; ``types(k, r)``: the filter type of row r of pass k (0..6; 0 without interlace)."""
    h, w, ch = samples.shape
    bpp = max(1, ch * depth // 8)
    out = b""
    if not interlace:
        return filter_bytes(pack_rows(samples, depth), bpp, [types(0, r) for r in range(h)])
    for k, (x0, y0, dx, dy) in enumerate(ref.ADAM7):
        sub = samples[y0::dy, x0::dx]
        if sub.shape[0] and sub.shape[1]:
            out += filter_bytes(pack_rows(sub, depth), bpp, [types(k, r) for r in range(sub.shape[0])])
    return out


def container(w, h, colour, depth, interlace, idats, palette=None, extra=b"", late=b""):
    ihdr = struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, interlace)
    plte = R1.chunk(b"PLTE", bytes(palette)) if palette is not None else b""
    return R1.SIGNATURE + R1.chunk(b"IHDR", ihdr) + plte + extra + b"".join(R1.chunk(b"IDAT", d) for d in idats) + late + R1.chunk(b"IEND", b"")


def written(samples, colour, depth, interlace=0, types=lambda k, r: 0, palette=None, extra=b"", late=b"", level=6):
    h, w, _ = samples.shape
    return container(w, h, colour, depth, interlace, [R1.deflate(filtered(samples, colour, depth, interlace, types), level=level)], palette, extra, late)


def samples(h, w, colour, depth, seed, top=None):
    rng = np.random.RandomState(seed)
    return rng.randint(0, top if top is not None else 1 << depth, size=(h, w, ref.CHANNELS[colour])).astype(np.int64)


def palette_of(entries, seed):
    return np.random.RandomState(seed).randint(0, 256, size=3 * entries).astype(np.uint8).tobytes()


def mixed(k, r):
    return (k + r) % 5


@functools.lru_cache(maxsize=None)
def crop():
    return np.ascontiguousarray(R1.photo()[100:196, 200:328])            # 96 x 128


@functools.lru_cache(maxsize=None)
def sound_cases():
    """[(name, file)]: every supported file of the set but the 375x500 photograph (``photo_cases``) and revision 1's (``r1_cases``)."""
    cases = []

    def add(name, *a, **kw):
        cases.append((name, written(*a, **kw)))
    # ---- every supported (colour type, depth) pair, interlaced and not
    for colour, depth in PAIRS:
        for il in (0, 1):
            pal = palette_of(1 << depth, 40 + depth) if colour == 3 else None
            add("pair_c%d_d%d_i%d" % (colour, depth, il), samples(11, 13, colour, depth, 10 * colour + depth), colour, depth, il, mixed, pal)
    # ---- every filter type at every filter unit, on a first row and on later rows
    for bpp, (colour, depth) in BPP_PAIRS.items():
        for ft in range(5):
            for il in (0, 1):
                add("filter%d_bpp%d_i%d" % (ft, bpp, il), samples(5, 9, colour, depth, 7 * bpp + ft), colour, depth, il, lambda k, r, ft=ft: ft)
    # ---- sizes at the edges: 1x1, 1x8, 8x1; 3x5 (passes absent); 7x9, 9x7; 33x65
    for h, w in ((1, 1), (1, 8), (8, 1), (3, 5), (7, 9), (9, 7), (33, 65)):
        for il in (0, 1):
            add("size_%dx%d_rgb_i%d" % (h, w, il), samples(h, w, 2, 8, h * 100 + w), 2, 8, il, mixed)
            add("size_%dx%d_p4_i%d" % (h, w, il), samples(h, w, 3, 4, h * 100 + w + 1), 3, 4, il, mixed, palette_of(16, h + w))
    add("rows65_ga8", samples(65, 5, 4, 8, 65), 4, 8, 0, lambda k, r: 4 if r % 64 else 3)          # one row past a strip of 64
    add("rows131_rgb16_i1", samples(131, 3, 2, 16, 131), 2, 16, 1, lambda k, r: 4 if r % 64 else 2)   # pass 7 has 65 rows
    # ---- sub-byte widths that do not fill the last byte
    for depth, widths in ((1, (1, 7, 9, 13)), (2, (5,)), (4, (3,))):
        for w in widths:
            for il in (0, 1):
                add("sub_g%d_w%d_i%d" % (depth, w, il), samples(3, w, 0, depth, 3 * w + depth), 0, depth, il, mixed)
                add("sub_p%d_w%d_i%d" % (depth, w, il), samples(3, w, 3, depth, 5 * w + depth), 3, depth, il, mixed, palette_of(1 << depth, w))
    # ---- palettes: 1, 2, 16 and 256 entries; shorter than the indices used; with tRNS
    add("plte_1", samples(4, 6, 3, 8, 1, top=1), 3, 8, 0, mixed, palette_of(1, 1))
    add("plte_2", samples(4, 6, 3, 1, 2), 3, 1, 1, mixed, palette_of(2, 2))
    add("plte_16", samples(4, 6, 3, 4, 3), 3, 4, 0, mixed, palette_of(16, 3))
    add("plte_256", samples(16, 16, 3, 8, 4), 3, 8, 1, mixed, palette_of(256, 4))
    add("plte_short_d8", samples(6, 7, 3, 8, 5, top=10), 3, 8, 0, mixed, palette_of(5, 5))
    add("plte_short_d4_i1", samples(6, 7, 3, 4, 6), 3, 4, 1, mixed, palette_of(3, 6))
    add("plte_short_d1", samples(3, 9, 3, 1, 7), 3, 1, 0, mixed, palette_of(1, 7))
    add("trns_palette", samples(6, 7, 3, 4, 8), 3, 4, 0, mixed, palette_of(16, 8), extra=R1.chunk(b"tRNS", bytes([0, 128, 255])))
    add("trns_grey", samples(6, 7, 0, 8, 9), 0, 8, 1, mixed, extra=R1.chunk(b"tRNS", struct.pack(">H", 7)))
    add("trns_rgb16", samples(6, 7, 2, 16, 10), 2, 16, 0, mixed, extra=R1.chunk(b"tRNS", struct.pack(">HHH", 1, 2, 3)))
    # ---- 16-bit files with non-zero low bytes (random samples have them; this one is the documented vector)
    vector = np.array([[[0x1234, 0xABCD, 0xFF01]]], np.int64)
    add("deep_vector", vector, 2, 16)
    add("deep_ga16_i1", samples(9, 7, 4, 16, 11), 4, 16, 1, mixed)
    # ---- the photograph crop: Pillow's ADAPTIVE palette file, the same indices as Adam7, the crop as Adam7 RGB
    pimg = Image.fromarray(crop()).convert("P", palette=Image.ADAPTIVE)
    buf = io.BytesIO()
    pimg.save(buf, "PNG")
    cases.append(("crop_adaptive_pil", buf.getvalue()))
    add("crop_adaptive_i1", np.asarray(pimg).astype(np.int64)[:, :, None], 3, 8, 1, mixed, bytes(pimg.getpalette()[:768]))
    add("crop_rgb_i1", crop().astype(np.int64), 2, 8, 1, mixed)
    # ---- Adam7 at 2x2: four of the seven passes absent (1x1, where the first pass alone exists, is among the sizes above)
    add("size_2x2_rgb_i1", samples(2, 2, 2, 8, 202), 2, 8, 1, mixed)
    add("size_2x2_p1_i1", samples(2, 2, 3, 1, 203), 3, 1, 1, mixed, palette_of(2, 4))
    assert len({n for n, _ in cases}) == len(cases)
    return cases


@functools.lru_cache(maxsize=None)
def photo_cases():
    """The 375x500 golden photograph once, as Adam7 RGB."""
    return [("photo_rgb_i1", written(R1.photo().astype(np.int64), 2, 8, 1, lambda k, r: (1, 2, 4)[(k + r) % 3]))]


@functools.lru_cache(maxsize=None)
def r1_cases():
    """Every sound file of tests/png_dec_cases.py: the full planner accepts all that revision 1 accepts."""
    return [("r1_" + name, data) for name, data, _ in R1.sound_cases() + R1.photo_cases()]


def all_sound():
    return sound_cases() + photo_cases() + r1_cases()


@functools.lru_cache(maxsize=None)
def _by_name():
    return dict(all_sound())


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement's frame of a sound case (R,G,B), computed once; read-only."""
    out = ref.decode(_by_name()[name])
    out.setflags(write=False)
    return out


def case(name):
    return _by_name()[name]


@functools.lru_cache(maxsize=None)
def refusals():
    """[(name, file, a word of the full planner's reason)]."""
    pal, s4 = palette_of(16, 1), samples(5, 6, 3, 4, 1)
    stream = [R1.deflate(filtered(s4, 3, 4))]
    deep_grey = dict((n, d) for n, d, _ in R1.refusals())["16bit"]
    sound = written(samples(5, 6, 2, 8, 2), 2, 8)
    bad_crc = bytearray(sound)
    bad_crc[R1.idat_payload(sound)[1][0][0] + 5] ^= 0x40
    return [("grey16", deep_grey, "16-bit grey"),
            ("grey16_i1", written(samples(5, 6, 0, 16, 3), 0, 16, 1), "16-bit grey"),
            ("no_plte", container(6, 5, 3, 4, 0, stream), "without PLTE"),
            ("late_plte", container(6, 5, 3, 4, 0, stream, late=R1.chunk(b"PLTE", pal)), "behind an IDAT"),
            ("plte_length", container(6, 5, 3, 4, 0, stream, palette=pal[:7]), "a PLTE of 7 bytes"),
            ("plte_empty", container(6, 5, 3, 4, 0, stream, palette=b""), "a PLTE of 0 bytes"),
            ("plte_long", container(6, 5, 3, 4, 0, stream, palette=bytes(771)), "a PLTE of 771 bytes"),
            ("pair_rgb4", written(samples(5, 6, 2, 4, 4), 2, 4), "not a pair"),
            ("pair_palette16", written(samples(5, 6, 3, 16, 5), 3, 16, palette=pal), "not a pair"),
            ("pair_grey3", written(samples(5, 6, 0, 2, 6), 0, 3), "not a pair"),
            ("colour5", written(samples(5, 6, 0, 8, 7), 5, 8), "colour type 5"),
            ("interlace2", written(samples(5, 6, 2, 8, 8), 2, 8, 2), "interlace method 2"),
            ("bad_crc", bytes(bad_crc), "CRC"),
            ("truncated", sound[:len(sound) * 6 // 10], "truncated")] + \
        [(n, d, word) for n, d, word in R1.refusals() if n in ("unknown_critical", "apng", "not_png", "empty")]


@functools.lru_cache(maxsize=None)
def damaged():
    """(name of the sound case they were made of, {kind: file}): an Adam7 RGB file of the photograph crop with 96 bytes of its IDAT
    payload overwritten (the chunk's CRC recomputed), with one byte of its Adler-32 flipped, and with a filter byte of 5 on the second row
    of pass 4 (a sound zlib stream: only the reconstruction can object).  The planner accepts all three."""
    frame = crop()[:33, :65].astype(np.int64)
    stream = R1.deflate(filtered(frame, 2, 8, 1, mixed))
    assert len(stream) > 400
    hurt = bytearray(stream)
    hurt[200:296] = np.random.RandomState(77).randint(0, 256, size=96).astype(np.uint8).tobytes()
    flipped = bytearray(stream)
    flipped[-2] ^= 0x10
    five = R1.deflate(filtered(frame, 2, 8, 1, lambda k, r: 5 if (k, r) == (3, 1) else mixed(k, r)))
    return {kind: container(65, 33, 2, 8, 1, [bytes(s)]) for kind, s in (("sound", stream), ("payload", hurt), ("adler", flipped), ("filter5", five))}
