"""A CPU restatement of the device PNG encoder's ``huffman`` mode (faster_rcnn_amd/csrc/png.hip, include/ext/frcnn_hip_png_huff.h):
plain numpy / Python, integer arithmetic only.  ``encode(frame)`` builds the whole file; the kernel is held to it byte for byte
(tests/test_png_huff_gpu.py), and zlib.decompress and PIL are its own arbiters (tests/test_png_huff_cpu.py).

The stream, rule by rule:
  filter   per row the type in 0..4 (None, Sub, Up, Average, Paeth) with the smallest sum of |filtered byte as int8|, the lowest type on a
           tie; row 0 sees a zero prior row; filters read the raw previous row.
  bands    BAND_ROWS rows each (the last may be shorter), one IDAT chunk per band; band 0's data starts with the zlib header 78 01.
  tokens   the band's filtered bytes are walked in tiles of TILE bytes.  Inside a tile a byte equal to its predecessor continues a run
           (never the tile's first byte); a maximal run of L continuing bytes is cut into pieces of 258 from its start, a piece of 3 or
           more is one match (length, distance 1), a shorter last piece is literals.  Every other byte is a literal.
  codes    literal/length counts (symbol 256 once) -> Huffman code lengths limited to 15 bits (``code_lengths``); the distance alphabet
           is code 0 alone, length 1, in every band; the header spells the 257..286 + 1 lengths out one by one (no symbols 16-18) with
           a code-length code limited to 7 bits, built by the same routine.
  block    BFINAL = 0, BTYPE = 10, the header, the tokens, end-of-block, then the sync flush (000, pad to a byte, 00 00 FF FF).  A band
           whose dynamic form is not strictly shorter than its stored form (5 bytes per 65535) is emitted as stored blocks.
  closing  an IDAT with the final empty stored block 01 00 00 FF FF and the Adler-32 of the filtered stream, then IEND.
"""
import struct
import zlib

import numpy as np

BAND_ROWS = 8           # frcnn_png_huff_band_rows()
TILE = 4096             # png.hip PNG_TILE
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def filter_rows(rgb):
    """rgb (h, w, 3) uint8 -> (filtered (h, 1 + 3w) uint8, types [h])."""
    h, w = rgb.shape[:2]
    x = rgb.reshape(h, 3 * w).astype(np.int32)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, 3:] = x[:-1, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cands = np.stack([x, x - a, x - b, x - (a + b) // 2, x - paeth]) & 255             # [5][h][3w]
    cost = np.where(cands < 128, cands, 256 - cands).astype(np.int64).sum(axis=2)     # [5][h]
    types = np.argmin(cost, axis=0)                                                    # (the first minimum: the lowest type)
    out = np.empty((h, 1 + 3 * w), np.uint8)
    out[:, 0] = types
    out[:, 1:] = cands[types, np.arange(h)]
    return out, [int(t) for t in types]


def tokens(band):
    """The band's filtered bytes -> [("lit", byte) | ("match", length)]."""
    out = []
    for t0 in range(0, len(band), TILE):
        tile = band[t0:t0 + TILE]
        i = 0
        while i < len(tile):
            out.append(("lit", int(tile[i])))
            e = i + 1
            while e < len(tile) and tile[e] == tile[i]:
                e += 1
            run = e - i - 1                     # bytes that continue
            while run >= 3:
                n = min(run, 258)
                out.append(("match", n))
                run -= n
            out.extend([("lit", int(tile[i]))] * run)
            i = e
    return out


def length_symbol(n):
    """match length 3..258 -> (symbol, extra bits, extra value)."""
    if n == 258:
        return 285, 0, 0
    m = n - 3
    if m < 8:
        return 257 + m, 0, 0
    eb = m.bit_length() - 3
    return 257 + 4 * eb + 4 + ((m >> eb) & 3), eb, m & ((1 << eb) - 1)


def tree_depths(freq):
    """Huffman depths without a limit, as {symbol: depth} over the symbols with a count.  Leaves sorted by (count, symbol); two queues
    (leaves, inner nodes in the order they were made); of a leaf and an inner node of equal weight the leaf is taken first."""
    order = sorted((f, s) for s, f in enumerate(freq) if f)
    m = len(order)
    assert m >= 2
    w = [f for f, _ in order]
    iw, pl, pi = [], [0] * m, [0] * (m - 1)
    li = ii = 0
    for k in range(m - 1):
        total = 0
        for _ in range(2):
            if li < m and (ii >= k or w[li] <= iw[ii]):
                pl[li] = k
                total += w[li]
                li += 1
            else:
                pi[ii] = k
                total += iw[ii]
                ii += 1
        iw.append(total)
    depth = [0] * (m - 1)
    for k in range(m - 3, -1, -1):
        depth[k] = depth[pi[k]] + 1
    return {s: depth[pl[i]] + 1 for i, (_, s) in enumerate(order)}


def code_lengths(freq, maxbits):
    """Code lengths [len(freq)] of a complete prefix code, none above ``maxbits``.  The tree's leaf depths are clamped to ``maxbits``
    and counted per length; for every unit (2^-maxbits) the Kraft sum then stands above 1, one leaf of the longest length below
    ``maxbits`` that has any moves one level down and takes a leaf of length ``maxbits`` up beside it (count[b] -= 1,
    count[b + 1] += 2, count[maxbits] -= 1).  The counts are dealt out over the symbols sorted by (count, symbol): longest first."""
    depths = tree_depths(freq)
    count = [0] * (maxbits + 1)
    for d in depths.values():
        count[min(d, maxbits)] += 1
    over = sum(c << (maxbits - l) for l, c in enumerate(count) if l) - (1 << maxbits)
    for _ in range(over):
        b = maxbits - 1
        while count[b] == 0:
            b -= 1
        count[b] -= 1
        count[b + 1] += 2
        count[maxbits] -= 1
    lengths = [0] * len(freq)
    order = sorted((f, s) for s, f in enumerate(freq) if f)
    l = maxbits
    for _, s in order:
        while count[l] == 0:
            l -= 1
        lengths[s] = l
        count[l] -= 1
    return lengths


def canonical(lengths):
    """RFC 1951 3.2.2: codes [len(lengths)] as integers, most significant bit first."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        out.append(nxt[l] if l else 0)
        nxt[l] += 1 if l else 0
    return out


class Bits:
    def __init__(self, head=b""):
        self.acc, self.n = int.from_bytes(head, "little"), 8 * len(head)

    def put(self, value, n):            # LSB first (header fields, extra bits)
        self.acc |= value << self.n
        self.n += n

    def put_code(self, code, n):        # Huffman codes: most significant bit first
        self.put(int(format(code, "0%db" % n)[::-1], 2) if n else 0, n)

    def flush(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def stored(band, head):
    out = bytearray(head)
    for k in range(0, len(band), 65535):
        part = band[k:k + 65535]
        out += struct.pack("<BHH", 0, len(part), len(part) ^ 0xFFFF) + bytes(part)
    return bytes(out)


def band_plan(band):
    """What the encoder derives from a band before it emits: its tokens, counts, both sets of code lengths, the header's size."""
    toks = tokens(band)
    freq = [0] * 286
    freq[256] = 1
    for kind, v in toks:
        freq[v if kind == "lit" else length_symbol(v)[0]] += 1
    lit_len = code_lengths(freq, 15)
    nlit = max(s for s in range(286) if lit_len[s]) + 1
    seq = lit_len[:nlit] + [1]                  # ... and the distance alphabet: code 0 alone
    cl_freq = [0] * 19
    for l in seq:
        cl_freq[l] += 1
    cl_len = code_lengths(cl_freq, 7)
    hclen = max(i for i, s in enumerate(CL_ORDER) if cl_len[s]) + 1
    return dict(tokens=toks, freq=freq, lit_len=lit_len, nlit=nlit, seq=seq, cl_freq=cl_freq, cl_len=cl_len, hclen=max(hclen, 4))


def deflate_band(band, first):
    """One band's IDAT data -> (bytes, "dynamic" | "stored")."""
    head = b"\x78\x01" if first else b""
    plan = band_plan(band)
    lit_len, cl_len = plan["lit_len"], plan["cl_len"]
    lit_code, cl_code = canonical(lit_len), canonical(cl_len)
    bits = Bits(head)
    bits.put(0, 1)
    bits.put(2, 2)
    bits.put(plan["nlit"] - 257, 5)
    bits.put(0, 5)
    bits.put(plan["hclen"] - 4, 4)
    for s in CL_ORDER[:plan["hclen"]]:
        bits.put(cl_len[s], 3)
    for l in plan["seq"]:
        bits.put_code(cl_code[l], cl_len[l])
    for kind, v in plan["tokens"]:
        if kind == "lit":
            bits.put_code(lit_code[v], lit_len[v])
        else:
            s, eb, ev = length_symbol(v)
            bits.put_code(lit_code[s], lit_len[s])
            bits.put(ev, eb)
            bits.put(0, 1)              # distance code 0
    bits.put_code(lit_code[256], lit_len[256])
    bits.put(0, 3)                      # the sync flush: an empty stored block
    dynamic = bits.flush() + b"\x00\x00\xff\xff"
    plain = stored(band, head)
    return (dynamic, "dynamic") if len(dynamic) < len(plain) else (plain, "stored")


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def encode(frame, bgr=False, band_rows=BAND_ROWS, info=None):
    """frame (h, w, 3) uint8, R,G,B per pixel (``bgr``: B,G,R) -> the file's bytes.  ``info`` (a dict) receives "types" (the row filters)
    and "forms" (per band "dynamic" or "stored")."""
    rgb = np.ascontiguousarray(frame[:, :, ::-1] if bgr else frame)
    h, w = rgb.shape[:2]
    filt, types = filter_rows(rgb)
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
    forms = []
    for r0 in range(0, h, band_rows):
        data, form = deflate_band(filt[r0:r0 + band_rows].reshape(-1), r0 == 0)
        forms.append(form)
        out += chunk(b"IDAT", data)
    out += chunk(b"IDAT", b"\x01\x00\x00\xff\xff" + struct.pack(">I", zlib.adler32(filt.tobytes())))
    if info is not None:
        info.update(types=types, forms=forms)
    return out + chunk(b"IEND", b"")
