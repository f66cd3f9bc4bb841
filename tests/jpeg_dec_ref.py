"""A CPU restatement of the device JPEG decoder (faster_rcnn_amd/csrc/jpeg_dec.hip, include/ext/frcnn_hip_jpeg_dec.h) and the definition
the kernels are held to byte for byte: ``decode(file)`` is the (h, w, 3) uint8 R,G,B frame.  Integer arithmetic only.  The pixels are
those of libjpeg-turbo's default decoder (ISLOW IDCT, fancy upsampling), which Pillow uses: tests/test_jpeg_dec_cpu.py holds this file
to ``np.asarray(Image.open(f).convert("RGB"))``.

The supported set (``plan`` raises ``Unsupported`` with the reason for everything else, from the headers alone): SOF0, 8 bits, one scan
holding all components; 1 component, or 3 components Y Cb Cr (JFIF, or an Adobe marker with transform 1, or neither and component ids
other than 'R' 'G' 'B'); luma sampled 1x1, 2x1 or 2x2 with chroma 1x1; DQT with 8-bit entries, any DHT with table ids 0..1; with or
without DRI; sides in 1..65535.

  plan      the marker parse.  The entropy-coded segment runs from behind the SOS header to the first 0xFF that is followed by anything
            but 0x00 or RST0..RST7 (so no other marker lies inside it: "any other marker ends the scan"), or to the end of the file.
            S = max(32, ceil(len / 1024) rounded up to a multiple of 4) raw bytes per subsequence, N = max(1, ceil(len / S)) <= 1024.
  reader    a position is a bit of the RAW segment.  ``window(p)``: five data bytes from byte p >> 3 on; behind a 0xFF byte a 0x00 is
            skipped; bytes past the segment read as zero; 0xFF followed by RSTm is a marker: it and everything behind it read as zero
            and the window remembers the bit at which it stands.  A symbol that needs bits at or past the marker is abandoned and the
            state becomes (byte behind the marker, block 0, zigzag 0, restart pending); one that ends in front of it is kept.  A symbol
            that needs bits past the end of the segment (the padding behind the last block starts one) is abandoned too and ends the
            walk: the position becomes the segment's end, nothing is flagged.
  symbol    a Huffman code (a code not in the table: 16 bits, symbol 0, STATUS_CODE), then its value bits: DC: category = symbol & 15
            (a symbol above 11: STATUS_TABLE), AC: run = symbol >> 4, size = symbol & 15 (above 10: STATUS_TABLE); 0x00 ends the block,
            0xF0 skips 16.  A coefficient whose zigzag index would pass 63 is dropped and ends the block (STATUS_ZIGZAG in the final walk).
  state     (bit position, block within the MCU, zigzag index, restart pending: set by a marker, cleared when the MCU behind it is
            complete; the first block of every component in that MCU is flagged "restart").  ``F(i, state)`` decodes whole symbols until the next
            would start at or past the end of subsequence i (or of the segment) and returns the exit state and the blocks completed.
  serial    one call of F over the whole segment (T.81 F.2.2).  parallel: entry[0] = (0, 0, 0), entry[i] guessed as the first bit of
            subsequence i; rounds of exit[i] = F(i, entry[i]) for every i whose entry changed, entry[i + 1] = exit[i], until nothing
            changes: at most N rounds.  An exclusive scan of the block counts, then a last walk that writes the coefficients (natural
            order, int16, DC as differences, zeros where the stream skips) and a restart flag per block.
  DC        per component a prefix sum of the differences, cut at the restart flags (int16 wrap).
  IDCT      dequantise, jidctint's ISLOW (CONST_BITS 13, PASS1_BITS 2, columns descaled by 11, rows by 18), + 128, clamp.
  upsample  libjpeg's "fancy" h2v1 / h2v2 triangle filters as the issue of this decoder states them; a chroma plane of width <= 2
            is replicated instead (libjpeg-turbo takes its plain upsampler there, both ways for h2v2).
  colour    16 fractional bits, FIX(x) = int(x * 65536 + 0.5); a single component is replicated.
"""
import numpy as np

STATUS_BLOCKS, STATUS_ZIGZAG, STATUS_CODE, STATUS_TABLE = 1, 2, 4, 8
MAX_LANES, MIN_S = 1024, 32
MAX_SCAN = 1 << 24                    # FRCNN_JPEG_DEC_MAX_SCAN: bounds the entropy kernel's worst case (the header says how)
LOOK = 9                              # bits of the lookahead table


class Unsupported(Exception):
    pass


def zigzag():
    order = []
    for d in range(15):
        cells = [(d - u, u) for u in range(8) if 0 <= d - u < 8]
        order += cells[::-1] if d % 2 else cells
    return [8 * v + u for v, u in order]


ZIGZAG = zigzag()


class Plan:
    """What frcnn_jpeg_dec_plan_t holds."""

    def __init__(self):
        self.h = self.w = self.ncomp = self.hs = self.vs = 0
        self.mcus_x = self.mcus_y = self.bpm = 0
        self.expected_blocks = self.restart_interval = 0
        self.scan_off = self.scan_len = self.file_len = 0
        self.dqt_off = [0, 0, 0]           # per component: offset of its 64 table bytes (zigzag order)
        self.dht_off = [[0, 0], [0, 0]]    # [class][id]: offset of BITS (16 bytes), HUFFVAL behind them
        self.dht_n = [[0, 0], [0, 0]]      # symbols
        self.comp_dc = [0, 0, 0]
        self.comp_ac = [0, 0, 0]
        self.S = self.N = 0


def subsequences(scan_len, min_s=MIN_S):
    s = max(min_s, (-(-scan_len // MAX_LANES) + 3) // 4 * 4)
    return s, max(1, -(-scan_len // s))


def plan(data, min_s=MIN_S):
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise Unsupported("not a JPEG file (no SOI)" if n else "empty file")
    p = Plan()
    p.file_len = n
    dqt, dht, sof, jfif, adobe, pos = {}, {}, None, False, None, 2
    while True:
        if pos + 4 > n:
            raise Unsupported("truncated: the headers end at byte %d before SOS" % pos)
        if data[pos] != 0xFF:
            raise Unsupported("no marker at byte %d" % pos)
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            pos += 2
            continue
        if m == 0xD9:
            raise Unsupported("EOI before SOS")
        seg = (data[pos + 2] << 8) | data[pos + 3]
        if seg < 2 or pos + 2 + seg > n:
            raise Unsupported("truncated: segment 0x%02X at byte %d runs past the file" % (m, pos))
        a, e = pos + 4, pos + 2 + seg
        if m == 0xC0:
            if sof is not None:
                raise Unsupported("two frame headers")
            if e - a < 6 or e - a != 6 + 3 * data[a + 5]:
                raise Unsupported("malformed SOF0")
            if data[a] != 8:
                raise Unsupported("%d-bit samples" % data[a])
            sof = (a, data[a + 5])
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise Unsupported({0xC2: "progressive", 0xC1: "extended sequential", 0xC9: "arithmetic coding"}.get(m, "frame type 0x%02X" % m))
        elif m == 0xCC:
            raise Unsupported("arithmetic coding")
        elif m == 0xDB:
            q = a
            while q < e:
                if data[q] >> 4:
                    raise Unsupported("16-bit DQT")
                if (data[q] & 15) > 3 or q + 65 > e:
                    raise Unsupported("malformed DQT")
                dqt[data[q] & 15] = q + 1
                q += 65
        elif m == 0xC4:
            q = a
            while q < e:
                if q + 17 > e:
                    raise Unsupported("malformed DHT")
                tc, th = data[q] >> 4, data[q] & 15
                bits = data[q + 1:q + 17]
                cnt = sum(bits)
                if tc > 1 or th > 1:
                    raise Unsupported("Huffman table class %d id %d outside baseline" % (tc, th))
                if cnt > 256 or q + 17 + cnt > e:
                    raise Unsupported("malformed DHT")
                code = 0
                for length in range(1, 17):
                    code += bits[length - 1]
                    if code > 1 << length:
                        raise Unsupported("malformed DHT: codes overflow length %d" % length)
                    code <<= 1
                dht[(tc, th)] = (q + 1, cnt)
                q += 17 + cnt
        elif m == 0xDD:
            if seg != 4:
                raise Unsupported("malformed DRI")
            p.restart_interval = (data[a] << 8) | data[a + 1]
        elif m == 0xE0 and e - a >= 5 and data[a:a + 5] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and e - a >= 12 and data[a:a + 5] == b"Adobe":
            adobe = data[a + 11]
        elif m == 0xDA:
            break
        pos = e
    if sof is None:
        raise Unsupported("SOS before a frame header")
    a, nc = sof
    p.h, p.w, p.ncomp = (data[a + 1] << 8) | data[a + 2], (data[a + 3] << 8) | data[a + 4], nc
    if p.h < 1 or p.w < 1:
        raise Unsupported("frame %dx%d: both sides must be at least 1" % (p.h, p.w))
    if nc not in (1, 3):
        raise Unsupported("%d components (CMYK / YCCK)" % nc if nc == 4 else "%d components" % nc)
    comps = [(data[a + 6 + 3 * c], data[a + 7 + 3 * c] >> 4, data[a + 7 + 3 * c] & 15, data[a + 8 + 3 * c]) for c in range(nc)]
    if nc == 3:
        if not jfif:
            if adobe is not None and adobe != 1:
                raise Unsupported("Adobe transform %d (not Y Cb Cr)" % adobe)
            if adobe is None and [c[0] for c in comps] == [82, 71, 66]:
                raise Unsupported("component ids R G B (not Y Cb Cr)")
        samp = (comps[0][1], comps[0][2])
        if samp not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            raise Unsupported("sampling factors " + ",".join("%dx%d" % (c[1], c[2]) for c in comps))
        p.hs, p.vs = samp
    else:
        p.hs = p.vs = 1                   # (a single component is coded block by block whatever its factors say)
    a, e = pos + 4, pos + 2 + ((data[pos + 2] << 8) | data[pos + 3])
    if e - a < 1:
        raise Unsupported("malformed SOS")
    if e - a != 4 + 2 * data[a] or data[a] != nc:
        raise Unsupported("a scan of %d of the %d components (multiple scans)" % (data[a], nc))
    for c in range(nc):
        if data[a + 1 + 2 * c] != comps[c][0]:
            raise Unsupported("scan components out of frame order")
        td, ta = data[a + 2 + 2 * c] >> 4, data[a + 2 + 2 * c] & 15
        if td > 1 or ta > 1 or (0, td) not in dht or (1, ta) not in dht:
            raise Unsupported("component %d names a Huffman table that is not defined" % c)
        if comps[c][3] not in dqt:
            raise Unsupported("component %d names a quantisation table that is not defined" % c)
        p.comp_dc[c], p.comp_ac[c], p.dqt_off[c] = td, ta, dqt[comps[c][3]]
    if (data[e - 3], data[e - 2], data[e - 1]) != (0, 63, 0):
        raise Unsupported("spectral selection / successive approximation in a baseline scan")
    for (tc, th), (off, cnt) in dht.items():
        p.dht_off[tc][th], p.dht_n[tc][th] = off, cnt
    p.scan_off = e
    q = e
    while q < n:
        if data[q] == 0xFF and q + 1 < n and data[q + 1] != 0 and not 0xD0 <= data[q + 1] <= 0xD7:
            break
        q += 1
    if q == e:
        raise Unsupported("truncated: no entropy-coded data behind SOS")
    p.scan_len = q - e
    if p.scan_len >= MAX_SCAN:
        raise Unsupported("entropy-coded segment of %d bytes" % p.scan_len)
    p.mcus_x, p.mcus_y = -(-p.w // (8 * p.hs)), -(-p.h // (8 * p.vs))
    p.bpm = p.hs * p.vs + 2 if nc == 3 else 1
    p.expected_blocks = p.mcus_x * p.mcus_y * p.bpm
    p.S, p.N = subsequences(p.scan_len, min_s)
    return p


# ------------------------------------------------------------------------------------------------------------------ entropy decode
class Huff:
    """Annex F.2.2.3: mincode / maxcode / valptr per length."""

    def __init__(self, data, off, n):
        self.bits = list(data[off:off + 16])
        self.vals = list(data[off + 16:off + 16 + n])
        self.maxcode, self.delta = [-1] * 17, [0] * 17
        code = k = 0
        for length in range(1, 17):
            if self.bits[length - 1]:
                self.delta[length] = k - code            # symbol index = code + delta
                code += self.bits[length - 1]
                k += self.bits[length - 1]
                self.maxcode[length] = code - 1
            code <<= 1

        # the kernel's shape: a lookahead table over LOOK bits, length << 8 | symbol, 0 for the longer codes
        self.look = [0] * (1 << LOOK)
        for length in range(1, LOOK + 1):
            for c in range(self.maxcode[length] - self.bits[length - 1] + 1, self.maxcode[length] + 1):
                k = c + self.delta[length]
                if 0 <= k < len(self.vals):
                    at = c << (LOOK - length)
                    self.look[at:at + (1 << (LOOK - length))] = [length << 8 | self.vals[k]] * (1 << (LOOK - length))

    def lookup(self, top16):
        """-> (length, symbol, status) of the code at the top of a 16-bit window."""
        e = self.look[top16 >> (16 - LOOK)]
        if e:
            return e >> 8, e & 255, 0
        for length in range(1, 17):
            c = top16 >> (16 - length)
            if c <= self.maxcode[length]:
                k = c + self.delta[length]
                if not 0 <= k < len(self.vals):
                    return length, 0, STATUS_TABLE
                return length, self.vals[k], 0
        return 16, 0, STATUS_CODE


class Entropy:
    def __init__(self, data, p):
        self.p = p
        self.scan = bytes(data[p.scan_off:p.scan_off + p.scan_len])
        self.L = p.scan_len
        self.dc = [Huff(data, p.dht_off[0][t], p.dht_n[0][t]) if p.dht_off[0][t] else None for t in range(2)]
        self.ac = [Huff(data, p.dht_off[1][t], p.dht_n[1][t]) if p.dht_off[1][t] else None for t in range(2)]
        self.luma = luma = p.hs * p.vs if p.ncomp == 3 else 1
        self.comp_of = [0] * luma + ([1, 2] if p.ncomp == 3 else [])
        self.coef = None
        self.flags = None
        self.status = 0

    def window(self, pos):
        """-> (40 bits from byte pos >> 3, raw index of each of the 5 data bytes, bit of the window at which an RSTm marker stands or
        None, the marker's raw index, the bit of the window at which the segment ends or None)."""
        scan, L = self.scan, self.L
        r = pos >> 3
        five = scan[r:r + 5]
        if len(five) == 5 and 0xFF not in five:             # the common case of the loop below
            return int.from_bytes(five, "big"), (r, r + 1, r + 2, r + 3, r + 4), None, 0, None
        w, idx, mbit, mraw, ebit = 0, [], None, 0, None
        for j in range(5):
            idx.append(r)
            if r >= L and ebit is None and mbit is None:
                ebit = 8 * j
            b = scan[r] if r < L else 0
            if mbit is not None:
                b = 0
            elif b == 0xFF:
                nxt = scan[r + 1] if r + 1 < L else 0
                if nxt == 0:
                    r += 1
                elif 0xD0 <= nxt <= 0xD7:
                    mbit, mraw, b = 8 * j, r, 0
            w = (w << 8) | b
            if mbit is None:
                r += 1
        return w, idx, mbit, mraw, ebit

    def run(self, i, state, first_block=None):
        """F_i.  With ``first_block`` (the index of the block the entry state stands in) it is the final walk and writes."""
        pos, b, z, rst = state
        p = self.p
        end = min((i + 1) * p.S, self.L) * 8 if i is not None else self.L * 8
        write, blk, done = first_block is not None, first_block or 0, 0
        coef, flags, nblk = self.coef, self.flags, p.expected_blocks
        while pos < end:
            w, idx, mbit, mraw, ebit = self.window(pos)
            o = pos & 7
            c = self.comp_of[b]
            table = self.dc[p.comp_dc[c]] if z == 0 else self.ac[p.comp_ac[c]]
            length, sym, st = table.lookup((w >> (24 - o)) & 0xFFFF)
            size = sym & 15
            if (z == 0 and sym > 11) or (z > 0 and size > 10):
                st |= STATUS_TABLE
            n = length + size
            if mbit is not None and o + n > mbit:          # the symbol reaches into a restart marker: abandoned
                if z > 0:
                    if write and blk < nblk:
                        coef[blk, [ZIGZAG[k] for k in range(z, 64)]] = 0
                    blk, done = blk + 1, done + 1
                pos, b, z, rst = (mraw + 2) * 8, 0, 0, 1
                continue
            if ebit is not None and o + n > ebit:           # ... past the end of the segment (the last padding): abandoned, the end
                pos = max(pos, self.L * 8)
                break
            if write:
                self.status |= st
            v = (w >> (40 - o - n)) & ((1 << size) - 1) if size else 0
            if size and v < 1 << (size - 1):
                v -= (1 << size) - 1
            if z == 0:
                if write and blk < nblk:
                    coef[blk, 0], flags[blk] = v, rst if b == 0 or b >= self.luma else 0
                z = 1
            else:
                run, keep = sym >> 4, 1
                if size == 0:                               # ZRL; EOB (and the undefined run << 4 | 0 symbols)
                    run, keep = 16 if run == 15 else 64 - z, 0
                if z + run + keep > 64:                     # past 63: the rest of the block is zero
                    if write:
                        self.status |= STATUS_ZIGZAG
                    run, keep = 64 - z, 0
                if write and blk < nblk:
                    for k in range(z, z + run):
                        coef[blk, ZIGZAG[k]] = 0
                    if keep:
                        coef[blk, ZIGZAG[z + run]] = v
                z += run + keep
            if z >= 64:
                blk, done, z = blk + 1, done + 1, 0
                b = b + 1 if b + 1 < p.bpm else 0
                rst = rst if b else 0
            q = o + n
            pos = idx[q >> 3] * 8 + (q & 7)
        return (pos, b, z, rst), done

    def begin(self):
        self.coef = np.zeros((self.p.expected_blocks, 64), np.int16)
        self.coef[:] = 0x5A5A                                # every coefficient of every decoded block is written by the walk
        self.flags = np.zeros(self.p.expected_blocks, np.uint8)
        self.status = 0

    def finish(self, total):
        if total != self.p.expected_blocks:
            self.status |= STATUS_BLOCKS
            self.coef[min(total, self.p.expected_blocks):] = 0      # (the device leaves them as they were; nobody reads a failed frame)
        return self.coef, self.flags, total, self.status

    def serial(self):
        self.begin()
        _, total = self.run(None, (0, 0, 0, 0), first_block=0)
        return self.finish(total)

    def parallel(self, info=None):
        p = self.p
        N, S = p.N, p.S
        entry = [(i * S * 8, 0, 0, 0) for i in range(N)]
        exit_, count, changed, rounds = [None] * N, [0] * N, [True] * N, 0
        while any(changed):
            assert rounds < N, "the fixed point takes at most N rounds"
            rounds += 1
            for i in range(N):
                if changed[i]:
                    exit_[i], count[i] = self.run(i, entry[i])
            changed = [False] * N
            for i in range(1, N):
                if entry[i] != exit_[i - 1]:
                    entry[i], changed[i] = exit_[i - 1], True
        first = np.concatenate([[0], np.cumsum(count)])
        self.begin()
        for i in range(N):
            out, done = self.run(i, entry[i], first_block=int(first[i]))
            assert out == exit_[i] and done == count[i]
        if info is not None:
            info.update(rounds=rounds, N=N, S=S)
        return self.finish(int(first[N]))


def dc_prefix(p, coef, flags):
    """DC differences -> values, per component, cut at the restart flags; int16 wrap."""
    nb = p.expected_blocks
    if p.ncomp == 1:
        comp = np.zeros(nb, np.int64)
    else:
        luma = p.hs * p.vs
        comp = np.maximum(np.arange(nb) % p.bpm - luma + 1, 0)
    out = coef.copy()
    for c in range(p.ncomp):
        at = np.nonzero(comp == c)[0]
        d = coef[at, 0].astype(np.int64)
        f = flags[at].astype(bool)
        f[:1] = True
        total = np.cumsum(d)
        start = np.maximum.accumulate(np.where(f, np.arange(len(at)), 0))
        base = total[start] - d[start]
        out[at, 0] = (total - base).astype(np.int64).astype(np.int16)
    return out


# ----------------------------------------------------------------------------------------------------------------------- pixels
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def idct_1d(x, shift):
    """jidctint's 8-point pass over the last axis of ``x`` (int64), descaled by ``shift``."""
    x0, x1, x2, x3, x4, x5, x6, x7 = [x[..., k] for k in range(8)]
    z1 = (x2 + x6) * F_0_541
    tmp2 = z1 - x6 * F_1_847
    tmp3 = z1 + x2 * F_0_765
    tmp0 = (x0 + x4) << 13
    tmp1 = (x0 - x4) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = x7, x5, x3, x1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F_1_175
    t0, t1, t2, t3 = t0 * F_0_298, t1 * F_2_053, t2 * F_3_072, t3 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = np.stack([tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3], -1)
    return (out + (1 << (shift - 1))) >> shift


def idct_blocks(coef, q_nat):
    """[n][64] coefficients (natural order) x [64] table -> [n][8][8] uint8 samples."""
    x = (coef.astype(np.int64) * q_nat[None]).reshape(-1, 8, 8)
    ws = idct_1d(x.transpose(0, 2, 1), 11).transpose(0, 2, 1)        # columns
    out = idct_1d(ws, 18)                                            # rows
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def planes(data, p, coef):
    """Component planes at padded size."""
    nm = p.mcus_x * p.mcus_y
    out = []
    blocks = coef.reshape(nm, p.bpm, 64)
    luma = p.hs * p.vs if p.ncomp == 3 else 1
    for c in range(p.ncomp):
        q = np.zeros(64, np.int64)
        q[ZIGZAG] = np.frombuffer(data[p.dqt_off[c]:p.dqt_off[c] + 64], np.uint8)
        if c == 0:
            px = idct_blocks(blocks[:, :luma].reshape(-1, 64), q).reshape(p.mcus_y, p.mcus_x, p.vs, p.hs, 8, 8)
            out.append(px.transpose(0, 2, 4, 1, 3, 5).reshape(p.mcus_y * p.vs * 8, p.mcus_x * p.hs * 8))
        else:
            px = idct_blocks(blocks[:, luma + c - 1], q).reshape(p.mcus_y, p.mcus_x, 8, 8)
            out.append(px.transpose(0, 2, 1, 3).reshape(p.mcus_y * 8, p.mcus_x * 8))
    return out


def upsample_h(s, n):
    """[rows][n] (int64; samples, or 3 near + far sums) -> [rows][2n] before the final shift: (3 s[i] + s[i -+ 1])."""
    left = np.concatenate([s[:, :1], s[:, :-1]], 1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
    return 3 * s + left, 3 * s + right


def upsample(plane, p):
    """A chroma plane (padded) -> [h][w] int64 at full size."""
    h, w = p.h, p.w
    if p.hs == 1:
        return plane[:h, :w].astype(np.int64)
    n = -(-w // 2)
    if p.vs == 1:
        s = plane[:h, :n].astype(np.int64)
        if n <= 2:
            return np.repeat(s, 2, 1)[:, :w]
        even, odd = upsample_h(s, n)
        even, odd = (even + 1) >> 2, (odd + 2) >> 2
        even[:, 0], odd[:, -1] = s[:, 0], s[:, -1]
        return np.stack([even, odd], 2).reshape(h, 2 * n)[:, :w]
    rows = -(-h // 2)
    s = plane[:rows, :n].astype(np.int64)
    if n <= 2:
        return np.repeat(np.repeat(s, 2, 0), 2, 1)[:h, :w]
    above = np.concatenate([s[:1], s[:-1]], 0)
    below = np.concatenate([s[1:], s[-1:]], 0)
    cs = np.stack([3 * s + above, 3 * s + below], 1).reshape(2 * rows, n)
    even, odd = upsample_h(cs, n)
    even, odd = (even + 8) >> 4, (odd + 7) >> 4
    even[:, 0], odd[:, -1] = (4 * cs[:, 0] + 8) >> 4, (4 * cs[:, -1] + 7) >> 4
    return np.stack([even, odd], 2).reshape(2 * rows, 2 * n)[:h, :w]


def fix(x):
    return int(x * 65536 + 0.5)


def colour(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    r = y + ((fix(1.40200) * cr + 32768) >> 16)
    b = y + ((fix(1.77200) * cb + 32768) >> 16)
    g = y + ((-fix(0.34414) * cb + 32768 - fix(0.71414) * cr) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def pixels(data, p, coef, bgr=False):
    pl = planes(data, p, coef)
    y = pl[0][:p.h, :p.w].astype(np.int64)
    if p.ncomp == 1:
        return np.repeat(y[:, :, None], 3, 2).astype(np.uint8)
    rgb = colour(y, upsample(pl[1], p), upsample(pl[2], p))
    return np.ascontiguousarray(rgb[:, :, ::-1]) if bgr else rgb


def coefficients(data, p=None, form="serial", info=None):
    """-> (coef int16 [blocks][64] natural order with DC values, block total, status)."""
    data = bytes(data)
    p = p or plan(data)
    e = Entropy(data, p)
    coef, flags, total, status = e.serial() if form == "serial" else e.parallel(info)
    return dc_prefix(p, coef, flags), total, status


def decode(data, bgr=False, form="serial", info=None):
    """The (h, w, 3) uint8 frame of a supported file; ``info`` (a dict) receives "status", "blocks", and from the parallel form
    "rounds", "N", "S"."""
    data = bytes(data)
    p = plan(data)
    coef, total, status = coefficients(data, p, form, info)
    if info is not None:
        info.update(status=status, blocks=total)
    return pixels(data, p, coef, bgr)
