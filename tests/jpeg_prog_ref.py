"""A CPU restatement of the device decoder for PROGRESSIVE JPEG files (faster_rcnn_amd/csrc/jpeg_dec_full.hip,
include/ext/frcnn_hip_jpeg_dec_full.h): ``plan(file)`` is the planner, field for field what frcnn_jpeg_dec_full_plan fills, and
``decode(file)`` the (h, w, 3) uint8 R,G,B frame.  The four scan decoders are serial and written for clarity (T.81 annex G, as
libjpeg's jdphuff.c walks them); the back half (IDCT, upsampling, colour) is tests/jpeg_dec_ref.py's.  tests/test_jpeg_prog_cpu.py holds
this file to ``np.asarray(Image.open(f).convert("RGB"))``.

  script    a DC scan has Ss = Se = 0 and may interleave components; an AC scan has 1 <= Ss <= Se <= 63 and one component; the first
            scan of a coefficient has Ah = 0, each later one Ah = the previous Al and Al = Ah - 1; no AC scan of a component before its
            DC scan; at the end every coefficient of every component stands at Al = 0.  Everything else raises ``Unsupported``.
  blocks    an interleaved scan visits the blocks in MCU order, padding included; a scan of one component visits the component's own
            ceil(w_c / 8) x ceil(h_c / 8) blocks in raster order, and its restart interval counts blocks.  ``block_index`` maps a scan's
            t-th block into the MCU-order coefficient array (int16, natural order, 64 per block), which starts as zeros.
  DC first  per block a Huffman-coded difference; value = (prediction + difference) << Al; the prediction is cut at restarts.
  DC refine one bit per block, ORed in at 1 << Al.
  AC first  symbols (run, size): size > 0 places a coefficient << Al behind ``run`` zeros; (15, 0) skips 16; (r < 15, 0) is EOBr: this
            block and (1 << r) + r extra bits - 1 more are complete.
  AC refine jdphuff's walk: a new coefficient is +-(1 << Al); every already non-zero coefficient that is passed, inside EOB runs too,
            takes one correction bit and moves away from zero by 1 << Al when it is set.
"""
import numpy as np

from tests import jpeg_dec_ref as D

Unsupported = D.Unsupported
MAX_SCANS = 64                         # FRCNN_JPEG_DEC_FULL_MAX_SCANS
STATUS_BLOCKS, STATUS_ZIGZAG, STATUS_CODE, STATUS_TABLE, STATUS_EOBRUN = 1, 2, 4, 8, 16
ZIGZAG = D.ZIGZAG


class Scan:
    """What frcnn_jpeg_dec_full_scan_t holds."""

    def __init__(self):
        self.off = self.len = self.restart_interval = self.subsequence_bytes = self.subsequences = 0
        self.dc_off, self.dc_count, self.ac_off, self.ac_count = [0] * 3, [0] * 3, [0] * 3, [0] * 3
        self.comps = self.ss = self.se = self.ah = self.al = 0

    @property
    def kind(self):
        return (2 if self.ss else 0) + (1 if self.ah else 0)    # 0 DC first, 1 DC refinement, 2 AC first, 3 AC refinement


class FullPlan:
    """What frcnn_jpeg_dec_full_plan_t holds: ``frame`` (a jpeg_dec_ref.Plan: the baseline's frame fields) and the scans."""

    def __init__(self):
        self.frame = D.Plan()
        self.scans = []


def plan(data):
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise Unsupported("not a JPEG file (no SOI)" if n else "empty file")
    fp = FullPlan()
    p = fp.frame
    p.file_len = n
    dqt, dht, sof, jfif, adobe, pos, restart, total = {}, {}, None, False, None, 2, 0, 0
    prog, comps, nc = [[-1] * 64 for _ in range(3)], None, 0
    while True:
        if pos + 4 > n:
            if pos + 2 <= n and data[pos] == 0xFF and data[pos + 1] == 0xD9 and fp.scans:
                break
            raise Unsupported("truncated: the file ends at byte %d before EOI" % pos)
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
            if not fp.scans:
                raise Unsupported("EOI before SOS")
            break
        seg = (data[pos + 2] << 8) | data[pos + 3]
        if seg < 2 or pos + 2 + seg > n:
            raise Unsupported("truncated: segment 0x%02X at byte %d runs past the file" % (m, pos))
        a, e = pos + 4, pos + 2 + seg
        if m == 0xC2:
            if sof is not None:
                raise Unsupported("two frame headers")
            if e - a < 6 or e - a != 6 + 3 * data[a + 5]:
                raise Unsupported("malformed SOF2")
            if data[a] != 8:
                raise Unsupported("%d-bit samples" % data[a])
            sof = a
        elif m == 0xC0:
            raise Unsupported("baseline (SOF0): the baseline planner's file")
        elif m in (0xC9, 0xCA, 0xCC):
            raise Unsupported("arithmetic coding")
        elif m == 0xC1:
            raise Unsupported("extended sequential")
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8):
            raise Unsupported("frame type 0x%02X" % m)
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
                if tc > 1 or th > 3:
                    raise Unsupported("Huffman table class %d id %d" % (tc, th))
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
            restart = (data[a] << 8) | data[a + 1]
        elif m == 0xE0 and e - a >= 5 and data[a:a + 5] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and e - a >= 12 and data[a:a + 5] == b"Adobe":
            adobe = data[a + 11]
        if m != 0xDA:
            pos = e
            continue

        # ---- a scan
        if sof is None:
            raise Unsupported("SOS before a frame header")
        if not fp.scans:                                       # the frame, as the baseline planner judges it
            nc = data[sof + 5]
            p.h, p.w, p.ncomp = (data[sof + 1] << 8) | data[sof + 2], (data[sof + 3] << 8) | data[sof + 4], nc
            if p.h < 1 or p.w < 1:
                raise Unsupported("frame %dx%d: both sides must be at least 1" % (p.h, p.w))
            if nc not in (1, 3):
                raise Unsupported("%d components (CMYK / YCCK)" % nc if nc == 4 else "%d components" % nc)
            comps = [(data[sof + 6 + 3 * c], data[sof + 7 + 3 * c] >> 4, data[sof + 7 + 3 * c] & 15, data[sof + 8 + 3 * c]) for c in range(nc)]
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
                p.hs = p.vs = 1
            p.mcus_x, p.mcus_y = -(-p.w // (8 * p.hs)), -(-p.h // (8 * p.vs))
            p.bpm = p.hs * p.vs + 2 if nc == 3 else 1
            p.expected_blocks = p.mcus_x * p.mcus_y * p.bpm
            p.restart_interval = restart
        k_scan = len(fp.scans)
        if k_scan == MAX_SCANS:
            raise Unsupported("more than %d scans" % MAX_SCANS)
        if e - a < 1 or not 1 <= data[a] <= nc or e - a != 4 + 2 * data[a]:
            raise Unsupported("malformed SOS")
        ns = data[a]
        s = Scan()
        s.ss, s.se, s.ah, s.al = data[e - 3], data[e - 2], data[e - 1] >> 4, data[e - 1] & 15
        if s.ss == 0:
            if s.se != 0:
                raise Unsupported("illegal script: scan %d mixes DC and AC (Ss=0 Se=%d)" % (k_scan, s.se))
        else:
            if s.ss > s.se or s.se > 63:
                raise Unsupported("illegal script: scan %d has Ss=%d Se=%d" % (k_scan, s.ss, s.se))
            if ns != 1:
                raise Unsupported("illegal script: AC scan %d holds %d components" % (k_scan, ns))
        if s.al > 13 or s.ah > 13:
            raise Unsupported("illegal script: scan %d has Ah=%d Al=%d" % (k_scan, s.ah, s.al))
        prev = -1
        for i in range(ns):
            ids = [c[0] for c in comps]
            c = ids.index(data[a + 1 + 2 * i]) if data[a + 1 + 2 * i] in ids else nc
            if c == nc or c <= prev:
                raise Unsupported("scan components out of frame order")
            prev = c
            s.comps |= 1 << c
            td, ta = data[a + 2 + 2 * i] >> 4, data[a + 2 + 2 * i] & 15
            if s.kind == 0:
                if (0, td) not in dht:
                    raise Unsupported("component %d names a Huffman table that is not defined" % c)
                s.dc_off[c], s.dc_count[c] = dht[(0, td)]
            elif s.kind >= 2:
                if (1, ta) not in dht:
                    raise Unsupported("component %d names a Huffman table that is not defined" % c)
                s.ac_off[c], s.ac_count[c] = dht[(1, ta)]
            if s.ss and prog[c][0] < 0:
                raise Unsupported("illegal script: AC scan %d of component %d before its DC scan" % (k_scan, c))
            for k in range(s.ss, s.se + 1):
                if (s.ah != 0) if prog[c][k] < 0 else (s.ah != prog[c][k] or s.al + 1 != s.ah):
                    raise Unsupported("illegal script: scan %d has Ah=%d Al=%d for coefficient %d of component %d, which stands at %d"
                                      % (k_scan, s.ah, s.al, k, c, prog[c][k]))
                prog[c][k] = s.al
            if s.kind == 0:                                    # the component's first scan: its quantisation table is latched here
                if comps[c][3] not in dqt:
                    raise Unsupported("component %d names a quantisation table that is not defined" % c)
                p.dqt_off[c] = dqt[comps[c][3]]
        s.restart_interval = restart
        s.off = e
        q = e
        while q < n:
            if data[q] == 0xFF and q + 1 < n and data[q + 1] != 0 and not 0xD0 <= data[q + 1] <= 0xD7:
                break
            q += 1
        if q == n:
            raise Unsupported("truncated: scan %d runs to the end of the file (no EOI)" % k_scan)
        if q == e:
            raise Unsupported("truncated: no entropy-coded data behind SOS")
        total += q - e
        if total >= D.MAX_SCAN:
            raise Unsupported("entropy-coded segments of %d bytes" % total)
        s.len = q - e
        s.subsequence_bytes, s.subsequences = D.subsequences(s.len)
        if not fp.scans:
            p.scan_off = s.off
        if (s.subsequences, s.subsequence_bytes) > (p.N, p.S):
            p.N, p.S = s.subsequences, s.subsequence_bytes
        fp.scans.append(s)
        pos = q
    p.scan_len = total
    for c in range(nc):
        for k in range(64):
            if prog[c][k] != 0:
                raise Unsupported("incomplete script: coefficient %d of component %d %s"
                                  % (k, c, "is never coded" if prog[c][k] < 0 else "is not refined to its last bit"))
    return fp


# ------------------------------------------------------------------------------------------------------------------ the scans
class Bits:
    """The entropy-coded segment bit by bit: a 0x00 behind 0xFF is skipped; an RSTm marker and what lies past the segment read as zero."""

    def __init__(self, seg):
        self.s, self.r, self.bit = seg, 0, 0

    def at(self, r):
        return self.s[r] if r < len(self.s) else 0

    def get(self):
        v = self.at(self.r)
        if v == 0xFF and 0xD0 <= self.at(self.r + 1) <= 0xD7:
            return 0
        b = (v >> (7 - self.bit)) & 1
        self.bit += 1
        if self.bit == 8:
            self.bit = 0
            self.r += 2 if v == 0xFF and self.at(self.r + 1) == 0 else 1
        return b

    def receive(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.get()
        return v

    def restart(self):
        """A restart is due: the padding of the byte is dropped, the marker behind it skipped -> 0, or STATUS_CODE where none stands."""
        if self.bit:
            self.r += 2 if self.at(self.r) == 0xFF and self.at(self.r + 1) == 0 else 1
            self.bit = 0
        if self.at(self.r) == 0xFF and 0xD0 <= self.at(self.r + 1) <= 0xD7:
            self.r += 2
            return 0
        return STATUS_CODE

    def symbol(self, table):
        """-> (symbol, status): the code bit by bit against maxcode / delta per length."""
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.get()
            if code <= table.maxcode[length]:
                k = code + table.delta[length]
                return (table.vals[k], 0) if 0 <= k < len(table.vals) else (0, STATUS_TABLE)
        return 0, STATUS_CODE


def scan_geometry(p, s):
    """-> (blocks the scan visits, blocks per MCU of the scan, blocks per row of a single component's scan or 0, the components)."""
    comps = [c for c in range(3) if s.comps >> c & 1]
    luma = p.hs * p.vs if p.ncomp == 3 else 1
    if len(comps) > 1:
        bps = sum(luma if c == 0 else 1 for c in comps)
        return p.mcus_x * p.mcus_y * bps, bps, 0, comps
    chroma = p.ncomp == 3 and comps[0] != 0
    wc, hc = (-(-p.w // p.hs), -(-p.h // p.vs)) if chroma else (p.w, p.h)
    row = -(-wc // 8)
    return row * -(-hc // 8), 1, row, comps


def block_index(p, s, t, geometry=None):
    """The scan's t-th block -> (its index in the MCU-order coefficient array, its component, is it the first of its component in its MCU)."""
    n, bps, row, comps = geometry or scan_geometry(p, s)
    luma = p.hs * p.vs if p.ncomp == 3 else 1
    if row == 0:
        order = []
        for c in comps:
            order += [(j, 0, j == 0) for j in range(luma)] if c == 0 else [(luma + c - 1, c, True)]
        at, c, first = order[t % bps]
        return (t // bps) * p.bpm + at, c, first
    by, bx = divmod(t, row)
    c = comps[0]
    if c == 0:
        return ((by // p.vs) * p.mcus_x + bx // p.hs) * p.bpm + (by % p.vs) * p.hs + bx % p.hs, 0, True
    return (by * p.mcus_x + bx) * p.bpm + luma + c - 1, c, True


def extend(v, size):
    return v - (1 << size) + 1 if size and v < 1 << (size - 1) else v


def wrap16(v):
    return ((v + 32768) & 0xFFFF) - 32768


def decode_scan(data, p, s, coef, info):
    """One scan into ``coef`` (int64 [blocks][64], natural order) -> its status bits."""
    bits = Bits(data[s.off:s.off + s.len])
    geometry = n, bps, row, comps = scan_geometry(p, s)
    kind, status = s.kind, 0
    tables = {}
    for c in comps:
        off, cnt = (s.dc_off[c], s.dc_count[c]) if kind == 0 else (s.ac_off[c], s.ac_count[c])
        if off:
            tables[c] = D.Huff(data, off, cnt)
    pred, eobrun, ri = [0, 0, 0], 0, s.restart_interval * bps
    p1 = 1 << s.al
    for t in range(n):
        if ri and t and t % ri == 0:
            status |= bits.restart()
            pred, eobrun = [0, 0, 0], 0
        if kind == 2 and eobrun:
            eobrun -= 1
            continue
        at, c, _ = block_index(p, s, t, geometry)
        blk = coef[at]
        if kind == 0:
            sym, st = bits.symbol(tables[c])
            status |= st | (STATUS_TABLE if sym > 11 else 0)
            pred[c] += extend(bits.receive(sym & 15), sym & 15)
            blk[0] = wrap16(wrap16(pred[c]) << s.al)
        elif kind == 1:
            if bits.get():
                blk[0] |= p1
        elif kind == 2:
            k = s.ss
            while k <= s.se:
                sym, st = bits.symbol(tables[c])
                status |= st
                r, size = sym >> 4, sym & 15
                if size:
                    status |= STATUS_TABLE if size > 10 else 0
                    k += r
                    v = extend(bits.receive(size), size)
                    if k > s.se:
                        status |= STATUS_ZIGZAG
                        break
                    blk[ZIGZAG[k]] = wrap16(v << s.al)
                    k += 1
                elif r == 15:
                    k += 16
                    status |= STATUS_ZIGZAG if k > s.se + 1 else 0
                else:
                    eobrun = (1 << r) + bits.receive(r)
                    info["max_eob_category"] = max(info.get("max_eob_category", 0), r)
                    if eobrun > n - t:
                        status |= STATUS_EOBRUN
                    eobrun -= 1
                    break
        else:
            k = s.ss

            def correct(z):
                if bits.get() and not blk[z] & p1:
                    blk[z] += p1 if blk[z] >= 0 else -p1

            if not eobrun:
                while k <= s.se:
                    sym, st = bits.symbol(tables[c])
                    status |= st
                    r, size, fresh = sym >> 4, sym & 15, 0
                    if size:
                        status |= STATUS_TABLE if size != 1 else 0
                        fresh = p1 if bits.get() else -p1
                    elif r != 15:
                        eobrun = (1 << r) + bits.receive(r)
                        info["max_eob_category"] = max(info.get("max_eob_category", 0), r)
                        if eobrun > n - t:
                            status |= STATUS_EOBRUN
                        break
                    while k <= s.se:
                        z = ZIGZAG[k]
                        if blk[z]:
                            correct(z)
                        else:
                            r -= 1
                            if r < 0:
                                break
                        k += 1
                    if fresh:
                        if k <= s.se:
                            blk[ZIGZAG[k]] = fresh
                        else:
                            status |= STATUS_ZIGZAG
                    k += 1
            if eobrun:
                while k <= s.se:
                    if blk[ZIGZAG[k]]:
                        correct(ZIGZAG[k])
                    k += 1
                eobrun -= 1
    if eobrun:
        status |= STATUS_EOBRUN
    return status


def coefficients(data, fp=None, info=None):
    """-> (coef int16 [blocks][64], natural order, blocks in MCU order padded to whole MCUs, DC as values; status)."""
    data = bytes(data)
    fp = fp or plan(data)
    info = {} if info is None else info
    coef = np.zeros((fp.frame.expected_blocks, 64), np.int64)
    status = 0
    for s in fp.scans:
        status |= decode_scan(data, fp.frame, s, coef, info)
    return coef.astype(np.int16), status


def decode(data, bgr=False, info=None):
    """The (h, w, 3) uint8 frame of a supported file; ``info`` (a dict) receives "status" and "max_eob_category"."""
    data = bytes(data)
    fp = plan(data)
    info = {} if info is None else info
    coef, status = coefficients(data, fp, info)
    info["status"] = status
    return D.pixels(data, fp.frame, coef, bgr)
