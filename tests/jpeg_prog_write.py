"""A small progressive JPEG writer for the tests of the device decoder (tests/jpeg_prog_cases.py): quantised coefficients (as
tests/jpeg_dec_ref.py extracts them from a baseline file), quantisation tables, sampling factors and a SCAN SCRIPT -> an SOF2 file.  It
exists because Pillow writes libjpeg's default scripts only.  The Huffman tables are fixed legal tables that hold every symbol (byte size
does not matter).  It is validated by Pillow, never by the code under test: Pillow's pixels of the written file equal Pillow's pixels of
the baseline file the coefficients came from (tests/test_jpeg_prog_cpu.py).  The encoder is T.81 annex G as libjpeg's jcphuff.c walks it.

A script is a list of scans, each a dict: ``comps`` (frame component indices), ``ss``, ``se``, ``ah``, ``al``, and optionally ``dri`` (a
DRI segment with this interval in front of the scan: valid from there on), ``table`` (the Huffman table id the scan's tables are
written under and named by, default 0) and ``raw`` (a function applied to the finished SOS header bytes: for illegal files)."""
import struct

from tests import jpeg_dec_ref as D

ZIGZAG = D.ZIGZAG
DC_BITS, DC_VALS = [0, 0, 0, 12] + [0] * 12, list(range(12))                 # twelve 4-bit codes: 0000 .. 1011
AC_BITS, AC_VALS = [0] * 7 + [254, 2] + [0] * 7, list(range(256))             # 254 8-bit codes, two 9-bit ones; no all-ones code


def codes(bits, vals):
    """symbol -> (code, length) of a canonical table."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


DC_CODES, AC_CODES = codes(DC_BITS, DC_VALS), codes(AC_BITS, AC_VALS)


class Out:
    def __init__(self):
        self.bytes, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, nbits):
        for i in range(nbits - 1, -1, -1):
            self.acc, self.n = (self.acc << 1) | ((value >> i) & 1), self.n + 1
            if self.n == 8:
                self.bytes.append(self.acc)
                if self.acc == 0xFF:
                    self.bytes.append(0)
                self.acc = self.n = 0

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)

    def marker(self, m):
        self.flush()
        self.bytes += bytes([0xFF, m])


def nbits_of(v):
    return int(v).bit_length()


def segment(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + bytes(payload)


def scan_blocks(frame, comps):
    """The blocks a scan visits, in its order -> [(index into the MCU-order coefficient array, component)], blocks per MCU of the scan."""
    h, w, nc, hs, vs = frame
    luma = hs * vs if nc == 3 else 1
    bpm = luma + 2 if nc == 3 else 1
    mcus_x, mcus_y = -(-w // (8 * hs)), -(-h // (8 * vs))
    if len(comps) > 1:
        order = []
        for c in comps:
            order += [(j, 0) for j in range(luma)] if c == 0 else [(luma + c - 1, c)]
        return [(m * bpm + at, c) for m in range(mcus_x * mcus_y) for at, c in order], len(order)
    c = comps[0]
    wc, hc = (-(-w // hs), -(-h // vs)) if nc == 3 and c else (w, h)
    out = []
    for by in range(-(-hc // 8)):
        for bx in range(-(-wc // 8)):
            if c == 0:
                out.append((((by // vs) * mcus_x + bx // hs) * bpm + (by % vs) * hs + bx % hs, 0))
            else:
                out.append(((by * mcus_x + bx) * bpm + luma + c - 1, c))
    return out, 1


def encode_scan(coef, frame, scan, restart):
    """The entropy-coded segment of one scan (jcphuff.c: encode_mcu_DC_first / AC_first / DC_refine / AC_refine)."""
    blocks, bps = scan_blocks(frame, scan["comps"])
    ss, se, ah, al = scan["ss"], scan["se"], scan["ah"], scan["al"]
    out, pred, state = Out(), [0, 0, 0], {"eobrun": 0, "be": []}

    def emit_eobrun():
        if state["eobrun"]:
            n = nbits_of(state["eobrun"]) - 1
            out.put(*AC_CODES[n << 4])
            out.put(state["eobrun"] & ((1 << n) - 1), n)
            state["eobrun"] = 0
        for b in state["be"]:
            out.put(b, 1)
        state["be"] = []

    for t, (at, c) in enumerate(blocks):
        if restart and t and t % (restart * bps) == 0:
            emit_eobrun()
            out.marker(0xD0 + (t // (restart * bps) - 1) % 8)
            pred = [0, 0, 0]
        blk = [int(v) for v in coef[at]]
        if ss == 0 and ah == 0:
            v = blk[0] >> al
            diff, pred[c] = v - pred[c], v
            n = nbits_of(abs(diff))
            out.put(*DC_CODES[n])
            out.put(diff if diff >= 0 else diff + (1 << n) - 1, n)
        elif ss == 0:
            out.put((blk[0] >> al) & 1, 1)
        elif ah == 0:
            r = 0
            for k in range(ss, se + 1):
                v = blk[ZIGZAG[k]]
                mag = abs(v) >> al
                if mag == 0:
                    r += 1
                    continue
                emit_eobrun()
                while r > 15:
                    out.put(*AC_CODES[0xF0])
                    r -= 16
                n = nbits_of(mag)
                out.put(*AC_CODES[(r << 4) + n])
                out.put(mag if v >= 0 else (~mag) & ((1 << n) - 1), n)
                r = 0
            if r:
                state["eobrun"] += 1
                if state["eobrun"] == 0x7FFF:
                    emit_eobrun()
        else:
            mags = {k: abs(blk[ZIGZAG[k]]) >> al for k in range(ss, se + 1)}
            eob = max([k for k in mags if mags[k] == 1], default=0)
            r, br = 0, []
            for k in range(ss, se + 1):
                mag = mags[k]
                if mag == 0:
                    r += 1
                    continue
                while r > 15 and k <= eob:
                    emit_eobrun()
                    out.put(*AC_CODES[0xF0])
                    r -= 16
                    for b in br:
                        out.put(b, 1)
                    br = []
                if mag > 1:
                    br.append(mag & 1)
                    continue
                emit_eobrun()
                out.put(*AC_CODES[(r << 4) + 1])
                out.put(0 if blk[ZIGZAG[k]] < 0 else 1, 1)
                for b in br:
                    out.put(b, 1)
                r, br = 0, []
            if r or br:
                state["eobrun"] += 1
                state["be"] += br
                if state["eobrun"] == 0x7FFF or len(state["be"]) > 1000 - 64 + 1:
                    emit_eobrun()
    emit_eobrun()
    out.flush()
    return bytes(out.bytes)


def write(coef, frame, qtables, script, sof=0xC2):
    """coef: int [blocks][64], natural order, blocks in MCU order (jpeg_dec_ref.coefficients); frame: (h, w, components, hs, vs);
    qtables: per component its 64 entries in zigzag order -> the file's bytes."""
    h, w, nc, hs, vs = frame
    out = bytearray(b"\xFF\xD8") + segment(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    for c in range(nc):
        out += segment(0xDB, bytes([c]) + bytes(qtables[c]))
    sof_body = struct.pack(">BHHB", 8, h, w, nc)
    for c in range(nc):
        sof_body += bytes([c + 1, ((hs << 4) | vs) if c == 0 and nc == 3 else 0x11, c])
    out += segment(sof, sof_body)
    restart = 0
    for scan in script:
        if "dri" in scan:
            restart = scan["dri"]
            out += segment(0xDD, struct.pack(">H", restart))
        table = scan.get("table", 0)
        if scan["ss"] == 0 and scan["ah"] == 0:
            out += segment(0xC4, bytes([table]) + bytes(DC_BITS) + bytes(DC_VALS))
        elif scan["ss"]:
            out += segment(0xC4, bytes([0x10 | table]) + bytes(AC_BITS) + bytes(AC_VALS))
        head = bytes([len(scan["comps"])]) + b"".join(bytes([c + 1, (table << 4) | table]) for c in scan["comps"])
        head += bytes([scan["ss"], scan["se"], (scan["ah"] << 4) | scan["al"]])
        sos = segment(0xDA, head)
        out += scan["raw"](sos) if "raw" in scan else sos
        out += encode_scan(coef, frame, scan, restart)
    return bytes(out + b"\xFF\xD9")
