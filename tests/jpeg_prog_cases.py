"""The files the device decoder for progressive JPEG files is tested on (tests/test_jpeg_prog_cpu.py holds the CPU restatement to Pillow
on them, tests/test_jpeg_prog_gpu.py the kernels to the restatement): the frames and sizes of tests/jpeg_dec_cases.py written by Pillow
with ``progressive=True`` (libjpeg's default scripts: 10 scans for colour, 6 for grey), a flat frame whose end-of-band runs reach category
14, and files written by tests/jpeg_prog_write.py under scripts Pillow cannot write.  7x9, 17x23 and 33x65 with 2x2 sampling are the
sizes at which the MCU-padded and the true block counts differ."""
import functools
import io

import numpy as np

from tests import jpeg_cases as J
from tests import jpeg_dec_cases as C
from tests import jpeg_dec_ref as D
from tests import jpeg_prog_ref as R
from tests import jpeg_prog_write as W

DAMAGE_OF = "64x136_s0_q100"
FLAT = (1032, 1040)                     # 129 x 130 = 16 770 blocks: one end-of-band run of category 14 per AC scan


@functools.lru_cache(None)
def pillow_files():
    """name -> the file's bytes, written by Pillow."""
    out = {"golden_000005": reencode(open(C.GOLDEN, "rb").read())}
    for h, w in C.SIZES:
        for ss in (0, 1, 2):
            for q in (10, 75, 100):
                if (h, w) == (64, 136) and (ss, q) not in C.LONG:
                    continue
                out["%dx%d_s%d_q%d" % (h, w, ss, q)] = C.write(C.frame(h, w), quality=q, subsampling=ss, progressive=True)
    for h, w in ((17, 23), (33, 65)):
        out["grey_%dx%d" % (h, w)] = C.write(C.frame(h, w), mode="L", quality=75, progressive=True)
        for blocks in (1, 16):
            out["%dx%d_s2_q75_rst%d" % (h, w, blocks)] = C.write(C.frame(h, w), quality=75, subsampling=2, progressive=True, restart_marker_blocks=blocks)
    out["photo_s2_q75_optimize"] = C.write(J.CASES["photo_96x128"], quality=75, subsampling=2, optimize=True, progressive=True)
    out["flat_grey"] = C.write(np.full(FLAT + (3,), 128, np.uint8), mode="L", quality=75, progressive=True)
    return out


def reencode(data):
    from PIL import Image
    out = io.BytesIO()
    Image.open(io.BytesIO(data)).save(out, "JPEG", quality=75, progressive=True)
    return out.getvalue()


def dc(comps, ah=0, al=0, **kw):
    return dict(comps=list(comps), ss=0, se=0, ah=ah, al=al, **kw)


def ac(comp, ss, se, ah=0, al=0, **kw):
    return dict(comps=[comp], ss=ss, se=se, ah=ah, al=al, **kw)


def scripts(nc=3):
    """name -> a legal, complete scan script for ``nc`` components."""
    cs = range(nc)
    successive = [dc(cs, 0, 2)] + [ac(c, 1, 63, 0, 2) for c in cs] + [dc(cs, 2, 1)] + [ac(c, 1, 63, 2, 1) for c in cs] + \
                 [dc(cs, 1, 0)] + [ac(c, 1, 63, 1, 0) for c in cs]
    return {
        "spectral_dc_apart": [dc([c]) for c in cs] + [ac(c, 1, 63) for c in cs],
        "successive_twice": successive,
        "narrow_bands": [dc(cs)] + [ac(c, lo, hi) for c in cs for lo, hi in ((1, 1), (2, 5), (6, 20), (21, 63))],
        "dri_changes": [dc(cs, 0, 1, dri=2), ac(0, 1, 63, 0, 1, dri=5)] + [ac(c, 1, 63, 0, 1, dri=0 if c == 1 else 3) for c in cs[1:]] +
                       [dc(cs, 1, 0, dri=4)] + [ac(c, 1, 63, 1, 0) for c in cs],
        "dht_ids_2_3": [dc(cs, table=2)] + [ac(c, 1, 63, table=3 if c else 2) for c in cs],
    }


SOURCES = ("33x65_s2_q75", "17x23_s0_q75")      # the baseline files (tests/jpeg_dec_cases.py) whose coefficients the writer re-codes


def source(name):
    """-> (the baseline file, coef, frame, qtables) for the writer."""
    data = C.files()[name]
    p = D.plan(data)
    coef, _, status = D.coefficients(data, p)
    assert status == 0
    return data, coef, (p.h, p.w, p.ncomp, p.hs, p.vs), [data[p.dqt_off[c]:p.dqt_off[c] + 64] for c in range(p.ncomp)]


@functools.lru_cache(None)
def written_files():
    """name -> (the file's bytes, the name of the baseline file it must decode like), written by tests/jpeg_prog_write.py."""
    out = {}
    for src in SOURCES:
        _, coef, frame, q = source(src)
        for name, script in scripts().items():
            out["%s_%s" % (src, name)] = (W.write(coef, frame, q, script), src)
    return out


@functools.lru_cache(None)
def files():
    """name -> bytes: every supported case."""
    out = dict(pillow_files())
    out.update({k: v[0] for k, v in written_files().items()})
    return out


LONG = tuple("64x136_s%d_q%d" % sq for sq in C.LONG)
SMALLEST = ("1x1_s0_q75", "1x1_s1_q75", "1x1_s2_q75")


def patch_sof(data, component, value):
    at = data.index(b"\xFF\xC2") + 4
    data = bytearray(data)
    data[at if component is None else at + 7 + 3 * component] = value
    return bytes(data)


@functools.lru_cache(None)
def unsupported():
    """name -> (bytes, a word of the reason)."""
    from PIL import Image
    f = C.frame(17, 23)
    _, coef, frame, q = source(SOURCES[0])
    s = scripts()
    cmyk = io.BytesIO()
    Image.fromarray(f).convert("CMYK").save(cmyk, "JPEG", quality=75, progressive=True)
    prog = C.write(f, quality=75, subsampling=1, progressive=True)
    third = R.plan(prog).scans[2]
    many = [dc(range(3))] + [ac(0, k, k) for k in range(1, 64)] + [ac(1, 1, 1)]
    return {
        "baseline": (C.files()["17x23_s1_q75"], "baseline"),
        "incomplete": (W.write(coef, frame, q, s["successive_twice"][:-1]), "incomplete"),
        "illegal_progression": (W.write(coef, frame, q, [dc(range(3), 0, 2), dc(range(3), 1, 0)]), "illegal"),
        "ac_two_components": (W.write(coef, frame, q, [dc(range(3)), dict(comps=[1, 2], ss=1, se=63, ah=0, al=0)]), "AC scan"),
        "ac_before_dc": (W.write(coef, frame, q, [dc([0]), ac(1, 1, 63)]), "before its DC"),
        "too_many_scans": (W.write(coef, frame, q, many), "more than"),
        "cmyk": (cmyk.getvalue(), "CMYK"),
        "sampling_1x2": (patch_sof(prog, 0, 0x12), "sampling"),
        "sampling_chroma_2x1": (patch_sof(prog, 1, 0x21), "sampling"),
        "12_bit": (patch_sof(prog, None, 12), "12-bit"),
        "rgb_ids": (C.write(f, quality=75, keep_rgb=True, progressive=True), "Adobe transform 0"),
        "cut_in_third_scan": (prog[:third.off + third.len // 2], "truncated"),
    }


def damaged():
    """name -> a supported file with 96 bytes of one scan overwritten (as jpeg_dec_cases.damaged does): its last AC-refinement scan, its
    DC-first scan.  The headers stand, so the planner takes it."""
    data = pillow_files()[DAMAGE_OF]
    scans = R.plan(data).scans
    out = {}
    for name, s in (("ac_refinement", [s for s in scans if s.kind == 3][-1]), ("dc_first", [s for s in scans if s.kind == 0][0])):
        at = s.off + s.len // 3
        assert s.len // 3 + 96 <= s.len, "the overwritten stretch lies inside the scan"
        hurt = bytearray(data)
        hurt[at:at + 96] = bytes([0x5A, 0x00, 0xA5, 0x0F] * 24)
        out[name] = bytes(hurt)
    return out
