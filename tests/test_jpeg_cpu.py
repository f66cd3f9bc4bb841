"""The device JPEG encoder, the parts that need no GPU: its C-ABI entry points in an extension header of their own
(include/ext/frcnn_hip_jpeg.h), their ctypes table and the built library; the size bound; annotate_video's options; and the CPU
restatement of the stream (tests/jpeg_ref.py) against Pillow -- structure, tables, and fidelity and size beside Pillow's own file at the
same quality, without subsampling and with the same restart interval."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from tests import jpeg_ref as R
from tests.jpeg_cases import CASES, RUNS, SPARSE_AT

Image = pytest.importorskip("PIL.Image")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("frcnn_jpeg_version", "frcnn_jpeg_restart_mcus", "frcnn_jpeg_header_bytes", "frcnn_jpeg_bound", "frcnn_jpeg_workspace_bytes",
               "frcnn_jpeg_encode_u8")

# Fidelity and size beside Pillow's file (same quality, subsampling=0, restart_marker_blocks=16), measured over RUNS with this file's
# test_fidelity_and_size_beside_pillow (it prints every figure).  Both encoders share tables and interval; the gaps come from the
# rounding of colour transform and DCT.  Observed: the restatement's PSNR is at most 0.041 dB below Pillow's (noise_13x21, quality 90) and
# at most 0.512 dB above it (9x1, quality 90); its file is at most 0.088 % longer (noise_64x136, quality 10) and at most 2.942 % shorter
# (photo_96x128, quality 100).  Each margin is twice the worst gap observed on its side, with floors of 0.1 dB and 0.5 %.
PSNR_DEFICIT_MARGIN_DB = 0.1            # 2 x 0.041 = 0.082: the floor
PSNR_SURPLUS_MARGIN_DB = 1.024          # 2 x 0.512
SIZE_EXCESS_MARGIN = 0.005              # 2 x 0.00088 = 0.0018: the floor
SIZE_SAVING_MARGIN = 0.0589             # 2 x 0.02942


def pillow_file(frame, quality):
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="JPEG", quality=quality, subsampling=0, restart_marker_blocks=R.RESTART_MCUS)
    return buf.getvalue()


def psnr(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    mse = float(np.mean(d * d))
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def decoded(data):
    img = Image.open(io.BytesIO(data))
    img.load()
    assert img.mode == "RGB"
    return img


def split(data):
    """-> ([(marker, payload)] SOI .. SOS, the entropy-coded bytes); asserts SOI at the start and EOI at the end."""
    assert data[:2] == b"\xFF\xD8" and data[-2:] == b"\xFF\xD9"
    segs, pos = [], 2
    while True:
        assert data[pos] == 0xFF
        marker, n = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        segs.append((marker, data[pos + 4:pos + 2 + n]))
        pos += 2 + n
        if marker == 0xDA:
            return segs, data[pos:-2]


def check_structure(data, h, w):
    """Segment order, restart markers in number and cyclic order, no unstuffed 0xFF in the entropy-coded data."""
    segs, ecs = split(data)
    assert [m for m, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert sum(4 + len(p) for _, p in segs) + 2 == R.HEADER_BYTES
    assert segs[0][1] == b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    assert segs[3][1][:5] == bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big")
    assert int.from_bytes(segs[8][1], "big") == R.RESTART_MCUS
    intervals = -(-(-(-h // 8) * -(-w // 8)) // R.RESTART_MCUS)
    markers, i = [], 0
    while i < len(ecs):
        if ecs[i] == 0xFF:
            assert i + 1 < len(ecs) and (ecs[i + 1] == 0 or 0xD0 <= ecs[i + 1] <= 0xD7), "unstuffed 0xFF at %d" % i
            if ecs[i + 1]:
                markers.append(ecs[i + 1] - 0xD0)
            i += 2
        else:
            i += 1
    assert markers == [k & 7 for k in range(intervals - 1)]
    return segs


def test_header_ctypes_and_library_agree_on_the_jpeg_symbols():
    """The pattern of tests/test_png_huff_cpu.py: every symbol the header declares is in _lib.JPEG_SIGNATURES with matching argument kinds
    and exported by the built library, and nothing else is in that table; the revisions agree; the other headers and tables do not know
    the new symbols and keep their revisions."""
    from faster_rcnn_amd import _lib
    from faster_rcnn_amd.build import build_library
    ext = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_jpeg.h")).read()
    version = int(re.search(r"#define FRCNN_JPEG_VERSION (\d+)", ext).group(1))
    assert version == _lib.JPEG_VERSION == 1 and re.search(r"^ \*   1 = ", ext, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    assert sorted(set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.JPEG_SIGNATURES) == sorted(NEW_SYMBOLS)
    build_library(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        m = re.search(r"\b(int|size_t) %s\s*\(([^)]*)\)" % name, code)
        assert m, name
        decls = [d for d in m.group(2).split(",") if d.strip() != "void"]
        restype, argtypes = _lib.JPEG_SIGNATURES[name]
        assert restype is {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[m.group(1)] and len(argtypes) == len(decls), name
        for decl, ct in zip(decls, argtypes):                            # pointers are pointers, sizes are sizes, ints are ints
            assert ("*" in decl) == (ct is ctypes.c_void_p), (name, decl)
            assert ("size_t" in decl) == (ct is ctypes.c_size_t), (name, decl)
        assert hasattr(lib, name), name
    loaded = _lib.load()
    assert loaded.frcnn_jpeg_version() == version
    core = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    others = "".join(open(os.path.join(ROOT, "include", "ext", f)).read() for f in ("frcnn_hip_png.h", "frcnn_hip_png_huff.h"))
    for name in NEW_SYMBOLS:
        assert name not in core and name not in others
        assert not any(name in t for t in (_lib.SIGNATURES, _lib.EXT_SIGNATURES, _lib.PNG_SIGNATURES, _lib.PNG_HUFF_SIGNATURES))
    assert loaded.frcnn_png_version() == _lib.PNG_VERSION == 1 and loaded.frcnn_png_huff_version() == _lib.PNG_HUFF_VERSION == 1
    assert loaded.frcnn_version() == _lib.ABI_VERSION == int(re.search(r"#define FRCNN_ABI_VERSION (\d+)", core).group(1))


def test_constants_and_bound():
    """The exported constants are the restatement's; the bound is its formula, monotone in both sides, and refused where the header says."""
    from faster_rcnn_amd import _lib, ops
    from faster_rcnn_amd._lib import FrcnnError
    lib = _lib.load()
    ext = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_jpeg.h")).read()
    assert lib.frcnn_jpeg_restart_mcus() == ops.JPEG_RESTART_MCUS == R.RESTART_MCUS == int(re.search(r"#define FRCNN_JPEG_RESTART_MCUS (\d+)", ext).group(1))
    assert lib.frcnn_jpeg_header_bytes() == ops.jpeg_header_bytes() == R.HEADER_BYTES == len(R.header(375, 1242, R.quant_tables(90)))
    sides = [1, 2, 7, 8, 9, 63, 64, 65, 375, 600, 1000, 1242]
    for h in sides:
        prev = 0
        for w in sides:
            b = ops.jpeg_bound(h, w)
            assert b == R.bound(h, w) and b >= prev and ops.jpeg_workspace_bytes(h, w) % 16 == 0, (h, w)
            assert ops.jpeg_bound(w, h) == b
            prev = b
    assert ops.jpeg_bound(375, 1242) == R.HEADER_BYTES + 2 + 416 * 3 * 7332 + 4 * 459
    assert ops.jpeg_bound(65535, 8) == R.bound(65535, 8) > 0
    for h, w in ((0, 5), (5, 0), (-1, 5), (65536, 8), (8, 65536), (65535, 65535)):      # (the last: a bound past 2^31 - 1)
        assert R.bound(h, w) == 0 and lib.frcnn_jpeg_bound(h, w) == 0 and lib.frcnn_jpeg_workspace_bytes(h, w) == 0
        with pytest.raises(FrcnnError):
            ops.jpeg_bound(h, w)
        with pytest.raises(FrcnnError):
            ops.jpeg_workspace_bytes(h, w)


def test_tables_are_annex_k():
    """Quantisation tables: the IJG rule at its ends and at 50; Huffman tables: prefix codes of at most 16 bits."""
    assert R.quant_tables(50)[0] == [R.K1_LUMA[n] for n in R.ZIGZAG] and R.quant_tables(50)[1] == [R.K2_CHROMA[n] for n in R.ZIGZAG]
    assert set(R.quant_tables(100)[0] + R.quant_tables(100)[1]) == {1}
    assert max(R.quant_tables(1)[0]) == 255 and min(R.quant_tables(1)[0]) == 255
    assert sorted(R.ZIGZAG) == list(range(64)) and R.ZIGZAG[:6] == [0, 1, 8, 16, 9, 2] and R.ZIGZAG[-3:] == [55, 62, 63]
    for bits, vals in R.HUFFMAN:
        assert sum(bits) == len(vals) == len(set(vals))
        codes = R.huffman_codes(bits, vals)
        assert max(l for _, l in codes.values()) <= 16
        kraft = sum(2 ** (16 - l) for _, l in codes.values())
        assert kraft <= 2 ** 16 - 1                                                 # a prefix code whose all-ones code stays free
        assert len(vals) != 162 or kraft == 2 ** 16 - 1                             # ... and the AC codes are complete but for it
    assert int(np.abs(R.COS).sum(axis=1).max()) <= 32768                         # the row pass stays below 2^22, the column pass below 2^28


@pytest.mark.parametrize("name,quality", RUNS)
def test_restatement_is_a_sound_file(name, quality):
    from faster_rcnn_amd import ops
    frame = CASES[name]
    h, w = frame.shape[:2]
    info = {}
    data = R.encode(frame, quality, info=info)
    assert len(data) <= R.bound(h, w) == ops.jpeg_bound(h, w)
    img = decoded(data)
    assert img.size == (w, h)
    segs = check_structure(data, h, w)
    pil = pillow_file(frame, quality)
    assert img.quantization == decoded(pil).quantization                       # the same DQT payloads as Pillow at this quality
    assert [p for m, p in segs if m == 0xDB] == [bytes([k] + t) for k, t in enumerate(R.quant_tables(quality))]
    assert [p for m, p in segs if m == 0xC4] == [p for m, p in split(pil)[0] if m == 0xC4]      # Pillow's DHT segments (no optimize)
    assert len(info["intervals"]) == -(-(-(-h // 8) * -(-w // 8)) // R.RESTART_MCUS) and info["intervals"][0] == R.HEADER_BYTES
    assert R.encode(np.ascontiguousarray(frame[:, :, ::-1]), quality, bgr=True) == data        # channel order: the same file
    if name == "flat_24x40":
        assert all(nz in ([], [0]) for nz in info["nonzero"]) and info["max_category"][1] == 0
    if name == "noise_64x136":
        assert len(info["intervals"]) == 9
    if name == "sparse_hf":
        assert info["nonzero"][0::3] == [[z] for z in SPARSE_AT] and not any(info["nonzero"][1::3] + info["nonzero"][2::3])
    if name == "extremes_16x16" and quality == 100:
        assert info["max_category"] == (11, 10) and 63 in info["nonzero"][0]


def test_fidelity_and_size_beside_pillow():
    """Over every run: the restatement's PSNR against the source and its length, beside those of Pillow's own file.  Runs whose Pillow
    file decodes to the source exactly (infinite PSNR) are left out of the PSNR comparison only."""
    worst = {"deficit": 0.0, "surplus": 0.0, "excess": 0.0, "saving": 0.0}
    for name, quality in RUNS:
        frame = CASES[name]
        mine, pil = R.encode(frame, quality), pillow_file(frame, quality)
        size_gap = (len(mine) - len(pil)) / len(pil)
        p_mine, p_pil = psnr(np.asarray(decoded(mine)), frame), psnr(np.asarray(decoded(pil)), frame)
        print("%-16s q%3d: %6d bytes, Pillow %6d (%+.3f %%); PSNR %.3f dB, Pillow %.3f" % (name, quality, len(mine), len(pil), 100 * size_gap,
                                                                                       p_mine, p_pil))
        worst["excess"], worst["saving"] = max(worst["excess"], size_gap), max(worst["saving"], -size_gap)
        assert -SIZE_SAVING_MARGIN <= size_gap <= SIZE_EXCESS_MARGIN, (name, quality, size_gap)
        if np.isinf(p_pil):
            continue
        worst["deficit"], worst["surplus"] = max(worst["deficit"], p_pil - p_mine), max(worst["surplus"], p_mine - p_pil)
        assert -PSNR_SURPLUS_MARGIN_DB <= p_pil - p_mine <= PSNR_DEFICIT_MARGIN_DB, (name, quality, p_mine, p_pil)
    print("worst gaps:", worst)


def test_option_check(monkeypatch):
    from faster_rcnn_amd import annotate_video as av
    for var in ("FRCNN_ANNOTATE_FRAME_FORMAT", "FRCNN_ANNOTATE_JPEG_ENCODER", "FRCNN_ANNOTATE_PNG_ENCODER", "FRCNN_ANNOTATE_PNG_COMPRESS"):
        monkeypatch.delenv(var, raising=False)
    p = av.build_parser()
    args = p.parse_args(["a", "b", "c"])
    assert (args.frame_format, args.jpeg_encoder, args.jpeg_quality) == ("png", "host", None)
    args = p.parse_args(["a", "b", "c", "--frame_format", "jpg", "--jpeg_encoder", "device", "--jpeg_quality", "75"])
    assert (args.frame_format, args.jpeg_encoder, args.jpeg_quality) == ("jpg", "device", 75)
    with pytest.raises(SystemExit):
        p.parse_args(["a", "b", "c", "--frame_format", "gif"])
    # every legal combination
    assert av.jpeg_options() == ("png", "host", 90)
    assert av.jpeg_options("png", "host", None, "device", "huffman") == ("png", "host", 90)
    assert av.jpeg_options("jpg") == ("jpg", "host", 90) and av.jpeg_options("jpg", "host", 100) == ("jpg", "host", 100)
    assert av.jpeg_options("jpg", "device") == ("jpg", "device", 90) and av.jpeg_options("jpg", "device", 1) == ("jpg", "device", 1)
    # every refused one
    for kw in (dict(frame_format="png", jpeg_encoder="device"), dict(frame_format="png", jpeg_quality=90), dict(jpeg_encoder="device"),
               dict(frame_format="jpg", png_encoder="device"), dict(frame_format="jpg", png_encoder="device", png_compress="huffman"),
               dict(frame_format="jpg", jpeg_quality=0), dict(frame_format="jpg", jpeg_quality=101), dict(frame_format="jpg", jpeg_quality=90.0),
               dict(frame_format="gif"), dict(frame_format="jpg", jpeg_encoder="gpu")):
        with pytest.raises(ValueError):
            av.jpeg_options(**kw)
    for argv in (["--jpeg_encoder", "device"], ["--jpeg_quality", "80"], ["--frame_format", "jpg", "--png_encoder", "device"],
                 ["--frame_format", "jpg", "--png_encoder", "device", "--png_compress", "huffman"], ["--frame_format", "jpg", "--jpeg_quality", "0"]):
        with pytest.raises(ValueError):                                     # ... before any model file is opened
            av.main(["no.npz", "no.npz", "nowhere"] + argv)
    with pytest.raises(ValueError):
        av.annotate_images(None, None, "nowhere", "nowhere", [], 600, 1000, jpeg_encoder="device")
    with pytest.raises(ValueError):
        av.annotate_images(None, None, "nowhere", "nowhere", [], 600, 1000, frame_format="jpg", png_encoder="device")
    monkeypatch.setenv("FRCNN_ANNOTATE_FRAME_FORMAT", "jpg")
    monkeypatch.setenv("FRCNN_ANNOTATE_JPEG_ENCODER", "device")
    args = av.build_parser().parse_args(["a", "b", "c"])
    assert (args.frame_format, args.jpeg_encoder) == ("jpg", "device") and av.jpeg_options(None, None, 80) == ("jpg", "device", 80)
    monkeypatch.setenv("FRCNN_ANNOTATE_FRAME_FORMAT", "bmp")
    with pytest.raises(ValueError):
        av.default_frame_format()
    monkeypatch.setenv("FRCNN_ANNOTATE_FRAME_FORMAT", "jpg")
    monkeypatch.setenv("FRCNN_ANNOTATE_JPEG_ENCODER", "gpu")
    with pytest.raises(ValueError):
        av.default_jpeg_encoder()
