"""The huffman mode of the device PNG encoder, the parts that need no GPU: its C-ABI entry points in an extension header of their own
(include/ext/frcnn_hip_png_huff.h), their ctypes table and the built library; the size bound; annotate_video's command line; and the CPU
restatement of the stream (tests/png_huff_ref.py) against Pillow and zlib, with the size condition on a photograph."""
import ctypes
import io
import os
import re
import zlib

import numpy as np
import pytest

from tests import png_huff_ref as R
from tests.png_huff_cases import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("frcnn_png_huff_version", "frcnn_png_huff_band_rows", "frcnn_png_huff_bound", "frcnn_png_huff_workspace_bytes",
               "frcnn_png_huff_encode_u8")


def test_header_ctypes_and_library_agree_on_the_huffman_symbols():
    """The pattern of tests/test_png_cpu.py: every symbol the header declares is in _lib.PNG_HUFF_SIGNATURES with matching argument kinds
    and exported by the built library, and nothing else is in that table; the revisions agree; the argument lists are those of the
    frcnn_png_* namesakes; the core header and the other tables do not know the new symbols."""
    from faster_rcnn_amd import _lib
    from faster_rcnn_amd.build import build_library
    ext = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_png_huff.h")).read()
    version = int(re.search(r"#define FRCNN_PNG_HUFF_VERSION (\d+)", ext).group(1))
    assert version == _lib.PNG_HUFF_VERSION == 1 and re.search(r"^ \*   1 = ", ext, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    assert sorted(set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.PNG_HUFF_SIGNATURES) == sorted(NEW_SYMBOLS)
    build_library(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        m = re.search(r"\b(int|size_t) %s\s*\(([^)]*)\)" % name, code)
        assert m, name
        decls = [d for d in m.group(2).split(",") if d.strip() != "void"]
        restype, argtypes = _lib.PNG_HUFF_SIGNATURES[name]
        assert restype is {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[m.group(1)] and len(argtypes) == len(decls), name
        for decl, ct in zip(decls, argtypes):                            # pointers are pointers, sizes are sizes, ints are ints
            assert ("*" in decl) == (ct is ctypes.c_void_p), (name, decl)
            assert ("size_t" in decl) == (ct is ctypes.c_size_t), (name, decl)
        assert hasattr(lib, name), name
        assert _lib.PNG_HUFF_SIGNATURES[name] == _lib.PNG_SIGNATURES[name.replace("_huff", "")], name
    assert _lib.load().frcnn_png_huff_version() == version
    core = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    png = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_png.h")).read()
    for name in NEW_SYMBOLS:
        assert name not in core and name not in png
        assert name not in _lib.SIGNATURES and name not in _lib.EXT_SIGNATURES and name not in _lib.PNG_SIGNATURES
    assert _lib.load().frcnn_png_version() == _lib.PNG_VERSION == 1
    assert _lib.load().frcnn_version() == _lib.ABI_VERSION == int(re.search(r"#define FRCNN_ABI_VERSION (\d+)", core).group(1))


def test_band_rows_constant():
    from faster_rcnn_amd import _lib, ops
    assert _lib.load().frcnn_png_huff_band_rows() == ops.PNG_HUFF_BAND_ROWS == R.BAND_ROWS and R.BAND_ROWS in (4, 8)
    assert _lib.load().frcnn_png_band_rows() == ops.PNG_BAND_ROWS == 1


def test_huffman_bound():
    """As tests/test_png_cpu.py's for the runs mode: monotone in both sides; never below the filtered stream plus the smallest framing
    (57 bytes); within 2 % (+ 4096) of the filtered stream for real frame sizes; refused for the same sizes."""
    from faster_rcnn_amd import ops
    from faster_rcnn_amd._lib import FrcnnError
    sides = [1, 2, 3, 7, 8, 9, 63, 64, 65, 375, 600, 1000, 1242, 21845, 21846]
    for h in sides:
        prev = 0
        for w in sides:
            b = ops.png_bound(h, w, "huffman")
            assert b > prev and b >= h * (1 + 3 * w) + 57, (h, w)
            prev = b
    for w in sides:
        prev = 0
        for h in sides:
            b = ops.png_bound(h, w, "huffman")
            assert b > prev, (h, w)
            prev = b
    for h, w in ((375, 1242), (600, 1000)):
        assert ops.png_bound(h, w, "huffman") <= h * (1 + 3 * w) * 1.02 + 4096
    for h, w in ((0, 5), (5, 0), (-1, 5), (1 << 20, 1 << 20)):              # (the last: a filtered stream past 2 GiB)
        with pytest.raises(FrcnnError):
            ops.png_bound(h, w, "huffman")
        with pytest.raises(FrcnnError):
            ops.png_bound(h, w)
    with pytest.raises(FrcnnError):
        ops.png_bound(5, 5, "deflate")
    assert ops.png_workspace_bytes(375, 1242, "huffman") >= ops.png_bound(375, 1242, "huffman") - 66
    assert ops.png_bound(375, 1242) == ops.png_bound(375, 1242, "runs")


def test_command_line(monkeypatch):
    from faster_rcnn_amd import annotate_video
    monkeypatch.delenv("FRCNN_ANNOTATE_PNG_COMPRESS", raising=False)
    monkeypatch.delenv("FRCNN_ANNOTATE_PNG_ENCODER", raising=False)
    p = annotate_video.build_parser()
    assert p.parse_args(["a", "b", "c"]).png_compress == "runs" and p.parse_args(["a", "b", "c"]).png_encoder == "host"
    args = p.parse_args(["a", "b", "c", "--png_encoder", "device", "--png_compress", "huffman"])
    assert (args.png_encoder, args.png_compress) == ("device", "huffman")
    assert annotate_video.png_options("device", "huffman") == ("device", "huffman")
    assert annotate_video.png_options(None, None) == ("host", "runs")
    with pytest.raises(SystemExit):
        p.parse_args(["a", "b", "c", "--png_compress", "lz77"])
    with pytest.raises(ValueError):
        annotate_video.png_options("host", "huffman")
    with pytest.raises(ValueError):                                         # ... before any model file is opened
        annotate_video.main(["no.npz", "no.npz", "nowhere", "--png_compress", "huffman"])
    with pytest.raises(ValueError):
        annotate_video.annotate_images(None, None, "nowhere", "nowhere", [], 600, 1000, png_encoder="host", png_compress="huffman")
    monkeypatch.setenv("FRCNN_ANNOTATE_PNG_COMPRESS", "huffman")
    assert annotate_video.build_parser().parse_args(["a", "b", "c"]).png_compress == "huffman"
    assert annotate_video.png_options("device", None) == ("device", "huffman")
    monkeypatch.setenv("FRCNN_ANNOTATE_PNG_COMPRESS", "zip")
    with pytest.raises(ValueError):
        annotate_video.default_png_compress()


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("bgr", [False, True])
def test_restatement_decodes(name, bgr):
    """Pillow decodes the restatement's file to the frame, zlib inflates its IDAT data to h * (1 + 3w) bytes (and checks the Adler-32),
    and the file is within the bound."""
    from faster_rcnn_amd import ops
    Image = pytest.importorskip("PIL.Image")
    frame = CASES[name]
    h, w = frame.shape[:2]
    info = {}
    png = R.encode(frame, bgr=bgr, info=info)
    assert len(png) <= ops.png_bound(h, w, "huffman")
    img = Image.open(io.BytesIO(png))
    img.load()
    assert img.mode == "RGB" and img.size == (w, h) and np.array_equal(np.asarray(img), frame[:, :, ::-1] if bgr else frame)
    pos, idat = 8, b""
    while pos < len(png):
        n, kind = int.from_bytes(png[pos:pos + 4], "big"), png[pos + 4:pos + 8]
        idat += png[pos + 8:pos + 8 + n] if kind == b"IDAT" else b""
        pos += 12 + n
    raw = zlib.decompress(idat)
    assert len(raw) == h * (1 + 3 * w) and [raw[r * (1 + 3 * w)] for r in range(h)] == info["types"]
    assert len(info["forms"]) == -(-h // R.BAND_ROWS)
    if name.startswith("noise"):
        assert set(info["forms"]) == {"stored"}
    if name == "five_filters":
        assert set(info["types"]) == {0, 1, 2, 3, 4}
    if name == "flat_64x100":
        assert len(png) <= frame.nbytes // 8
    if name in ("fibonacci_band", "code_length_ladder_band") and not bgr:
        plan = R.band_plan(np.frombuffer(raw, np.uint8))
        assert info["forms"] == ["dynamic"]
        if name == "fibonacci_band":
            assert max(R.tree_depths(plan["freq"]).values()) > 15 and max(plan["lit_len"]) == 15
        else:
            assert max(R.tree_depths(plan["cl_freq"]).values()) > 7 and max(plan["cl_len"]) == 7


def test_code_lengths_are_complete_and_limited():
    """Random counts, sparse and dense: no length above the limit, the Kraft sum exactly 1, a rarer symbol never shorter."""
    rs = np.random.RandomState(0)
    for trial in range(40):
        n, limit = ((286, 15), (19, 7))[trial % 2]
        freq = (rs.randint(0, 3, n) * rs.randint(1, 1 << rs.randint(1, 16), n) * (rs.rand(n) < rs.rand())).tolist()
        freq[0], freq[n // 2] = 1 + trial, 1
        lengths = R.code_lengths(freq, limit)
        assert all((l > 0) == (f > 0) for l, f in zip(lengths, freq)) and max(lengths) <= limit
        assert sum(1 << (limit - l) for l in lengths if l) == 1 << limit
        used = sorted((f, s) for s, f in enumerate(freq) if f)
        assert all(lengths[a[1]] >= lengths[b[1]] for a, b in zip(used, used[1:]))


def test_size_condition_on_a_photograph():
    """The restatement's file for the VOC fixture is at most 1.10 x the size of Pillow's compress_level=1 file of the same pixels."""
    Image = pytest.importorskip("PIL.Image")
    rgb = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "VOC_test", "JPEGImages", "000005.jpg")).convert("RGB"))
    assert rgb.shape == (375, 500, 3)
    png = R.encode(rgb)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(png))), rgb)
    host = io.BytesIO()
    Image.fromarray(rgb).save(host, format="PNG", compress_level=1)
    ratio = len(png) / len(host.getvalue())
    print("huffman mode: %d bytes, PIL compress_level=1: %d bytes, ratio %.4f" % (len(png), len(host.getvalue()), ratio))
    assert ratio <= 1.10, ratio
