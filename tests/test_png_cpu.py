"""The device PNG encoder, the parts that need no GPU: its C-ABI entry points in an extension header of their own
(include/ext/frcnn_hip_png.h), the third ctypes table and the built library; the size bound; annotate_video's command line."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("frcnn_png_version", "frcnn_png_band_rows", "frcnn_png_bound", "frcnn_png_workspace_bytes", "frcnn_png_encode_u8")


def test_header_ctypes_and_library_agree_on_the_png_symbols():
    """The pattern of tests/test_vgg_canvas_cpu.py: every symbol the header declares is in _lib.PNG_SIGNATURES with matching argument
    kinds and exported by the built library, and nothing else is in that table; the revisions agree; the core header, its table and the
    VGG16 canvas table do not know the new symbols."""
    from faster_rcnn_amd import _lib
    from faster_rcnn_amd.build import build_library
    ext = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_png.h")).read()
    version = int(re.search(r"#define FRCNN_PNG_VERSION (\d+)", ext).group(1))
    assert version == _lib.PNG_VERSION == 1 and re.search(r"^ \*   1 = ", ext, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    assert sorted(set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.PNG_SIGNATURES) == sorted(NEW_SYMBOLS)
    build_library(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        m = re.search(r"\b(int|size_t) %s\s*\(([^)]*)\)" % name, code)
        assert m, name
        decls = [d for d in m.group(2).split(",") if d.strip() != "void"]
        restype, argtypes = _lib.PNG_SIGNATURES[name]
        assert restype is {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[m.group(1)] and len(argtypes) == len(decls), name
        for decl, ct in zip(decls, argtypes):                            # pointers are pointers, sizes are sizes, ints are ints
            assert ("*" in decl) == (ct is ctypes.c_void_p), (name, decl)
            assert ("size_t" in decl) == (ct is ctypes.c_size_t), (name, decl)
        assert hasattr(lib, name), name
    assert _lib.load().frcnn_png_version() == version
    core = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    assert not any(name in core or name in _lib.SIGNATURES or name in _lib.EXT_SIGNATURES for name in NEW_SYMBOLS)
    assert "png" not in core.lower()
    assert _lib.load().frcnn_version() == _lib.ABI_VERSION == int(re.search(r"#define FRCNN_ABI_VERSION (\d+)", core).group(1))
    assert _lib.load().frcnn_vgg_canvas_version() == _lib.VGG_CANVAS_VERSION


def test_band_rows_constant():
    from faster_rcnn_amd import _lib, ops
    assert _lib.load().frcnn_png_band_rows() == ops.PNG_BAND_ROWS >= 1


def test_png_bound():
    """Monotone in both sides; never below the filtered stream plus the smallest framing (signature, IHDR, one empty IDAT, IEND: 57
    bytes); within 2 % (+ 4096) of the filtered stream for real frame sizes, which keeps the read-back copy the size of the raw one."""
    import pytest
    from faster_rcnn_amd import ops
    from faster_rcnn_amd._lib import FrcnnError
    sides = [1, 2, 3, 7, 8, 9, 63, 64, 65, 375, 600, 1000, 1242, 21845, 21846]
    for h in sides:
        prev = 0
        for w in sides:
            b = ops.png_bound(h, w)
            assert b > prev and b >= h * (1 + 3 * w) + 57, (h, w)
            prev = b
    for w in sides:
        prev = 0
        for h in sides:
            b = ops.png_bound(h, w)
            assert b > prev, (h, w)
            prev = b
    for h, w in ((375, 1242), (600, 1000)):
        assert ops.png_bound(h, w) <= h * (1 + 3 * w) * 1.02 + 4096
    for h, w in ((0, 5), (5, 0), (-1, 5), (1 << 20, 1 << 20)):              # (the last: a filtered stream past 2 GiB)
        with pytest.raises(FrcnnError):
            ops.png_bound(h, w)
    assert ops.png_workspace_bytes(375, 1242) >= ops.png_bound(375, 1242) - 66


def test_command_line():
    from faster_rcnn_amd import annotate_video
    p = annotate_video.build_parser()
    assert p.parse_args(["a", "b", "c"]).png_encoder == "host"
    assert p.parse_args(["a", "b", "c", "--png_encoder", "device"]).png_encoder == "device"
    assert p.parse_args(["a", "b", "c", "--png_encoder", "host"]).png_encoder == "host"
    import pytest
    with pytest.raises(SystemExit):
        p.parse_args(["a", "b", "c", "--png_encoder", "gpu"])
