"""The gathered-residual extension (include/ext/frcnn_hip_roi_res.h) without a GPU: header, ctypes table and built library agree; the host
query frcnn_conv2d_roi_res_available answers per engine, tile code and form; bad arguments are refused before anything is launched."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("frcnn_roi_res_version", "frcnn_roi_tap_table", "frcnn_conv2d_roi_res_available", "frcnn_conv2d_fwd_h3_roi_res")
E_ARG, E_UNSUPPORTED = -1, -4


def _desc(_lib, n=1200, hw=7, cin=512, cout=2048, k=1, tile=0, layout=0, **kw):
    d = _lib.ConvDesc(n=n, h=hw, w=hw, cin=cin, cout=cout, kh=k, kw=k, stride=1, pad_top=k // 2, pad_left=k // 2, ho=hw, wo=hw,
                      act=1, ldy=0, ldres=0, tile=tile, layout=layout)
    for key, v in kw.items():
        setattr(d, key, v)
    return d


def test_header_table_and_library_agree():
    from faster_rcnn_amd import _lib
    from faster_rcnn_amd.build import build_library
    ext = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_roi_res.h")).read()
    version = int(re.search(r"#define FRCNN_ROI_RES_VERSION (\d+)", ext).group(1))
    assert version == _lib.ROI_RES_VERSION == 1 and re.search(r"^ \*   1 = ", ext, flags=re.M)
    assert int(re.search(r"#define FRCNN_ROI_TAP_BYTES (\d+)", ext).group(1)) == _lib.ROI_TAP_BYTES == 32
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    assert sorted(set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.ROI_RES_SIGNATURES) == sorted(NEW_SYMBOLS)
    build_library(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint %s\s*\(([^)]*)\)" % name, code)
        assert m, name
        decls = [d for d in m.group(1).split(",") if d.strip() != "void"]
        restype, argtypes = _lib.ROI_RES_SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(decls), name
        for decl, ct in zip(decls, argtypes):
            assert ("*" in decl) == (ct is ctypes.c_void_p), (name, decl)
            assert ("float " in decl and "*" not in decl) == (ct is ctypes.c_float), (name, decl)
        assert hasattr(lib, name), name
    assert _lib.load().frcnn_roi_res_version() == version
    assert ctypes.sizeof(_lib.RoiRes) == 32
    # the core ABI does not know the new symbols and keeps its revision
    core = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name not in core and name not in _lib.SIGNATURES and name not in _lib.EXT_SIGNATURES
    assert _lib.load().frcnn_version() == _lib.ABI_VERSION == int(re.search(r"#define FRCNN_ABI_VERSION (\d+)", core).group(1))


def test_query_answers_per_engine_tile_and_form():
    from faster_rcnn_amd import _lib
    q = _lib.load().frcnn_conv2d_roi_res_available
    H3, X6, NATIVE = 2, 1, 0
    head = _desc(_lib)                                      # res5a_branch2c of a four-image pass: 58 800 x 2048, k = 512
    assert _lib.load().frcnn_conv2d_h3_config(ctypes.byref(head), 0) == 86
    assert q(ctypes.byref(head), H3, 1) == 1 and q(ctypes.byref(head), H3, 0) == 1
    assert q(ctypes.byref(_desc(_lib, layout=1)), H3, 1) == 1
    assert q(ctypes.byref(_desc(_lib, tile=50)), H3, 1) == 1
    for engine in (NATIVE, X6):
        assert q(ctypes.byref(head), engine, 0) == 0 and q(ctypes.byref(head), engine, 1) == 0
    for tile in (81, 82, 83, 84, 87, 184, 181):
        assert q(ctypes.byref(_desc(_lib, tile=tile)), H3, 0) == 0, tile
    for tile in (86, 85):
        assert q(ctypes.byref(_desc(_lib, n=11, cin=64, cout=256, tile=tile)), H3, 1) == 1, tile
    assert q(ctypes.byref(_desc(_lib, n=8)), H3, 1) == 0    # a small grid: the policy's 64x64 tiles
    # plane input on a long reduction walks the three-stage ring, which has no gathered residual; code 85 keeps the two buffers
    long_k = dict(cin=2048, cout=512)
    ring_off = os.environ.get("FRCNN_H3_RING") == "0"
    assert q(ctypes.byref(_desc(_lib, **long_k)), H3, 1) == (1 if ring_off else 0)
    assert q(ctypes.byref(_desc(_lib, **long_k)), H3, 0) == 1 and q(ctypes.byref(_desc(_lib, tile=85, **long_k)), H3, 1) == 1
    # strided rows, channel counts the 16-byte pieces do not divide, more than 32 taps
    assert q(ctypes.byref(_desc(_lib, ldy=4096)), H3, 1) == 0 and q(ctypes.byref(_desc(_lib, ldres=4096)), H3, 1) == 0
    assert q(ctypes.byref(_desc(_lib, cout=2050)), H3, 1) == 0 and q(ctypes.byref(_desc(_lib, cin=500)), H3, 1) == 0
    assert q(ctypes.byref(_desc(_lib, k=7)), H3, 0) == 0
    assert q(None, H3, 0) == E_ARG and q(ctypes.byref(head), 7, 0) == E_ARG


def test_bad_arguments_are_refused_before_any_launch():
    from faster_rcnn_amd import _lib
    lib = _lib.load()
    tab = lib.frcnn_roi_tap_table
    one = ctypes.c_void_p(16)                               # never dereferenced: every call below fails its checks first
    assert tab(9, 13, 255, one, 11, 6, 2, 7, 0, one, None) == E_ARG            # c % 4
    assert tab(0, 13, 256, one, 11, 6, 2, 7, 0, one, None) == E_ARG
    assert tab(9, 13, 256, one, 11, 6, 2, 7, 2, one, None) == E_ARG            # layout
    assert tab(9, 13, 256, one, 13, 6, 2, 7, 0, one, None) == E_ARG            # more RoIs than n_maps * n_per_img
    assert tab(9, 13, 256, one, 11, 6, 0, 7, 0, one, None) == E_ARG
    assert tab(9, 13, 256, None, 11, 6, 2, 7, 0, one, None) == E_ARG
    assert tab(9, 13, 256, one, 11, 6, 2, 7, 0, ctypes.c_void_p(8), None) == E_ARG     # table alignment
    assert tab(4096, 4096, 2048, one, 11, 0, 1, 7, 0, one, None) == E_UNSUPPORTED      # a map over 2 GiB
    assert tab(9, 13, 256, None, 0, 6, 2, 7, 0, None, None) == 0                       # no RoIs: nothing to do
    assert b"roi_tap_table" in lib.frcnn_last_error()
    fwd = lib.frcnn_conv2d_fwd_h3_roi_res
    d = _desc(_lib, n=11, cin=64, cout=256, tile=86)

    def call(res, desc=d, x=one, x_amax=one, y=one):
        return fwd(ctypes.byref(desc), x, None, x_amax, one, None, None, ctypes.byref(res) if res is not None else None, None, y, None, None, 0.0, 0.0, None)
    good = dict(map=16, taps=32, fill=48, map_rows=234, reserved=0)
    for bad in (dict(map=None), dict(taps=None), dict(map_rows=0), dict(reserved=1), dict(map=20), dict(taps=40), dict(fill=52)):
        assert call(_lib.RoiRes(**{**good, **bad})) == E_ARG, bad
    assert call(_lib.RoiRes(**good), x_amax=None) == E_ARG
    assert call(_lib.RoiRes(**good), y=None) == E_ARG                                   # no output
    for tile in (81, 82, 84, 87):
        assert call(_lib.RoiRes(**good), desc=_desc(_lib, n=11, cin=64, cout=256, tile=tile)) == E_UNSUPPORTED, tile
    assert call(_lib.RoiRes(**good), desc=_desc(_lib, n=11, cin=64, cout=256, tile=86, ldy=512)) == E_UNSUPPORTED
    assert b"roi_res" in lib.frcnn_last_error()
