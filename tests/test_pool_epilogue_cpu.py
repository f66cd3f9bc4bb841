"""The pooled-epilogue extension (include/ext/frcnn_hip_pool_epilogue.h) without a GPU: the tile / slot / wave-row walk that
x6_epilogue_vec<.., POOL> (csrc/conv_f32_common.h) is written against, restated in numpy; header, ctypes table and built library agree;
the host query answers per engine, tile code and form; the entry point refuses what the query refuses before anything is launched."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("frcnn_pool_epilogue_version", "frcnn_conv2d_pool_available", "frcnn_conv2d_fwd_h3_pool")
E_ARG, E_UNSUPPORTED = -1, -4

# the <2,1,4,4> form: 256 x 128 tile, four wave-rows of 64 rows, 1 024 threads
BM, BN, HB, WM, NT = 256, 128, 64, 4, 1024
WINDOW = 49
GROUPS = min(BM // WINDOW, NT // BN)


def tiles_m(n_rois):
    return (n_rois + GROUPS - 1) // GROUPS


def walk(n_rois, t, j, h):
    """The rows (of the GEMM) that thread (j, c) of tile t adds in wave-row h, in the order it adds them: the kernel's index arithmetic."""
    m0 = t * GROUPS * WINDOW
    out_row = m0 // WINDOW + j
    if j >= GROUPS or out_row * WINDOW >= n_rois * WINDOW:
        return out_row, []
    lo, hi = max(j * WINDOW, h * HB), min((j + 1) * WINDOW, (h + 1) * HB)
    return out_row, [m0 + r for r in range(lo, hi)]


def test_groups_and_tiles_of_the_benchmark():
    assert GROUPS == 5 and GROUPS * WINDOW == 245 <= BM and GROUPS * BN == 640 <= NT
    assert tiles_m(1200) == 240 and (1200 * WINDOW + BM - 1) // BM == 230


@pytest.mark.parametrize("n_rois", range(1, 13))
def test_every_row_of_every_roi_once_and_in_order(n_rois):
    M = n_rois * WINDOW
    seen = {}
    for t in range(tiles_m(n_rois)):
        for j in range(NT // BN):                           # every thread row of the workgroup, the three beyond the slots too
            rows = []
            for h in range(WM):                             # the wave-rows are walked in order, the register is kept across them
                out_row, part = walk(n_rois, t, j, h)
                assert all(t * GROUPS * WINDOW + h * HB <= m < t * GROUPS * WINDOW + (h + 1) * HB for m in part)      # inside the staged wave-row
                assert all(m - t * GROUPS * WINDOW < GROUPS * WINDOW for m in part)                                  # never the rows behind the tile's RoIs
                rows += part
            if rows:
                assert j < GROUPS and out_row < n_rois and out_row not in seen
                seen[out_row] = rows
            else:
                assert j >= GROUPS or out_row >= n_rois
    assert sorted(seen) == list(range(n_rois))
    for roi, rows in seen.items():
        assert rows == list(range(roi * WINDOW, (roi + 1) * WINDOW))            # 49 rows, ascending, each once
        assert rows[-1] < M


@pytest.mark.parametrize("n_rois", range(1, 13))
def test_residual_requests_cover_the_summed_rows_only(n_rois):
    """The epilogue asks for the residual of tile row r only if r < 245 and m0 + r < M: exactly the rows some sum reads."""
    M = n_rois * WINDOW
    for t in range(tiles_m(n_rois)):
        m0 = t * GROUPS * WINDOW
        asked = {m0 + r for r in range(BM) if r < GROUPS * WINDOW and m0 + r < M}
        summed = {m for j in range(GROUPS) for h in range(WM) for m in walk(n_rois, t, j, h)[1]}
        assert asked == summed


def test_sequential_sum_then_one_division_is_k_pools_arithmetic():
    """acc = 0.0f; 49 additions in raster order; one division: a lone -0.0f pools to +0.0f, and the order matters."""
    v = np.full(WINDOW, -0.0, np.float32)
    acc = np.float32(0.0)
    for x in v:
        acc = np.float32(acc + x)
    assert not np.signbit(acc / np.float32(WINDOW))
    rs = np.random.RandomState(0)
    v = (rs.rand(WINDOW).astype(np.float32) + 1) * np.where(np.arange(WINDOW) % 2 == 0, np.float32(2.0 ** 20), np.float32(1.0)).astype(np.float32)
    fwd = bwd = np.float32(0.0)
    for x in v:
        fwd = np.float32(fwd + x)
    for x in v[::-1]:
        bwd = np.float32(bwd + x)
    assert fwd != bwd


def _desc(_lib, n=1200, hw=7, cin=512, cout=2048, k=1, tile=0, layout=0, **kw):
    d = _lib.ConvDesc(n=n, h=hw, w=hw, cin=cin, cout=cout, kh=k, kw=k, stride=1, pad_top=k // 2, pad_left=k // 2, ho=hw, wo=hw,
                      act=1, ldy=0, ldres=0, tile=tile, layout=layout)
    for key, v in kw.items():
        setattr(d, key, v)
    return d


def test_header_table_and_library_agree():
    from faster_rcnn_amd import _lib
    from faster_rcnn_amd.build import build_library
    ext = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_pool_epilogue.h")).read()
    version = int(re.search(r"#define FRCNN_POOL_EPILOGUE_VERSION (\d+)", ext).group(1))
    assert version == _lib.POOL_EPILOGUE_VERSION == 1 and re.search(r"^ \*   1 = ", ext, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    assert sorted(set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.POOL_EPILOGUE_SIGNATURES) == sorted(NEW_SYMBOLS)
    build_library(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint %s\s*\(([^)]*)\)" % name, code)
        assert m, name
        decls = [d for d in m.group(1).split(",") if d.strip() != "void"]
        restype, argtypes = _lib.POOL_EPILOGUE_SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(decls), name
        for decl, ct in zip(decls, argtypes):
            assert ("*" in decl) == (ct is ctypes.c_void_p), (name, decl)
        assert hasattr(lib, name), name
    assert _lib.load().frcnn_pool_epilogue_version() == version
    # the core ABI and the gathered-residual extension do not know the new symbols and keep their revisions
    core = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name not in core and name not in _lib.SIGNATURES and name not in _lib.EXT_SIGNATURES and name not in _lib.ROI_RES_SIGNATURES
    assert _lib.load().frcnn_version() == _lib.ABI_VERSION == int(re.search(r"#define FRCNN_ABI_VERSION (\d+)", core).group(1))
    assert _lib.load().frcnn_roi_res_version() == _lib.ROI_RES_VERSION == 1


def test_query_answers_per_engine_tile_and_form():
    from faster_rcnn_amd import _lib
    q = _lib.load().frcnn_conv2d_pool_available
    H3, X6, NATIVE = 2, 1, 0
    head = _desc(_lib)                                      # res5c_branch2c of a four-image pass: 58 800 x 2048, k = 512
    assert _lib.load().frcnn_conv2d_h3_config(ctypes.byref(head), 0) == 86
    assert q(ctypes.byref(head), H3, 1, 49) == 1
    assert q(ctypes.byref(head), H3, 0, 49) == 0            # f32 activations
    assert q(ctypes.byref(_desc(_lib, tile=50)), H3, 1, 49) == 1
    assert q(ctypes.byref(_desc(_lib, layout=1)), H3, 1, 49) == 0
    for engine in (NATIVE, X6):
        assert q(ctypes.byref(head), engine, 1, 49) == 0
    for tile in (81, 82, 83, 84, 87, 184, 181):
        assert q(ctypes.byref(_desc(_lib, tile=tile)), H3, 1, 49) == 0, tile
    for tile in (86, 85):
        assert q(ctypes.byref(_desc(_lib, n=11, cin=64, cout=256, tile=tile)), H3, 1, 49) == 1, tile
    assert q(ctypes.byref(_desc(_lib, n=8)), H3, 1, 49) == 0    # a small grid: the policy's 64x64 tiles
    # rows in whole windows only; any window a 256-row tile holds
    assert q(ctypes.byref(head), H3, 1, 48) == 1 and q(ctypes.byref(head), H3, 1, 47) == 0     # 58 800 = 48 x 1 225
    assert q(ctypes.byref(_desc(_lib, n=11, cin=64, cout=256, tile=86)), H3, 1, 48) == 0
    assert q(ctypes.byref(head), H3, 1, 0) == 0 and q(ctypes.byref(head), H3, 1, 300) == 0
    # plane input on a long reduction walks the three-stage ring, which has no pooled form; code 85 keeps the two buffers
    long_k = dict(cin=2048, cout=512)
    ring_off = os.environ.get("FRCNN_H3_RING") == "0"
    assert q(ctypes.byref(_desc(_lib, **long_k)), H3, 1, 49) == (1 if ring_off else 0)
    assert q(ctypes.byref(_desc(_lib, tile=85, **long_k)), H3, 1, 49) == 1
    # 3x3, a stride, strided rows, channel counts the 16-byte pieces do not divide
    assert q(ctypes.byref(_desc(_lib, k=3)), H3, 1, 49) == 0
    assert q(ctypes.byref(_desc(_lib, stride=2, ho=4, wo=4)), H3, 1, 16) == 0
    assert q(ctypes.byref(_desc(_lib, ldy=4096)), H3, 1, 49) == 0 and q(ctypes.byref(_desc(_lib, ldres=4096)), H3, 1, 49) == 0
    assert q(ctypes.byref(_desc(_lib, cout=2050)), H3, 1, 49) == 0 and q(ctypes.byref(_desc(_lib, cin=500)), H3, 1, 49) == 0
    assert q(None, H3, 1, 49) == E_ARG and q(ctypes.byref(head), 7, 1, 49) == E_ARG


def test_refusals_before_any_launch():
    from faster_rcnn_amd import _lib
    lib = _lib.load()
    fwd = lib.frcnn_conv2d_fwd_h3_pool
    one = ctypes.c_void_p(16)                               # never dereferenced: every call below fails its checks first
    planes = _lib.H3Planes(planes=16, exponent=32, status=None)
    good = _desc(_lib, n=11, cin=64, cout=256, tile=86)

    def call(desc=good, x=None, xp=planes, x_amax=one, res_planes=None, mask=None, window=49, y=one, y_planes=None):
        return fwd(ctypes.byref(desc), x, ctypes.byref(xp) if xp is not None else None, x_amax, one, None, None, None,
                   ctypes.byref(res_planes) if res_planes is not None else None, mask, window, y, None,
                   ctypes.byref(y_planes) if y_planes is not None else None, None)
    assert call(y=None) == E_ARG and call(x_amax=None) == E_ARG
    assert call(xp=_lib.H3Planes(planes=20, exponent=32, status=None)) == E_ARG         # misaligned planes
    assert call(xp=_lib.H3Planes(planes=16, exponent=None, status=None)) == E_ARG
    kw = dict(n=11, cin=64, cout=256)
    refused = {
        "f32 in": call(x=one, xp=None), "no input": call(xp=None), "residual planes": call(res_planes=planes), "mask": call(mask=one),
        "plane output": call(y_planes=planes), "rows": call(window=48), "window": call(window=0),
        "3x3": call(desc=_desc(_lib, k=3, tile=86, **kw)), "stride": call(desc=_desc(_lib, tile=86, stride=2, ho=4, wo=4, **kw), window=16),
        "layout": call(desc=_desc(_lib, tile=86, layout=1, **kw)), "cout % 4": call(desc=_desc(_lib, n=11, cin=64, cout=258, tile=86)),
        "ldy": call(desc=_desc(_lib, tile=86, ldy=512, **kw)), "ldres": call(desc=_desc(_lib, tile=86, ldres=512, **kw)),
        "policy": call(desc=_desc(_lib, **kw)),
    }
    for tile in (81, 82, 84, 87, 184, 181):
        refused["tile %d" % tile] = call(desc=_desc(_lib, tile=tile, **kw))
    assert all(v == E_UNSUPPORTED for v in refused.values()), refused
    assert b"conv2d_fwd_h3_pool" in lib.frcnn_last_error()
