"""VGG16 canvas passes, the parts that need no GPU: the five-level chain of true extents (nets.VggExtents), the new C-ABI entry
points in the extension header (include/ext/frcnn_hip_vgg_canvas.h), the ctypes table and the built library, and the planner's canvas classes holding every member at offset 0."""
import collections
import ctypes
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("frcnn_vgg_canvas_version", "frcnn_pool2d_fwd_extents", "frcnn_pool2d_fwd_bf16_extents", "frcnn_vgg_conv1_bf16_fwd_extents")

# the entry-point test's list (tests/test_vgg_canvas_gpu.py): seven geometries, even and odd sides, all at most 330 x 512
ENTRY_SIZES = [(320, 480), (318, 470), (306, 451), (321, 466), (310, 480), (289, 449), (330, 512)]


def entry_histogram(per_size=2):
    return collections.Counter({s: per_size for s in ENTRY_SIZES})


def test_vgg_extents_chain():
    """Every level is the floor-half of the one before; the last is the reference's conv map size (vgg.py:60-61: h // 16, w // 16) and the
    oracle's, for every height in 16..1100 and a few hundred widths."""
    from faster_rcnn_amd import nets, vgg
    from oracle import np_ref
    assert nets.VggExtents.LEVELS == 5 and nets.VggExtents.CONV_LEVEL == 4 and nets.VggBase.extents_class is nets.VggExtents
    assert nets.Extents.LEVELS == 3 and nets.Extents.CONV_LEVEL == 2 and nets.ResNetBase.extents_class is nets.Extents
    widths = sorted(set(range(16, 1101, 7)) | set(range(16, 80)) | set(range(990, 1101)))
    assert len(widths) > 300
    for h in range(16, 1101):
        for w in widths:
            lv = nets.VggExtents.levels_of(h, w)
            assert len(lv) == 5 and lv[0] == (h, w)
            for a, b in zip(lv, lv[1:]):
                assert b == (a[0] // 2, a[1] // 2)
            assert lv[4] == np_ref.conv_dims_vgg(h, w) == (h // 16, w // 16) == vgg.get_conv_rows_cols(h, w)
    # an image sits in the corner of its canvas whatever its parities; a ResNet image behind the zero row / column of an odd side
    assert nets.VggExtents.offset_of(321, 479) == (0, 0) and nets.Extents.offset_of(321, 480) == (1, 0)
    # the ResNet chain is what it was
    from faster_rcnn_amd import resnet
    assert len(nets.Extents.levels_of(600, 1000)) == 3 and nets.Extents.levels_of(601, 999)[2] == tuple(resnet.get_conv_rows_cols(601, 999))


def test_networks_take_extents():
    from faster_rcnn_amd import nets
    for fn in (nets.VggBase.__call__, nets.ResNetBase.__call__):
        p = inspect.signature(fn).parameters
        assert "extents" in p and p["extents"].default is None, fn.__qualname__


def test_header_ctypes_and_library_agree_on_the_new_symbols():
    """The pattern of tests/test_abi.py on the extension header: every symbol it declares is in _lib.EXT_SIGNATURES with matching
    argument kinds and exported by the built library, and nothing else is in that table; the revisions agree; the core header,
    its revision and its table do not know the new symbols (additions only, in a header of their own)."""
    from faster_rcnn_amd import _lib
    from faster_rcnn_amd.build import build_library
    ext = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_vgg_canvas.h")).read()
    version = int(re.search(r"#define FRCNN_VGG_CANVAS_VERSION (\d+)", ext).group(1))
    assert version == _lib.VGG_CANVAS_VERSION >= 1 and re.search(r"^ \*   1 = ", ext, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    assert sorted(set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.EXT_SIGNATURES) == sorted(NEW_SYMBOLS)
    build_library(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint %s\s*\(([^)]*)\)" % name, code)
        assert m, name
        decls = [d for d in m.group(1).split(",") if d.strip() != "void"]
        restype, argtypes = _lib.EXT_SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(decls), name
        for decl, ct in zip(decls, argtypes):                            # pointers are pointers, ints are ints
            assert ("*" in decl) == (ct is ctypes.c_void_p), (name, decl)
        assert hasattr(lib, name), name
    assert _lib.load().frcnn_vgg_canvas_version() == version
    core = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    assert not any(name in core or name in _lib.SIGNATURES for name in NEW_SYMBOLS)
    assert _lib.load().frcnn_version() == _lib.ABI_VERSION == int(re.search(r"#define FRCNN_ABI_VERSION (\d+)", core).group(1))


def test_planned_canvases_hold_every_member_at_offset_zero():
    """plan_canvas_classes on a VOC-like histogram (short side 600 or long side 1000 after util.resize_imgs, odd sides among them): few
    classes, and every geometry fits its class's canvas from the corner -- which is where a VGG16 frame sits."""
    from faster_rcnn_amd import entry
    rs = np.random.RandomState(5)
    counts = collections.Counter()
    for _ in range(400):
        src_w, src_h = 500, int(rs.choice([375, 333, 334, 332, 375, 400, 281, 500, 357, 374]))
        if rs.rand() < 0.25:
            src_w, src_h = src_h, src_w
        ratio = min(600.0 / min(src_h, src_w), 1000.0 / max(src_h, src_w))
        counts[(int(round(src_h * ratio)), int(round(src_w * ratio)))] += 1
    assert len(counts) >= 8 and any(h & 1 or w & 1 for h, w in counts)
    plan = entry.plan_canvas_classes(counts)
    assert set(plan) == set(counts) and 1 <= len(set(plan.values())) <= entry.CANVAS_MAX_CLASSES
    from faster_rcnn_amd import nets
    for (h, w), (hc, wc) in plan.items():
        oy, ox = nets.VggExtents.offset_of(h, w)                          # where entry._canvas_frame puts a VGG16 frame: (0, 0)
        assert (oy, ox) == (0, 0) and hc % 2 == 0 and wc % 2 == 0 and h + oy <= hc and w + ox <= wc
        assert nets.VggExtents.levels_of(h, w)[4] <= nets.VggExtents.levels_of(hc, wc)[4]      # ... and its map inside the canvas's
    assert entry.plan_canvas_classes(counts) == plan                      # deterministic
    # the list of the GPU entry-point test: at most three classes, written down here so that a planner change shows on the CPU first
    small = entry.plan_canvas_classes(entry_histogram())
    assert len(set(small.values())) <= 3, small
    for (h, w), (hc, wc) in small.items():
        assert h <= hc and w <= wc and h <= 330 and w <= 512
