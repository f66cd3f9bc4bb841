"""The f32 conv launch policy as a table: every host-side policy query of the library over a fixed grid of descriptors, against
tests/golden/conv_policy_table.npz (written by tests/golden/make_conv_policy_table.py).  The queries are pure host code, so the
table pins the tile choice, split-K / stream-K and workspace rules of all three f32 engines without a GPU."""
import ctypes
import hashlib
import itertools
import os

import numpy as np
import pytest

pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "golden", "conv_policy_table.npz")

# the policy's dev knobs: a table recorded with the defaults says nothing about a run that overrides one
KNOBS = ("FRCNN_FORCE_TILE", "FRCNN_GROUP_M", "FRCNN_SCALAR_EPILOGUE", "FRCNN_SK_SHARED", "FRCNN_X6_SK128_MIN",
         "FRCNN_H3_BIG_MIN_TILES_SHARED", "FRCNN_H3_SHARED_SMALL", "FRCNN_H3_SHARED_SMALL_ROWS", "FRCNN_WGRAD_BIG",
         "FRCNN_WGRAD_BIG_BF16", "FRCNN_WGRAD_TARGET", "FRCNN_WGRAD_TARGET_BIG", "FRCNN_WGRAD_TARGET_X6")

# every tile code the library knows, and a few with a hundreds digit (forced split-K factor)
TILES = [1, 2, 3, 4, 11, 12, 13, 14, 21, 22, 23, 24, 25, 26, 30, 32, 41, 42, 43, 44, 45, 46, 47, 48, 61, 62,
         71, 72, 73, 74, 75, 76, 77, 78, 81, 82, 83, 84, 85, 86, 87, 88,
         100, 150, 300, 322, 323, 361, 374, 378, 484, 488, 950, 1623, 1688, 4000, 4023]
N1 = (0, 64, 128, 512)
CODES = (["config"] + [f"x6_config_{n1}" for n1 in N1] + [f"h3_config_{n1}" for n1 in N1]
         + ["dual_config_ws0", "dual_config_ws1"] + [f"engine_{p}_ws{w}" for p in (0, 1, 2) for w in (0, 1)])
BYTES = ["ws_native", "ws_dual", "ws_x6", "ws_h3", "ws_wgrad"]
COLUMNS = CODES + BYTES


def _shape(n, h, w, cin, cout, k, stride, layout, tile):
    ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride        # 'same' padding
    ph, pw = max((ho - 1) * stride + k - h, 0), max((wo - 1) * stride + k - w, 0)
    return (n, h, w, cin, cout, k, k, stride, ph // 2, pw // 2, ho, wo, 0, 0, 0, tile, layout)


def grid():
    """int32 [N][17] frcnn_conv_desc rows: every shape of the grid with tiles 0 and 50, plus four codes of TILES in rotation."""
    rows = []
    shapes = itertools.product((1, 4, 64, 300), ((7, 7), (14, 14), (38, 63), (75, 125)), (0, 1),
                               (3, 4, 48, 64, 256, 1024, 2048), (36, 64, 101, 256, 512, 2048), (1, 3, 7), (1, 2))
    for i, (n, (h, w), layout, cin, cout, k, stride) in enumerate(shapes):
        for tile in [0, 50] + [TILES[(4 * i + j) % len(TILES)] for j in range(4)]:
            rows.append(_shape(n, h, w, cin, cout, k, stride, layout, tile))
    # past the limits: inputs over 2 GiB (v1 kernels only, no h3 planes), filters of 36 and 81 taps, one very tall 1x1
    for (n, h, w, cin, cout, k), layout, tile in itertools.product(
            [(64, 128, 128, 1024, 256, 1), (300, 38, 63, 1024, 512, 3), (4, 38, 63, 256, 256, 6), (1, 75, 125, 64, 64, 9),
             (16, 600, 1000, 64, 64, 1), (2, 600, 1000, 64, 256, 3)], (0, 1), [0, 50] + TILES):
        rows.append(_shape(n, h, w, cin, cout, k, 1, layout, tile))
    return np.array(rows, np.int32)


def query(lib, descs):
    """int64 [N][len(COLUMNS)]: the library's answers for every descriptor."""
    from faster_rcnn_amd._lib import ConvDesc
    out = np.zeros((len(descs), len(COLUMNS)), np.int64)
    d = ConvDesc()
    p = ctypes.byref(d)
    for i, row in enumerate(descs.tolist()):
        ctypes.memmove(p, (ctypes.c_int32 * 17)(*row), ctypes.sizeof(d))
        out[i] = ([lib.frcnn_conv2d_config(p)] + [lib.frcnn_conv2d_x6_config(p, n1) for n1 in N1]
                  + [lib.frcnn_conv2d_h3_config(p, n1) for n1 in N1]
                  + [lib.frcnn_conv2d_dual_config(p, 0), lib.frcnn_conv2d_dual_config(p, 1)]
                  + [lib.frcnn_conv2d_engine(p, pref, ws) for pref in (0, 1, 2) for ws in (0, 1)]
                  + [lib.frcnn_conv2d_workspace_bytes(p), lib.frcnn_conv2d_dual_workspace_bytes(p),
                     lib.frcnn_conv2d_x6_workspace_bytes(p), lib.frcnn_conv2d_h3_workspace_bytes(p),
                     lib.frcnn_conv2d_wgrad_workspace_bytes(p)])
    return out


def grid_digest(descs):
    return hashlib.sha256(descs.tobytes()).hexdigest()


def test_policy_table_matches_the_recorded_one():
    set_knobs = [k for k in KNOBS if k in os.environ]
    if set_knobs:
        pytest.skip(f"policy dev knobs set: {', '.join(set_knobs)}")
    from faster_rcnn_amd import _lib
    descs = grid()
    got = query(_lib.load(), descs)
    rec = np.load(TABLE)
    assert list(rec["columns"]) == COLUMNS
    assert str(rec["grid_sha256"]) == grid_digest(descs), "the descriptor grid changed: record the table again from the parent commit"
    want = np.concatenate([rec["codes"], rec["bytes"]]).T
    assert want.shape == got.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"policy differs in {len(bad)} places: " + "; ".join(
        f"desc {descs[i].tolist()} {COLUMNS[j]}: {got[i, j]} != {want[i, j]}" for i, j in bad[:10])
