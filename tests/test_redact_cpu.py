"""The redaction rule without a GPU: properties and hand-worked literals of its numpy restatement (tests/redact_ref.py), annotate_video's
command line (``redact_from_args``), and the extension's header (include/ext/frcnn_hip_redact.h) against its ctypes table."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import redact_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pixels(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def some_dets(h, w, n, seed, classes=4):
    rs = np.random.RandomState(seed)
    x = rs.randint(-w // 4, w + w // 4 + 1, (n, 2))
    y = rs.randint(-h // 4, h + h // 4 + 1, (n, 2))
    return np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1), rs.randint(0, classes, n)


MODES = [("fill", 0), ("pixelate", 5), ("blur", 3)]


# ----------------------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("mode,size", MODES)
def test_row_order_does_not_matter(mode, size):
    frame = pixels(37, 53, 1)
    bbox, cls = some_dets(37, 53, 9, 2)
    table = np.array([0, 1, 1, 0], dtype=np.uint8)
    want = R.redact(frame, bbox, cls, 9, table, mode, size, margin=2)
    assert (want != frame).any()
    for seed in range(3):
        p = np.random.RandomState(seed).permutation(9)
        assert np.array_equal(R.redact(frame, bbox[p], cls[p], 9, table, mode, size, margin=2), want)


@pytest.mark.parametrize("mode,size", MODES)
def test_unmasked_pixels_are_untouched_and_dead_rows_unread(mode, size):
    frame = pixels(40, 60, 3)
    bbox, cls = some_dets(40, 60, 12, 4)
    table = np.array([1, 0, 1, 1], dtype=np.uint8)
    m = R.mask(40, 60, bbox, cls, 5, table)
    out = R.redact(frame, bbox, cls, 5, table, mode, size)
    assert m.any() and not m.all()
    assert np.array_equal(out[~m], frame[~m])
    assert np.array_equal(out[m], R.replacement(frame, mode, size)[m])
    assert np.array_equal(m, R.mask(40, 60, bbox[:5], cls[:5], 5, table))         # rows >= n_dets are not read
    assert not R.mask(40, 60, bbox, cls, 0, table).any()


def test_fill_is_zero_exactly_on_the_mask():
    frame = np.maximum(pixels(30, 30, 5), 1)                               # no zero in the source
    bbox, cls = some_dets(30, 30, 6, 6)
    table = np.ones(4, dtype=np.uint8)
    out = R.redact(frame, bbox, cls, 6, table, "fill")
    assert np.array_equal((out == 0).all(axis=2), R.mask(30, 30, bbox, cls, 6, table))
    assert np.array_equal((out == 0).any(axis=2), (out == 0).all(axis=2))


@pytest.mark.parametrize("P", [2, 5, 16, 64])
def test_a_pixelated_cell_is_constant(P):
    frame = pixels(33, 70, 7)
    out = R.pixelated(frame, P)
    for y0 in range(0, 33, P):
        for x0 in range(0, 70, P):
            cell = out[y0:y0 + P, x0:x0 + P].reshape(-1, 3)
            assert (cell == cell[0]).all()
            src = frame[y0:y0 + P, x0:x0 + P].reshape(-1, 3).astype(np.int64)
            assert np.array_equal(cell[0], (src.sum(axis=0) + len(src) // 2) // len(src))


@pytest.mark.parametrize("mode,size", [("pixelate", 2), ("pixelate", 64), ("blur", 1), ("blur", 32)])
def test_a_uniform_frame_is_a_fixed_point(mode, size):
    for value in (0, 1, 127, 254, 255):
        frame = np.empty((9, 13, 3), dtype=np.uint8)
        frame[...] = (value, 255 - value, value // 2)
        assert np.array_equal(R.replacement(frame, mode, size), frame)
        out = R.redact(frame, [[-5, -5, 50, 50]], [0], 1, [1], mode, size)
        assert np.array_equal(out, frame)
    frame = np.zeros((9, 13, 3), dtype=np.uint8)
    assert np.array_equal(R.redact(frame, [[2, 2, 5, 5]], [0], 1, [1], "fill"), frame)


def test_a_box_outside_masks_nothing_and_a_crossing_box_is_clipped():
    h, w = 20, 30
    table = [1]
    for box in ([-9, 3, -1, 8], [30, 3, 40, 8], [3, -9, 8, -1], [3, 20, 8, 33]):
        assert not R.mask(h, w, [box], [0], 1, table).any(), box
    for box, rows, cols in (([-4, 2, 3, 5], slice(2, 6), slice(0, 4)), ([25, 2, 40, 5], slice(2, 6), slice(25, 30)),
                            ([3, -7, 6, 1], slice(0, 2), slice(3, 7)), ([3, 18, 6, 99], slice(18, 20), slice(3, 7))):
        want = np.zeros((h, w), dtype=bool)
        want[rows, cols] = True
        assert np.array_equal(R.mask(h, w, [box], [0], 1, table), want), box
    assert R.mask(h, w, [[-100, -100, 100, 100]], [0], 1, table).all()
    # inverted corners are the same box; x1 == x2 is one column; a class off the table, or out of range, is not redacted
    assert np.array_equal(R.mask(h, w, [[9, 12, 4, 6]], [0], 1, table), R.mask(h, w, [[4, 6, 9, 12]], [0], 1, table))
    assert R.mask(h, w, [[7, 3, 7, 9]], [0], 1, table).sum() == 7
    assert not R.mask(h, w, [[4, 6, 9, 12]], [1], 1, [1, 0]).any()
    assert not R.mask(h, w, [[4, 6, 9, 12]] * 2, [-1, 5], 2, [1, 1]).any()


@pytest.mark.parametrize("margin", [0, 1, 3, 64])
def test_margin_grows_the_mask_by_that_many_pixels_and_clips(margin):
    h, w = 40, 50
    m = R.mask(h, w, [[20, 10, 26, 13]], [0], 1, [1], margin)
    want = np.zeros((h, w), dtype=bool)
    want[max(10 - margin, 0):min(13 + margin, h - 1) + 1, max(20 - margin, 0):min(26 + margin, w - 1) + 1] = True
    assert np.array_equal(m, want)
    assert m.sum() == (min(13 + margin, h - 1) - max(10 - margin, 0) + 1) * (min(26 + margin, w - 1) - max(20 - margin, 0) + 1)
    # a box just outside comes into the frame with a margin that reaches it
    assert R.mask(h, w, [[-3, 5, -2, 6]], [0], 1, [1], margin).any() == (margin >= 2)


# ----------------------------------------------------------------------------------------------------------- hand literals
def test_pixelate_literal_4x4_P2():
    g = np.array([[0, 1, 10, 20],
                  [2, 3, 30, 41],
                  [255, 255, 7, 7],
                  [255, 254, 7, 8]], dtype=np.uint8)
    frame = np.stack([g, g, g], axis=2)
    frame[:, :, 1] = 255 - g
    # cells: (0+1+2+3 + 2) // 4 = 2 (1.5 rounds up); (10+20+30+41 + 2) // 4 = 25 (25.25); (1019 + 2) // 4 = 255 (254.75); (29 + 2) // 4 = 7
    want_g = np.array([[2, 2, 25, 25],
                       [2, 2, 25, 25],
                       [255, 255, 7, 7],
                       [255, 255, 7, 7]], dtype=np.uint8)
    # the second channel: (255+254+253+252 + 2) // 4 = 254 (253.5 up); (245+235+225+214 + 2) // 4 = 230; (0+0+0+1 + 2) // 4 = 0; (991 + 2) // 4 = 248
    want_1 = np.array([[254, 254, 230, 230],
                       [254, 254, 230, 230],
                       [0, 0, 248, 248],
                       [0, 0, 248, 248]], dtype=np.uint8)
    out = R.pixelated(frame, 2)
    assert np.array_equal(out[:, :, 0], want_g) and np.array_equal(out[:, :, 2], want_g) and np.array_equal(out[:, :, 1], want_1)
    # only the masked pixel of a cell changes: box (1,1)-(2,2)
    red = R.redact(frame, [[1, 1, 2, 2]], [0], 1, [1], "pixelate", 2)
    assert red[1, 1, 0] == 2 and red[1, 2, 0] == 25 and red[2, 1, 0] == 255 and red[2, 2, 0] == 7
    keep = np.ones((4, 4), dtype=bool)
    keep[1:3, 1:3] = False
    assert np.array_equal(red[keep], frame[keep])


def test_blur_literal_1x5_r1():
    row = np.array([0, 10, 20, 31, 255], dtype=np.uint8)
    frame = np.repeat(row[None, :, None], 3, axis=2)
    # H, k = 3, x clamped: (0+0+10 + 1) // 3 = 3; (0+10+20 + 1) // 3 = 10; (10+20+31 + 1) // 3 = 20; (20+31+255 + 1) // 3 = 102;
    # (31+255+255 + 1) // 3 = 180.  The one row is its own neighbour above and below: R = (3 H + 1) // 3 = H.
    want = np.array([3, 10, 20, 102, 180], dtype=np.uint8)
    out = R.blurred(frame, 1)
    assert out.shape == (1, 5, 3) and all(np.array_equal(out[0, :, c], want) for c in range(3))
    # a column of the same numbers: the vertical stage alone
    col = np.repeat(row[:, None, None], 3, axis=2)
    assert np.array_equal(R.blurred(col, 1)[:, 0, 0], want)
    # a window wider than the frame: every tap beyond an end repeats the end; r = 3, k = 7, x = 0: (4 * 0 + 10 + 20 + 31 + 3) // 7 = 9
    assert R.blurred(frame, 3)[0, 0, 0] == 9 and R.blurred(frame, 3)[0, 4, 0] == (10 + 20 + 31 + 4 * 255 + 3) // 7


# ----------------------------------------------------------------------------------------------------------- the command line
def _args(*argv):
    from faster_rcnn_amd import annotate_video
    return annotate_video.build_parser().parse_args(["rpn.npz", "det.npz", "frames"] + list(argv))


def test_redact_from_args():
    from faster_rcnn_amd.annotate_video import redact_from_args
    from faster_rcnn_amd.data.voc_data_helpers import KITTI_CLASS_MAPPING, VOC_CLASS_MAPPING
    for mapping, pair, foreign in ((VOC_CLASS_MAPPING, ("person", "car"), "Cyclist"), (KITTI_CLASS_MAPPING, ("Cyclist", "DontCare"), "aeroplane")):
        assert all(n in mapping for n in pair) and foreign not in mapping
        assert redact_from_args(_args(), mapping) is None
        assert redact_from_args(_args("--no_draw"), mapping) is None and _args("--no_draw").no_draw and not _args().no_draw
        assert redact_from_args(_args("--redact", "all"), mapping) == ("all", "pixelate", 16, 0)
        assert redact_from_args(_args("--redact", ",".join(pair)), mapping) == (pair, "pixelate", 16, 0)
        assert redact_from_args(_args("--redact", pair[0], "--redact_mode", "blur"), mapping) == ((pair[0],), "blur", 12, 0)
        assert redact_from_args(_args("--redact", "all", "--redact_mode", "blur", "--redact_size", "32", "--redact_margin", "7"), mapping) \
            == ("all", "blur", 32, 7)
        assert redact_from_args(_args("--redact", "all", "--redact_mode", "pixelate", "--redact_size", "2"), mapping) == ("all", "pixelate", 2, 0)
        assert redact_from_args(_args("--redact", "all", "--redact_mode", "fill"), mapping) == ("all", "fill", 0, 0)
        # unknown names: the message lists the valid ones
        with pytest.raises(ValueError) as e:
            redact_from_args(_args("--redact", pair[0] + "," + foreign), mapping)
        assert foreign in str(e.value) and all(n in str(e.value) for n in mapping if n != "bg")
        with pytest.raises(ValueError):
            redact_from_args(_args("--redact", "bg"), mapping)             # the background is no class to hide
        # settings of the redaction without it
        for extra in (("--redact_mode", "blur"), ("--redact_mode", "pixelate"), ("--redact_size", "8"), ("--redact_margin", "0")):
            with pytest.raises(ValueError) as e:
                redact_from_args(_args(*extra), mapping)
            assert extra[0] in str(e.value) and "--redact" in str(e.value)
        # sizes out of range for the mode
        for mode, size in (("pixelate", 1), ("pixelate", 65), ("pixelate", 0), ("blur", 0), ("blur", 33), ("fill", 1), ("fill", 16)):
            with pytest.raises(ValueError) as e:
                redact_from_args(_args("--redact", "all", "--redact_mode", mode, "--redact_size", str(size)), mapping)
            assert mode in str(e.value)
        with pytest.raises(ValueError):
            redact_from_args(_args("--redact", "all", "--redact_size", "65"), mapping)       # (the default mode's range)
        with pytest.raises(ValueError):
            redact_from_args(_args("--redact", "all", "--redact_margin", "-1"), mapping)


def test_parser_defaults_are_unchanged():
    a = _args()
    assert (a.redact, a.redact_mode, a.redact_size, a.redact_margin, a.no_draw) == (None, None, None, None, False)
    assert (a.frame_format, a.png_encoder, a.out_video) == ("png", "host", None)


# ----------------------------------------------------------------------------------------------------------- header and binding
def test_header_binding_and_library_agree():
    from faster_rcnn_amd import _lib, ops
    from faster_rcnn_amd.build import build_library
    ext = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_redact.h")).read()
    version = int(re.search(r"#define FRCNN_REDACT_VERSION (\d+)", ext).group(1))
    assert version == _lib.REDACT_VERSION == 1 and re.search(r"^ \*   1 = ", ext, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    names = sorted(set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", code)))
    assert names == sorted(_lib.REDACT_SIGNATURES) == ["frcnn_redact_u8", "frcnn_redact_version", "frcnn_redact_ws_bytes"]
    build_library(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        m = re.search(r"\b(int|size_t) %s\s*\(([^)]*)\)" % name, code)
        assert m, name
        decls = [d for d in m.group(2).split(",") if d.strip() != "void"]
        restype, argtypes = _lib.REDACT_SIGNATURES[name]
        assert restype is {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[m.group(1)] and len(argtypes) == len(decls), name
        for decl, ct in zip(decls, argtypes):
            assert ("*" in decl) == (ct is ctypes.c_void_p), (name, decl)
            assert ("size_t" in decl) == (ct is ctypes.c_size_t), (name, decl)
        assert hasattr(lib, name), name
    define = lambda k: int(re.search(r"#define FRCNN_REDACT_%s (\d+)" % k, ext).group(1))
    assert {k: define(k.upper()) for k in _lib.REDACT_MODES} == _lib.REDACT_MODES
    assert _lib.REDACT_SIZES["pixelate"][:2] == (define("PIXELATE_MIN"), define("PIXELATE_MAX"))
    assert _lib.REDACT_SIZES["blur"][:2] == (define("BLUR_MIN"), define("BLUR_MAX")) and _lib.REDACT_SIZES["fill"] == (0, 0, 0)
    assert _lib.REDACT_SIZES == R.SIZES and ops.REDACT_SIZES is _lib.REDACT_SIZES and define("MAX_ROWS") == _lib.REDACT_MAX_ROWS == 512
    # the core header and the other extensions do not know the new symbols, and the core revision is what it was
    core = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    ext_dir = os.path.join(ROOT, "include", "ext")
    others = "".join(open(os.path.join(ext_dir, f)).read() for f in sorted(os.listdir(ext_dir)) if f != "frcnn_hip_redact.h")
    assert not any(n in core or n in others for n in names)
    loaded = _lib.load()
    assert loaded.frcnn_redact_version() == version
    assert loaded.frcnn_version() == _lib.ABI_VERSION == int(re.search(r"#define FRCNN_ABI_VERSION (\d+)", core).group(1))


def test_workspace_sizes_and_host_helpers():
    """frcnn_redact_ws_bytes runs on the host; the class list and size helpers need no device."""
    from faster_rcnn_amd import ops
    assert ops.redact_ws_bytes(33, 70, "fill", None) == 0
    assert ops.redact_ws_bytes(33, 70, "pixelate", 16) == 3 * 5 * 3 and ops.redact_ws_bytes(33, 70, "pixelate", 64) == 1 * 2 * 3
    assert ops.redact_ws_bytes(33, 70, "pixelate") == ops.redact_ws_bytes(33, 70, "pixelate", 16)
    assert ops.redact_ws_bytes(33, 70, "blur", 1) == ops.redact_ws_bytes(33, 70, "blur") == 33 * 70 * 3
    assert ops.redact_ws_bytes(32768, 32768, "blur", 1) == 3 * 32768 * 32768
    for mode, size in (("pixelate", 1), ("pixelate", 65), ("blur", 0), ("blur", 33), ("fill", 2)):
        with pytest.raises(ValueError):
            ops.redact_ws_bytes(8, 8, mode, size)
    names = ["bg", "car", "", "person"]
    assert ops.redact_class_list(names, "all") == ("car", "person") and ops.redact_class_list(names, ["person"]) == ("person",)
    with pytest.raises(ValueError) as e:
        ops.redact_class_list(names, ["person", "dog"])
    assert "dog" in str(e.value) and "car, person" in str(e.value)
