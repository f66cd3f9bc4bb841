"""annotate_video without a GPU: the label number's formula (what csrc/annotate.hip computes) against Python's own format, the
reference's filter, the glyph table, the command line, the file selection, and that importing the module starts no HIP."""
import os
import subprocess
import sys

import numpy as np

from tests.annotate_ref import is_drawn, paint_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_number(p):
    """frcnn_annotate_u8's "{:6.2f}" for finite float32 p: v = rint((double)p * 100) (exact product, ties to even),
    printed as v / 100 "." v % 100, right-aligned in 6 columns."""
    v = np.rint(np.asarray(p, dtype=np.float32).astype(np.float64) * 100.0)
    out = []
    for x, neg in zip(v.tolist(), np.signbit(np.asarray(p, dtype=np.float32)).tolist()):
        iv = int(abs(x))
        out.append(("-" if neg else "") + "%d.%02d" % (iv // 100, iv % 100))
    return [s.rjust(6) for s in out]


def test_label_number_formula_at_every_tie_and_random_values():
    ties = np.array([(k + 0.5) / 100 for k in range(100)], dtype=np.float32)
    near = (ties.view(np.int32)[:, None] + np.arange(-4, 5)[None, :]).astype(np.int32).view(np.float32).ravel()
    rand = np.random.RandomState(0).rand(10 ** 6).astype(np.float32)
    extra = np.array([0.0, -0.0, 0.125, 0.995, 1.0, -0.004, 1234.5], dtype=np.float32)
    for vals in (near, extra, rand):
        got = kernel_number(vals)
        want = ["{:6.2f}".format(p) for p in vals]
        bad = [(float(p), g, w) for p, g, w in zip(vals, got, want) if g != w]
        assert not bad, bad[:5]
    assert kernel_number([0.125, 0.995]) == ["  0.12", "  1.00"]


def test_filter_edge_cases():
    w, h = 100, 50

    def det(bbox, name="car"):
        return {"bbox": np.array(bbox, dtype=np.int64), "cls_name": name, "prob": np.float32(0.5)}
    assert is_drawn(det([0, 0, 100, 50]), w, h)                   # x2 == width, y2 == height: kept
    assert not is_drawn(det([-1, 0, 10, 10]), w, h)               # x1 == -1: dropped
    assert not is_drawn(det([0, -1, 10, 10]), w, h)
    assert not is_drawn(det([0, 0, 101, 10]), w, h)
    assert not is_drawn(det([0, 0, 10, 51]), w, h)
    assert not is_drawn(det([1, 1, 10, 10], "DontCare"), w, h)
    assert not is_drawn(det([1, 1, 10, 10], "Misc"), w, h)
    assert is_drawn(det([1, 1, 10, 10], "Cyclist"), w, h)
    from faster_rcnn_amd import annotate_video, ops
    assert tuple(ops.ANNOTATE_SKIP) == ("DontCare", "Misc")
    for d in (det([0, 0, 100, 50]), det([-1, 0, 10, 10]), det([1, 1, 10, 10], "Misc"), det([50, 5, 3, 40])):
        assert annotate_video.drawn(d, w, h) == is_drawn(d, w, h)


def test_glyph_table():
    from faster_rcnn_amd import annotate_font
    g = annotate_font.GLYPHS
    assert g.shape == (95, 7) and g.dtype == np.uint8 and int(g.max()) < 32
    assert not g[0].any() and all(g[i].any() for i in range(1, 95))          # blank space, every other glyph visible
    assert len({bytes(r) for r in g}) == 95                                   # no two glyphs alike
    assert np.array_equal(annotate_font.glyph("\x01"), annotate_font.glyph("?"))
    assert np.array_equal(annotate_font.glyph("~"), g[-1])


def test_restatement_paints_box_and_label():
    from faster_rcnn_amd.annotate_font import GLYPHS
    d = {"bbox": np.array([10, 5, 30, 20], dtype=np.int64), "cls_name": "car", "prob": np.float32(1.0)}
    m = paint_mask(60, 120, [d], GLYPHS)
    assert m[4:7, 9:32].all() and m[19:22, 9:32].all() and m[4:22, 9:12].all() and m[4:22, 29:32].all()
    assert not m[8:18, 13:28].any()                                          # the box's inside stays
    assert m[23:37].any()                                                    # the label: rows y2 + 3 .. y2 + 16
    assert not paint_mask(60, 120, [dict(d, cls_name="Misc")], GLYPHS).any()


def test_parser_matches_the_reference():
    """annotate_video.py:48-64 of the reference: three positionals, --kitti, --resize_dims 600,1000, --out_dir '.';
    the mirror adds voc_dets' --network / --anchor_scales."""
    from faster_rcnn_amd import annotate_video
    p = annotate_video.build_parser()
    a = p.parse_args(["r.npz", "d.npz", "frames"])
    assert (a.step3_model_path, a.step4_model_path, a.input_dir) == ("r.npz", "d.npz", "frames")
    assert a.kitti is False and a.resize_dims == "600,1000" and a.out_dir == "."
    assert a.network == "resnet50" and a.anchor_scales == "128,256,512"
    b = p.parse_args(["r", "d", "in", "--kitti", "--resize_dims", "600,1500", "--out_dir", "out", "--network", "resnet101",
                      "--anchor_scales", "16,32,64,128,256,512"])
    assert b.kitti and b.resize_dims == "600,1500" and b.out_dir == "out" and b.network == "resnet101"
    positional = [x.dest for x in p._actions if not x.option_strings]
    assert positional == ["step3_model_path", "step4_model_path", "input_dir"]


def test_png_selection_and_order(tmp_path):
    from faster_rcnn_amd import annotate_video
    for name in ("b.png", "a.png", "c.jpg", "000010.png", "000002.png", "x.PNG", "notes.txt"):
        (tmp_path / name).write_bytes(b"")
    assert annotate_video.png_filenames(str(tmp_path)) == ["000002.png", "000010.png", "a.png", "b.png"]


def test_import_starts_no_hip():
    code = ("import faster_rcnn_amd.annotate_video, faster_rcnn_amd.annotate_font, torch; "
            "assert not torch.cuda.is_initialized(), 'HIP started on import'")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
