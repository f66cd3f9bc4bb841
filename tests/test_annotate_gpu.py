"""Detections drawn on frames on the device (csrc/annotate.hip, entry.DetectionEntry's annotating passes, annotate_video.py)
against the numpy restatement of the drawing rule in tests/annotate_ref.py: bit for bit."""
import contextlib
import io
import os
import re

import numpy as np
import pytest

from tests.annotate_ref import annotate as restate

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()) as buf:
        res = fn(*a, **k)
    return res, buf.getvalue()


def same_dets(a, b, tol=1e-4):
    """tests/test_entry_gpu.py's bar: classes and boxes identical, in order; scores within ``tol``."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x["cls_name"] == y["cls_name"] and np.array_equal(x["bbox"], y["bbox"]), (x, y)
        assert abs(float(x["prob"]) - float(y["prob"])) <= tol, (x, y)


_DET_LINE = re.compile(r"^\{'bbox': array\(\[([-\d,\s]*)\]\), 'cls_name': '([^']*)', 'prob': (?:np\.float32\()?([^)}]+)\)?\}$")


def printed_dets(lines):
    """The det dicts a run printed (numpy's repr of a float32 round-trips exactly)."""
    out = []
    for line in lines:
        m = _DET_LINE.match(line)
        assert m, line
        out.append({"bbox": np.array([int(v) for v in m.group(1).replace(",", " ").split()], dtype=np.int64),
                    "cls_name": m.group(2), "prob": np.float32(m.group(3))})
    return out


def frame_pixels(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


# ----------------------------------------------------------------------------------------------------------- the kernel
def _kernel_case(h, w, n, rows, seed, names):
    rs = np.random.RandomState(seed)
    C = len(names)
    dets = []
    ties = [np.float32((k + 0.5) / 100) for k in range(100)]
    specials = [np.float32(v) for v in (0.0, -0.0, 1.0, 0.125, 0.995, -0.004, 1234.5, 3.0e38, np.nan, np.inf, -np.inf)]
    for i in range(n):
        kind = i % 8
        x1, y1 = rs.randint(0, w + 1), rs.randint(0, h + 1)
        x2, y2 = min(w, x1 + rs.randint(0, w // 6 + 2)), min(h, y1 + rs.randint(0, h // 6 + 2))
        if kind == 1:
            x1, y1, x2, y2 = 0, 0, w, h                                  # on the edges: x2 == width, y2 == height kept
        elif kind == 2:
            x1, x2, y1, y2 = x2, x1, y2, y1                              # inverted corners
        elif kind == 3:
            x1 -= rs.randint(1, 5)                                       # out of bounds: dropped
        elif kind == 4:
            x2 += rs.randint(1, 5)
        elif kind == 5:
            y1, y2 = max(0, h - 3), h                                    # label below the frame: clipped away
        elif kind == 6:
            x1 = max(0, w - 20)                                          # label past the right edge
        prob = ties[rs.randint(100)] if i % 3 else (specials[i // 3 % len(specials)] if i % 2 else np.float32(rs.rand()))
        dets.append({"bbox": np.array([x1, y1, x2, y2], dtype=np.int64), "cls_name": names[rs.randint(C - 1)], "prob": prob})
    packed = np.zeros(4 + 7 * rows, dtype=np.int32)
    packed[0] = n
    bbox = packed[4:4 + 4 * rows].reshape(rows, 4)
    cls = packed[4 + 4 * rows:4 + 5 * rows]
    prob = packed[4 + 5 * rows:4 + 6 * rows].view(np.float32)
    # rows past n_dets hold boxes that WOULD be drawn: the kernel must not read them
    bbox[:] = [0, 0, max(1, w // 2), max(1, h // 2)]
    cls[:] = 0
    prob[:] = 0.5
    for k, d in enumerate(dets):
        bbox[k] = d["bbox"]
        cls[k] = names.index(d["cls_name"])
        prob[k] = d["prob"]
    return frame_pixels(h, w, seed + 1), dets, packed


@pytest.mark.parametrize("h,w", [(375, 1242), (37, 53), (1, 1)])
@pytest.mark.parametrize("n", [0, 1, 512])
def test_annotate_u8_equals_the_restatement(h, w, n):
    from faster_rcnn_amd import ops
    from faster_rcnn_amd.data.voc_data_helpers import KITTI_CLASS_MAPPING
    names = [k for k, _ in sorted(KITTI_CLASS_MAPPING.items(), key=lambda kv: kv[1])]
    tables = ops.annotate_tables(names)
    frame, dets, packed = _kernel_case(h, w, n, 512, 1000 * h + n, names)
    dev = torch.from_numpy(frame.copy()).cuda()
    ops.annotate_u8(dev, torch.from_numpy(packed).cuda(), tables)
    got = dev.cpu().numpy()
    want = restate(frame, dets)
    assert np.array_equal(got, want), (h, w, n, int((got != want).any(axis=2).sum()))
    if n == 512 and h > 1:
        assert (want != frame).any() and any(d["cls_name"] in ("DontCare", "Misc") for d in dets)


def test_annotate_u8_rejects_bad_arguments():
    from faster_rcnn_amd import _lib, ops
    tables = ops.annotate_tables(["car", "bg"])
    frame = torch.zeros((4, 4, 3), dtype=torch.uint8, device="cuda")
    big = torch.zeros(4 + 7 * 513, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.FrcnnError):
        ops.annotate_u8(frame, big, tables)                              # max_rows 513 > 512


# ----------------------------------------------------------------------------------------------------------- captured passes
@pytest.fixture(scope="module")
def f32_models():
    from faster_rcnn_amd import resnet, util
    from faster_rcnn_amd.data.voc_data_helpers import VOC_CLASS_MAPPING
    from faster_rcnn_amd.det_util import DetTrainingManager
    from faster_rcnn_amd.pipeline import InferencePipeline
    from faster_rcnn_amd.weights import calibrate_classifier, synthetic_resnet
    anchors = util.get_anchors([128, 256, 512])
    w = synthetic_resnet(50, anchors_per_loc=9, num_classes=21, seed=1)
    rpn = resnet.resnet50_rpn(resnet.resnet50_base(weights=w), include_conv=True, anchors_per_loc=9)
    det = resnet.resnet50_classifier(64, 21, weights=w)
    x = resnet.preprocess(frame_pixels(320, 480, 99))[None].astype(np.float32)
    out = InferencePipeline(rpn, det, anchors).forward_dev(torch.from_numpy(x).cuda())
    n = int(out["n_rois"].item())
    det.get_layer("dense_class_21").set_weights(calibrate_classifier(w, 21, out["cls"][:n].cpu().numpy()))
    mgr = DetTrainingManager(rpn_model=rpn, class_mapping=VOC_CLASS_MAPPING, preprocess_func=resnet.preprocess, anchor_dims=anchors)
    return mgr, det, w


@pytest.fixture(scope="module")
def bf16_models():
    from faster_rcnn_amd import resnet, util
    from faster_rcnn_amd.data.voc_data_helpers import KITTI_CLASS_MAPPING
    from faster_rcnn_amd.det_util import DetTrainingManager
    from faster_rcnn_amd.weights import synthetic_resnet
    anchors = util.get_anchors([16, 32, 64, 128, 256, 512])
    w = synthetic_resnet(101, anchors_per_loc=len(anchors), num_classes=len(KITTI_CLASS_MAPPING), seed=1)
    rpn = resnet.resnet101_rpn(resnet.resnet101_base(weights=w, dtype="bf16"), include_conv=True, anchors_per_loc=len(anchors))
    det = resnet.resnet101_classifier(64, len(KITTI_CLASS_MAPPING), weights=w, dtype="bf16")
    mgr = DetTrainingManager(rpn_model=rpn, class_mapping=KITTI_CLASS_MAPPING, preprocess_func=resnet.preprocess, anchor_dims=anchors)
    return mgr, det, w


def _named(name, pixels=None, path=None, size=None):
    from faster_rcnn_amd import shapes
    h, w = pixels.shape[:2] if pixels is not None else size
    return shapes.Image(shapes.Metadata(name, w, h, [], path or "none"), pixels)


def _fold(per_image):
    by_cls = {}
    for name, dets in per_image:
        for d in dets:
            by_cls.setdefault(d["cls_name"], {}).setdefault(name, []).append(d)
    return by_cls


@pytest.mark.parametrize("which,B", [("f32", 4), ("bf16", 8)])
def test_captured_annotating_passes(which, B, request, tmp_path, monkeypatch):
    """B frames per annotating pass, in-memory BGR frames and file-backed PNGs (uploaded RGB): every frame is the restatement of
    THAT pass's dets, the dets are get_dets_by_cls's, and get_dets_by_cls gives the same results before and after."""
    from PIL import Image as PilImage
    from faster_rcnn_amd import entry, util, voc_dets
    monkeypatch.setattr(voc_dets, "CAPTURE_MIN", 1)
    mgr, det, _ = request.getfixturevalue(which + "_models")
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight(which))
    assert eng.batch == B
    srcs = [frame_pixels(200, 330, 300 + i) for i in range(B)]
    mem = [_named("m%d" % i, pixels=s) for i, s in enumerate(srcs)]
    files = []
    for i, s in enumerate(srcs):
        p = str(tmp_path / ("f%d.png" % i))
        PilImage.fromarray(s[:, :, ::-1]).save(p)                        # the same BGR frame, as a file
        files.append(_named("f%d" % i, path=p, size=s.shape[:2]))
    before = {}
    for kind, imgs in (("mem", mem), ("file", files)):
        resized, ratios = util.resize_imgs(imgs, min_size=320, max_size=540)
        before[kind], _ = quiet(voc_dets.get_dets_by_cls, mgr, det, ratios, resized)
        pixels = [eng.host_pixels(r) for r in resized]
        assert (pixels[0][0].shape[2], bool(pixels[0][4] & 2)) == (3, kind == "file")
        res = eng.collect_batch(eng.submit_batch(resized, ratios, 0.0, pixels, batch=B, annotate=True))
        assert len(res) == B and all(len(r) == 3 for r in res)
        drawn_any = False
        for (n_rois, dets, frame), src in zip(res, srcs):
            upload = src if kind == "mem" else src[:, :, ::-1]
            assert frame.shape == upload.shape and frame.dtype == np.uint8
            assert np.array_equal(frame, restate(upload, dets)), kind
            drawn_any |= bool((frame != upload).any())
        assert sum(len(r[1]) for r in res) > 0 and (drawn_any or which == "bf16")      # (the f32 head is calibrated: many classes fire)
        got = _fold([(img.name, r[1]) for img, r in zip(resized, res)])
        assert list(got) == list(before[kind])
        for c in got:
            assert list(got[c]) == list(before[kind][c])
            for name in got[c]:
                same_dets(got[c][name], before[kind][c][name])
        after, _ = quiet(voc_dets.get_dets_by_cls, mgr, det, ratios, resized)
        assert list(after) == list(before[kind])
        for c in after:
            for name in after[c]:
                same_dets(after[c][name], before[kind][c][name], tol=0.0)
    assert any(k[-1:] == ("annotate",) for k in eng.cache.keys()) and any(k[-1:] != ("annotate",) for k in eng.cache.keys())


# ----------------------------------------------------------------------------------------------------------- annotate_video
def test_get_annotated_frame_in_place_and_eager_path(f32_models):
    from faster_rcnn_amd import annotate_video, shapes, voc_dets
    mgr, det, _ = f32_models
    src = frame_pixels(220, 300, 7)
    outs = {}
    for fast in (True, False):
        voc_dets.FAST_ENTRY = fast
        try:
            frame = src.copy()
            img = shapes.InMemoryImage(data=frame, width=frame.shape[1], height=frame.shape[0])
            ret, text = quiet(annotate_video.get_annotated_frame, mgr, det, frame, img, 320, 540)
        finally:
            voc_dets.FAST_ENTRY = True
        assert ret is frame and (frame != src).any()
        lines = text.splitlines()
        assert lines[0].startswith("num rois: ")
        dets = printed_dets(lines[1:])
        assert dets and all(annotate_video.drawn(d, 300, 220) for d in dets)
        assert np.array_equal(frame, restate(src, dets))
        outs[fast] = (lines[0], dets)
    assert outs[True][0] == outs[False][0]
    same_dets(outs[True][1], outs[False][1])


def test_main_round_trip(f32_models, tmp_path):
    """``python -m faster_rcnn_amd.annotate_video`` on .npz weights and a directory of PNGs of two sizes (plus a .jpg it must
    ignore): one PNG out per PNG in, pixels = the restatement of the printed dets, printed lines = a one-by-one loop's."""
    from PIL import Image as PilImage
    from faster_rcnn_amd import annotate_video, shapes, util
    from faster_rcnn_amd.weights import save_npz
    _, _, w = f32_models
    npz = str(tmp_path / "w.npz")
    save_npz(npz, w)
    d_in, d_out = tmp_path / "frames", tmp_path / "out"
    d_in.mkdir()
    frames = {}
    for i in range(5):
        rgb = frame_pixels(180, 260, 40 + i) if i < 3 else frame_pixels(150, 200, 40 + i)
        frames["%06d.png" % i] = rgb
        PilImage.fromarray(rgb).save(str(d_in / ("%06d.png" % i)))
    PilImage.fromarray(frame_pixels(180, 260, 9)).save(str(d_in / "skip.jpg"))
    argv = [npz, npz, str(d_in), "--resize_dims", "320,540", "--out_dir", str(d_out)]
    _, text = quiet(annotate_video.main, argv)
    assert sorted(os.listdir(d_out)) == sorted(frames)
    # the one-by-one loop: the reference's annotate_images body, same models
    from faster_rcnn_amd import resnet
    from faster_rcnn_amd.data.voc_data_helpers import VOC_CLASS_MAPPING
    from faster_rcnn_amd.det_util import DetTrainingManager
    anchors = util.get_anchors([128, 256, 512])
    rpn = resnet.rpn_from_h5(npz, anchors_per_loc=9, depth=50)
    det = resnet.det_from_h5(npz, num_classes=21, depth=50)
    mgr = DetTrainingManager(rpn_model=rpn, class_mapping=VOC_CLASS_MAPPING, preprocess_func=resnet.preprocess, anchor_dims=anchors)
    one = []
    for name in sorted(frames):
        one.append("processing {}".format(os.path.join(str(d_in), name)))
        bgr = np.ascontiguousarray(frames[name][:, :, ::-1])
        img = shapes.InMemoryImage(data=bgr, width=bgr.shape[1], height=bgr.shape[0])
        _, t = quiet(annotate_video.get_annotated_frame, mgr, det, bgr, img, 320, 540)
        one += t.splitlines()
    lines = text.splitlines()
    assert len(lines) == len(one)
    is_det = [ln.startswith("{") for ln in lines]
    assert is_det == [ln.startswith("{") for ln in one]
    assert [a for a, d in zip(lines, is_det) if not d] == [b for b, d in zip(one, is_det) if not d]
    same_dets(printed_dets([a for a, d in zip(lines, is_det) if d]), printed_dets([b for b, d in zip(one, is_det) if d]))
    # output pixels: each file = the restatement of the dets printed for it
    blocks, cur = {}, None
    for ln in lines:
        if ln.startswith("processing "):
            cur = os.path.basename(ln[len("processing "):])
            blocks[cur] = []
        elif ln.startswith("{"):
            blocks[cur].append(ln)
    assert sum(len(v) for v in blocks.values()) > 0
    for name, rgb in frames.items():
        out = np.asarray(PilImage.open(str(d_out / name)).convert("RGB"))
        assert np.array_equal(out, restate(rgb, printed_dets(blocks[name]))), name
