"""The post-process option without a GPU: the five command-line arguments of voc_dets and annotate_video and their refusals, the
extension header against the ctypes table and the built library, and the engine table's key."""
import os
import re

import pytest

from faster_rcnn_amd import _lib, annotate_video, ops, voc_dets
from faster_rcnn_amd.args_util import post_from_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AV = ["rpn.h5", "det.h5", "frames"]
VD = ["rpn.h5", "det.h5", "--voc_path", "voc"]


@pytest.mark.parametrize("parser,base", [(annotate_video.build_parser, AV), (voc_dets.build_parser, VD)], ids=["annotate_video", "voc_dets"])
def test_arguments(parser, base):
    p = parser()
    assert post_from_args(p.parse_args(base)) is None                         # without the arguments nothing changes
    assert post_from_args(p.parse_args(base + ["--nms", "hard"])) == ("hard", 0.5, 0.5, None, None)
    assert post_from_args(p.parse_args(base + ["--nms", "soft_linear", "--nms_thresh", "0.3"])) == ("soft_linear", 0.3, 0.5, None, None)
    assert post_from_args(p.parse_args(base + ["--nms", "soft_gaussian", "--nms_sigma", "0.25", "--nms_min_score", "0.01", "--box_vote"])) \
        == ("soft_gaussian", 0.5, 0.25, 0.01, 0.5)
    assert post_from_args(p.parse_args(base + ["--box_vote", "0.7"])) == ("hard", 0.5, 0.5, None, 0.7)      # voting goes with every mode
    assert post_from_args(p.parse_args(base + ["--nms_thresh", "0.4"])) == ("hard", 0.4, 0.5, None, None)
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--nms", "soft"])


@pytest.mark.parametrize("parser,base", [(annotate_video.build_parser, AV), (voc_dets.build_parser, VD)], ids=["annotate_video", "voc_dets"])
@pytest.mark.parametrize("extra,word", [(["--nms_sigma", "0.5"], "--nms_sigma"), (["--nms", "soft_linear", "--nms_sigma", "0.5"], "--nms_sigma"),
                                        (["--nms_min_score", "0.1"], "--nms_min_score"), (["--nms", "hard", "--nms_min_score", "0.1"], "--nms_min_score"),
                                        (["--box_vote", "1.5"], "vote_iou"), (["--box_vote", "0"], "vote_iou"),
                                        (["--nms", "soft_gaussian", "--nms_sigma", "0"], "sigma"), (["--nms_thresh", "2"], "nms_thresh"),
                                        (["--nms", "soft_linear", "--nms_min_score", "1.5"], "min_score")])
def test_refusals_by_name(parser, base, extra, word):
    with pytest.raises(ValueError) as e:
        post_from_args(parser().parse_args(base + extra))
    assert word in str(e.value)


def test_annotate_video_refuses_before_any_model_is_loaded():
    """main() gets as far as the option check and no further: the checkpoints do not exist."""
    with pytest.raises(ValueError) as e:
        annotate_video.main(AV + ["--out_dir", "out", "--nms_sigma", "0.5"])
    assert "--nms_sigma" in str(e.value)
    with pytest.raises(ValueError) as e:
        annotate_video.annotate_images(None, None, "frames", "out", [], 600, 1000, post=("soft",))
    assert "mode" in str(e.value)
    with pytest.raises(ValueError) as e:                                       # the same failure from both tools
        voc_dets.main(VD + ["--nms", "hard", "--nms_min_score", "0.5"])
    assert "--nms_min_score" in str(e.value)


def test_header_and_table():
    """The pattern of the other extension headers: every symbol the header declares is in _lib.DETECT_POST_SIGNATURES with as many
    arguments, the library exports it, and the core tables do not know it."""
    hdr = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_detect_post.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", code)))
    assert names == sorted(_lib.DETECT_POST_SIGNATURES) == ["frcnn_detect_post_version", "frcnn_detections_post", "frcnn_detections_post_dyn"]
    lib = _lib.load()
    for name in names:
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, code, flags=re.S).group(1)
        n_args = 0 if decl.strip() == "void" else len(decl.split(","))
        restype, argtypes = _lib.DETECT_POST_SIGNATURES[name]
        assert len(argtypes) == n_args, name
        assert getattr(lib, name).argtypes == argtypes
        assert name not in _lib.SIGNATURES and name not in _lib.EXT_SIGNATURES
    assert lib.frcnn_detect_post_version() == _lib.DETECT_POST_VERSION == int(re.search(r"#define FRCNN_DETECT_POST_VERSION (\d+)", hdr).group(1))
    for i, mode in enumerate(ops.DET_POST_MODES):
        assert int(re.search(r"#define FRCNN_NMS_%s (\d+)" % mode.upper(), hdr).group(1)) == i
    # the two new signatures are the old ones plus (int, double, double, double) in front of the stream
    for old, new in (("frcnn_detections", "frcnn_detections_post"), ("frcnn_detections_dyn", "frcnn_detections_post_dyn")):
        a, b = _lib.SIGNATURES[old][1], _lib.DETECT_POST_SIGNATURES[new][1]
        assert b == a[:-1] + [_lib.I, _lib.c_double, _lib.c_double, _lib.c_double] + a[-1:]
    # the library refuses on the host, with a reason, before any device is touched
    assert lib.frcnn_detections_post(1, 1, 8, 1, 1, 21, 20, 0.0, 16.0, 1.0, 0.5, 1, 1, 1, 1, 1, 7, 0.5, -1.0, 0.0, None) == -1
    assert b"nms_mode" in lib.frcnn_last_error()


def test_build_flags():
    from faster_rcnn_amd import build
    assert build.SOURCES["detect_post.hip"] == build.SOURCES["detect.hip"] == ["-ffp-contract=off"]


def test_engine_key_carries_the_option(monkeypatch):
    """for_models: the option, normalised, is part of the table key; without it the key is the one it always was."""
    from faster_rcnn_amd import entry
    made = []

    class Fake:
        def __init__(self, manager, detector, num_rois, stride, in_flight, post=None):
            self.detector, self.post = detector, post
            made.append(self)

        usable = staticmethod(lambda *a: True)

    class Manager:
        pass

    monkeypatch.setattr(entry, "DetectionEntry", Fake)
    monkeypatch.setattr(entry.torch.cuda, "is_available", lambda: True)
    m, det = Manager(), object()
    a = entry.for_models(m, det, 64, 16, 1)
    b = entry.for_models(m, det, 64, 16, 1, post=("soft_gaussian", None, 0.5, None, 0.5))
    c = entry.for_models(m, det, 64, 16, 1, post={"mode": "soft_gaussian", "vote_iou": 0.5})
    assert a is not b and b is c and len(made) == 2 and a.post is None and b.post == ("soft_gaussian", 0.5, 0.5, None, 0.5)
    assert entry.for_models(m, det, 64, 16, 1) is a
    assert sorted(m._entries, key=len) == [(id(det), 64, 16, 1), (id(det), 64, 16, 1, b.post)]
    with pytest.raises(ValueError):
        entry.for_models(m, det, 64, 16, 1, post=("soft",))
