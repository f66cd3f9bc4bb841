"""bf16 VGG16, the parts that need no GPU: the builders, loaders and command lines take the precision, the header declares the new
entry points at ABI revision 110, and the storage-model helper of the GPU tests (tests/vgg_bf16_ref.py) is sound -- with its
quantisers off it IS the oracle's VGG16."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_builders_and_loaders_take_dtype():
    from faster_rcnn_amd import nets, resnet, vgg
    for fn in (vgg.vgg16_base, vgg.vgg16_classifier, vgg.rpn_from_h5, vgg.det_from_h5, resnet.rpn_from_h5, resnet.det_from_h5):
        p = inspect.signature(fn).parameters
        assert "dtype" in p and p["dtype"].default == "f32", fn.__name__
    for cls in (nets.VggBase, nets.VggHead):
        p = inspect.signature(cls.__init__).parameters
        assert "dtype" in p and p["dtype"].default == "f32", cls.__name__
    assert hasattr(nets.VggHead, "forward_batched")


@pytest.mark.parametrize("mod", ["voc_dets", "annotate_video"])
def test_command_lines_parse_dtype(mod, capsys):
    import importlib
    m = importlib.import_module("faster_rcnn_amd." + mod)
    tail = ["--voc_path", "x"] if mod == "voc_dets" else ["frames"]
    assert m.build_parser().parse_args(["a.npz", "b.npz"] + tail).dtype == "f32"
    assert m.build_parser().parse_args(["a.npz", "b.npz"] + tail + ["--dtype", "bf16"]).dtype == "bf16"
    with pytest.raises(SystemExit):
        m.build_parser().parse_args(["a.npz", "b.npz"] + tail + ["--dtype", "fp8"])
    assert "invalid choice" in capsys.readouterr().err
    assert "reference has no such flag" in " ".join(m.build_parser().format_help().split())


def test_header_declares_the_new_entry_points_at_revision_110():
    from faster_rcnn_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    assert int(re.search(r"#define FRCNN_ABI_VERSION (\d+)", hdr).group(1)) == 110 == _lib.ABI_VERSION
    assert re.search(r"^ \* 110 = ", hdr, flags=re.M)
    for name in ("frcnn_vgg_conv1_bf16_packed_elems", "frcnn_pack_vgg_conv1_weights_bf16", "frcnn_vgg_conv1_bf16_fwd", "frcnn_pool2d_fwd_bf16"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.SIGNATURES, name
    assert "vgg.py:96-97" in hdr and "vgg.py:100, 108, 118, 128" in hdr
    assert len(_lib.SIGNATURES) == 123


def _small_vgg(rs, C=8, num_classes=5):
    """VGG16's layer names on a few channels (the oracle's graphs go by name and shape)."""
    w, cin = {}, 3
    for blk, n in ((1, 2), (2, 2), (3, 3), (4, 3), (5, 3)):
        for i in range(1, n + 1):
            w["block%d_conv%d" % (blk, i)] = [rs.randn(3, 3, cin, C) * np.sqrt(2.0 / (9 * cin)), rs.randn(C) * 0.1]
            cin = C
    w["fc1"] = [rs.randn(49 * C, 32) * np.sqrt(2.0 / (49 * C)), rs.randn(32) * 0.1]
    w["fc2"] = [rs.randn(32, 32) * np.sqrt(2.0 / 32), rs.randn(32) * 0.1]
    w["dense_class_%d" % num_classes] = [rs.randn(32, num_classes) * 0.2, rs.randn(num_classes) * 0.1]
    w["dense_reg_%d" % num_classes] = [rs.randn(32, 4 * (num_classes - 1)) * 0.1, rs.randn(4 * (num_classes - 1)) * 0.1]
    return w


def test_storage_model_helper_without_rounding_is_the_oracle():
    import torch
    from oracle.keras_ref import KerasGraphs
    from tests.vgg_bf16_ref import VggBf16Graphs
    rs = np.random.RandomState(11)
    w = _small_vgg(rs)
    x = (rs.randint(0, 256, (1, 67, 85, 3)).astype(np.float64) - np.array([103.939, 116.779, 123.68])) / 64.0
    ref, mine = KerasGraphs(w, torch.float64), VggBf16Graphs(w, torch.float64, mixed=False)
    f_ref, f_mine = ref.vgg_base(x), mine.vgg_base(x)
    assert f_ref.shape == (1, 4, 5, 8) and torch.equal(f_ref, f_mine)
    rois = np.array([[0, 0, 4, 3], [1, 1, 3, 2], [2, 0, 2, 3]], dtype=np.float32)
    for a, b in zip(ref.vgg_classifier(f_ref, rois, 5), mine.vgg_classifier(f_ref, rois, 5)):
        assert torch.equal(a, b)


def test_storage_model_helper_rounds_what_the_product_stores():
    import torch
    from oracle.keras_ref import KerasGraphs
    from tests.vgg_bf16_ref import VggBf16Graphs
    for name in ("block1_conv1", "block5_conv3", "fc1", "fc2", "rpn_conv1", "res2a_branch2a"):
        assert VggBf16Graphs._bf16_layer(name), name
    for name in ("rpn_out_cls", "rpn_out_bbreg", "dense_class_21", "dense_reg_21", "conv1"):
        assert not VggBf16Graphs._bf16_layer(name), name
    rs = np.random.RandomState(12)
    w = _small_vgg(rs)
    x = (rs.randint(0, 256, (1, 35, 40, 3)).astype(np.float64) - np.array([103.939, 116.779, 123.68])) / 64.0
    f = VggBf16Graphs(w, torch.float64, mixed=True).vgg_base(x)
    assert torch.equal(f, f.to(torch.bfloat16).to(torch.float64))              # the stored map is bf16-representable
    exact = KerasGraphs(w, torch.float64).vgg_base(x)
    rel = float((f - exact).pow(2).mean().sqrt() / exact.pow(2).mean().sqrt())
    assert 0.0 < rel < 2e-2, rel
