"""The scale kernel (csrc/scale.hip) against tests/scale_ref.py, byte for byte, on random frames: the smallest shapes at which it can go
wrong, one KITTI-size frame, the batched form with its strides, its count word and unaligned segments, every refusal, and the two
constant frames that would show a rounding that overflows or drifts."""
import ctypes

import numpy as np
import pytest
import torch

from tests import scale_ref as R

pytestmark = pytest.mark.gpu

E_ARG = -1                                                                   # FRCNN_E_ARG
MAX_SIDE, MAX_FRAMES = 32768, 64                                             # FRCNN_REDACT_MAX_SIDE, FRCNN_TRACK_MAX_FRAMES
# (h, w) -> (H, W): the smallest frame; the identity, with 15-byte rows; an exact 2x box mean; ragged weights on both axes; the 16x limit;
# a ratio above 8; several column tiles with the last one partial (57 and 300 output bytes); nearly the identity, where every output
# pixel straddles two source pixels
SHAPES = [((1, 1), (1, 1)), ((7, 5), (7, 5)), ((8, 8), (4, 4)), ((9, 7), (4, 3)), ((16, 16), (1, 1)), ((33, 65), (3, 5)),
          ((17, 300), (2, 19)), ((17, 300), (5, 100)), ((40, 20), (39, 19))]
KITTI = ((375, 1242), (188, 621))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def noise(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def run(frame, H, W):
    from faster_rcnn_amd import ops
    out = ops.downscale_u8(dev(frame), H, W)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("src,dst", SHAPES + [KITTI], ids=lambda s: "%dx%d" % s)
def test_kernel_matches_the_rule(src, dst):
    frame = noise(*src, seed=src[0] * 1000 + dst[1])
    got = run(frame, *dst)
    assert got.shape == dst + (3,) and got.dtype == np.uint8
    assert np.array_equal(got, R.downscale(frame, *dst))


def test_identity_and_box_mean():
    frame = noise(7, 5, seed=3)
    assert np.array_equal(run(frame, 7, 5), frame)
    frame = noise(8, 8, seed=4)
    box = (frame.reshape(4, 2, 4, 2, 3).astype(np.int64).sum(axis=(1, 3)) + 2) // 4
    assert np.array_equal(run(frame, 4, 4), box.astype(np.uint8))


@pytest.mark.parametrize("value", [0, 255])
@pytest.mark.parametrize("src,dst", [((16, 16), (1, 1)), ((33, 65), (3, 5)), ((40, 20), (39, 19)), ((375, 1242), (188, 621))],
                         ids=lambda s: "%dx%d" % s)
def test_constant_frames_stay_constant(src, dst, value):
    got = run(np.full(src + (3,), value, dtype=np.uint8), *dst)
    assert got.shape == dst + (3,) and (got == value).all()


def test_batched_strides_count_word_and_unaligned_segments():
    from faster_rcnn_amd import ops
    (h, w), (H, W) = (9, 7), (4, 3)
    frames = [noise(h, w, seed=10 + f) for f in range(3)]
    npix, nout = 3 * h * w, 3 * H * W
    # source segments 16-byte aligned but no multiple of a frame apart (189 bytes a frame, 208 apart), behind 16 bytes of lead; the
    # outputs 41 bytes apart for 36 bytes a frame: the strides are larger than the frames, and the gaps must stay what they were
    src_stride, dst_stride, lead = 208, 41, 16
    src = np.full(lead + 3 * src_stride, 0x5A, dtype=np.uint8)
    for f in range(3):
        src[lead + f * src_stride:lead + f * src_stride + npix] = frames[f].reshape(-1)
    src_dev = dev(src)
    want = [R.downscale(fr, H, W).reshape(-1) for fr in frames]
    for n_frames, written in ((None, 3), (3, 3), (2, 2), (0, 0), (-1, 0), (7, 3)):
        dst_dev = torch.full((3 * dst_stride,), 0xA5, dtype=torch.uint8, device="cuda")
        word = None if n_frames is None else torch.tensor([n_frames], dtype=torch.int32, device="cuda")
        src_view = src_dev[lead:].as_strided((3, h, w, 3), (src_stride, 3 * w, 3, 1))
        out_view = dst_dev.as_strided((3, H, W, 3), (dst_stride, 3 * W, 3, 1))
        assert ops.downscale_u8(src_view, H, W, out=out_view, n_frames=word) is out_view
        torch.cuda.synchronize()
        got = dst_dev.cpu().numpy()
        for f in range(3):
            seg = got[f * dst_stride:(f + 1) * dst_stride]
            if f < written:
                assert np.array_equal(seg[:nout], want[f]), (n_frames, f)
                assert (seg[nout:] == 0xA5).all(), (n_frames, f)
            else:
                assert (seg == 0xA5).all(), (n_frames, f)
    assert np.array_equal(src_dev.cpu().numpy(), src)                       # the source is read only


def test_frames_at_every_byte_offset():
    """A frame may start at any byte: the aligned chunks that hold a row reach over both ends of the frame."""
    from faster_rcnn_amd import ops
    (h, w), (H, W) = (5, 11), (3, 4)
    frame = noise(h, w, seed=21)
    want = R.downscale(frame, H, W)
    for off in (1, 2, 3, 7, 13, 15):
        buf = torch.zeros(off + 3 * h * w, dtype=torch.uint8, device="cuda")
        buf[off:] = dev(frame).view(-1)
        got = ops.downscale_u8(buf[off:].view(h, w, 3), H, W)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want), off


def test_bad_arguments_launch_nothing():
    from faster_rcnn_amd import _lib
    lib = _lib.load()
    h, w, H, W = 8, 8, 4, 4
    src = torch.zeros(4 * 3 * h * w, dtype=torch.uint8, device="cuda")
    dst = torch.full((4 * 3 * H * W,), 0xA5, dtype=torch.uint8, device="cuda")
    word = torch.ones(1, dtype=torch.int32, device="cuda")
    S, D = src.data_ptr(), dst.data_ptr()
    full, out = 3 * h * w, 3 * H * W
    cases = {
        "null src": (None, full, 1, word.data_ptr(), h, w, D, out, H, W),
        "null dst": (S, full, 1, word.data_ptr(), h, w, None, out, H, W),
        "frames 0": (S, full, 0, None, h, w, D, out, H, W),
        "frames 65": (S, full, MAX_FRAMES + 1, None, h, w, D, out, H, W),
        "h 0": (S, full, 1, None, 0, w, D, out, H, W),
        "w 0": (S, full, 1, None, h, 0, D, out, H, W),
        "h too large": (S, full, 1, None, MAX_SIDE + 1, w, D, out, MAX_SIDE + 1, W),
        "w too large": (S, full, 1, None, h, MAX_SIDE + 1, D, out, H, MAX_SIDE + 1),
        "H 0": (S, full, 1, None, h, w, D, out, 0, W),
        "W 0": (S, full, 1, None, h, w, D, out, H, 0),
        "H > h": (S, full, 1, None, h, w, D, out, h + 1, W),
        "W > w": (S, full, 1, None, h, w, D, out, H, w + 1),
        "h > 16 H": (S, full, 1, None, 17, w, D, out, 1, W),
        "w > 16 W": (S, full, 1, None, h, 17, D, out, H, 1),
        "src stride": (S, full - 1, 2, None, h, w, D, out, H, W),
        "dst stride": (S, full, 2, None, h, w, D, out - 1, H, W),
        "negative stride": (S, -full, 2, None, h, w, D, out, H, W),
    }
    for name, args in cases.items():
        assert lib.frcnn_downscale_u8(*args, None) == E_ARG, name
        assert b"downscale_u8" in lib.frcnn_last_error(), name
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0xA5).all()
    # the strides of a single frame are not read, and the largest ratio is accepted
    assert lib.frcnn_downscale_u8(S, 0, 1, None, h, w, D, 0, H, W, None) == 0
    assert lib.frcnn_downscale_u8(S, 0, 1, None, 16, 4, D, 0, 1, 4, None) == 0
    torch.cuda.synchronize()
    assert (dst.cpu().numpy()[:out] == 0).all()
    assert isinstance(lib.frcnn_scale_version(), int) and ctypes.sizeof(ctypes.c_longlong) == 8


def test_ops_refuses_before_the_launch():
    from faster_rcnn_amd import ops
    from faster_rcnn_amd._lib import FrcnnError
    frame = dev(noise(8, 8))
    for H, W in ((9, 4), (4, 9), (0, 4)):
        with pytest.raises(FrcnnError, match="downscale_u8"):
            ops.downscale_u8(frame, H, W)
    with pytest.raises(FrcnnError, match="downscale_u8: out must be"):
        ops.downscale_u8(frame, 4, 4, out=torch.empty((4, 5, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(FrcnnError, match="downscale_u8: frame must be"):
        ops.downscale_u8(frame.view(-1), 4, 4)
