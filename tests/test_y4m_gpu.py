"""csrc/y4m.hip against its contract, tests/y4m_ref.py, bit for bit: every input chroma mode x both ranges x the sizes of
tests/y4m_cases.py for the decoder, both output modes x both ranges x bgr for the encoder, and the batched decoder (mixed items, a
duplicated item) against the single calls.  (The decoders' tests have no launch-count helper: that clause of the batch test is left
out.)"""
import numpy as np
import pytest

from tests import y4m_cases as C
from tests import y4m_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ops():
    from faster_rcnn_amd import ops
    return ops


def _dev(data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


@pytest.mark.parametrize("range_", R.RANGES)
@pytest.mark.parametrize("chroma", R.CHROMAS)
def test_decode_equals_restatement(ops, chroma, range_):
    for h, w in C.SIZES:
        data = C.frame(h, w, chroma)
        plan = ops.y4m_plan(h, w, chroma, range_)
        assert int(plan.frame_bytes) == len(data) == ops.y4m_frame_bytes(h, w, chroma)
        for bgr in (False, True):
            got = ops.y4m_decode_u8(_dev(data), plan, bgr=bgr).cpu().numpy()
            assert np.array_equal(got, R.decode(data, h, w, chroma, range_, bgr)), (chroma, range_, h, w, bgr)
    # a frame that starts at an odd byte of its buffer: the word paths must fall back to bytes
    h, w = 17, 33
    data = C.frame(h, w, chroma, seed=1)
    shifted = _dev(b"\x55" + data)[1:]
    out = torch.empty(h * w * 3 + 1, dtype=torch.uint8, device="cuda")[1:]
    ops.y4m_decode_u8(shifted, ops.y4m_plan(h, w, chroma, range_), out=out)
    assert np.array_equal(out.cpu().numpy().reshape(h, w, 3), R.decode(data, h, w, chroma, range_))


@pytest.mark.parametrize("range_", R.RANGES)
def test_decode_sweep_hits_every_clamp(ops, range_):
    lo, hi = 255, 0
    for y in C.SWEEP_Y:
        data = C.sweep_444(y)
        got = ops.y4m_decode_u8(data, ops.y4m_plan(256, 256, "444", range_)).cpu().numpy()
        assert np.array_equal(got, R.decode(data, 256, 256, "444", range_)), (range_, y)
        lo, hi = min(lo, int(got.min())), max(hi, int(got.max()))
    assert (lo, hi) == (0, 255)                                           # both clamps were reached


@pytest.mark.parametrize("bgr", (False, True))
@pytest.mark.parametrize("range_", R.RANGES)
@pytest.mark.parametrize("chroma", R.OUT_CHROMAS)
def test_encode_equals_restatement(ops, chroma, range_, bgr):
    for h, w in C.SIZES:
        rgb = C.rgb_frame(h, w)
        got = ops.y4m_encode_u8(torch.from_numpy(rgb).cuda(), chroma, range_, bgr=bgr)
        assert got.dim() == 1 and got.numel() == ops.y4m_frame_bytes(h, w, chroma)
        assert got.cpu().numpy().tobytes() == R.encode(rgb, chroma, range_, bgr), (chroma, range_, bgr, h, w)
    # several frames in one launch, from a buffer whose frames lie an odd stride apart
    h, w, n = 17, 33, 3
    stride = h * w * 3 + 5
    frames = [C.rgb_frame(h, w, seed=k) for k in range(n)]
    buf = torch.zeros(n * stride, dtype=torch.uint8)
    for k, f in enumerate(frames):
        buf[k * stride:k * stride + f.size] = torch.from_numpy(f.reshape(-1))
    out = ops.y4m_encode_frames_u8(buf.cuda(), stride, n, h, w, chroma, range_, bgr=bgr).cpu().numpy()
    for k, f in enumerate(frames):
        assert out[k].tobytes() == R.encode(f, chroma, range_, bgr), k


def test_encode_sweep_all_rgb_planes(ops):
    """Every (R, G) pair at a few B values: 256 x 256 frames."""
    g, r = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for b in (0, 1, 127, 254, 255):
        rgb = np.stack([r, g, np.full_like(r, b)], axis=2).astype(np.uint8)
        for range_ in R.RANGES:
            got = ops.y4m_encode_u8(torch.from_numpy(rgb).cuda(), "444", range_)
            assert got.cpu().numpy().tobytes() == R.encode(rgb, "444", range_), (b, range_)


def test_batch_equals_single_calls(ops):
    """Three frames of different sizes, modes and ranges in one call equal the three single calls; a duplicated item (the padding of a
    short group: the same file bytes, two outputs) is decoded once per output."""
    specs = [(17, 33, "420jpeg", "limited"), (130, 258, "422", "full"), (5, 7, "mono", "limited")]
    datas = [C.frame(h, w, c, seed=2) for h, w, c, _ in specs]
    plans = [ops.y4m_plan(h, w, c, r) for h, w, c, r in specs]
    file_off, at = [], 3                                                  # (an odd start)
    for d in datas:
        file_off.append(at)
        at += len(d)
    files = bytearray(at)
    for o, d in zip(file_off, datas):
        files[o:o + len(d)] = d
    order = [0, 1, 2, 0]                                                  # item 3: item 0's bytes again
    out_off, total = [], 0
    for k in order:
        out_off.append(total)
        total += specs[k][0] * specs[k][1] * 3 + 1                        # (outputs at odd offsets too)
    items = ops.y4m_batch_items([plans[k] for k in order], [file_off[k] for k in order], out_off)
    out = torch.full((total,), 0xEE, dtype=torch.uint8, device="cuda")
    ops.y4m_decode_batch_u8(_dev(bytes(files)), items, out)
    got = out.cpu().numpy()
    for k, o in zip(order, out_off):
        h, w, c, r = specs[k]
        single = ops.y4m_decode_u8(datas[k], plans[k]).cpu().numpy()
        assert np.array_equal(single, R.decode(datas[k], h, w, c, r))
        assert np.array_equal(got[o:o + h * w * 3].reshape(h, w, 3), single), k
        assert got[o + h * w * 3] == 0xEE                                 # nothing written past a frame


def test_arguments_are_checked_on_the_host(ops):
    from faster_rcnn_amd._lib import FrcnnError
    plan = ops.y4m_plan(4, 4, "420jpeg")
    with pytest.raises(FrcnnError):
        ops.y4m_decode_u8(torch.zeros(int(plan.frame_bytes) - 1, dtype=torch.uint8, device="cuda"), plan)
    with pytest.raises(FrcnnError):
        ops.y4m_decode_u8(torch.zeros(int(plan.frame_bytes), dtype=torch.uint8, device="cuda"), plan,
                          out=torch.zeros(47, dtype=torch.uint8, device="cuda"))
    bad = ops.y4m_plan(4, 4, "420jpeg")
    bad.frame_bytes = 23
    with pytest.raises(FrcnnError):
        ops.y4m_decode_u8(torch.zeros(64, dtype=torch.uint8, device="cuda"), bad)
    with pytest.raises(FrcnnError):
        ops.y4m_encode_u8(torch.zeros((4, 4, 3), dtype=torch.uint8, device="cuda"), "422")
    items = ops.y4m_batch_items([plan, plan], [0, 0], [0, 10])            # overlapping outputs
    with pytest.raises(FrcnnError):
        ops.y4m_decode_batch_u8(torch.zeros(64, dtype=torch.uint8, device="cuda"), items, torch.zeros(200, dtype=torch.uint8, device="cuda"))
