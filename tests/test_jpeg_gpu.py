"""The device JPEG encoder (faster_rcnn_amd/csrc/jpeg.hip through ops.jpeg_encode_u8 / ops.jpeg_bytes) against its CPU restatement
(tests/jpeg_ref.py): the device file equals the restatement's byte for byte, in both channel orders, on the smallest frames at which each
mechanism can break (tests/jpeg_cases.py); it is the same from run to run, within the bound, and Pillow decodes it."""
import io

import numpy as np
import pytest

from tests import jpeg_ref as R
from tests.jpeg_cases import CASES, RUNS, noise

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
Image = pytest.importorskip("PIL.Image")


@pytest.fixture(scope="module")
def ops():
    from faster_rcnn_amd import ops as o
    return o


@pytest.fixture(scope="module")
def want():
    """(case, quality) -> (the restatement's file, its info): computed once, shared by the tests."""
    table = {}
    for name, quality in RUNS:
        info = {}
        table[name, quality] = (R.encode(CASES[name], quality, info=info), info)
    return table


def assert_same_file(got, expected, info):
    """Byte for byte; a mismatch names the first differing offset and the restart interval it falls in."""
    if got == expected:
        return
    first = next((i for i, (a, b) in enumerate(zip(got, expected)) if a != b), min(len(got), len(expected)))
    interval = sum(1 for start in info["intervals"] if start <= first) - 1
    where = "the header" if interval < 0 else "restart interval %d (of %d, at byte %d)" % (interval, len(info["intervals"]), info["intervals"][interval])
    raise AssertionError("device file (%d bytes) differs from the restatement's (%d) at byte %d, in %s" % (len(got), len(expected), first, where))


@pytest.mark.parametrize("name,quality", RUNS)
@pytest.mark.parametrize("bgr", [False, True])
def test_equals_the_restatement(ops, want, name, quality, bgr):
    frame = CASES[name]
    h, w = frame.shape[:2]
    expected, info = want[name, quality]
    dev = torch.from_numpy(np.ascontiguousarray(frame[:, :, ::-1] if bgr else frame)).cuda()
    data = ops.jpeg_bytes(dev, quality=quality, bgr=bgr)
    assert ops.jpeg_bytes(dev, quality=quality, bgr=bgr) == data, "two encodes of one frame differ"
    assert len(data) <= ops.jpeg_bound(h, w)
    img = Image.open(io.BytesIO(data))
    img.load()
    assert img.mode == "RGB" and img.size == (w, h)
    assert_same_file(data, expected, info)


def test_exported_constants(ops):
    from faster_rcnn_amd import _lib
    lib = _lib.load()
    assert lib.frcnn_jpeg_restart_mcus() == ops.JPEG_RESTART_MCUS == R.RESTART_MCUS
    assert lib.frcnn_jpeg_header_bytes() == ops.jpeg_header_bytes() == R.HEADER_BYTES
    assert lib.frcnn_jpeg_version() == _lib.JPEG_VERSION


def test_default_quality_is_90(ops, want):
    dev = torch.from_numpy(CASES["photo_96x128"]).cuda()
    assert_same_file(ops.jpeg_bytes(dev), *want["photo_96x128", 90])


def test_caller_buffers_at_an_odd_offset(ops, want):
    """jpeg_encode_u8 into the caller's out / out_len / workspace, ``out`` starting at an odd address: the file is the restatement's and
    the bytes beyond its length (and in front of ``out``) stay as they were."""
    name, quality = "noise_64x136", 90
    frame = CASES[name]
    h, w = frame.shape[:2]
    bound = ops.jpeg_bound(h, w)
    for offset in (1, 3):
        backing = torch.full((bound + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        out_len = torch.zeros(1, dtype=torch.int32, device="cuda")
        ws = torch.zeros(ops.jpeg_workspace_bytes(h, w), dtype=torch.uint8, device="cuda")
        out, n = ops.jpeg_encode_u8(torch.from_numpy(frame).cuda(), quality=quality, out=backing[offset:offset + bound], out_len=out_len, workspace=ws)
        assert n is out_len and out.data_ptr() == backing.data_ptr() + offset
        host, n = backing.cpu().numpy(), int(out_len.item())
        assert_same_file(host[offset:offset + n].tobytes(), *want[name, quality])
        assert (host[:offset] == 0xA5).all() and (host[offset + n:] == 0xA5).all()


def test_graph_replay(ops):
    """jpeg_encode_u8 captured once, replayed twice over frames written into the same input tensor: each result is its frame's own file."""
    h, w, quality = 21, 34, 85
    frames = [noise(h, w, 11), CASES["banded_40x131"][:h, :w].copy()]
    src = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    out = torch.zeros(ops.jpeg_bound(h, w), dtype=torch.uint8, device="cuda")
    out_len = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.zeros(ops.jpeg_workspace_bytes(h, w), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.jpeg_encode_u8(src, quality=quality, bgr=True, out=out, out_len=out_len, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        ops.jpeg_encode_u8(src, quality=quality, bgr=True, out=out, out_len=out_len, workspace=ws)
    files = []
    for f in frames:
        src.copy_(torch.from_numpy(f).cuda())
        g.replay()
        torch.cuda.synchronize()
        n = int(out_len.item())
        assert 0 < n <= out.numel()
        files.append(out[:n].cpu().numpy().tobytes())
        info = {}
        assert_same_file(files[-1], R.encode(f, quality, bgr=True, info=info), info)
    assert files[0] != files[1]


def test_bad_arguments_raise(ops):
    """Refused before anything is launched: quality 0 and 101, a short ``out``, h = 0 (and the other malformed frames)."""
    from faster_rcnn_amd._lib import FrcnnError
    good = torch.zeros((4, 5, 3), dtype=torch.uint8, device="cuda")
    for q in (0, 101, 90.0, None):
        with pytest.raises(FrcnnError):
            ops.jpeg_encode_u8(good, quality=q)
    for bad in (torch.zeros((0, 5, 3), dtype=torch.uint8, device="cuda"), torch.zeros((4, 0, 3), dtype=torch.uint8, device="cuda"),
                torch.zeros((4, 5), dtype=torch.uint8, device="cuda"), torch.zeros((4, 5, 4), dtype=torch.uint8, device="cuda"),
                torch.zeros((4, 5, 3), dtype=torch.float32, device="cuda")):
        with pytest.raises(FrcnnError):
            ops.jpeg_encode_u8(bad)
    with pytest.raises(FrcnnError):
        ops.jpeg_encode_u8(good, out=torch.zeros(ops.jpeg_bound(4, 5) - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(FrcnnError):
        ops.jpeg_encode_u8(good, workspace=torch.zeros(16, dtype=torch.uint8, device="cuda"))
    # the C entry itself: status, not a launch
    from faster_rcnn_amd import _lib
    lib, p = _lib.load(), ops._p
    out = torch.zeros(ops.jpeg_bound(4, 5), dtype=torch.uint8, device="cuda")
    n = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.zeros(ops.jpeg_workspace_bytes(4, 5), dtype=torch.uint8, device="cuda")
    args = lambda h, q, cap: (p(good), h, 5, 0, q, p(out), cap, p(n), p(ws), None)
    assert lib.frcnn_jpeg_encode_u8(*args(4, 0, out.numel())) != 0 and lib.frcnn_jpeg_encode_u8(*args(4, 101, out.numel())) != 0
    assert lib.frcnn_jpeg_encode_u8(*args(4, 90, out.numel() - 1)) != 0 and lib.frcnn_jpeg_encode_u8(*args(0, 90, out.numel())) != 0
    torch.cuda.synchronize()                                                # nothing was launched, nothing faulted
    assert int(n.item()) == 0 and not out.any()
    out, n = ops.jpeg_encode_u8(good)
    assert 0 < int(n.item()) <= out.numel() == ops.jpeg_bound(4, 5)
