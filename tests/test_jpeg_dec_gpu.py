"""The device JPEG decoder on the GPU: ops.jpeg_decode_u8 against the CPU restatement (tests/jpeg_dec_ref.py, which
tests/test_jpeg_dec_cpu.py holds to Pillow) byte for byte, between guard bytes, with the status word; two files back to back through one
workspace; a damaged scan."""
import functools

import numpy as np
import pytest

from tests import jpeg_dec_cases as C
from tests import jpeg_dec_ref as D

pytestmark = pytest.mark.gpu
GUARD = 256


@functools.lru_cache(None)
def reference(name):
    return D.decode(C.files()[name])


def decode_guarded(data, bgr=False, workspace=None, status=None):
    """-> (frame, status, guards intact): decoded into the middle of a buffer of 0xA7 bytes."""
    import torch
    from faster_rcnn_amd import ops
    plan = ops.jpeg_dec_plan(data)
    n = plan.h * plan.w * 3
    buf = torch.full((n + 2 * GUARD,), 0xA7, dtype=torch.uint8, device="cuda")
    out = buf[GUARD:GUARD + n].view(plan.h, plan.w, 3)
    file_dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    got, status = ops.jpeg_decode_u8(file_dev, plan, bgr=bgr, out=out, status=status, workspace=workspace)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    intact = bool((host[:GUARD] == 0xA7).all() and (host[GUARD + n:] == 0xA7).all())
    return host[GUARD:GUARD + n].reshape(plan.h, plan.w, 3), status, intact


@pytest.mark.parametrize("name", sorted(C.files()))
def test_decode_is_the_restatement(name):
    """Every file of the CPU tests (1x1, 7x9 and 17x23 the smallest; the 375x500 golden image and 64x136 noise at quality 100 the
    largest): the same bytes, R,G,B and B,G,R, the guards intact, status 0."""
    assert set(C.SMALLEST + C.LARGEST) <= set(C.files())
    want = reference(name)
    for bgr in (False, True):
        got, status, intact = decode_guarded(C.files()[name], bgr=bgr)
        assert intact, name
        assert int(status.item()) == 0, name
        ref = want[:, :, ::-1] if bgr else want
        assert np.array_equal(got, ref), (name, bgr, int(np.abs(got.astype(int) - ref).max()), int((got != ref).sum()))


def test_bytes_and_defaults():
    """The convenience form: the file's bytes in, everything allocated."""
    from faster_rcnn_amd import ops
    out, status = ops.jpeg_decode_u8(C.files()["17x23_s2_q100"])
    assert tuple(out.shape) == (17, 23, 3) and int(status.item()) == 0
    assert np.array_equal(out.cpu().numpy(), reference("17x23_s2_q100"))


def test_two_files_back_to_back_one_workspace():
    """Two decodes on one stream through one workspace and one status word, no synchronisation between them."""
    import torch
    from faster_rcnn_amd import ops
    names = ("golden_000005", "33x65_s1_q75")
    plans = [ops.jpeg_dec_plan(C.files()[n]) for n in names]
    ws = torch.empty(max(ops.jpeg_dec_workspace_bytes(p) for p in plans), dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    files = [torch.frombuffer(bytearray(C.files()[n]), dtype=torch.uint8).cuda() for n in names]
    outs = [ops.jpeg_decode_u8(f, p, workspace=ws, status=status)[0] for f, p in zip(files, plans)]
    outs.append(ops.jpeg_decode_u8(files[0], plans[0], workspace=ws, status=status)[0])
    assert int(status.item()) == 0
    for out, n in zip(outs, names + names[:1]):
        assert np.array_equal(out.cpu().numpy(), reference(n)), n


def test_damaged_scan_sets_the_status_word():
    """The damaged file of the CPU tests: the run ends, the status word is the restatement's (non-zero), the guards are intact; the
    word is sticky: a sound file decoded behind it leaves it as it is."""
    from faster_rcnn_amd import ops
    data = C.damaged()
    want = D.coefficients(data)[2]
    assert want != 0
    got, status, intact = decode_guarded(data)
    assert intact
    assert int(status.item()) == want
    _, status, intact = decode_guarded(C.files()["8x8_s0_q75"], status=status)
    assert intact and int(status.item()) == want


def test_argument_errors_launch_nothing():
    import torch
    from faster_rcnn_amd import ops
    from faster_rcnn_amd._lib import FrcnnError
    data = C.files()["16x16_s2_q75"]
    plan = ops.jpeg_dec_plan(data)
    file_dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    out = torch.full((16 * 16 * 3,), 0xA7, dtype=torch.uint8, device="cuda")
    with pytest.raises(FrcnnError):
        ops.jpeg_decode_u8(file_dev, plan, out=out[:-1])
    with pytest.raises(FrcnnError):
        ops.jpeg_decode_u8(file_dev[:-8], plan)
    with pytest.raises(FrcnnError):
        ops.jpeg_decode_u8(file_dev)
    with pytest.raises(FrcnnError):
        ops.jpeg_decode_u8(file_dev, plan, workspace=torch.empty(64, dtype=torch.uint8, device="cuda"))
    bad = ops.jpeg_dec_plan(data)
    bad.scan_len = bad.file_len
    with pytest.raises(FrcnnError):
        ops.jpeg_decode_u8(file_dev, bad)
    with pytest.raises(ops.JpegUnsupported):
        ops.jpeg_decode_u8(C.unsupported()["progressive"][0])
    torch.cuda.synchronize()
    assert bool((out == 0xA7).all())
