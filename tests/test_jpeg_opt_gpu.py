"""The device JPEG encoder's 4:2:0 and optimised-Huffman modes (faster_rcnn_amd/csrc/jpeg_opt.hip through ops.jpeg_encode_u8 /
ops.jpeg_bytes with ``subsampling`` / ``huffman``, and ops.jpeg_build_tables) against the CPU restatement (tests/jpeg_opt_ref.py): the
device file equals the restatement's byte for byte in every mode pair and both channel orders on the frames of tests/jpeg_opt_cases.py;
(444, standard) through the new entry point is revision 1's file; the table kernel reproduces Pillow's own DHT payloads; one capture
replays on two frames; the project's device decoder reads the file as Pillow does; bad arguments are refused before any launch."""
import io

import numpy as np
import pytest

from tests import jpeg_opt_ref as O
from tests.jpeg_opt_cases import CASES, QUALITIES, RUNS, fibonacci_histogram, noise, pillow_tables, reference

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
Image = pytest.importorskip("PIL.Image")

GUARD = 32


@pytest.fixture(scope="module")
def ops():
    from faster_rcnn_amd import ops as o
    return o


def assert_same_file(got, expected, info):
    if got == expected:
        return
    first = next((i for i, (a, b) in enumerate(zip(got, expected)) if a != b), min(len(got), len(expected)))
    interval = sum(1 for start in info["intervals"] if start <= first) - 1
    where = "the header" if interval < 0 else "restart interval %d (of %d, at byte %d)" % (interval, len(info["intervals"]), info["intervals"][interval])
    raise AssertionError("device file (%d bytes) differs from the restatement's (%d) at byte %d, in %s" % (len(got), len(expected), first, where))


def guarded_encode(ops, frame, quality, subsampling, huffman, bgr):
    """Encode into the middle of a buffer of 0xA5 bytes -> (the file by ``out_len``, the whole buffer on the host)."""
    h, w = frame.shape[:2]
    bound = ops.jpeg_bound(h, w, subsampling, huffman)
    backing = torch.full((bound + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out_len = torch.zeros(1, dtype=torch.int32, device="cuda")
    dev = torch.from_numpy(np.ascontiguousarray(frame[:, :, ::-1] if bgr else frame)).cuda()
    ops.jpeg_encode_u8(dev, quality=quality, bgr=bgr, out=backing[GUARD:GUARD + bound], out_len=out_len, subsampling=subsampling, huffman=huffman)
    host, n = backing.cpu().numpy(), int(out_len.item())
    assert 0 < n <= bound
    return host[GUARD:GUARD + n].tobytes(), host, n


@pytest.mark.parametrize("name,quality,subsampling,huffman", RUNS)
def test_equals_the_restatement(ops, name, quality, subsampling, huffman):
    frame = CASES[name]
    expected, info = reference(name, quality, subsampling, huffman)
    data, host, n = guarded_encode(ops, frame, quality, subsampling, huffman, bgr=False)
    assert_same_file(data, expected, info)
    assert n == len(expected)                                                       # out_len is the file's length
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + n:] == 0xA5).all()         # nothing in front of out, nothing behind the file
    swapped, host, n = guarded_encode(ops, frame, quality, subsampling, huffman, bgr=True)
    assert swapped == data, "B,G,R input gives another file"
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + n:] == 0xA5).all()
    assert ops.jpeg_bytes(torch.from_numpy(frame).cuda(), quality=quality, subsampling=subsampling, huffman=huffman) == data


@pytest.mark.parametrize("name,quality", QUALITIES)
def test_444_standard_through_the_new_entry_is_revision_1(ops, name, quality):
    """ops takes frcnn_jpeg_encode_u8 for the default pair; frcnn_jpeg_opt_encode_u8 itself, asked for (444, standard), writes the
    same bytes."""
    from faster_rcnn_amd import _lib
    frame = CASES[name]
    h, w = frame.shape[:2]
    dev = torch.from_numpy(frame).cuda()
    old = ops.jpeg_bytes(dev, quality=quality)
    lib = _lib.load()
    assert lib.frcnn_jpeg_opt_bound(h, w, 444) == ops.jpeg_bound(h, w)
    out = torch.zeros(ops.jpeg_bound(h, w), dtype=torch.uint8, device="cuda")
    n = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.zeros(lib.frcnn_jpeg_opt_workspace_bytes(h, w, 444, 0), dtype=torch.uint8, device="cuda")
    _lib.call("frcnn_jpeg_opt_encode_u8", ops._p(dev), h, w, 0, quality, 444, 0, ops._p(out), out.numel(), ops._p(n), ops._p(ws), ops._stream())
    assert out[:int(n.item())].cpu().numpy().tobytes() == old == reference(name, quality, 444, "standard")[0]


def test_table_kernel_builds_pillows_tables(ops):
    """ops.jpeg_build_tables on the symbol histograms of Pillow's own optimize=True files gives those files' BITS / HUFFVAL, and on the
    Fibonacci histogram (where the length limit acts) the restatement's table."""
    for label, hist, tables in pillow_tables():
        got = ops.jpeg_tables_from_records(ops.jpeg_build_tables(hist))
        assert got == [(list(b), list(v)) for b, v in tables], label
    fib = np.zeros((4, 256), np.int64)
    fib[1] = fibonacci_histogram()
    fib[2, 7] = 5                                                   # one symbol: a one-bit code; histograms 0 and 3 are empty
    got = ops.jpeg_tables_from_records(ops.jpeg_build_tables(fib))
    assert got == [O.optimal_table(fib[k]) for k in range(4)]
    assert got[0] == ([0] * 16, []) and got[2] == ([1] + [0] * 15, [7]) and sum(got[1][0]) == 30 and got[1][0][15] > 0
    big = np.zeros((4, 256), np.int64)                              # counts at the top of uint32: the sums need more than 32 bits
    big[0, :40] = 2 ** 32 - 1 - np.arange(40)
    assert ops.jpeg_tables_from_records(ops.jpeg_build_tables(big))[0] == O.optimal_table(big[0])


def test_graph_replay_clears_the_histograms(ops):
    """An optimised 4:2:0 encode captured once, replayed on two frames into the same buffers: each gives its own frame's file, so the
    histograms are cleared inside the call."""
    h, w, quality = 21, 34, 85
    frames = [noise(h, w, 21), CASES["photo_96x128"][:h, :w].copy()]
    mode = dict(subsampling=420, huffman="optimized")
    src = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    out = torch.zeros(ops.jpeg_bound(h, w, **mode), dtype=torch.uint8, device="cuda")
    out_len = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.zeros(ops.jpeg_workspace_bytes(h, w, **mode), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.jpeg_encode_u8(src, quality=quality, out=out, out_len=out_len, workspace=ws, **mode)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        ops.jpeg_encode_u8(src, quality=quality, out=out, out_len=out_len, workspace=ws, **mode)
    files = []
    for f in frames + frames[:1]:
        src.copy_(torch.from_numpy(f).cuda())
        g.replay()
        torch.cuda.synchronize()
        n = int(out_len.item())
        assert 0 < n <= out.numel()
        files.append(out[:n].cpu().numpy().tobytes())
        info = {}
        assert_same_file(files[-1], O.encode(f, quality, 420, "optimized", info=info), info)
    assert files[0] != files[1] and files[0] == files[2]


@pytest.mark.parametrize("name,quality", [("noise_33x47", 90), ("photo_96x128", 90), ("noise_48x352", 10), ("grey_24x40", 90)])
def test_device_decoder_reads_the_file_as_pillow_does(ops, name, quality):
    dev = torch.from_numpy(CASES[name]).cuda()
    data = ops.jpeg_bytes(dev, quality=quality, subsampling=420, huffman="optimized")
    pixels, status = ops.jpeg_decode_u8(data)
    assert int(status.item()) == 0
    assert np.array_equal(pixels.cpu().numpy(), np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))


def test_bad_arguments_raise(ops):
    """Refused before anything is launched: capacity below the bound, unknown modes, null pointers."""
    from faster_rcnn_amd import _lib
    from faster_rcnn_amd._lib import FrcnnError
    good = torch.zeros((20, 5, 3), dtype=torch.uint8, device="cuda")
    for kw in (dict(subsampling=422), dict(subsampling="420"), dict(subsampling=True), dict(huffman="optimised"), dict(huffman=1),
               dict(subsampling=420, quality=0)):
        with pytest.raises(FrcnnError):
            ops.jpeg_encode_u8(good, **kw)
    with pytest.raises(FrcnnError):
        ops.jpeg_bound(20, 5, subsampling=411)
    with pytest.raises(FrcnnError):
        ops.jpeg_workspace_bytes(20, 5, huffman="fast")
    with pytest.raises(FrcnnError):
        ops.jpeg_encode_u8(good, subsampling=420, out=torch.zeros(ops.jpeg_bound(20, 5, 420) - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(FrcnnError):
        ops.jpeg_encode_u8(good, huffman="optimized", workspace=torch.zeros(ops.jpeg_workspace_bytes(20, 5), dtype=torch.uint8, device="cuda"))
    with pytest.raises(FrcnnError):
        ops.jpeg_build_tables(np.zeros((3, 256), np.int64))
    # the C entries themselves: a status, not a launch
    lib, p = _lib.load(), ops._p
    out = torch.zeros(ops.jpeg_bound(20, 5, 420), dtype=torch.uint8, device="cuda")
    n = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.zeros(ops.jpeg_workspace_bytes(20, 5, 420, "optimized"), dtype=torch.uint8, device="cuda")
    call = lambda frame=p(good), sub=420, huff=1, o=p(out), cap=out.numel(), ln=p(n), w=p(ws): \
        lib.frcnn_jpeg_opt_encode_u8(frame, 20, 5, 0, 90, sub, huff, o, cap, ln, w, None)
    E_ARG = -1                                                              # include/frcnn_hip.h FRCNN_E_ARG
    for kw in (dict(cap=out.numel() - 1), dict(sub=422), dict(sub=0), dict(huff=2), dict(huff=-1), dict(frame=None), dict(o=None), dict(ln=None),
               dict(w=None)):
        assert call(**kw) == E_ARG, kw
    assert lib.frcnn_jpeg_opt_build_tables(None, p(ws), None) != 0 and lib.frcnn_jpeg_opt_build_tables(p(ws), None, None) != 0
    assert lib.frcnn_jpeg_opt_bound(20, 5, 422) == 0 and lib.frcnn_jpeg_opt_workspace_bytes(20, 5, 420, 2) == 0
    assert lib.frcnn_jpeg_opt_restart_mcus(444) == 16 and lib.frcnn_jpeg_opt_restart_mcus(420) == 8 and lib.frcnn_jpeg_opt_restart_mcus(1) == 0
    torch.cuda.synchronize()                                                # nothing was launched, nothing faulted
    assert int(n.item()) == 0 and not out.any()
    assert call() == 0
    torch.cuda.synchronize()
    assert 0 < int(n.item()) <= out.numel()
