"""The huffman mode of the device PNG encoder (faster_rcnn_amd/csrc/png.hip through ops.png_encode_u8 / ops.png_bytes with
compress="huffman") against its CPU restatement (tests/png_huff_ref.py): the device file equals the restatement's byte for byte, in both
channel orders, on the smallest frames at which each mechanism can break (tests/png_huff_cases.py); it is the same from run to run, a
sound chunk sequence with correct CRCs, and Pillow decodes it to the frame."""
import io
import struct
import zlib

import numpy as np
import pytest

from tests import png_huff_ref as R
from tests.png_huff_cases import CASES, banded

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
Image = pytest.importorskip("PIL.Image")

SIGNATURE = b"\x89PNG\r\n\x1a\n"


@pytest.fixture(scope="module")
def ops():
    from faster_rcnn_amd import ops as o
    return o


def chunks_of(png):
    """[(type, data)] of a PNG file; asserts the signature, every CRC, and that nothing follows IEND."""
    assert png[:8] == SIGNATURE
    out, pos = [], 8
    while pos < len(png):
        n, kind = struct.unpack(">I4s", png[pos:pos + 8])
        data = png[pos + 8:pos + 8 + n]
        assert len(data) == n
        assert struct.unpack(">I", png[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + data), (kind, len(out))
        out.append((kind, data))
        pos += 12 + n
        if kind == b"IEND":
            break
    assert pos == len(png), "bytes behind IEND"
    return out


def block_types(chunks):
    """BTYPE of the first deflate block of every band's IDAT (every band starts on a byte; band 0 behind the zlib header)."""
    return [(d[2] if i == 0 else d[0]) >> 1 & 3 for i, (_, d) in enumerate(chunks[1:-2])]


def check(ops, frame, bgr=False):
    h, w = frame.shape[:2]
    dev = torch.from_numpy(np.ascontiguousarray(frame)).cuda()
    png = ops.png_bytes(dev, bgr=bgr, compress="huffman")
    assert ops.png_bytes(dev, bgr=bgr, compress="huffman") == png, "two encodes of one frame differ"
    assert len(png) <= ops.png_bound(h, w, "huffman")
    chunks = chunks_of(png)
    assert chunks[0] == (b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
    assert chunks[-1] == (b"IEND", b"") and len(chunks) == 3 + -(-h // ops.PNG_HUFF_BAND_ROWS)
    assert all(kind == b"IDAT" for kind, _ in chunks[1:-1])
    raw = zlib.decompress(b"".join(data for _, data in chunks[1:-1]))      # (checks the Adler-32 too)
    assert len(raw) == h * (1 + 3 * w)
    img = Image.open(io.BytesIO(png))
    img.load()
    assert img.mode == "RGB" and img.size == (w, h)
    assert np.array_equal(np.asarray(img), frame[:, :, ::-1] if bgr else frame)
    info = {}
    want = R.encode(frame, bgr=bgr, info=info)
    if png != want:
        first = next((i for i, (a, b) in enumerate(zip(png, want)) if a != b), min(len(png), len(want)))
        raise AssertionError("device file (%d bytes) differs from the restatement's (%d) at byte %d" % (len(png), len(want), first))
    return png, chunks, raw, info


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("bgr", [False, True])
def test_equals_the_restatement(ops, name, bgr):
    frame = CASES[name]
    h, w = frame.shape[:2]
    png, chunks, raw, info = check(ops, frame, bgr=bgr)
    kinds = block_types(chunks)
    if name.startswith("noise"):
        assert set(kinds) == {0} and set(info["forms"]) == {"stored"}       # BTYPE 00: the stored fallback
    if name == "noise_long_band":
        assert ops.PNG_HUFF_BAND_ROWS * (1 + 3 * w) > 65535 and len(chunks[1][1]) > 65535 + 2 + 10      # two stored blocks
    if name == "flat_64x100":
        assert len(png) <= frame.nbytes // 8, len(png)
    if name.startswith("banded") or name.endswith("_band") and not name.startswith("noise"):
        assert set(kinds) == {2}, kinds                                     # BTYPE 10
    if name == "five_filters":
        assert set(raw[::1 + 3 * w]) == {0, 1, 2, 3, 4}
    if name in ("fibonacci_band", "code_length_ladder_band") and not bgr:
        # the property the case exists for, from the restatement's own tree: without the limit the code would be too long
        plan = R.band_plan(np.frombuffer(raw, np.uint8))
        if name == "fibonacci_band":
            assert max(R.tree_depths(plan["freq"]).values()) > 15 and max(plan["lit_len"]) == 15
        else:
            assert max(R.tree_depths(plan["cl_freq"]).values()) > 7 and max(plan["cl_len"]) == 7


def test_band_rows_cases_cover_partial_bands(ops):
    assert ops.PNG_HUFF_BAND_ROWS == R.BAND_ROWS
    assert CASES["banded_plus"].shape[0] == 12 * R.BAND_ROWS + 1 and CASES["banded_minus"].shape[0] == 12 * R.BAND_ROWS - 1


def test_bad_arguments_raise(ops):
    from faster_rcnn_amd._lib import FrcnnError
    good = torch.zeros((4, 5, 3), dtype=torch.uint8, device="cuda")
    for bad in (torch.zeros((4, 5), dtype=torch.uint8, device="cuda"), torch.zeros((4, 5, 4), dtype=torch.uint8, device="cuda"),
                torch.zeros((0, 5, 3), dtype=torch.uint8, device="cuda"), torch.zeros((4, 0, 3), dtype=torch.uint8, device="cuda"),
                torch.zeros((4, 5, 3), dtype=torch.float32, device="cuda")):
        with pytest.raises(FrcnnError):
            ops.png_encode_u8(bad, compress="huffman")
    with pytest.raises(FrcnnError):
        ops.png_encode_u8(good, out=torch.zeros(ops.png_bound(4, 5, "huffman") - 1, dtype=torch.uint8, device="cuda"), compress="huffman")
    with pytest.raises(FrcnnError):
        ops.png_encode_u8(good, workspace=torch.zeros(16, dtype=torch.uint8, device="cuda"), compress="huffman")
    with pytest.raises(FrcnnError):
        ops.png_encode_u8(good, compress="lz77")
    with pytest.raises(FrcnnError):
        ops.png_bound(0, 5, "huffman")
    with pytest.raises(FrcnnError):
        ops.png_bound(4, 5, "lz77")
    torch.cuda.synchronize()                                                # nothing was launched, nothing faulted
    out, n = ops.png_encode_u8(good, compress="huffman")
    assert 0 < int(n.item()) <= out.numel() == ops.png_bound(4, 5, "huffman")


def test_graph_replay(ops):
    """png_encode_u8(compress="huffman") captured once, replayed over three frames written into the same input tensor: each result is the
    eager encode of its frame."""
    h, w = 21, 34
    frames = [banded(h, w), np.random.RandomState(2).randint(0, 256, (h, w, 3)).astype(np.uint8), np.full((h, w, 3), 5, np.uint8)]
    src = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    out = torch.zeros(ops.png_bound(h, w, "huffman"), dtype=torch.uint8, device="cuda")
    out_len = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.zeros(ops.png_workspace_bytes(h, w, "huffman"), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.png_encode_u8(src, bgr=True, out=out, out_len=out_len, workspace=ws, compress="huffman")
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        ops.png_encode_u8(src, bgr=True, out=out, out_len=out_len, workspace=ws, compress="huffman")
    lengths = []
    for f in frames:
        src.copy_(torch.from_numpy(f).cuda())
        g.replay()
        torch.cuda.synchronize()
        n = int(out_len.item())
        assert 0 < n <= out.numel()
        png = out[:n].cpu().numpy().tobytes()
        chunks_of(png)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(png))), f[:, :, ::-1])
        assert png == ops.png_bytes(torch.from_numpy(f).cuda(), bgr=True, compress="huffman") == R.encode(f, bgr=True)
        lengths.append(n)
    assert len(set(lengths)) == 3, lengths


def test_runs_mode_is_what_it_was(ops):
    """compress="runs" is the call without the argument, byte for byte."""
    for name in ("banded_plus", "noise_37x53", "five_filters"):
        dev = torch.from_numpy(CASES[name]).cuda()
        for bgr in (False, True):
            assert ops.png_bytes(dev, bgr=bgr, compress="runs") == ops.png_bytes(dev, bgr=bgr)
            assert ops.png_bytes(dev, bgr=bgr, compress="runs") != ops.png_bytes(dev, bgr=bgr, compress="huffman")
    assert ops.png_bound(97, 131, "runs") == ops.png_bound(97, 131)
    assert ops.png_workspace_bytes(97, 131, "runs") == ops.png_workspace_bytes(97, 131)
