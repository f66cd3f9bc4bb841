"""The device PNG encoder (faster_rcnn_amd/csrc/png.hip through ops.png_encode_u8 / ops.png_bytes) against Pillow's decoder and the
standard library's zlib: every file decodes to its frame, is a well-formed chunk sequence with correct CRCs and Adler-32, stays under
ops.png_bound and is the same bytes from run to run.  The shapes are the smallest at which each mechanism of the encoder can break."""
import io
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
Image = pytest.importorskip("PIL.Image")

SIGNATURE = b"\x89PNG\r\n\x1a\n"
TILE = 4096                     # filtered bytes one workgroup tokenises at a time (png.hip PNG_TILE): runs are cut there


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


def check(ops, frame, bgr=False):
    """Encode ``frame`` (numpy (h, w, 3) uint8) twice and check everything the module docstring lists; -> (the file, its chunks)."""
    h, w = frame.shape[:2]
    dev = torch.from_numpy(np.ascontiguousarray(frame)).cuda()
    png = ops.png_bytes(dev, bgr=bgr)
    assert ops.png_bytes(dev, bgr=bgr) == png, "two encodes of one frame differ"
    assert len(png) <= ops.png_bound(h, w)
    chunks = chunks_of(png)
    assert chunks[0] == (b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
    assert chunks[-1] == (b"IEND", b"") and len(chunks) >= 3
    assert all(kind == b"IDAT" for kind, _ in chunks[1:-1])
    raw = zlib.decompress(b"".join(data for _, data in chunks[1:-1]))      # (checks the Adler-32 too)
    assert len(raw) == h * (1 + 3 * w)
    img = Image.open(io.BytesIO(png))
    img.load()
    assert img.mode == "RGB" and img.size == (w, h)
    assert np.array_equal(np.asarray(img), frame[:, :, ::-1] if bgr else frame)
    return png, chunks


def banded(h, w):
    """Flat bands with a green rectangle: what a drawn frame looks like."""
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([(x // 7 * 3) % 256, (y // 5 * 9) % 256, ((x + y) // 11 * 5) % 256], -1).astype(np.uint8)
    a[h // 5:h // 2, w // 6:w // 6 * 4] = (0, 255, 0)
    return a


def run_rows(w, lengths):
    """One row per entry of ``lengths``, whose Sub-filtered bytes hold one run of exactly that many bytes equal to their predecessor.
    Neighbouring pixels differ in every channel (no other zeros); pixels 3 .. 3 + p share a colour (3p zeros: a first zero and 3p - 1
    repeats of it), and the pixel behind them shares that colour's first 0, 1 or 2 channels, which adds as many zeros."""
    i = np.arange(w)
    base = np.stack([(i * 37 + 11) % 256, (i * 59 + 3) % 256, (i * 83 + 7) % 256], -1).astype(np.uint8)
    f = np.zeros((len(lengths), w, 3), np.uint8)
    for r, run in enumerate(lengths):
        p, extra = divmod(run + 1, 3)
        assert p + 6 < w
        row = base.copy()
        row[3:4 + p] = row[3]
        row[4 + p, :extra] = row[3, :extra]
        f[r] = row
    return f


def zero_runs(frame):
    """Lengths of the maximal runs of bytes equal to their predecessor, per row of the Sub-filtered stream."""
    x = frame.astype(np.int16)
    sub = x.copy()
    sub[:, 1:] -= x[:, :-1]
    filt = np.concatenate([np.ones((frame.shape[0], 1), np.uint8), (sub & 255).astype(np.uint8).reshape(frame.shape[0], -1)], axis=1)
    out = []
    for row in filt:
        same = np.concatenate([[False], row[1:] == row[:-1], [False]])
        edges = np.flatnonzero(same[1:] != same[:-1])
        out.append([int(b - a) for a, b in zip(edges[::2], edges[1::2])])
    return out


def cases():
    rs = np.random.RandomState(3)
    from faster_rcnn_amd import ops
    band = ops.PNG_BAND_ROWS
    wide = (TILE + 200) // 3                                                # a row that spans two tiles of the tokeniser
    return {
        "1x1": np.array([[[1, 2, 3]]], np.uint8),
        "1x7": rs.randint(0, 256, (1, 7, 3)).astype(np.uint8),
        "7x1": rs.randint(0, 256, (7, 1, 3)).astype(np.uint8),
        "noise_37x53": rs.randint(0, 256, (37, 53, 3)).astype(np.uint8),
        "noise_high_40x60": rs.randint(144, 256, (40, 60, 3)).astype(np.uint8),
        "flat_64x100": np.full((64, 100, 3), 77, np.uint8),
        "banded_plus": banded(12 * band + 1, 131),                         # one row more / fewer than whole bands, 12 and more bands
        "banded_minus": banded(12 * band - 1, 131),
        # each pixel four times over: literals of both code lengths between short matches, so the fixed form wins and is what is checked
        "noise_x4_9x80": np.repeat(rs.randint(0, 256, (9, 20, 3)).astype(np.uint8), 4, axis=1),
        "flat_two_tiles": np.full((3, wide, 3), 200, np.uint8),
        "banded_two_tiles": banded(5, wide),
    }


CASES = cases()


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("bgr", [False, True])
def test_decodes_and_is_well_formed(ops, name, bgr):
    frame = CASES[name]
    assert frame.shape[0] >= 3 * ops.PNG_BAND_ROWS or not name.startswith("banded_")
    png, chunks = check(ops, frame, bgr=bgr)
    if name == "noise_high_40x60":
        # every literal costs 9 bits: each band must have fallen back to stored blocks (BFINAL = 0, BTYPE = 00 -> a first byte 0x00)
        datas = [d for _, d in chunks[1:-1]]
        assert datas[0][:2] == b"\x78\x01" and datas[0][2] == 0 and all(d[0] == 0 for d in datas[1:-1])
    if name == "flat_64x100":
        # fixed-code literals alone cannot get under the raw size: an eighth of it proves run matching (a condition, not a measurement)
        assert len(png) <= frame.nbytes // 8, len(png)
    if name == "noise_x4_9x80":
        assert all((d[2] if i == 0 else d[0]) & 7 == 2 for i, (_, d) in enumerate(chunks[1:-2])), "expected fixed-Huffman blocks"
        assert len(png) < frame.nbytes


def test_runs_that_end_at_258_259_260(ops):
    """Runs of exactly 258, 259 and 260 repeats in separate rows of a wide frame: one full match; a full match and a literal; a full match
    and a tail of 2, which is below the shortest match and must become literals."""
    frame = run_rows(120, [258 - 1, 258, 259, 260, 258 + 3])
    runs = zero_runs(frame)
    assert [max(r) for r in runs] == [257, 258, 259, 260, 261], runs
    check(ops, frame)
    check(ops, frame, bgr=True)


def test_band_longer_than_a_stored_block(ops):
    """A band is PNG_BAND_ROWS scanlines, so a wide enough frame makes one of more than 65535 filtered bytes; as noise it takes the stored
    form, which must then be split into blocks of at most 65535."""
    w = 65535 // (3 * ops.PNG_BAND_ROWS) + 40
    assert ops.PNG_BAND_ROWS * (1 + 3 * w) > 65535
    frame = np.random.RandomState(8).randint(0, 256, (2 * ops.PNG_BAND_ROWS, w, 3)).astype(np.uint8)
    png, chunks = check(ops, frame)
    assert all(len(d) > 65535 + 10 for _, d in chunks[1:-2])
    # ... and the same width flat: the fixed form across seventeen tiles
    png, _ = check(ops, np.full((ops.PNG_BAND_ROWS, w, 3), 9, np.uint8))
    assert len(png) < 3 * w // 8


def test_bad_arguments_raise(ops):
    from faster_rcnn_amd._lib import FrcnnError
    good = torch.zeros((4, 5, 3), dtype=torch.uint8, device="cuda")
    for bad in (torch.zeros((4, 5), dtype=torch.uint8, device="cuda"), torch.zeros((4, 5, 4), dtype=torch.uint8, device="cuda"),
                torch.zeros((0, 5, 3), dtype=torch.uint8, device="cuda"), torch.zeros((4, 0, 3), dtype=torch.uint8, device="cuda"),
                torch.zeros((4, 5, 3), dtype=torch.float32, device="cuda")):
        with pytest.raises(FrcnnError):
            ops.png_encode_u8(bad)
    with pytest.raises(FrcnnError):
        ops.png_encode_u8(good, out=torch.zeros(ops.png_bound(4, 5) - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(FrcnnError):
        ops.png_encode_u8(good, workspace=torch.zeros(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(FrcnnError):
        ops.png_bound(0, 5)
    torch.cuda.synchronize()                                                # nothing was launched, nothing faulted
    out, n = ops.png_encode_u8(good)
    assert 0 < int(n.item()) <= out.numel() == ops.png_bound(4, 5)


def test_graph_replay(ops):
    """png_encode_u8 captured once, replayed over three frames written into the same input tensor: each result decodes to its frame and
    the length word follows the content."""
    h, w = 21, 34
    frames = [banded(h, w), np.random.RandomState(2).randint(0, 256, (h, w, 3)).astype(np.uint8), np.full((h, w, 3), 5, np.uint8)]
    src = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    out = torch.zeros(ops.png_bound(h, w), dtype=torch.uint8, device="cuda")
    out_len = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.zeros(ops.png_workspace_bytes(h, w), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.png_encode_u8(src, bgr=True, out=out, out_len=out_len, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        _, _ = ops.png_encode_u8(src, bgr=True, out=out, out_len=out_len, workspace=ws)
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
        assert png == ops.png_bytes(torch.from_numpy(f).cuda(), bgr=True)
        lengths.append(n)
    assert len(set(lengths)) == 3, lengths
