"""The device JPEG encoder's 4:2:0 and optimised-Huffman modes, the parts that need no GPU: the C-ABI entry points in an extension header
of their own (include/ext/frcnn_hip_jpeg_opt.h), their ctypes table and the built library; the CPU restatement of the stream
(tests/jpeg_opt_ref.py) -- (444, standard) is tests/jpeg_ref.py's file, every mode's file is sound, the table construction is Pillow's
(libjpeg's jpeg_gen_optimal_table) byte for byte, fidelity and size lie beside Pillow's own file in the same mode; and annotate_video's
option grammar."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from tests import jpeg_dec_ref as D
from tests import jpeg_opt_ref as O
from tests import jpeg_ref as R
from tests.jpeg_opt_cases import CASES, QUALITIES, RUNS, fibonacci_histogram, pillow_tables, reference

Image = pytest.importorskip("PIL.Image")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("frcnn_jpeg_opt_version", "frcnn_jpeg_opt_restart_mcus", "frcnn_jpeg_opt_bound", "frcnn_jpeg_opt_workspace_bytes",
               "frcnn_jpeg_opt_encode_u8", "frcnn_jpeg_opt_build_tables")

# Fidelity and size beside Pillow's file (same quality, subsampling, optimize, restart_marker_blocks = the mode's interval), measured over
# RUNS with this file's test_fidelity_and_size_beside_pillow (it prints every figure), separately for 444 and for 420.  At 4:4:4 both
# encoders share tables and interval and the gaps come from the rounding of colour transform and DCT.  At 4:2:0 libjpeg also pads
# differently: it replicates the frame to whole 8x8 blocks per component and fills the blocks an MCU needs beyond them with the last
# block's DC, where this stream replicates the frame to whole 16x16 MCUs; frames whose sides are no multiple of 16 show it.  Observed
# worst gaps (PSNR deficit dB, PSNR surplus dB, size excess, size saving):
#   444: 0.051 dB (noise_13x21, quality 90), 0.297 dB (photo_96x128, quality 100), 0.188 % (photo_96x128, quality 10, optimized),
#        3.077 % (photo_96x128, quality 100, optimized)
#   420: 0.125 dB (photo_96x128, quality 100), 0.004 dB (noise_16x16, quality 90), 11.377 % (grey_24x40, quality 90, optimized: 24 rows,
#        so libjpeg codes the MCU rows' lower halves as DC-only blocks), 1.375 % (photo_96x128, quality 100, optimized);
#        on the frames that are whole MCUs the two files differ by at most 0.05 % at quality 90 and below
# Each margin is twice the worst gap observed on its side, with floors of 0.1 dB and 0.5 %.
MARGINS = {
    444: dict(deficit=0.1027, surplus=0.5941, excess=0.005, saving=0.0616),        # 2 x 0.05133, 2 x 0.29703, the floor (2 x 0.00188), 2 x 0.03078
    420: dict(deficit=0.2499, surplus=0.1, excess=0.2276, saving=0.0276),          # 2 x 0.12494, the floor (2 x 0.0043), 2 x 0.11378, 2 x 0.01376
}


def pillow_file(frame, quality, subsampling, huffman):
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="JPEG", quality=quality, subsampling=2 if subsampling == 420 else 0, optimize=huffman == "optimized",
                                restart_marker_blocks=O.RESTART[subsampling])
    return buf.getvalue()


def psnr(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    mse = float(np.mean(d * d))
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def decoded(data):
    img = Image.open(io.BytesIO(data))
    img.load()
    assert img.mode == "RGB"
    return img


def split(data):
    """-> ([(marker, payload)] SOI .. SOS, the entropy-coded bytes); asserts SOI at the start and EOI at the end."""
    assert data[:2] == b"\xFF\xD8" and data[-2:] == b"\xFF\xD9"
    segs, pos = [], 2
    while True:
        assert data[pos] == 0xFF
        marker, n = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        segs.append((marker, data[pos + 4:pos + 2 + n]))
        pos += 2 + n
        if marker == 0xDA:
            return segs, data[pos:-2]


def test_header_ctypes_and_library_agree_on_the_jpeg_opt_symbols():
    """The pattern of tests/test_jpeg_cpu.py: every symbol the header declares is in _lib.JPEG_OPT_SIGNATURES with matching argument
    kinds and exported by the built library, and nothing else is in that table; the revisions agree; the other headers and tables do not
    know the new symbols and keep their revisions."""
    from faster_rcnn_amd import _lib
    from faster_rcnn_amd.build import build_library
    ext = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_jpeg_opt.h")).read()
    version = int(re.search(r"#define FRCNN_JPEG_OPT_VERSION (\d+)", ext).group(1))
    assert version == _lib.JPEG_OPT_VERSION == 1 and re.search(r"^ \*   1 = ", ext, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    assert sorted(set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.JPEG_OPT_SIGNATURES) == sorted(NEW_SYMBOLS)
    build_library(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        m = re.search(r"\b(int|size_t) %s\s*\(([^)]*)\)" % name, code)
        assert m, name
        decls = [d for d in m.group(2).split(",") if d.strip() != "void"]
        restype, argtypes = _lib.JPEG_OPT_SIGNATURES[name]
        assert restype is {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[m.group(1)] and len(argtypes) == len(decls), name
        for decl, ct in zip(decls, argtypes):                            # pointers are pointers, sizes are sizes, ints are ints
            assert ("*" in decl) == (ct is ctypes.c_void_p), (name, decl)
            assert ("size_t" in decl) == (ct is ctypes.c_size_t), (name, decl)
        assert hasattr(lib, name), name
    loaded = _lib.load()
    assert loaded.frcnn_jpeg_opt_version() == version
    assert int(re.search(r"#define FRCNN_JPEG_OPT_444 (\d+)", ext).group(1)) == 444 and int(re.search(r"#define FRCNN_JPEG_OPT_420 (\d+)", ext).group(1)) == 420
    assert {k: int(re.search(r"#define FRCNN_JPEG_OPT_%s (\d+)" % k.upper(), ext).group(1)) for k in O.HUFFMANS} == _lib.JPEG_OPT_HUFFMANS
    assert tuple(_lib.JPEG_OPT_SUBSAMPLINGS) == O.SUBSAMPLINGS and ctypes.sizeof(_lib.JpegOptTable) == 276
    # all other revisions unchanged, and nobody else knows the new symbols
    core = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    ext_dir = os.path.join(ROOT, "include", "ext")
    others = "".join(open(os.path.join(ext_dir, f)).read() for f in sorted(os.listdir(ext_dir)) if f != "frcnn_hip_jpeg_opt.h")
    for name in NEW_SYMBOLS:
        assert name not in core and name not in others
        assert not any(name in t for t in (_lib.SIGNATURES, _lib.EXT_SIGNATURES, _lib.PNG_SIGNATURES, _lib.PNG_HUFF_SIGNATURES, _lib.JPEG_SIGNATURES,
                                           _lib.JPEG_DEC_SIGNATURES, _lib.JPEG_DEC_BATCH_SIGNATURES))
    assert loaded.frcnn_png_version() == _lib.PNG_VERSION == 1 and loaded.frcnn_png_huff_version() == _lib.PNG_HUFF_VERSION == 1
    assert loaded.frcnn_jpeg_version() == _lib.JPEG_VERSION == 1 and loaded.frcnn_jpeg_dec_version() == _lib.JPEG_DEC_VERSION == 1
    assert loaded.frcnn_jpeg_dec_batch_version() == _lib.JPEG_DEC_BATCH_VERSION == 1 and loaded.frcnn_vgg_canvas_version() == _lib.VGG_CANVAS_VERSION == 1
    assert loaded.frcnn_version() == _lib.ABI_VERSION == int(re.search(r"#define FRCNN_ABI_VERSION (\d+)", core).group(1))


def test_constants_and_bound():
    """The exported constants are the restatement's; the bound is its formula in both samplings, the same for both table modes, equal to
    revision 1's at 4:4:4, and refused where the header says."""
    from faster_rcnn_amd import _lib, ops
    from faster_rcnn_amd._lib import FrcnnError
    lib = _lib.load()
    assert [lib.frcnn_jpeg_opt_restart_mcus(s) for s in (444, 420, 422, 0)] == [16, 8, 0, 0]
    assert ops.jpeg_restart_mcus() == O.RESTART[444] == R.RESTART_MCUS and ops.jpeg_restart_mcus(420) == O.RESTART[420]
    sides = [1, 2, 8, 9, 15, 16, 17, 65, 375, 1242]
    for s in O.SUBSAMPLINGS:
        for h in sides:
            prev = 0
            for w in sides:
                b = ops.jpeg_bound(h, w, s)
                assert b == O.bound(h, w, s) == lib.frcnn_jpeg_opt_bound(h, w, s) == ops.jpeg_bound(h, w, s, "optimized") and b >= prev, (h, w, s)
                assert s != 444 or b == R.bound(h, w) == lib.frcnn_jpeg_bound(h, w)
                for f in O.HUFFMANS:
                    assert ops.jpeg_workspace_bytes(h, w, s, f) % 16 == 0
                assert ops.jpeg_workspace_bytes(h, w, s, "optimized") > ops.jpeg_workspace_bytes(h, w, s, "standard") > 0
                prev = b
    assert ops.jpeg_bound(375, 1242, 420) == R.HEADER_BYTES + 2 + 416 * 6 * 24 * 78 + 4 * 234
    assert ops.jpeg_bound(375, 1242) == R.HEADER_BYTES + 2 + 416 * 3 * 7332 + 4 * 459           # the default pair: revision 1's entry
    for h, w in ((0, 5), (5, 0), (-1, 5), (65536, 8), (8, 65536), (65535, 65535)):
        for s in O.SUBSAMPLINGS:
            assert O.bound(h, w, s) == 0 and lib.frcnn_jpeg_opt_bound(h, w, s) == 0 and lib.frcnn_jpeg_opt_workspace_bytes(h, w, s, 1) == 0
            with pytest.raises(FrcnnError):
                ops.jpeg_bound(h, w, s)
            with pytest.raises(FrcnnError):
                ops.jpeg_workspace_bytes(h, w, s, "optimized")
    assert lib.frcnn_jpeg_opt_bound(16, 16, 422) == 0 and lib.frcnn_jpeg_opt_workspace_bytes(16, 16, 420, 2) == 0
    for kw in (dict(subsampling=422), dict(subsampling="420"), dict(huffman="optimised"), dict(huffman=1)):
        with pytest.raises(FrcnnError):
            ops.jpeg_bound(16, 16, **kw)
        with pytest.raises(FrcnnError):
            ops.jpeg_workspace_bytes(16, 16, **kw)


@pytest.mark.parametrize("name,quality", QUALITIES)
def test_444_standard_is_revision_1(name, quality):
    frame = CASES[name]
    assert reference(name, quality, 444, "standard")[0] == R.encode(frame, quality)
    assert O.encode(np.ascontiguousarray(frame[:, :, ::-1]), quality, 420, "optimized", bgr=True) == reference(name, quality, 420, "optimized")[0]


def check_prefix_code(bits, vals, limit):
    """A (BITS, HUFFVAL) pair is a prefix code of at most 16 bits whose all-ones code stays free."""
    assert len(bits) == 16 and sum(bits) == len(vals) == len(set(vals)) and 1 <= len(vals) <= limit
    codes = R.huffman_codes(list(bits), list(vals))
    assert max(l for _, l in codes.values()) <= 16
    assert sum(2 ** (16 - l) for _, l in codes.values()) <= 2 ** 16 - 1                      # Kraft, with room for the all-ones code
    longest = max(l for _, l in codes.values())
    assert all(c != (1 << l) - 1 for c, l in codes.values() if l == longest)
    by_code = sorted(codes.values(), key=lambda cl: (cl[1], cl[0]))
    for (c1, l1), (c2, l2) in zip(by_code, by_code[1:]):                                      # no code is a prefix of a longer one
        assert (c2 >> (l2 - l1)) > c1


@pytest.mark.parametrize("name,quality,subsampling,huffman", RUNS)
def test_restatement_is_a_sound_file(name, quality, subsampling, huffman):
    from faster_rcnn_amd import ops
    frame = CASES[name]
    h, w = frame.shape[:2]
    data, info = reference(name, quality, subsampling, huffman)
    assert len(data) <= O.bound(h, w, subsampling) == ops.jpeg_bound(h, w, subsampling, huffman)
    img = decoded(data)
    assert img.size == (w, h)
    segs, ecs = split(data)
    assert [m for m, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    header = sum(4 + len(p) for _, p in segs) + 2
    assert header == info["intervals"][0] and (header == R.HEADER_BYTES if huffman == "standard" else header <= R.HEADER_BYTES)
    sof = segs[3][1]
    assert sof[:5] == bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big")
    assert sof[5:] == bytes([3, 1, 0x22 if subsampling == 420 else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])     # the sampling factors
    assert int.from_bytes(segs[8][1], "big") == O.RESTART[subsampling] == (8 if subsampling == 420 else 16)
    assert [p for m, p in segs if m == 0xDB] == [bytes([k] + t) for k, t in enumerate(R.quant_tables(quality))]
    my, mx = O.mcu_grid(h, w, subsampling)
    intervals = -(-(my * mx) // O.RESTART[subsampling])
    assert len(info["intervals"]) == intervals
    markers, i = [], 0
    while i < len(ecs):
        if ecs[i] == 0xFF:
            assert i + 1 < len(ecs) and (ecs[i + 1] == 0 or 0xD0 <= ecs[i + 1] <= 0xD7), "unstuffed 0xFF at %d" % i
            if ecs[i + 1]:
                markers.append(ecs[i + 1] - 0xD0)
            i += 2
        else:
            i += 1
    assert markers == [k & 7 for k in range(intervals - 1)]
    dht = [p for m, p in segs if m == 0xC4]
    assert [p[0] for p in dht] == list(O.TABLE_IDS)
    if huffman == "standard":
        assert [(list(p[1:17]), list(p[17:])) for p in dht] == [(b, v) for b, v in R.HUFFMAN]
    else:
        shorter = reference(name, quality, subsampling, "standard")[0]
        assert len(data) <= len(shorter), "the optimised file is longer than the standard one"
        for p, (bits, vals), hist, limit in zip(dht, info["tables"], info["hist"], (12, 162, 12, 162)):
            assert (list(p[1:17]), list(p[17:])) == (list(bits), list(vals))
            check_prefix_code(bits, vals, limit)
            assert sorted(vals) == [s for s in range(256) if hist[s]]                       # exactly the symbols the frame uses
    assert np.array_equal(D.decode(data), np.asarray(img)), "tests/jpeg_dec_ref.py and Pillow decode the file differently"
    if name == "noise_48x352" and subsampling == 420:
        assert intervals == 9 and markers[-2:] == [6, 7] and my * mx == 66
    if name == "flat_32x48" and huffman == "optimized":
        assert info["tables"][1] == ([1] + [0] * 15, [0]) and info["tables"][3] == ([1] + [0] * 15, [0])      # AC: EOB alone, one bit
    if name == "grey_24x40" and huffman == "optimized":
        assert info["tables"][2][1] == [0] and info["tables"][3][1] == [0]                   # chroma: category 0 and EOB only


def test_the_construction_is_pillows():
    """The restatement's table builder, fed the symbol histograms of Pillow's own optimize=True files (decoded by
    tests/jpeg_dec_ref.Entropy.serial()), returns each file's own BITS / HUFFVAL for all four tables; and on a Fibonacci histogram,
    whose unconstrained depth is 29, the length-limiting loop gives a legal table."""
    tables_seen, longest = 0, 0
    for label, hist, tables in pillow_tables():
        for k in range(4):
            assert O.optimal_table(hist[k]) == tables[k], (label, k)
            tables_seen += 1
            longest = max(longest, max(i + 1 for i, n in enumerate(tables[k][0]) if n))
    assert tables_seen == 4 * 36 and longest == 16
    hist = fibonacci_histogram()
    assert int(np.count_nonzero(hist)) == 30
    bits, vals = O.optimal_table(hist)
    assert len(bits) == 16 and sum(bits) == len(vals) == 30
    assert sum(n << (16 - (i + 1)) for i, n in enumerate(bits)) <= 2 ** 16 - 1               # Kraft; lengths <= 16 by the table's shape
    depth = {}                                                                               # the unconstrained depths: a plain Huffman tree
    import heapq
    heap = [(int(c), [s]) for s, c in enumerate(hist) if c] + [(1, [256])]
    heapq.heapify(heap)
    while len(heap) > 1:
        (a, x), (b, y) = heapq.heappop(heap), heapq.heappop(heap)
        for s in x + y:
            depth[s] = depth.get(s, 0) + 1
        heapq.heappush(heap, (a + b, x + y))
    assert max(depth.values()) >= 29 and bits[15] > 0                                        # ... so the limiting loop acted
    lengths = [i + 1 for i, n in enumerate(bits) for _ in range(n)]
    assert list(zip(lengths, vals)) == sorted(zip(lengths, vals)) and sorted(vals) == [s for s in range(256) if hist[s]]     # by (length, symbol)
    check_prefix_code(bits, vals, 162)
    assert O.optimal_table(np.zeros(256, np.int64)) == ([0] * 16, [])


def test_fidelity_and_size_beside_pillow():
    """Over every run: the restatement's PSNR against the source and its length, beside those of Pillow's own file in the same mode;
    separately for 444 and for 420.  Runs whose Pillow file decodes to the source exactly (infinite PSNR) are left out of the PSNR
    comparison only."""
    worst = {s: {"deficit": 0.0, "surplus": 0.0, "excess": 0.0, "saving": 0.0} for s in O.SUBSAMPLINGS}
    failures = []
    for name, quality, s, f in RUNS:
        frame = CASES[name]
        mine, pil = reference(name, quality, s, f)[0], pillow_file(frame, quality, s, f)
        size_gap = (len(mine) - len(pil)) / len(pil)
        p_mine, p_pil = psnr(np.asarray(decoded(mine)), frame), psnr(np.asarray(decoded(pil)), frame)
        print("%-16s q%3d %d %-9s: %6d bytes, Pillow %6d (%+.3f %%); PSNR %.3f dB, Pillow %.3f" % (name, quality, s, f, len(mine), len(pil),
                                                                                                 100 * size_gap, p_mine, p_pil))
        w, m = worst[s], MARGINS[s]
        w["excess"], w["saving"] = max(w["excess"], size_gap), max(w["saving"], -size_gap)
        if not -m["saving"] <= size_gap <= m["excess"]:
            failures.append((name, quality, s, f, "size", size_gap))
        if np.isinf(p_pil):
            continue
        w["deficit"], w["surplus"] = max(w["deficit"], p_pil - p_mine), max(w["surplus"], p_mine - p_pil)
        if not -m["surplus"] <= p_pil - p_mine <= m["deficit"]:
            failures.append((name, quality, s, f, "psnr", p_mine, p_pil))
    print("worst gaps:", worst)
    assert not failures, failures


def test_option_check(monkeypatch):
    from faster_rcnn_amd import annotate_video as av
    for var in ("FRCNN_ANNOTATE_FRAME_FORMAT", "FRCNN_ANNOTATE_JPEG_ENCODER", "FRCNN_ANNOTATE_PNG_ENCODER", "FRCNN_ANNOTATE_PNG_COMPRESS",
                "FRCNN_ANNOTATE_JPEG_SUBSAMPLING", "FRCNN_ANNOTATE_JPEG_HUFFMAN"):
        monkeypatch.delenv(var, raising=False)
    p = av.build_parser()
    args = p.parse_args(["a", "b", "c"])
    assert (args.frame_format, args.jpeg_subsampling, args.jpeg_huffman) == ("png", 444, "standard")
    args = p.parse_args(["a", "b", "c", "--frame_format", "jpg", "--jpeg_subsampling", "420", "--jpeg_huffman", "optimized"])
    assert (args.frame_format, args.jpeg_subsampling, args.jpeg_huffman) == ("jpg", 420, "optimized")
    for argv in (["--jpeg_subsampling", "422"], ["--jpeg_subsampling", "4:2:0"], ["--jpeg_huffman", "optimised"]):
        with pytest.raises(SystemExit):
            p.parse_args(["a", "b", "c", "--frame_format", "jpg"] + argv)
    assert av.jpeg_options() == ("png", "host", 90) and av.jpeg_options("jpg", "device", 1) == ("jpg", "device", 1)      # signature and 3-tuple as before
    # every legal combination: both options with jpg frames, whichever encoder; the defaults with png frames
    assert av.jpeg_size_options("png") == (444, "standard") and av.jpeg_size_options("png", 444, "standard") == (444, "standard")
    for s in (444, 420):
        for f in ("standard", "optimized"):
            assert av.jpeg_size_options("jpg", s, f) == (s, f)
    assert av.jpeg_size_options("jpg") == (444, "standard") and av.jpeg_size_options("jpg", None, "optimized") == (444, "optimized")
    assert av.jpeg_size_options("jpg", np.int64(420)) == (420, "standard")
    # every refused one
    for args in (("png", 420), ("png", None, "optimized"), ("png", 420, "optimized"), ("jpg", 422), ("jpg", "420"), ("jpg", True), ("jpg", 420.5),
                 ("jpg", 444, "optimised"), ("jpg", 444, 1), ("jpg", 0), ("png", 411)):
        with pytest.raises(ValueError):
            av.jpeg_size_options(*args)
    for argv in (["--jpeg_subsampling", "420"], ["--jpeg_huffman", "optimized"], ["--jpeg_subsampling", "420", "--jpeg_huffman", "optimized"],
                 ["--png_encoder", "device", "--jpeg_huffman", "optimized"]):
        with pytest.raises(ValueError):                                     # ... before any model file is opened
            av.main(["no.npz", "no.npz", "nowhere"] + argv)
    for kw in (dict(jpeg_subsampling=420), dict(jpeg_huffman="optimized"), dict(frame_format="png", jpeg_subsampling=420, jpeg_huffman="optimized"),
               dict(frame_format="jpg", jpeg_subsampling=422), dict(frame_format="jpg", jpeg_huffman="best"),
               dict(frame_format="jpg", jpeg_encoder="device", jpeg_subsampling=411)):
        with pytest.raises(ValueError):
            av.annotate_images(None, None, "nowhere", "nowhere", [], 600, 1000, **kw)
    # the environment variables set the defaults of flags and keywords alike
    monkeypatch.setenv("FRCNN_ANNOTATE_JPEG_SUBSAMPLING", "420")
    monkeypatch.setenv("FRCNN_ANNOTATE_JPEG_HUFFMAN", "optimized")
    args = av.build_parser().parse_args(["a", "b", "c"])
    assert (args.jpeg_subsampling, args.jpeg_huffman) == (420, "optimized")
    assert av.jpeg_size_options("jpg") == (420, "optimized") and av.jpeg_size_options("jpg", 444) == (444, "optimized")
    with pytest.raises(ValueError):
        av.jpeg_size_options("png")                                         # the defaults now ask for JPEG settings
    with pytest.raises(ValueError):
        av.main(["no.npz", "no.npz", "nowhere"])
    monkeypatch.setenv("FRCNN_ANNOTATE_JPEG_SUBSAMPLING", "422")
    with pytest.raises(ValueError):
        av.default_jpeg_subsampling()
    monkeypatch.setenv("FRCNN_ANNOTATE_JPEG_SUBSAMPLING", "444")
    monkeypatch.setenv("FRCNN_ANNOTATE_JPEG_HUFFMAN", "fast")
    with pytest.raises(ValueError):
        av.default_jpeg_huffman()


def test_host_leg_passes_the_options_to_pil(tmp_path):
    """annotate_video's host writer: subsampling=0|2 and optimize= reach PIL, and the defaults write the file they wrote before."""
    from faster_rcnn_amd import annotate_video as av
    frame = CASES["photo_96x128"]
    sizes = {}
    for s, f in [(444, "standard"), (444, "optimized"), (420, "standard"), (420, "optimized")]:
        path = str(tmp_path / ("%d_%s.jpg" % (s, f)))
        av._write_jpg(path, frame, 90, s, f)
        data = open(path, "rb").read()
        buf = io.BytesIO()
        Image.fromarray(frame).save(buf, format="JPEG", quality=90, subsampling=2 if s == 420 else 0, optimize=f == "optimized")
        assert data == buf.getvalue()
        assert D.plan(data).hs == (2 if s == 420 else 1)
        sizes[s, f] = len(data)
    assert sizes[420, "optimized"] < sizes[420, "standard"] < sizes[444, "standard"] and sizes[444, "optimized"] < sizes[444, "standard"]
    path = str(tmp_path / "default.jpg")
    av._write_jpg(path, frame, 90)
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="JPEG", quality=90, subsampling=0)
    assert open(path, "rb").read() == buf.getvalue()
