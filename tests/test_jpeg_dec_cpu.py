"""The device JPEG decoder without a GPU: the CPU restatement (tests/jpeg_dec_ref.py) against Pillow byte for byte, its parallel form
against its serial form, the planner (the restatement's and the library's) on supported, unsupported and truncated files, a damaged
scan, and the options that switch the decoder on."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from tests import jpeg_dec_cases as C
from tests import jpeg_dec_ref as D

Image = pytest.importorskip("PIL.Image")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["frcnn_jpeg_dec_version", "frcnn_jpeg_dec_plan", "frcnn_jpeg_dec_workspace_bytes", "frcnn_jpeg_decode_u8"]
ROUNDS = {}          # file -> (rounds, N, S) of the parallel form, printed by test_parallel_form_is_the_serial_form


def pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.mark.parametrize("name", sorted(C.files()))
def test_restatement_is_pillow(name):
    """decode(file) == Pillow's RGB pixels, byte for byte: every sampling class, the ends of the quality scale, custom Huffman tables,
    restart intervals of 1 and 16 MCUs, a grey file, and the sizes that hit every edge rule of the upsampling."""
    data = C.files()[name]
    info = {}
    got = D.decode(data, info=info)
    want = pillow(data)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), (name, int(np.abs(got.astype(int) - want).max()), int((got != want).sum()))
    assert info["status"] == 0 and info["blocks"] == D.plan(data).expected_blocks
    assert np.array_equal(D.decode(data, bgr=True), want[:, :, ::-1])


def test_the_cases_cover_the_supported_set():
    plans = {name: D.plan(data) for name, data in C.files().items()}
    assert {(p.ncomp, p.hs, p.vs) for p in plans.values()} == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    assert {p.restart_interval for p in plans.values()} == {0, 1, 16}
    assert any(-(-p.w // 2) <= 2 and p.hs == 2 for p in plans.values()) and any(p.w % 2 and p.h % 2 and p.vs == 2 for p in plans.values())
    golden = plans["golden_000005"]
    assert (golden.h, golden.w, golden.hs, golden.vs, golden.restart_interval) == (375, 500, 2, 2, 0)
    assert {p.S for p in plans.values()} >= {D.MIN_S, golden.S} and golden.S > D.MIN_S and plans["64x136_s0_q100"].S > D.MIN_S
    assert all(p.S % 4 == 0 and p.S >= D.MIN_S and 1 <= p.N <= D.MAX_LANES and p.N * p.S >= p.scan_len for p in plans.values())
    # custom Huffman tables: an optimised file's DHT payloads differ from the golden file's Annex K tables
    def tables(data, p):
        return [data[p.dht_off[c][t]:p.dht_off[c][t] + 16 + p.dht_n[c][t]] for c in (0, 1) for t in (0, 1)]
    annex_k = tables(C.files()["golden_000005"], golden)
    assert tables(C.files()["17x23_s2_q75"], plans["17x23_s2_q75"]) == annex_k
    assert tables(C.files()["photo_s2_q75_optimize"], plans["photo_s2_q75_optimize"]) != annex_k


@pytest.mark.parametrize("name", sorted(C.files()))
def test_parallel_form_is_the_serial_form(name):
    """The same coefficients, block total and status from the subsequence form as from the serial walk, within N rounds (asserted inside
    ``Entropy.parallel``: the loop may not start round N + 1), for S at its minimum and where S has grown with the file."""
    data = C.files()[name]
    p = D.plan(data)
    info = {}
    serial = D.coefficients(data, p, "serial")
    parallel = D.coefficients(data, p, "parallel", info)
    assert np.array_equal(serial[0], parallel[0]) and serial[1:] == parallel[1:] == (p.expected_blocks, 0)
    assert 1 <= info["rounds"] <= info["N"] == p.N and info["S"] == p.S
    ROUNDS[name] = (info["rounds"], p.N, p.S)
    print("rounds", name, ROUNDS[name])


def test_library_planner_is_the_restatement():
    """frcnn_jpeg_dec_plan fills the fields the restatement's plan does, on every file; the header, the ctypes table and the exported
    symbols agree; the other extensions keep their revisions."""
    from faster_rcnn_amd import _lib, ops
    ext = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_jpeg_dec.h")).read()
    version = int(re.search(r"#define FRCNN_JPEG_DEC_VERSION (\d+)", ext).group(1))
    assert version == _lib.JPEG_DEC_VERSION == 1 and re.search(r"^ \*   1 = ", ext, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    assert sorted(set(re.findall(r"\b(frcnn_jpeg_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.JPEG_DEC_SIGNATURES) == sorted(NEW_SYMBOLS)
    lib = _lib.load()
    assert lib.frcnn_jpeg_dec_version() == version and lib.frcnn_jpeg_version() == _lib.JPEG_VERSION == 1
    for bit in ("BLOCKS", "ZIGZAG", "CODE", "TABLE"):
        assert int(re.search(r"#define FRCNN_JPEG_DEC_%s (\d+)" % bit, ext).group(1)) == getattr(_lib, "JPEG_DEC_" + bit) == getattr(D, "STATUS_" + bit)
    fields = re.search(r"typedef struct frcnn_jpeg_dec_plan \{(.*?)\}", code, flags=re.S).group(1)
    names = [n.split("[")[0] for decl in fields.split(";") if decl.strip() for n in re.sub(r"^\s*\w+\s", "", decl.strip()).replace(" ", "").split(",")]
    assert names == [f[0] for f in _lib.JpegDecPlan._fields_]
    for name, data in C.files().items():
        p, q = ops.jpeg_dec_plan(data), D.plan(data)
        assert (p.h, p.w, p.components, p.hs, p.vs, p.mcus_x, p.mcus_y, p.blocks_per_mcu) == (q.h, q.w, q.ncomp, q.hs, q.vs, q.mcus_x, q.mcus_y, q.bpm), name
        assert (p.expected_blocks, p.restart_interval, p.file_len, p.scan_off, p.scan_len) == (q.expected_blocks, q.restart_interval, len(data), q.scan_off, q.scan_len)
        assert list(p.dqt_off)[:q.ncomp] == q.dqt_off[:q.ncomp] and [list(r) for r in p.dht_off] == q.dht_off and [list(r) for r in p.dht_count] == q.dht_n
        assert list(p.comp_dc)[:q.ncomp] == q.comp_dc[:q.ncomp] and list(p.comp_ac)[:q.ncomp] == q.comp_ac[:q.ncomp]
        assert (p.subsequence_bytes, p.subsequences) == (q.S, q.N)
        need = ops.jpeg_dec_workspace_bytes(p)
        assert need % 16 == 0 and q.expected_blocks * 193 <= need <= q.expected_blocks * 193 + 16 * 5
    bad = ops.jpeg_dec_plan(C.files()["golden_000005"])
    bad.subsequences = 2000
    assert lib.frcnn_jpeg_dec_workspace_bytes(ctypes.byref(bad)) == 0
    with pytest.raises(_lib.FrcnnError):
        ops.jpeg_dec_workspace_bytes(bad)


def both_planners_refuse(data, word):
    from faster_rcnn_amd import ops
    with pytest.raises(D.Unsupported) as e:
        D.plan(data)
    assert word in str(e.value), (word, str(e.value))
    with pytest.raises(ops.JpegUnsupported) as e:
        ops.jpeg_dec_plan(data)
    assert word in str(e.value) and str(e.value).endswith(str(D.Unsupported(e.value)).split("jpeg_dec_plan: ")[-1])
    return str(e.value)


def test_planner_refuses_what_is_outside_the_set():
    """Decided from the headers, with the reason: progressive, CMYK, R G B kept (Adobe transform 0), other sampling factors, 12 bits;
    an empty file; a file that is no JPEG; and a supported file cut at every marker boundary of its headers (and one byte either side)."""
    for name, (data, word) in C.unsupported().items():
        if name in ("progressive", "cmyk", "rgb_ids"):
            assert pillow(data).shape == (17, 23, 3)                # (Pillow reads what it wrote: the caller's fallback)
        both_planners_refuse(data, word)
    both_planners_refuse(b"", "empty")
    both_planners_refuse(b"\x89PNG\r\n\x1a\n" + bytes(32), "not a JPEG")
    for name in ("golden_000005", "photo_s1_q90_optimize_rst16", "grey_17x23_q75"):
        data = C.files()[name]
        p = D.plan(data)
        cuts, pos = [], 2
        while pos < p.scan_off:                                       # the marker boundaries SOI | APP0 | DQT ... | SOS |
            cuts.append(pos)
            pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
        assert pos == p.scan_off and len(cuts) >= 6
        for cut in sorted({c + d for c in cuts + [p.scan_off] for d in (-1, 0, 1) if c + d <= p.scan_off} | {1, 2, 3}):
            both_planners_refuse(data[:cut], "truncated" if cut >= 4 else "not a JPEG")
        assert D.plan(data[:p.scan_off + 2]).scan_len == 2             # a cut scan is the status word's business


def test_damaged_scan_yields_a_status_not_a_fault():
    """A stretch of the scan overwritten: both forms end (the parallel one within N rounds), agree, report the same non-zero status with
    the block total off, and write nothing outside the coefficient array (the restatement indexes numpy arrays: an index past the end
    raises)."""
    data = C.damaged()
    p = D.plan(data)
    assert (p.h, p.w, p.expected_blocks) == (33, 65, D.plan(C.files()[C.DAMAGE_OF]).expected_blocks)
    info = {}
    serial = D.coefficients(data, p, "serial")
    parallel = D.coefficients(data, p, "parallel", info)
    assert serial[2] != 0 and serial[2] & D.STATUS_BLOCKS and serial[1] != p.expected_blocks
    assert np.array_equal(serial[0], parallel[0]) and serial[1:] == parallel[1:]
    assert info["rounds"] <= p.N
    assert D.pixels(data, p, serial[0]).shape == (33, 65, 3)
    # every byte of the scan overwritten in turn by patterns that hold markers and long codes: still an end and an agreement
    for pattern in (b"\xFF\xD0", b"\xFF\xFF", b"\xFF", b"\x00"):
        worse = bytearray(C.files()["17x23_s2_q75_rst1"])
        q = D.plan(bytes(worse))
        worse[q.scan_off + 40:q.scan_off + 40 + 64] = (pattern * 64)[:64]
        q = D.plan(bytes(worse))
        a, b = D.coefficients(bytes(worse), q, "serial"), D.coefficients(bytes(worse), q, "parallel")
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:] and a[2] != 0, pattern


def test_decoder_options(tmp_path, monkeypatch):
    """--jpeg_decoder and the two environment variables: the default is "host" everywhere, anything but host / device is refused with the
    setting's name, set_jpeg_decoder wins over the environment, and the input-frame listing takes .jpg / .jpeg only with the device
    decoder (png_filenames is the reference's, untouched)."""
    from faster_rcnn_amd import annotate_video as A, entry, feed, shapes, voc_dets
    monkeypatch.delenv("FRCNN_ENTRY_JPEG_DECODER", raising=False)
    monkeypatch.delenv("FRCNN_FEED_JPEG_DECODER", raising=False)
    entry.set_jpeg_decoder(None)
    assert entry.jpeg_decoder() == "host" and feed.default_jpeg_decoder() == "host"
    assert A.build_parser().parse_args(["a", "b", "c"]).jpeg_decoder is None
    assert voc_dets.build_parser().parse_args(["a", "b", "--voc_path", "v"]).jpeg_decoder is None
    assert A.build_parser().parse_args(["a", "b", "c", "--jpeg_decoder", "device"]).jpeg_decoder == "device"
    assert voc_dets.build_parser().parse_args(["a", "b", "--voc_path", "v", "--jpeg_decoder", "host"]).jpeg_decoder == "host"
    for parser, argv in ((A.build_parser(), ["a", "b", "c"]), (voc_dets.build_parser(), ["a", "b", "--voc_path", "v"])):
        with pytest.raises(SystemExit):
            parser.parse_args(argv + ["--jpeg_decoder", "gpu"])
    monkeypatch.setenv("FRCNN_ENTRY_JPEG_DECODER", "device")
    monkeypatch.setenv("FRCNN_FEED_JPEG_DECODER", "device")
    assert entry.jpeg_decoder() == "device" and feed.default_jpeg_decoder() == "device"
    entry.set_jpeg_decoder("host")
    assert entry.jpeg_decoder() == "host"
    entry.set_jpeg_decoder(None)
    assert entry.jpeg_decoder() == "device"
    for name, ask in (("FRCNN_ENTRY_JPEG_DECODER", entry.jpeg_decoder), ("FRCNN_FEED_JPEG_DECODER", feed.default_jpeg_decoder)):
        monkeypatch.setenv(name, "gpu")
        with pytest.raises(ValueError, match=name):
            ask()
        monkeypatch.setenv(name, "")
        assert ask() == "host"
    with pytest.raises(ValueError, match="jpeg_decoder"):
        entry.set_jpeg_decoder("gpu")
    assert entry._JPEG_DECODER is None
    for f in ("b.png", "a.jpg", "c.JPEG", "d.jpeg", "e.txt", "f.PNG"):
        (tmp_path / f).write_bytes(b"")
    assert A.png_filenames(str(tmp_path)) == A.frame_filenames(str(tmp_path)) == A.frame_filenames(str(tmp_path), "host") == ["b.png"]
    assert A.frame_filenames(str(tmp_path), "device") == ["a.jpg", "b.png", "c.JPEG", "d.jpeg"]
    with pytest.raises(ValueError):
        A.frame_filenames(str(tmp_path), "gpu")
    # raw_file: the file's bytes, None for in-memory pixels; plan_file: supported files only
    img = shapes.Image(shapes.Metadata("g", 500, 375, [], C.GOLDEN))
    assert img.raw_file() == C.files()["golden_000005"]
    assert shapes.Image(shapes.Metadata("m", 4, 4, [], "none"), np.zeros((4, 4, 3), np.uint8)).raw_file() is None
    assert not isinstance(getattr(shapes.Image, "raw_file"), property)
    data, plan = feed.plan_file(img)
    assert (plan.h, plan.w, len(data)) == (375, 500, 84988)
    prog = tmp_path / "p.jpg"
    prog.write_bytes(C.unsupported()["progressive"][0])
    assert feed.plan_file(shapes.Image(shapes.Metadata("p", 23, 17, [], str(prog)))) is None
    assert feed.plan_file(shapes.Image(shapes.Metadata("m", 4, 4, [], "none"), np.zeros((4, 4, 3), np.uint8))) is None
