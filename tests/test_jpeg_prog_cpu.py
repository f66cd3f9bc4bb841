"""The device decoder for progressive JPEG files without a GPU: the CPU restatement (tests/jpeg_prog_ref.py) against Pillow byte for
byte, the writer of the unusual scan scripts (tests/jpeg_prog_write.py) validated by Pillow, the planner (the restatement's and the
library's) on supported and unsupported files, a contradictory plan, and the settings that switch the decoder on."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from tests import jpeg_dec_cases as C
from tests import jpeg_prog_cases as P
from tests import jpeg_prog_ref as R

Image = pytest.importorskip("PIL.Image")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["frcnn_jpeg_dec_full_version", "frcnn_jpeg_dec_full_plan", "frcnn_jpeg_dec_full_workspace_bytes",
               "frcnn_jpeg_dec_full_batch_layout", "frcnn_jpeg_decode_full_batch_u8", "frcnn_jpeg_decode_full_u8"]


def pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.mark.parametrize("name", sorted(P.files()))
def test_restatement_is_pillow(name):
    """decode(file) == Pillow's RGB pixels, byte for byte, status 0: libjpeg's default scripts at every sampling class and both ends of
    the quality scale, restart intervals, grey files, and the written scripts."""
    data = P.files()[name]
    info = {}
    got = R.decode(data, info=info)
    want = pillow(data)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), (name, int(np.abs(got.astype(int) - want).max()), int((got != want).sum()))
    assert info["status"] == 0
    if name == "flat_grey":
        assert info["max_eob_category"] == 14                     # the longest end-of-band run there is
        assert np.array_equal(R.decode(data, bgr=True), want[:, :, ::-1])


@pytest.mark.parametrize("name", sorted(P.written_files()))
def test_writer_is_validated_by_pillow(name):
    """Pillow's pixels of a written file are Pillow's pixels of the baseline file its coefficients came from."""
    data, src = P.written_files()[name]
    assert np.array_equal(pillow(data), pillow(C.files()[src])), name


def test_the_cases_cover_the_supported_set():
    plans = {name: R.plan(data) for name, data in P.files().items()}
    assert {(p.frame.ncomp, p.frame.hs, p.frame.vs) for p in plans.values()} == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    assert {s.kind for p in plans.values() for s in p.scans} == {0, 1, 2, 3}
    assert {len(plans[n].scans) for n in ("17x23_s2_q75", "grey_17x23")} == {10, 6}
    assert {s.restart_interval for p in plans.values() for s in p.scans} >= {0, 1, 2, 3, 4, 5, 16}
    # padded and true block counts differ, in luma (single-component scans) against the MCU-order array
    for name in ("7x9_s2_q75", "17x23_s2_q75", "33x65_s2_q75"):
        p = plans[name]
        luma = [R.scan_geometry(p.frame, s)[0] for s in p.scans if s.comps == 1 and s.ss]
        assert luma and all(n < p.frame.mcus_x * p.frame.mcus_y * 4 for n in luma), name
    multi = plans["33x65_s2_q75_dri_changes"]
    assert len({s.restart_interval for s in multi.scans}) >= 4
    ids = plans["33x65_s2_q75_dht_ids_2_3"]
    data = P.files()["33x65_s2_q75_dht_ids_2_3"]
    assert {data[s.dc_off[0] - 1] for s in ids.scans if s.kind == 0} == {0x02}
    assert {data[s.ac_off[c] - 1] for s in ids.scans if s.kind == 2 for c in range(3) if s.comps >> c & 1} == {0x12, 0x13}
    assert all(len(p.scans) <= R.MAX_SCANS for p in plans.values())


def same_plan(p, q, data):
    f, g = p.frame, q.frame
    assert (f.h, f.w, f.components, f.hs, f.vs, f.mcus_x, f.mcus_y, f.blocks_per_mcu) == (g.h, g.w, g.ncomp, g.hs, g.vs, g.mcus_x, g.mcus_y, g.bpm)
    assert (f.expected_blocks, f.restart_interval, f.file_len, f.scan_off, f.scan_len) == (g.expected_blocks, g.restart_interval, len(data), g.scan_off, g.scan_len)
    assert list(f.dqt_off)[:g.ncomp] == g.dqt_off[:g.ncomp] and (f.subsequence_bytes, f.subsequences) == (g.S, g.N)
    assert [list(r) for r in f.dht_off] == [[0, 0], [0, 0]] and list(f.comp_dc) == [0] * 4
    assert p.scans == len(q.scans)
    for k, t in enumerate(q.scans):
        s = p.scan[k]
        assert (s.off, s.len, s.restart_interval, s.subsequence_bytes, s.subsequences) == (t.off, t.len, t.restart_interval, t.subsequence_bytes, t.subsequences), k
        assert (s.comps, s.ss, s.se, s.ah, s.al) == (t.comps, t.ss, t.se, t.ah, t.al), k
        assert (list(s.dc_off), list(s.dc_count), list(s.ac_off), list(s.ac_count)) == (t.dc_off, t.dc_count, t.ac_off, t.ac_count), k


def test_library_planner_is_the_restatement():
    """frcnn_jpeg_dec_full_plan fills the fields the restatement's plan does, on every file; the header, the ctypes tables and the
    exported symbols agree; the baseline decoder's revisions stand."""
    from faster_rcnn_amd import _lib, ops
    ext = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_jpeg_dec_full.h")).read()
    version = int(re.search(r"#define FRCNN_JPEG_DEC_FULL_VERSION (\d+)", ext).group(1))
    assert version == _lib.JPEG_DEC_FULL_VERSION == 1 and re.search(r"^ \*   1 = ", ext, flags=re.M)
    assert int(re.search(r"#define FRCNN_JPEG_DEC_FULL_MAX_SCANS (\d+)", ext).group(1)) == _lib.JPEG_DEC_FULL_MAX_SCANS == R.MAX_SCANS
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    assert sorted(set(re.findall(r"\b(frcnn_jpeg_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.JPEG_DEC_FULL_SIGNATURES) == sorted(NEW_SYMBOLS)
    lib = _lib.load()
    assert lib.frcnn_jpeg_dec_full_version() == version
    assert lib.frcnn_jpeg_dec_version() == _lib.JPEG_DEC_VERSION == 1 and lib.frcnn_jpeg_dec_batch_version() == _lib.JPEG_DEC_BATCH_VERSION == 1
    for bit in ("BLOCKS", "ZIGZAG", "CODE", "TABLE", "EOBRUN"):
        assert int(re.search(r"#define FRCNN_JPEG_DEC_FULL_%s (\d+)" % bit, ext).group(1)) == getattr(_lib, "JPEG_DEC_FULL_" + bit) == getattr(R, "STATUS_" + bit)
    for struct, table in (("scan", _lib.JpegDecFullScan), ("plan", _lib.JpegDecFullPlan), ("batch_item", _lib.JpegDecFullBatchItem)):
        fields = re.search(r"typedef struct frcnn_jpeg_dec_full_%s \{(.*?)\}" % struct, code, flags=re.S).group(1)
        names = [n.split("[")[0] for decl in fields.split(";") if decl.strip() for n in re.sub(r"^\s*\w+\s", "", decl.strip()).replace(" ", "").split(",")]
        assert names == [f[0] for f in table._fields_], struct
    for name, data in P.files().items():
        p = ops.jpeg_dec_full_plan(data)
        same_plan(p, R.plan(data), data)
        assert (p.h, p.w, p.file_len) == (p.frame.h, p.frame.w, len(data)) and ops.decoder_of(p) is ops.JPEG_FULL_DECODER
        need = ops.jpeg_dec_full_workspace_bytes(p)
        assert need % 16 == 0 and p.frame.expected_blocks * 193 <= need <= p.frame.expected_blocks * 193 + 16 * 5
    offs, total = ops.jpeg_dec_full_batch_layout([ops.jpeg_dec_full_plan(P.files()[n]) for n in P.SMALLEST])
    assert offs[0] == 0 and sorted(offs) == offs and total > offs[-1] and all(o % 16 == 0 for o in offs)


def test_a_contradictory_plan_is_refused():
    """Every field the kernels' bounds rest on: a plan that disagrees with itself has no workspace size, no layout, and the decode call
    answers FRCNN_E_ARG before it looks at a device pointer."""
    from faster_rcnn_amd import _lib, ops
    lib = _lib.load()
    data = P.files()["33x65_s2_q75"]

    def spoil(**frame):
        p = ops.jpeg_dec_full_plan(data)
        for k, v in frame.items():
            setattr(p.frame, k, v)
        return p

    bad = [spoil(expected_blocks=91), spoil(mcus_x=6), spoil(h=0), spoil(hs=3), spoil(file_len=100)]
    for field, value in (("len", 1 << 24), ("off", len(data) + 1), ("subsequences", 2000), ("subsequence_bytes", 30), ("comps", 8), ("comps", 0),
                         ("se", 64), ("al", 14), ("restart_interval", 1 << 16)):
        p = ops.jpeg_dec_full_plan(data)
        setattr(p.scan[3], field, value)
        bad.append(p)
    p = ops.jpeg_dec_full_plan(data)
    p.scan[0].dc_off[1] = 0                                        # a DC-first scan without the table of one of its components
    bad.append(p)
    p = ops.jpeg_dec_full_plan(data)
    p.scan[2].ac_off[1] = len(data) - 8                            # a table that runs past the file
    bad.append(p)
    p = ops.jpeg_dec_full_plan(data)
    p.scan[1].comps = 3                                            # an AC scan of two components
    bad.append(p)
    for scans in (0, 65):
        p = ops.jpeg_dec_full_plan(data)
        p.scans = scans
        bad.append(p)
    for p in bad:
        assert lib.frcnn_jpeg_dec_full_workspace_bytes(ctypes.byref(p)) == 0
        with pytest.raises(_lib.FrcnnError):
            ops.jpeg_dec_full_workspace_bytes(p)
        with pytest.raises(_lib.FrcnnError):
            ops.jpeg_dec_full_batch_layout([p])
        item = _lib.JpegDecFullBatchItem()
        item.plan = p
        one = ctypes.c_void_p(4096)                               # never dereferenced: the plan is refused first
        code = lib.frcnn_jpeg_decode_full_batch_u8(ctypes.byref(item), one, 1, one, 1 << 30, 0, one, 1 << 30, one, one, 1 << 30, None)
        assert code == -1 and b"contradicts itself" in lib.frcnn_last_error(), lib.frcnn_last_error()
    assert lib.frcnn_jpeg_dec_full_workspace_bytes(None) == 0


def both_planners_refuse(data, word):
    from faster_rcnn_amd import ops
    with pytest.raises(R.Unsupported) as e:
        R.plan(data)
    assert word in str(e.value), (word, str(e.value))
    mine = str(e.value)
    with pytest.raises(ops.JpegUnsupported) as e:
        ops.jpeg_dec_full_plan(data)
    assert word in str(e.value) and str(e.value) == "jpeg_dec_full_plan: " + mine
    return mine


@pytest.mark.parametrize("name", sorted(P.unsupported()))
def test_planner_refuses_what_is_outside_the_set(name):
    data, word = P.unsupported()[name]
    if name in ("baseline", "cmyk", "rgb_ids"):
        assert pillow(data).shape == (17, 23, 3)                   # (Pillow reads what it wrote: the caller's fallback)
    both_planners_refuse(data, word)


def test_planner_refuses_cut_files():
    """An empty file, no JPEG, and a supported file cut at every marker boundary (and one byte either side) up to its EOI."""
    both_planners_refuse(b"", "empty")
    both_planners_refuse(b"\x89PNG\r\n\x1a\n" + bytes(32), "not a JPEG")
    for name in ("17x23_s2_q75_rst1", "grey_17x23", "17x23_s0_q75_dht_ids_2_3"):
        data = P.files()[name]
        p = R.plan(data)
        cuts = {s.off + d for s in p.scans for d in (-1, 0, 1)} | {s.off + s.len + d for s in p.scans for d in (-1, 0, 1)} | {1, 2, 3, len(data) - 1}
        for cut in sorted(cuts):
            both_planners_refuse(data[:cut], "truncated" if cut >= 4 else "not a JPEG")
        assert R.plan(data[:-2] + b"\xFF\xD9").frame.scan_len == p.frame.scan_len


def test_damaged_scans_yield_a_status():
    """The restatement on the damaged files: it ends, with a status, and indexes nothing outside the coefficient array (numpy raises)."""
    for name, data in P.damaged().items():
        info = {}
        assert R.decode(data, info=info).shape == (64, 136, 3)
        assert R.plan(data).frame.expected_blocks == R.plan(P.files()[P.DAMAGE_OF]).frame.expected_blocks
        assert info["status"] != 0 or not np.array_equal(R.decode(data), pillow(P.files()[P.DAMAGE_OF])), name


def test_decoder_settings(tmp_path, monkeypatch):
    """"device_full" is a JPEG decoder setting everywhere "device" is one; anything else still raises, naming the choices; under it
    ``feed.plan_file`` returns a baseline plan for a baseline file and a full plan for a progressive one, and "device" keeps refusing
    the progressive file."""
    from faster_rcnn_amd import _lib, annotate_video as A, entry, feed, shapes, voc_dets
    assert feed.JPEG_DECODERS == A.JPEG_DECODERS == ("host", "device", "device_full")
    assert feed.jpeg_decoder_option("device_full", "x") == "device_full" and feed.jpeg_decoder_option(None, "x") == "host"
    with pytest.raises(ValueError, match="host, device, device_full"):
        feed.jpeg_decoder_option("gpu", "x")
    assert A.build_parser().parse_args(["a", "b", "c", "--jpeg_decoder", "device_full"]).jpeg_decoder == "device_full"
    assert voc_dets.build_parser().parse_args(["a", "b", "--voc_path", "v", "--jpeg_decoder", "device_full"]).jpeg_decoder == "device_full"
    for parser, argv in ((A.build_parser(), ["a", "b", "c"]), (voc_dets.build_parser(), ["a", "b", "--voc_path", "v"])):
        with pytest.raises(SystemExit):
            parser.parse_args(argv + ["--jpeg_decoder", "full"])
    entry.set_jpeg_decoder(None)
    monkeypatch.setenv("FRCNN_ENTRY_JPEG_DECODER", "device_full")
    monkeypatch.setenv("FRCNN_FEED_JPEG_DECODER", "device_full")
    assert entry.jpeg_decoder() == "device_full" and feed.default_jpeg_decoder() == "device_full"
    entry.set_jpeg_decoder("device")
    assert entry.jpeg_decoder() == "device"
    entry.set_jpeg_decoder("device_full")
    assert entry.jpeg_decoder() == "device_full"
    entry.set_jpeg_decoder(None)
    for f in ("b.png", "a.jpg", "e.txt"):
        (tmp_path / f).write_bytes(b"")
    assert A.frame_filenames(str(tmp_path), "device_full") == ["a.jpg", "b.png"] and A.frame_filenames(str(tmp_path)) == ["b.png"]
    prog = tmp_path / "p.jpg"
    prog.write_bytes(P.files()["17x23_s1_q75"])
    base = shapes.Image(shapes.Metadata("g", 500, 375, [], C.GOLDEN))
    image = shapes.Image(shapes.Metadata("p", 23, 17, [], str(prog)))
    data, plan = feed.plan_file(base)
    assert isinstance(plan, _lib.JpegDecPlan) and (plan.h, plan.w) == (375, 500)
    data, plan = feed.plan_file(image)
    assert isinstance(plan, _lib.JpegDecFullPlan) and (plan.h, plan.w, plan.scans) == (17, 23, 10) and data == P.files()["17x23_s1_q75"]
    assert isinstance(feed.plan_feed_file(image)[1], _lib.JpegDecFullPlan) and isinstance(feed.plan_entry_file(image, jpeg="device_full")[1], _lib.JpegDecFullPlan)
    assert feed.plan_entry_file(image, jpeg=True) is None and feed.plan_entry_file(image, jpeg="device") is None
    assert isinstance(feed.plan_entry_file(base, jpeg="device_full")[1], _lib.JpegDecPlan)
    assert feed._still_wanted(plan) and feed._still_wanted(feed.plan_file(base)[1])
    monkeypatch.setenv("FRCNN_FEED_JPEG_DECODER", "device")
    assert feed.plan_file(image) is None and isinstance(feed.plan_file(base)[1], _lib.JpegDecPlan)
    assert not feed._still_wanted(plan) and feed._still_wanted(feed.plan_file(base)[1])
    monkeypatch.setenv("FRCNN_FEED_JPEG_DECODER", "host")
    assert feed.plan_feed_file(image) is None and feed.plan_feed_file(base) is None
    bad = tmp_path / "c.jpg"
    bad.write_bytes(P.unsupported()["cmyk"][0])
    assert feed.plan_file(shapes.Image(shapes.Metadata("c", 23, 17, [], str(bad))), full=True) is None       # neither planner: PIL's
