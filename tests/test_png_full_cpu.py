"""The full-format device PNG decoder without a GPU: the restatement (tests/png_full_ref.py) against Pillow on every sound case, the
extension header against the ctypes table and the built library, the planner (a host function) on the supported set and on every
refusal, revision 1's planner unchanged, the argument errors of frcnn_png_decode_full_batch_u8 (the call returns before it touches a
device, so the pointers here are plain host numbers), and the options of entry / annotate_video / feed."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

from tests import png_dec_cases as R1
from tests import png_full_cases as F
from tests import png_full_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["frcnn_png_dec_full_version", "frcnn_png_dec_full_plan", "frcnn_png_dec_full_spans", "frcnn_png_dec_full_workspace_bytes",
           "frcnn_png_dec_full_batch_layout", "frcnn_png_decode_full_batch_u8"]
E_ARG = -1


def _built():
    from faster_rcnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfrcnn_hip.so is not built")
    return _lib


def test_the_restatement_equals_pillow_on_every_sound_case():
    """None skipped, none tolerated: numpy.asarray(PIL.Image.open(f).convert("RGB")) byte for byte; and the list covers what it must."""
    cases = F.all_sound()
    names = {n for n, _ in cases}
    assert len(names) == len(cases) > 200
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                             # (Pillow's advice on tRNS in a palette file)
        for name, data in cases:
            want = R1.pil_rgb(data)
            got = F.expected(name)
            assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), name
        assert np.array_equal(R1.pil_rgb(F.damaged()["sound"]), ref.decode(F.damaged()["sound"]))
    with pytest.raises(ref.BadFilter):
        ref.decode(F.damaged()["filter5"])
    assert np.array_equal(F.expected("deep_vector"), np.array([[[18, 171, 255]]], np.uint8))
    seen = {(ref.parse(d)["colour"], ref.parse(d)["depth"], ref.parse(d)["interlace"]) for _, d in F.sound_cases()}
    assert seen == {(c, d, i) for c, d in F.PAIRS for i in (0, 1)}
    for name in ("size_3x5_rgb_i1", "size_1x1_p4_i1", "rows65_ga8", "rows131_rgb16_i1", "sub_g1_w13_i1", "sub_p2_w5_i0", "sub_g4_w3_i1",
                 "plte_short_d8", "trns_palette", "crop_adaptive_pil", "crop_rgb_i1", "photo_rgb_i1", "r1_photo_l6", "filter4_bpp6_i0"):
        assert name in names, name
    assert F.expected("photo_rgb_i1").shape == (375, 500, 3) and F.expected("crop_adaptive_pil").shape == (96, 128, 3)
    assert len(ref.passes(5, 3, 1)) < 7 and ref.passes(131, 3, 1)[-1][5] == 65
    assert (F.expected("plte_short_d8") == 0).all(axis=2).any()     # an index beyond the PLTE's entries: black


def test_header_is_the_table_is_the_library():
    _lib = _built()
    ext = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_png_dec_full.h")).read()
    version = int(re.search(r"#define FRCNN_PNG_DEC_FULL_VERSION (\d+)", ext).group(1))
    assert version == _lib.PNG_DEC_FULL_VERSION == 1
    assert int(re.search(r"#define FRCNN_PNG_DEC_FULL_PLTE_BYTES (\d+)", ext).group(1)) == _lib.PNG_DEC_FULL_PLTE_BYTES == 768
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    assert sorted(set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.PNG_DEC_FULL_SIGNATURES) == sorted(SYMBOLS)
    for name in SYMBOLS:
        decl = re.search(r"(\w[\w\s\*]*?)\b%s\s*\(([^)]*)\)" % name, code, flags=re.S)
        args = [a.strip() for a in decl.group(2).split(",") if a.strip() and a.strip() != "void"]
        restype, argtypes = _lib.PNG_DEC_FULL_SIGNATURES[name]
        assert len(args) == len(argtypes), name
        assert restype is (ctypes.c_size_t if decl.group(1).split()[-1] == "size_t" else ctypes.c_int), name
        for a, t in zip(args, argtypes):
            want = ctypes.c_void_p if "*" in a else (ctypes.c_size_t if a.startswith("size_t") else ctypes.c_int)
            assert t is want, (name, a)
    for struct, cls in (("frcnn_png_dec_full_plan", _lib.PngDecFullPlan), ("frcnn_png_dec_full_batch_item", _lib.PngDecFullBatchItem)):
        fields = re.search(r"typedef struct %s \{(.*?)\}" % struct, code, flags=re.S).group(1)
        names = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
        assert names == [f[0] for f in cls._fields_], struct
    assert ctypes.sizeof(_lib.PngDecFullPlan) == 48 and ctypes.sizeof(_lib.PngDecFullBatchItem) == 80
    lib = _lib.load()
    assert lib.frcnn_png_dec_full_version() == version and lib.frcnn_png_dec_version() == _lib.PNG_DEC_VERSION == 1
    for name in SYMBOLS:
        assert not any(name in t for t in (_lib.SIGNATURES, _lib.EXT_SIGNATURES, _lib.PNG_SIGNATURES, _lib.PNG_HUFF_SIGNATURES, _lib.JPEG_SIGNATURES,
                                           _lib.JPEG_OPT_SIGNATURES, _lib.JPEG_DEC_SIGNATURES, _lib.JPEG_DEC_BATCH_SIGNATURES, _lib.PNG_DEC_SIGNATURES))
    assert "frcnn_hip_png_dec_full.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_planner_accepts_the_supported_set():
    """Every field of the plan, inflated_len included, the spans, the staged stream and the 768 palette bytes, for every sound case and
    for the damaged files."""
    _built()
    from faster_rcnn_amd import ops
    for name, data in F.all_sound() + sorted(F.damaged().items()):
        plan = ops.png_dec_full_plan(data)
        info = ref.parse(data)
        bits = ref.CHANNELS[info["colour"]] * info["depth"]
        assert (plan.h, plan.w, plan.colour_type, plan.bit_depth, plan.interlace) == tuple(info[k] for k in ("h", "w", "colour", "depth", "interlace")), name
        assert plan.file_len == len(data) and plan.idat_count == len(info["spans"]) and plan.idat_off == info["spans"][0][0] - 8, name
        assert plan.stream_len == len(info["stream"]) and plan.inflated_len == ref.inflated_len(info["h"], info["w"], bits, info["interlace"]), name
        assert (plan.plte_off, plan.plte_entries) == (info["plte_off"], info["entries"]), name
        assert ops.png_dec_full_spans(data, plan) == info["spans"], name
        stream, palette = ops.png_dec_full_stream(data, plan)
        assert stream == info["stream"] and palette == info["palette"] and len(palette) == (768 if info["colour"] == 3 else 0), name
        assert ops.png_dec_full_workspace_bytes(plan) == (plan.inflated_len + 15) // 16 * 16, name
    # One chunk walker serves both planners.  A revision-1 plan restated says, field for field, what the full planner says, for every
    # file of both tables that both accept; what revision 1 refuses of the full set it refuses with ITS words, by ITS order of precedence
    # (palette, grey + alpha, depth, interlace).
    both = 0
    for name, data in F.all_sound() + sorted(F.damaged().items()):
        full = ops.png_dec_full_plan(data)
        if (full.colour_type in (0, 2, 6), full.bit_depth, full.interlace) == (True, 8, 0):
            restated = ops.png_dec_full_of(ops.png_dec_plan(data))
            assert [getattr(restated, f) for f, _ in full._fields_] == [getattr(full, f) for f, _ in full._fields_], name
            both += 1
        else:
            want = ("palette (colour type 3)" if full.colour_type == 3 else "grey + alpha (colour type 4)" if full.colour_type == 4 else
                    "%d-bit samples" % full.bit_depth if full.bit_depth != 8 else "interlaced (Adam7)")
            with pytest.raises(ops.PngUnsupported) as err:
                ops.png_dec_plan(data)
            assert str(err.value) == "png_dec_plan: " + want, name
    # (every file of revision 1's table is in the first class; of the 2 x 14 pair files all but (0, 8), (2, 8), (6, 8) without interlace in the second)
    assert both >= len(F.r1_cases()) + 3 and len(F.all_sound()) + len(F.damaged()) - both >= 2 * len(F.PAIRS) - 3


def test_planner_refuses_with_the_reason():
    _lib = _built()
    from faster_rcnn_amd import ops
    refusals = F.refusals()
    assert {"grey16", "no_plte", "late_plte", "plte_length", "pair_rgb4", "bad_crc"} <= {n for n, _, _ in refusals}
    for name, data, word in refusals:
        with pytest.raises(ops.PngUnsupported, match=re.escape(word)) as err:
            ops.png_dec_full_plan(data)
        assert "png_dec_full_plan" in str(err.value), name
    with pytest.raises(_lib.FrcnnError):
        ops.png_dec_full_plan("a string")
    lib = _lib.load()
    assert lib.frcnn_png_dec_full_plan(b"x", 1, None) == E_ARG
    sound = F.damaged()["sound"]
    plan = ops.png_dec_full_plan(sound)
    with pytest.raises(_lib.FrcnnError, match="png_dec_full_spans"):
        ops.png_dec_full_spans(sound + b"x", plan)
    big = R1.png_file(4, 4, 3, [b"\x78\x9c" + bytes(1 << 23)] * 2)
    with pytest.raises(ops.PngUnsupported, match="IDAT payload"):
        ops.png_dec_full_plan(big)
    with pytest.raises(ops.PngUnsupported, match="2\\^31"):              # 1-bit grey, 65535 x 65535, Adam7: below the cap; RGBA 16: above
        ops.png_dec_full_plan(F.container(65535, 65535, 6, 16, 1, [R1.deflate(b"")]))
    assert ops.png_dec_full_plan(F.container(65535, 65535, 0, 1, 1, [R1.deflate(b"")])).inflated_len == ref.inflated_len(65535, 65535, 1, 1)


def test_revision_1_is_unchanged():
    """Revision 1's planner refuses what it refused, with the same words, the files of the new set among them."""
    _built()
    from faster_rcnn_amd import ops
    for name, data, word in R1.refusals():
        with pytest.raises(ops.PngUnsupported, match=re.escape(word)):
            ops.png_dec_plan(data)
    for name, word in (("pair_c3_d8_i0", "palette"), ("pair_c3_d1_i1", "palette"), ("pair_c2_d16_i0", "16-bit"), ("pair_c4_d8_i0", "grey + alpha"),
                       ("pair_c0_d4_i0", "4-bit"), ("pair_c2_d8_i1", "Adam7"), ("crop_adaptive_pil", "palette")):
        with pytest.raises(ops.PngUnsupported, match=re.escape(word)) as err:
            ops.png_dec_plan(F.case(name))
        assert "png_dec_plan:" in str(err.value)


def test_layout():
    _lib = _built()
    from faster_rcnn_amd import ops
    plans = [ops.png_dec_full_plan(d) for _, d in F.sound_cases()[:_lib.PNG_DEC_BATCH_MAX]]
    needs = [ops.png_dec_full_workspace_bytes(p) for p in plans]
    offs, total = ops.png_dec_full_batch_layout(plans)
    assert all(o % 16 == 0 for o in offs) and total == sum(needs)
    assert all(a + n <= b for a, n, b in zip(offs, needs, offs[1:] + [total]))
    lib = _lib.load()
    out = (ctypes.c_uint64 * 2)(7, 7)
    arr = (_lib.PngDecFullPlan * 2)(*plans[:2])
    arr[1].inflated_len += 1
    assert lib.frcnn_png_dec_full_batch_layout(arr, 2, out) == 0 and list(out) == [7, 7]
    assert lib.frcnn_png_dec_full_batch_layout(arr, 0, out) == 0 and lib.frcnn_png_dec_full_batch_layout(arr, 65, out) == 0
    with pytest.raises(_lib.FrcnnError):
        ops.png_dec_full_batch_layout([])
    with pytest.raises(_lib.FrcnnError):
        ops.png_dec_full_workspace_bytes(arr[1])


class Batch:
    """Four sound items packed back to back (a palette file last: its 768 palette bytes end the file area) and the capacities that just
    hold them; the device pointers are numbers that are never followed: every case below must return before the library touches a
    device."""
    NAMES = ("pair_c2_d16_i1", "r1_pil_33x65_c4_l6", "sub_g1_w7_i0", "pair_c3_d4_i1")

    def __init__(self):
        from faster_rcnn_amd import ops
        self.plans = [ops.png_dec_full_plan(F.case(n)) for n in self.NAMES]
        self.ws_off, self.ws = ops.png_dec_full_batch_layout(self.plans)
        self.file_off, self.plte_off, self.out_off, f, o = [], [], [], 0, 0
        for p in self.plans:
            self.file_off.append(f)
            self.plte_off.append(f + p.stream_len)
            self.out_off.append(o)
            f += p.stream_len + (768 if p.colour_type == 3 else 0)
            o += p.h * p.w * 3
        self.files, self.out = f, o
        self.items = ops.png_full_batch_items(self.plans, self.file_off, self.out_off, self.ws_off, self.plte_off)
        self.ptr = dict(items_dev=0x10000, files=0x20000, out=0x30000, status=0x40000, workspace=0x50000)

    def call(self, n=None, items="own", **kw):
        from faster_rcnn_amd import _lib
        lib = _lib.load()
        p = dict(self.ptr, **{k: v for k, v in kw.items() if k in self.ptr})
        cap = dict(files=self.files, out=self.out, ws=self.ws)
        cap.update({k[4:]: v for k, v in kw.items() if k.startswith("cap_")})
        code = lib.frcnn_png_decode_full_batch_u8(self.items if items == "own" else items, p["items_dev"], len(self.items) if n is None else n,
                                                  p["files"], cap["files"], 0, p["out"], cap["out"], p["status"], p["workspace"], cap["ws"], None)
        return code, (lib.frcnn_last_error() or b"").decode()


def refused(b, word, **kw):
    code, msg = b.call(**kw)
    assert code == E_ARG, (kw, code, msg)
    assert "png_decode_full_batch_u8" in msg and word in msg, (kw, msg)
    return msg


def test_argument_errors_return_before_any_device_call():
    """No GPU is present here and the pointers lead nowhere: a call that launched, copied or asked the runtime anything could not
    return FRCNN_E_ARG with its own message."""
    _built()
    b = Batch()
    for name in ("items_dev", "files", "out", "status", "workspace"):
        refused(b, "null", **{name: None})
    refused(b, "null", items=None)
    refused(b, "n=0", n=0)
    refused(b, "n=65", n=65)
    refused(b, "workspace must be 16-byte aligned", workspace=0x50008)
    refused(b, "status_dev must be 4-byte aligned", status=0x40002)
    refused(b, "items_dev must be 8-byte aligned", items_dev=0x10004)
    assert "item 3" in refused(b, "plte_off", cap_files=b.files - 1)       # the last item's 768 palette bytes leave files_capacity
    assert "item 3" in refused(b, "out_capacity", cap_out=b.out - 1)
    assert "item 3" in refused(b, "workspace_capacity", cap_ws=b.ws - 1)
    b.items[3].plte_off = 2 ** 63                                           # (no wrap-around: the sum is never formed)
    assert "item 3" in refused(b, "plte_off")
    b = Batch()
    b.items[2].plte_off = 2 ** 63                                           # a grey file's plte_off is not looked at: the next error is the capacity's
    assert "item 3" in refused(b, "files_capacity", cap_files=b.files - 769)
    b = Batch()
    b.items[1].file_off = 2 ** 63
    assert "item 1" in refused(b, "files_capacity")
    b = Batch()
    b.items[1].ws_off += 8
    assert "item 1" in refused(b, "ws_off", cap_ws=b.ws + 16)
    b = Batch()
    b.items[2].out_off = b.items[1].out_off + 3
    assert "overlap" in refused(b, "output ranges")
    b = Batch()
    b.items[3].ws_off = b.items[0].ws_off
    assert "overlap" in refused(b, "workspace regions")
    for item, field, value, what in ((2, "inflated_len", 5, "inflated length"), (2, "colour_type", 5, "colour type"), (2, "w", 0, "sides outside 1..65535"),
                                     (2, "stream_len", 1 << 24, "stream length"), (2, "bit_depth", 16, "16-bit grey"), (0, "bit_depth", 4, "depth / colour type pair"),
                                     (0, "interlace", 2, "interlace"), (0, "interlace", 0, "inflated length"),
                                     (3, "plte_entries", 0, "palette entries outside 1..256"), (3, "plte_entries", 257, "palette entries outside 1..256")):
        b = Batch()
        setattr(b.items[item].plan, field, value)
        assert "item %d" % item in refused(b, "contradicts itself (%s)" % what)


def test_argument_errors_agree_between_the_two_entry_points():
    """One argument check serves frcnn_png_decode_batch_u8 and frcnn_png_decode_full_batch_u8: on the same four files and the same wrong
    argument, the same FRCNN_E_ARG text but for the entry point's name.  Neither call reaches a device."""
    _lib = _built()
    from faster_rcnn_amd import ops
    lib = _lib.load()
    datas = [F.case("r1_" + n) for n in ("pil_17x23_c3_l6", "pil_33x65_c4_l6", "pil_1x7_c1_l6", "fixed")]

    def message(setting, wrong):
        dec = ops.PNG_DECODERS[setting]
        plans = [dec.plan(d) for d in datas]
        ws_off, ws = dec.layout(plans)
        file_off = [sum(p.stream_len for p in plans[:i]) for i in range(5)]
        out_off = [sum(p.h * p.w * 3 for p in plans[:i]) for i in range(5)]
        a = dict(items=dec.items(plans, file_off, out_off, ws_off), items_dev=0x10000, n=4, files=0x20000, cap_files=file_off[4], out=0x30000,
                 cap_out=out_off[4], status=0x40000, workspace=0x50000, cap_ws=ws)
        wrong(a)
        who = dec.decode_stem + "_batch_u8"
        code = getattr(lib, "frcnn_" + who)(a["items"], a["items_dev"], a["n"], a["files"], a["cap_files"], 0, a["out"], a["cap_out"], a["status"],
                                            a["workspace"], a["cap_ws"], None)
        msg = (lib.frcnn_last_error() or b"").decode()
        assert code == E_ARG and msg.startswith(who + ": "), (setting, code, msg)
        return msg[len(who):]

    def item(i, field, value, **more):
        def wrong(a):
            setattr(a["items"][i], field, value(a))
            a.update({k: v(a) for k, v in more.items()})
        return wrong
    cases = [("null", lambda a, k=k: a.update({k: None})) for k in ("items", "items_dev", "files", "out", "status", "workspace")]
    cases += [("n=0 outside 1..64", lambda a: a.update(n=0)), ("n=65 outside 1..64", lambda a: a.update(n=65)),
              ("workspace must be", lambda a: a.update(workspace=0x50008)), ("status_dev must be", lambda a: a.update(status=0x40002)),
              ("items_dev must be", lambda a: a.update(items_dev=0x10004)),
              ("item 1: ws_off=", item(1, "ws_off", lambda a: a["items"][1].ws_off + 8, cap_ws=lambda a: a["cap_ws"] + 16)),
              ("item 3: file_off=", lambda a: a.update(cap_files=a["cap_files"] - 1)),
              ("item 3: out_off=", lambda a: a.update(cap_out=a["cap_out"] - 1)),
              ("item 3: ws_off=", lambda a: a.update(cap_ws=a["cap_ws"] - 1)),
              ("the output ranges of items 1 and 2 overlap", item(2, "out_off", lambda a: a["items"][1].out_off + 3)),
              ("the workspace regions of items 0 and 3 overlap", item(3, "ws_off", lambda a: a["items"][0].ws_off))]
    for word, wrong in cases:
        one, full = message("device", wrong), message("device_full", wrong)
        assert one == full and word in one, (word, one, full)


def test_decoder_options(monkeypatch, tmp_path):
    """"device_full" is accepted wherever "device" is; "gpu" is still refused; the two lists stay equal."""
    import inspect
    from faster_rcnn_amd import annotate_video, entry, feed
    monkeypatch.delenv("FRCNN_ENTRY_PNG_DECODER", raising=False)
    monkeypatch.delenv("FRCNN_FEED_PNG_DECODER", raising=False)
    entry.set_png_decoder(None)
    assert feed.PNG_DECODERS == annotate_video.PNG_DECODERS == ("host", "device", "device_full")
    assert entry.png_decoder() == "host" and feed.default_png_decoder() == "host"
    monkeypatch.setenv("FRCNN_ENTRY_PNG_DECODER", "device_full")
    assert entry.png_decoder() == "device_full" and entry.jpeg_decoder() == "host"
    entry.set_png_decoder("device")
    assert entry.png_decoder() == "device"
    entry.set_png_decoder("device_full")
    monkeypatch.delenv("FRCNN_ENTRY_PNG_DECODER")
    assert entry.png_decoder() == "device_full"
    entry.set_png_decoder(None)
    assert entry.png_decoder() == "host"
    with pytest.raises(ValueError, match="png_decoder"):
        entry.set_png_decoder("gpu")
    assert feed.png_decoder_option("device_full", "x") == "device_full"
    for value in ("host", "device", "device_full"):
        monkeypatch.setenv("FRCNN_FEED_PNG_DECODER", value)
        assert feed.default_png_decoder() == value
    monkeypatch.setenv("FRCNN_FEED_PNG_DECODER", "gpu")
    with pytest.raises(ValueError, match="FRCNN_FEED_PNG_DECODER"):
        feed.default_png_decoder()
    (tmp_path / "a.png").write_bytes(b"")
    assert annotate_video.frame_filenames(str(tmp_path), png_decoder="device_full") == ["a.png"]
    with pytest.raises(ValueError, match="png_decoder"):
        annotate_video.frame_filenames(str(tmp_path), png_decoder="gpu")
    parser = annotate_video.build_parser()
    assert parser.parse_args(["a.npz", "b.npz", "frames", "--png_decoder", "device_full"]).png_decoder == "device_full"
    with pytest.raises(SystemExit):
        parser.parse_args(["a.npz", "b.npz", "frames", "--png_decoder", "gpu"])
    assert inspect.signature(annotate_video.annotate_images).parameters["png_decoder"].default is None


def test_the_planners_of_entry_and_feed(tmp_path, monkeypatch):
    """plan_entry_file(png="full") plans through the full planner; png=True keeps returning None for a palette file; a file the full
    planner refuses is None under either; the feed's new planner follows FRCNN_FEED_PNG_DECODER; feed.plan_file never takes a .png."""
    _built()
    from faster_rcnn_amd import _lib, feed, shapes
    files = {"palette.png": F.case("crop_adaptive_pil"), "rgb.png": F.case("r1_pil_33x65_c3_l6"), "grey16.png": F.refusals()[0][1]}
    paths = {}
    for name, data in files.items():
        paths[name] = str(tmp_path / name)
        with open(paths[name], "wb") as f:
            f.write(data)

    def img(name, h, w):
        return shapes.Image(shapes.Metadata("x", w, h, [], paths[name]))
    palette, rgb, grey = img("palette.png", 96, 128), img("rgb.png", 33, 65), img("grey16.png", 17, 23)
    assert feed.plan_entry_file(palette, png=True) is None and feed.plan_entry_file(palette, png=False) is None
    data, plan = feed.plan_entry_file(palette, jpeg=False, png="full")
    info = ref.parse(files["palette.png"])
    assert isinstance(plan, _lib.PngDecFullPlan) and (plan.h, plan.w, plan.colour_type) == (96, 128, 3)
    assert data == info["stream"] + info["palette"] and len(data) == plan.stream_len + 768
    data, plan = feed.plan_entry_file(rgb, png="full")
    assert isinstance(plan, _lib.PngDecFullPlan) and data == ref.parse(files["rgb.png"])["stream"]
    assert isinstance(feed.plan_entry_file(rgb, png=True)[1], _lib.PngDecPlan)
    assert feed.plan_entry_file(grey, png="full") is None and feed.plan_entry_file(grey, png=True) is None
    golden = shapes.Image(shapes.Metadata("x", 500, 375, [], R1.PHOTO))
    assert isinstance(feed.plan_entry_file(golden, jpeg=True, png="full")[1], _lib.JpegDecPlan)
    # a frame planned ahead under another setting is planned again
    rgb.png_planned = feed.plan_png(files["rgb.png"])
    assert isinstance(feed.plan_entry_file(rgb, png="full")[1], _lib.PngDecFullPlan) and feed.plan_entry_file(rgb, png=True) is rgb.png_planned
    # the training feed
    monkeypatch.delenv("FRCNN_FEED_JPEG_DECODER", raising=False)
    monkeypatch.delenv("FRCNN_FEED_PNG_DECODER", raising=False)
    for image in (palette, rgb, grey):
        assert feed.plan_file(image) is None and feed.plan_feed_file(image) is None
    monkeypatch.setenv("FRCNN_FEED_PNG_DECODER", "device")
    assert feed.plan_feed_file(palette) is None and isinstance(feed.plan_feed_file(rgb)[1], _lib.PngDecPlan)
    monkeypatch.setenv("FRCNN_FEED_PNG_DECODER", "device_full")
    assert isinstance(feed.plan_feed_file(palette)[1], _lib.PngDecFullPlan) and isinstance(feed.plan_feed_file(rgb)[1], _lib.PngDecFullPlan)
    assert feed.plan_feed_file(grey) is None and feed.plan_feed_file(golden) is None
    for image in (palette, rgb, grey):
        assert feed.plan_file(image) is None
    monkeypatch.setenv("FRCNN_FEED_JPEG_DECODER", "device")
    assert isinstance(feed.plan_feed_file(golden)[1], _lib.JpegDecPlan)
