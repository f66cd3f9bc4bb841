"""The device PNG decoder without a GPU: the case writer against Pillow, the extension header against the ctypes table and the built
library, the planner (a host function) on the supported set and on every refusal, the argument errors of frcnn_png_decode_batch_u8 (the
call returns before it touches a device, so the pointers here are plain host numbers), and the options of entry / annotate_video."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import png_dec_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["frcnn_png_dec_version", "frcnn_png_dec_plan", "frcnn_png_dec_spans", "frcnn_png_dec_workspace_bytes", "frcnn_png_dec_batch_layout",
           "frcnn_png_decode_batch_u8"]
E_ARG = -1


def _built():
    from faster_rcnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfrcnn_hip.so is not built")
    return _lib


def test_cases_decode_under_pillow_to_their_frames():
    """Every file of the set is a PNG that Pillow reads to the expected pixels: for the writer's files those are the generating frame."""
    cases = C.sound_cases() + C.photo_cases()
    assert len({name for name, _, _ in cases}) == len(cases) > 60
    for name, data, want in cases:
        assert want.dtype == np.uint8 and want.ndim == 3 and want.shape[2] == 3, name
        assert np.array_equal(C.pil_rgb(data), want), name
    sound, rgb, hurt, flipped = C.damaged()
    assert np.array_equal(C.pil_rgb(sound), rgb) and len(hurt) == len(flipped) == len(sound)
    sizes = [len(C.idat_payload(d)[0]) for _, d, _ in C.photo_cases()]
    assert all(s > 250000 for s in sizes), sizes               # (the realistic largest: five IDATs of Pillow's 64 KiB each)


def test_header_is_the_table_is_the_library():
    _lib = _built()
    ext = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_png_dec.h")).read()
    version = int(re.search(r"#define FRCNN_PNG_DEC_VERSION (\d+)", ext).group(1))
    assert version == _lib.PNG_DEC_VERSION == 1
    assert int(re.search(r"#define FRCNN_PNG_DEC_BATCH_MAX (\d+)", ext).group(1)) == _lib.PNG_DEC_BATCH_MAX == 64
    assert int(re.search(r"#define FRCNN_PNG_DEC_WINDOW_BYTES (\d+)", ext).group(1)) == _lib.PNG_DEC_WINDOW_BYTES
    assert re.search(r"#define FRCNN_PNG_DEC_MAX_STREAM \(1u << 24\)", ext) and _lib.PNG_DEC_MAX_STREAM == 1 << 24
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    assert sorted(set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.PNG_DEC_SIGNATURES) == sorted(SYMBOLS)
    for name in SYMBOLS:
        decl = re.search(r"(\w[\w\s\*]*?)\b%s\s*\(([^)]*)\)" % name, code, flags=re.S)
        args = [a.strip() for a in decl.group(2).split(",") if a.strip() and a.strip() != "void"]
        restype, argtypes = _lib.PNG_DEC_SIGNATURES[name]
        assert len(args) == len(argtypes), name
        assert restype is (ctypes.c_size_t if decl.group(1).split()[-1] == "size_t" else ctypes.c_int), name
        for a, t in zip(args, argtypes):
            want = ctypes.c_void_p if "*" in a else (ctypes.c_size_t if a.startswith("size_t") else ctypes.c_int)
            assert t is want, (name, a)
    for struct, cls in (("frcnn_png_dec_plan", _lib.PngDecPlan), ("frcnn_png_dec_batch_item", _lib.PngDecBatchItem)):
        fields = re.search(r"typedef struct %s \{(.*?)\}" % struct, code, flags=re.S).group(1)
        names = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
        assert names == [f[0] for f in cls._fields_], struct
    assert ctypes.sizeof(_lib.PngDecPlan) == 32 and ctypes.sizeof(_lib.PngDecBatchItem) == 56
    for bit in ("CODE", "BLOCK", "OVERSUBSCRIBED", "DISTANCE", "OVERRUN", "UNDERRUN", "ADLER", "FILTER"):
        assert int(re.search(r"#define FRCNN_PNG_DEC_%s (\d+)" % bit, ext).group(1)) == getattr(_lib, "PNG_DEC_" + bit)
    lib = _lib.load()
    assert lib.frcnn_png_dec_version() == version
    assert lib.frcnn_jpeg_dec_version() == _lib.JPEG_DEC_VERSION == 1 and lib.frcnn_jpeg_dec_batch_version() == _lib.JPEG_DEC_BATCH_VERSION == 1
    assert lib.frcnn_png_version() == _lib.PNG_VERSION == 1 and lib.frcnn_png_huff_version() == _lib.PNG_HUFF_VERSION == 1
    for name in SYMBOLS:
        assert not any(name in t for t in (_lib.SIGNATURES, _lib.EXT_SIGNATURES, _lib.PNG_SIGNATURES, _lib.PNG_HUFF_SIGNATURES, _lib.JPEG_SIGNATURES,
                                           _lib.JPEG_OPT_SIGNATURES, _lib.JPEG_DEC_SIGNATURES, _lib.JPEG_DEC_BATCH_SIGNATURES))
    assert "frcnn_hip_png_dec.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_planner_accepts_the_supported_set():
    """h, w, channels, the spans and both lengths for every sound case; the staged stream is the IDAT payloads back to back."""
    _built()
    from faster_rcnn_amd import ops
    for name, data, want in C.sound_cases() + C.photo_cases() + [("damaged", C.damaged()[2], C.damaged()[1]), ("flipped", C.damaged()[3], C.damaged()[1])]:
        plan = ops.png_dec_plan(data)
        stream, spans = C.idat_payload(data)
        assert (plan.h, plan.w) == want.shape[:2] and plan.channels == {0: 1, 2: 3, 6: 4}[data[25]], name
        assert plan.file_len == len(data) and plan.idat_count == len(spans) and plan.idat_off == spans[0][0] - 8, name
        assert plan.stream_len == len(stream) and plan.inflated_len == plan.h * (1 + plan.w * plan.channels), name
        assert ops.png_dec_spans(data, plan) == spans and ops.png_dec_stream(data, plan) == stream, name
        assert ops.png_dec_workspace_bytes(plan) == (plan.inflated_len + 15) // 16 * 16, name
    assert {len(C.idat_payload(d)[1]) for _, d, _ in C.photo_cases()} == {5}


def test_planner_refuses_with_the_reason():
    _lib = _built()
    from faster_rcnn_amd import ops
    for name, data, word in C.refusals():
        with pytest.raises(ops.PngUnsupported, match=re.escape(word)) as err:
            ops.png_dec_plan(data)
        assert "png_dec_plan" in str(err.value), name
    with pytest.raises(_lib.FrcnnError):
        ops.png_dec_plan("a string")
    lib = _lib.load()
    assert lib.frcnn_png_dec_plan(b"x", 1, None) == E_ARG
    sound = C.damaged()[0]
    plan = ops.png_dec_plan(sound)
    with pytest.raises(_lib.FrcnnError, match="png_dec_spans"):
        ops.png_dec_spans(sound + b"x", plan)
    # a stream at the cap is refused by its size alone (the IDATs' CRCs are right, nothing is inflated on the host)
    big = C.png_file(4, 4, 3, [b"\x78\x9c" + bytes(1 << 23)] * 2)
    with pytest.raises(ops.PngUnsupported, match="IDAT payload"):
        ops.png_dec_plan(big)


def test_layout():
    _lib = _built()
    from faster_rcnn_amd import ops
    plans = [ops.png_dec_plan(d) for _, d, _ in C.sound_cases()[:_lib.PNG_DEC_BATCH_MAX]]
    needs = [ops.png_dec_workspace_bytes(p) for p in plans]
    offs, total = ops.png_dec_batch_layout(plans)
    assert all(o % 16 == 0 for o in offs) and total == sum(needs)
    assert all(a + n <= b for a, n, b in zip(offs, needs, offs[1:] + [total]))
    lib = _lib.load()
    out = (ctypes.c_uint64 * 2)(7, 7)
    arr = (_lib.PngDecPlan * 2)(*plans[:2])
    arr[1].inflated_len += 1
    assert lib.frcnn_png_dec_batch_layout(arr, 2, out) == 0 and list(out) == [7, 7]
    assert lib.frcnn_png_dec_batch_layout(arr, 0, out) == 0 and lib.frcnn_png_dec_batch_layout(arr, 65, out) == 0
    with pytest.raises(_lib.FrcnnError):
        ops.png_dec_batch_layout([])
    with pytest.raises(_lib.FrcnnError):
        ops.png_dec_workspace_bytes(arr[1])


class Batch:
    """Four sound items packed back to back and the capacities that just hold them; the device pointers are numbers that are never
    followed: every case below must return before the library touches a device."""
    NAMES = ("pil_17x23_c3_l6", "pil_33x65_c4_l6", "pil_1x7_c1_l6", "fixed")

    def __init__(self):
        from faster_rcnn_amd import ops
        files = {name: data for name, data, _ in C.sound_cases()}
        self.plans = [ops.png_dec_plan(files[n]) for n in self.NAMES]
        self.ws_off, self.ws = ops.png_dec_batch_layout(self.plans)
        self.file_off, self.out_off, f, o = [], [], 0, 0
        for p in self.plans:
            self.file_off.append(f)
            self.out_off.append(o)
            f += p.stream_len
            o += p.h * p.w * 3
        self.files, self.out = f, o
        self.items = ops.png_batch_items(self.plans, self.file_off, self.out_off, self.ws_off)
        self.ptr = dict(items_dev=0x10000, files=0x20000, out=0x30000, status=0x40000, workspace=0x50000)

    def call(self, n=None, items="own", **kw):
        from faster_rcnn_amd import _lib
        lib = _lib.load()
        p = dict(self.ptr, **{k: v for k, v in kw.items() if k in self.ptr})
        cap = dict(files=self.files, out=self.out, ws=self.ws)
        cap.update({k[4:]: v for k, v in kw.items() if k.startswith("cap_")})
        code = lib.frcnn_png_decode_batch_u8(self.items if items == "own" else items, p["items_dev"], len(self.items) if n is None else n,
                                             p["files"], cap["files"], 0, p["out"], cap["out"], p["status"], p["workspace"], cap["ws"], None)
        return code, (lib.frcnn_last_error() or b"").decode()


def refused(b, word, **kw):
    code, msg = b.call(**kw)
    assert code == E_ARG, (kw, code, msg)
    assert "png_decode_batch_u8" in msg and word in msg, (kw, msg)
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
    assert "item 3" in refused(b, "files_capacity", cap_files=b.files - 1)
    assert "item 3" in refused(b, "out_capacity", cap_out=b.out - 1)
    assert "item 3" in refused(b, "workspace_capacity", cap_ws=b.ws - 1)
    b.items[1].file_off = 2 ** 63                               # (no wrap-around: the sum is never formed)
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
    for field, value, what in (("inflated_len", 5, "inflated length"), ("channels", 2, "channels"), ("w", 0, "sides outside 1..65535"), ("stream_len", 1 << 24, "stream length")):
        b = Batch()
        setattr(b.items[2].plan, field, value)
        assert "item 2" in refused(b, "contradicts itself (%s)" % what)


def test_decoder_options(monkeypatch):
    """entry.set_png_decoder / FRCNN_ENTRY_PNG_DECODER: ``host`` unless asked, anything else refused with its name; the JPEG decoder's
    setting is another one; the training feed's planner keeps refusing .png files (it decodes them on the host)."""
    from faster_rcnn_amd import annotate_video, entry, feed
    monkeypatch.delenv("FRCNN_ENTRY_PNG_DECODER", raising=False)
    monkeypatch.delenv("FRCNN_ENTRY_JPEG_DECODER", raising=False)
    entry.set_png_decoder(None)
    assert entry.png_decoder() == "host"
    monkeypatch.setenv("FRCNN_ENTRY_PNG_DECODER", "device")
    assert entry.png_decoder() == "device" and entry.jpeg_decoder() == "host"
    entry.set_png_decoder("host")
    assert entry.png_decoder() == "host"
    entry.set_png_decoder(None)
    monkeypatch.setenv("FRCNN_ENTRY_PNG_DECODER", "gpu")
    with pytest.raises(ValueError, match="FRCNN_ENTRY_PNG_DECODER"):
        entry.png_decoder()
    monkeypatch.delenv("FRCNN_ENTRY_PNG_DECODER")
    with pytest.raises(ValueError, match="png_decoder"):
        entry.set_png_decoder("gpu")
    assert entry.png_decoder() == "host"
    assert feed.png_decoder_option(None, "x") == feed.png_decoder_option("", "x") == "host" and feed.PNG_DECODERS == annotate_video.PNG_DECODERS
    assert issubclass(entry.PngFile, entry.JpegFile)


def test_frame_filenames_and_the_command_line(tmp_path):
    from faster_rcnn_amd import annotate_video
    for name in ("b.png", "a.png", "c.jpg", "d.txt"):
        (tmp_path / name).write_bytes(b"")
    assert annotate_video.frame_filenames(str(tmp_path)) == ["a.png", "b.png"]
    assert annotate_video.frame_filenames(str(tmp_path), png_decoder="device") == ["a.png", "b.png"]
    assert annotate_video.frame_filenames(str(tmp_path), "device", "device") == ["a.png", "b.png", "c.jpg"]
    with pytest.raises(ValueError, match="png_decoder"):
        annotate_video.frame_filenames(str(tmp_path), png_decoder="gpu")
    parser = annotate_video.build_parser()
    args = parser.parse_args(["a.npz", "b.npz", "frames"])
    assert args.png_decoder is None and args.jpeg_decoder is None
    assert parser.parse_args(["a.npz", "b.npz", "frames", "--png_decoder", "device"]).png_decoder == "device"
    assert parser.parse_args(["a.npz", "b.npz", "frames", "--png_decoder", "host"]).png_decoder == "host"
    with pytest.raises(SystemExit):
        parser.parse_args(["a.npz", "b.npz", "frames", "--png_decoder", "gpu"])
    import inspect
    assert inspect.signature(annotate_video.annotate_images).parameters["png_decoder"].default is None


def test_plan_entry_file(tmp_path):
    """The entry's planner takes a .png by its signature only when asked, hands a .jpg on to the JPEG planner, and returns None for a
    file the PNG planner refuses; feed.plan_file (the training feed's) never takes a .png."""
    _built()
    from faster_rcnn_amd import _lib, feed, shapes
    sound = C.damaged()[0]
    paths = {}
    for name, data in (("sound.png", sound), ("palette.png", C.refusals()[0][1])):
        paths[name] = str(tmp_path / name)
        with open(paths[name], "wb") as f:
            f.write(data)

    def img(path, h, w):
        return shapes.Image(shapes.Metadata("x", w, h, [], path))
    image = img(paths["sound.png"], 33, 65)
    assert feed.plan_file(image) is None and feed.plan_entry_file(image, jpeg=True, png=False) is None
    stream, plan = feed.plan_entry_file(image, jpeg=False, png=True)
    assert isinstance(plan, _lib.PngDecPlan) and (plan.h, plan.w, plan.channels) == (33, 65, 3) and stream == C.idat_payload(sound)[0]
    assert feed.plan_entry_file(img(paths["palette.png"], 17, 23), png=True) is None
    golden = img(C.PHOTO, 375, 500)
    assert isinstance(feed.plan_entry_file(golden, jpeg=True, png=True)[1], _lib.JpegDecPlan)
    assert feed.plan_entry_file(golden, jpeg=False, png=True) is None
