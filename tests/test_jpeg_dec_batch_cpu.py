"""The batched device JPEG decoder without a GPU: the extension header against the ctypes table and the built library, the workspace
layout, every argument error of frcnn_jpeg_decode_batch_u8 (the call returns before it touches a device, so the pointers here are
plain host numbers), and the switch that keeps the per-file loop reachable."""
import ctypes
import os
import re

import pytest

from tests import jpeg_dec_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["frcnn_jpeg_dec_batch_version", "frcnn_jpeg_dec_batch_layout", "frcnn_jpeg_decode_batch_u8"]
NAMES = ("17x23_s2_q75", "grey_17x23_q75", "33x65_s1_q75", "7x9_s0_q75")
E_ARG = -1


def test_header_is_the_table_is_the_library():
    """Every symbol the new header declares is in _lib.JPEG_DEC_BATCH_SIGNATURES with matching argument kinds and is exported by the
    built library; revision 1; the item is the header's struct; the older extensions keep their revisions and their tables."""
    from faster_rcnn_amd import _lib
    ext = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_jpeg_dec_batch.h")).read()
    version = int(re.search(r"#define FRCNN_JPEG_DEC_BATCH_VERSION (\d+)", ext).group(1))
    assert version == _lib.JPEG_DEC_BATCH_VERSION == 1 and re.search(r"^ \*   1 = ", ext, flags=re.M)
    assert int(re.search(r"#define FRCNN_JPEG_DEC_BATCH_MAX (\d+)", ext).group(1)) == _lib.JPEG_DEC_BATCH_MAX == 64
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    assert sorted(set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", code))) == sorted(_lib.JPEG_DEC_BATCH_SIGNATURES) == sorted(NEW_SYMBOLS)
    for name in NEW_SYMBOLS:
        decl = re.search(r"(\w[\w\s\*]*?)\b%s\s*\(([^)]*)\)" % name, code, flags=re.S)
        args = [a.strip() for a in decl.group(2).split(",") if a.strip() and a.strip() != "void"]
        restype, argtypes = _lib.JPEG_DEC_BATCH_SIGNATURES[name]
        assert len(args) == len(argtypes), name
        assert restype is (ctypes.c_size_t if decl.group(1).split()[-1] == "size_t" else ctypes.c_int), name
        for a, t in zip(args, argtypes):
            want = ctypes.c_void_p if "*" in a else (ctypes.c_size_t if a.startswith("size_t") else ctypes.c_int)
            assert t is want, (name, a)
    fields = re.search(r"typedef struct frcnn_jpeg_dec_batch_item \{(.*?)\}", code, flags=re.S).group(1)
    names = [decl.split()[-1] for decl in fields.split(";") if decl.strip()]
    assert names == [f[0] for f in _lib.JpegDecBatchItem._fields_] == ["plan", "file_off", "out_off", "ws_off"]
    assert ctypes.sizeof(_lib.JpegDecBatchItem) == ctypes.sizeof(_lib.JpegDecPlan) + 24 and ctypes.sizeof(_lib.JpegDecBatchItem) % 8 == 0
    lib = _lib.load()
    assert lib.frcnn_jpeg_dec_batch_version() == version
    assert lib.frcnn_jpeg_dec_version() == _lib.JPEG_DEC_VERSION == 1 and lib.frcnn_jpeg_version() == _lib.JPEG_VERSION == 1
    assert lib.frcnn_png_version() == _lib.PNG_VERSION == 1 and lib.frcnn_png_huff_version() == _lib.PNG_HUFF_VERSION == 1
    assert lib.frcnn_vgg_canvas_version() == _lib.VGG_CANVAS_VERSION == 1
    core = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    dec = open(os.path.join(ROOT, "include", "ext", "frcnn_hip_jpeg_dec.h")).read()
    for name in NEW_SYMBOLS:
        assert name not in core and name not in dec
        assert not any(name in t for t in (_lib.SIGNATURES, _lib.EXT_SIGNATURES, _lib.PNG_SIGNATURES, _lib.PNG_HUFF_SIGNATURES,
                                           _lib.JPEG_SIGNATURES, _lib.JPEG_DEC_SIGNATURES))
    assert "frcnn_hip_jpeg_dec_batch.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_layout():
    """Offsets 16-aligned and disjoint, each region at least the plan's own need, the total their sum; 0 for a refused plan, for no
    plans and for more than a batch holds."""
    from faster_rcnn_amd import _lib, ops
    names = sorted(C.files())[:_lib.JPEG_DEC_BATCH_MAX]         # (a full batch: every sampling class, grey, the golden image)
    plans = [ops.jpeg_dec_plan(C.files()[n]) for n in names]
    needs = [ops.jpeg_dec_workspace_bytes(p) for p in plans]
    offs, total = ops.jpeg_dec_batch_layout(plans)
    assert len(offs) == len(plans) and all(o % 16 == 0 for o in offs)
    ends = [o + n for o, n in zip(offs, needs)]
    order = sorted(range(len(offs)), key=lambda i: offs[i])
    assert all(ends[a] <= offs[b] for a, b in zip(order, order[1:])) and max(ends) <= total
    assert total == sum(needs)
    lib = _lib.load()
    out = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    arr = (_lib.JpegDecPlan * 4)(*plans[:4])
    arr[2].subsequences = 2000                                  # (a plan the planner never makes)
    assert lib.frcnn_jpeg_dec_batch_layout(arr, 4, out) == 0 and list(out) == [7, 7, 7, 7]
    assert lib.frcnn_jpeg_dec_batch_layout(arr, 0, out) == 0 and lib.frcnn_jpeg_dec_batch_layout(arr, 65, out) == 0
    assert lib.frcnn_jpeg_dec_batch_layout(None, 4, out) == 0 and lib.frcnn_jpeg_dec_batch_layout(arr, 4, None) == 0
    with pytest.raises(_lib.FrcnnError):
        ops.jpeg_dec_batch_layout(list(arr))
    with pytest.raises(_lib.FrcnnError):
        ops.jpeg_dec_batch_layout([])
    with pytest.raises(_lib.FrcnnError):
        ops.jpeg_dec_batch_layout(plans[:1] * 65)


class Batch:
    """Four sound items packed back to back, and the capacities that just hold them; the device pointers are numbers that are never
    followed: every case below must return before the library touches a device."""

    def __init__(self):
        from faster_rcnn_amd import ops
        self.plans = [ops.jpeg_dec_plan(C.files()[n]) for n in NAMES]
        self.ws_off, self.ws = ops.jpeg_dec_batch_layout(self.plans)
        self.file_off, self.out_off, f, o = [], [], 0, 0
        for p in self.plans:
            self.file_off.append(f)
            self.out_off.append(o)
            f += p.file_len
            o += p.h * p.w * 3
        self.files, self.out = f, o
        self.items = ops.jpeg_batch_items(self.plans, self.file_off, self.out_off, self.ws_off)
        self.ptr = dict(items_dev=0x10000, files=0x20000, out=0x30000, status=0x40000, workspace=0x50000)

    def call(self, n=None, items="own", **kw):
        from faster_rcnn_amd import _lib
        lib = _lib.load()
        p = dict(self.ptr, **{k: v for k, v in kw.items() if k in self.ptr})
        cap = dict(files=self.files, out=self.out, ws=self.ws)
        cap.update({k[4:]: v for k, v in kw.items() if k.startswith("cap_")})
        code = lib.frcnn_jpeg_decode_batch_u8(self.items if items == "own" else items, p["items_dev"], len(self.items) if n is None else n,
                                              p["files"], cap["files"], 0, p["out"], cap["out"], p["status"], p["workspace"], cap["ws"], None)
        return code, (lib.frcnn_last_error() or b"").decode()


def refused(b, word, **kw):
    code, msg = b.call(**kw)
    assert code == E_ARG, (kw, code, msg)
    assert "jpeg_decode_batch_u8" in msg and word in msg, (kw, msg)
    return msg


def test_argument_errors_return_before_any_device_call():
    """No GPU is present here and the pointers lead nowhere: a call that launched, copied or asked the runtime anything could not
    return FRCNN_E_ARG with its own message."""
    b = Batch()
    for name in ("items_dev", "files", "out", "status", "workspace"):
        refused(b, "null", **{name: None})
    refused(b, "null", items=None)
    refused(b, "n=0", n=0)
    refused(b, "n=65", n=65)
    refused(b, "n=-1", n=-1)
    refused(b, "workspace must be 16-byte aligned", workspace=0x50008)
    refused(b, "status_dev must be 4-byte aligned", status=0x40002)
    refused(b, "items_dev must be 8-byte aligned", items_dev=0x10004)
    # an item past each capacity: the last item of each area ends one byte beyond it
    assert "item 3" in refused(b, "files_capacity", cap_files=b.files - 1)
    assert "item 3" in refused(b, "out_capacity", cap_out=b.out - 1)
    assert "item %d" % max(range(4), key=lambda i: b.ws_off[i]) in refused(b, "workspace_capacity", cap_ws=b.ws - 1)
    b.items[1].file_off = 2 ** 63                               # (no wrap-around: the sum is never formed)
    assert "item 1" in refused(b, "files_capacity")
    b = Batch()
    b.items[1].ws_off += 8
    assert "item 1" in refused(b, "ws_off", cap_ws=b.ws + 16)
    b = Batch()
    b.items[2].out_off = b.items[1].out_off + 3                 # overlapping outputs
    msg = refused(b, "output ranges")
    assert "1" in msg and "2" in msg and "overlap" in msg
    b = Batch()
    b.items[3].out_off = b.items[0].out_off                     # ... the same start, the smaller frame inside the larger
    refused(b, "output ranges")
    b = Batch()
    b.items[3].ws_off = b.items[0].ws_off + 16
    assert "overlap" in refused(b, "workspace regions")
    b = Batch()
    b.items[2].plan.expected_blocks += 1                        # a self-contradicting plan at index 2 of 4
    assert "item 2" in refused(b, "contradicts itself (block total)")
    b = Batch()
    b.items[2].plan.scan_len = b.items[2].plan.file_len
    assert "item 2" in refused(b, "scan outside the file")


def test_batch_switch(monkeypatch):
    """FRCNN_ENTRY_JPEG_BATCH: on by default and when empty, "0" keeps the per-file loop, anything else is refused with its name; the
    decoder's own default stays the host."""
    from faster_rcnn_amd import entry
    monkeypatch.delenv("FRCNN_ENTRY_JPEG_BATCH", raising=False)
    monkeypatch.delenv("FRCNN_ENTRY_JPEG_DECODER", raising=False)
    assert entry.jpeg_batch() is True
    for value, want in (("1", True), ("0", False), ("", True)):
        monkeypatch.setenv("FRCNN_ENTRY_JPEG_BATCH", value)
        assert entry.jpeg_batch() is want
    for value in ("2", "yes", "off"):
        monkeypatch.setenv("FRCNN_ENTRY_JPEG_BATCH", value)
        with pytest.raises(ValueError, match="FRCNN_ENTRY_JPEG_BATCH"):
            entry.jpeg_batch()
    entry.set_jpeg_decoder(None)
    assert entry.jpeg_decoder() == "host"
