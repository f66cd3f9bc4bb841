"""The device decoder for progressive JPEG files on the GPU: ops.jpeg_decode_full_u8 and ops.jpeg_decode_full_batch_u8 against the CPU
restatement (tests/jpeg_prog_ref.py) and Pillow byte for byte; batches packed as tightly as the interface allows, with guard bytes
between the frames and between the workspace regions; damaged and cut files; the argument errors."""
import functools
import io

import numpy as np
import pytest

from tests import jpeg_dec_cases as C
from tests import jpeg_prog_cases as P
from tests import jpeg_prog_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
Image = pytest.importorskip("PIL.Image")
GUARD = 256
FILL = 0xA7
BATCH = P.LONG + P.SMALLEST + ("33x65_s2_q75_successive_twice", "grey_33x65", "17x23_s2_q75_rst1")


@functools.lru_cache(None)
def reference(name):
    return R.decode(P.files()[name])


@pytest.mark.parametrize("name", sorted(P.files()))
def test_decode_is_the_restatement_and_pillow(name):
    """Every supported case: the same bytes as the restatement and as Pillow, R,G,B and B,G,R."""
    from faster_rcnn_amd import ops
    data = P.files()[name]
    want = reference(name)
    assert np.array_equal(want, np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))
    for bgr in (False, True):
        got = ops.jpeg_decode_full_u8(data, bgr=bgr).cpu().numpy()
        ref = want[:, :, ::-1] if bgr else want
        assert got.shape == ref.shape and np.array_equal(got, ref), (name, bgr, int(np.abs(got.astype(int) - ref).max()), int((got != ref).sum()))


def run_batch(datas, bgr=False, preset=None):
    """-> (frames, status words, guards intact, the plans) of one ops.jpeg_decode_full_batch_u8 over ``datas``: the files from byte 1 of
    the file area on, back to back; the frames back to back between guards; the workspace regions GUARD bytes apart; everything that is
    not an item's own is FILL before the call and must be FILL after it."""
    import torch
    from faster_rcnn_amd import ops
    plans = [ops.jpeg_dec_full_plan(d) for d in datas]
    needs = [ops.jpeg_dec_full_workspace_bytes(p) for p in plans]
    sizes = [p.h * p.w * 3 for p in plans]
    file_off = [1 + sum(len(d) for d in datas[:i]) for i in range(len(datas))]
    out_off = [GUARD + sum(sizes[:i]) for i in range(len(datas))]
    ws_off = [GUARD + sum(n + GUARD for n in needs[:i]) for i in range(len(datas))]
    assert all(o % 16 == 0 for o in ws_off)
    area = np.full(1 + sum(len(d) for d in datas) + GUARD, FILL, np.uint8)
    for o, d in zip(file_off, datas):
        area[o:o + len(d)] = np.frombuffer(d, np.uint8)
    files = torch.from_numpy(area).cuda()
    out = torch.full((sum(sizes) + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    ws = torch.full((ws_off[-1] + needs[-1] + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    status = torch.zeros(len(datas), dtype=torch.int32, device="cuda") if preset is None else torch.tensor(preset, dtype=torch.int32, device="cuda")
    items = ops.jpeg_full_batch_items(plans, file_off, out_off, ws_off)
    got = ops.jpeg_decode_full_batch_u8(files, items, out, bgr=bgr, status=status, workspace=ws)
    assert got.data_ptr() == status.data_ptr()
    host, wsh = out.cpu().numpy(), ws.cpu().numpy()
    intact = bool((host[:GUARD] == FILL).all() and (host[-GUARD:] == FILL).all() and np.array_equal(files.cpu().numpy(), area))
    for i in range(len(datas) + 1):                                         # the gap in front of every region and behind the last
        lo = ws_off[i] - GUARD if i < len(datas) else ws_off[-1] + needs[-1]
        intact = intact and bool((wsh[lo:lo + GUARD] == FILL).all())
    frames = [host[o:o + n].reshape(p.h, p.w, 3) for o, n, p in zip(out_off, sizes, plans)]
    return frames, status.cpu().numpy(), intact, plans


def test_one_batch_of_very_different_items():
    """The 64x136 cases (they size the grids: every other item's workgroups past its own extent return), the 1x1 cases, a written script
    with both refinement kinds, a grey file, restart intervals: the single-file decodes, the guards untouched, every status 0."""
    from faster_rcnn_amd import ops
    frames, status, intact, plans = run_batch([P.files()[n] for n in BATCH])
    assert status.tolist() == [0] * len(BATCH) and intact
    for got, name in zip(frames, BATCH):
        assert np.array_equal(got, reference(name)), name
        assert np.array_equal(got, ops.jpeg_decode_full_u8(P.files()[name]).cpu().numpy()), name
    blocks = [p.frame.expected_blocks for p in plans]
    assert max(blocks) == blocks[0] == 8 * 17 * 3 and min(blocks) == 3      # the grid is the largest item's: 408 blocks, beside one of 3


def test_channel_order_and_sticky_status():
    names = BATCH[2:6]
    frames, status, intact, _ = run_batch([P.files()[n] for n in names], bgr=True, preset=[32, 0, 5, 0])
    assert status.tolist() == [32, 0, 5, 0] and intact
    for got, name in zip(frames, names):
        assert np.array_equal(got, reference(name)[:, :, ::-1]), name


def test_damaged_and_cut_items_keep_to_themselves():
    """Each damaged file once, and a file whose third scan is cut to half its bytes (the markers behind it stand, so the planner takes
    it), between sound neighbours: a non-zero status each, the neighbours exact, the guards untouched."""
    data = P.files()["33x65_s2_q75"]
    third = R.plan(data).scans[2]
    cut = data[:third.off + third.len // 2] + data[third.off + third.len:]
    hurt = P.damaged()
    names = ("33x65_s2_q75", "17x23_s1_q75", "grey_17x23", "1x1_s2_q75")
    datas = [P.files()[names[0]], hurt["ac_refinement"], P.files()[names[1]], hurt["dc_first"], P.files()[names[2]], cut, P.files()[names[3]]]
    frames, status, intact, _ = run_batch(datas)
    assert intact
    assert [int(s) for s in status[0::2]] == [0, 0, 0, 0] and all(int(s) != 0 for s in status[1::2]), status.tolist()
    for got, name in zip(frames[0::2], names):
        assert np.array_equal(got, reference(name)), name


def test_argument_errors():
    import torch
    from faster_rcnn_amd import _lib, ops
    data = P.files()["17x23_s2_q75"]
    plan = ops.jpeg_dec_full_plan(data)
    need = ops.jpeg_dec_full_workspace_bytes(plan)
    files = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    out = torch.empty(17 * 23 * 3, dtype=torch.uint8, device="cuda")
    items = ops.jpeg_full_batch_items([plan], [0], [0], [0])
    assert int(ops.jpeg_decode_full_batch_u8(files, items, out).cpu()[0]) == 0
    with pytest.raises(_lib.FrcnnError, match="files must be"):
        ops.jpeg_decode_full_batch_u8(files.cpu(), items, out)
    with pytest.raises(_lib.FrcnnError, match="out must be"):
        ops.jpeg_decode_full_batch_u8(files, items, out.to(torch.int32))
    with pytest.raises(_lib.FrcnnError, match="status must be"):
        ops.jpeg_decode_full_batch_u8(files, items, out, status=torch.zeros(1, dtype=torch.int64, device="cuda"))
    with pytest.raises(_lib.FrcnnError, match="beyond workspace_capacity"):
        ops.jpeg_decode_full_batch_u8(files, items, out, workspace=torch.empty(need - 16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.FrcnnError, match="beyond out_capacity"):
        ops.jpeg_decode_full_batch_u8(files, items, out[:-1])
    with pytest.raises(_lib.FrcnnError, match="beyond files_capacity"):
        ops.jpeg_decode_full_batch_u8(files[:-1], items, out)
    base = ops.jpeg_dec_plan(C.files()["17x23_s2_q75"])
    with pytest.raises(_lib.FrcnnError, match="jpeg_full_batch_items"):
        ops.jpeg_decode_full_batch_u8(files, ops.jpeg_batch_items([base], [0], [0], [0]), out)
    with pytest.raises(_lib.FrcnnError, match="jpeg_batch_items"):
        ops.jpeg_decode_batch_u8(files, items, out)
    with pytest.raises(ops.JpegUnsupported, match="baseline"):
        ops.jpeg_decode_full_u8(C.files()["17x23_s2_q75"])
    with pytest.raises(_lib.FrcnnError, match="damaged"):
        ops.jpeg_decode_full_u8(P.damaged()["dc_first"])
    torch.cuda.synchronize()
