"""The batched device JPEG decoder on the GPU: ops.jpeg_decode_batch_u8 against the CPU restatement (tests/jpeg_dec_ref.py) byte for
byte.  Every batch here is packed as tightly as the interface allows -- files back to back at unaligned offsets, frames back to back,
workspace regions with guard bytes between them -- so that an item that reads or writes a neighbour's bytes shows."""
import functools

import numpy as np
import pytest

from tests import jpeg_dec_cases as C
from tests import jpeg_dec_ref as D

pytestmark = pytest.mark.gpu
GUARD = 256
FILL = 0xA7
MIXED = ("1x1_s2_q75", "64x136_s0_q100", "grey_17x23_q75", "7x9_s1_q100", "17x23_s2_q75_rst1", "33x65_s2_q10_optimize_rst1",
         "photo_s1_q90_optimize_rst16")


@functools.lru_cache(None)
def reference(name):
    return D.decode(C.files()[name])


def run_batch(datas, bgr=False, preset=None):
    """-> (frames, status words, guards intact) of one ops.jpeg_decode_batch_u8 over ``datas``: the files from byte 1 of the file area
    on, back to back; the frames back to back between guards; the workspace regions GUARD bytes apart (the layout padded by hand);
    everything that is not an item's own is FILL before the call and must be FILL after it."""
    import torch
    from faster_rcnn_amd import ops
    plans = [ops.jpeg_dec_plan(d) for d in datas]
    needs = [ops.jpeg_dec_workspace_bytes(p) for p in plans]
    sizes = [p.h * p.w * 3 for p in plans]
    file_off = [1 + sum(len(d) for d in datas[:i]) for i in range(len(datas))]
    out_off = [GUARD + sum(sizes[:i]) for i in range(len(datas))]
    ws_off = [GUARD + sum(n + GUARD for n in needs[:i]) for i in range(len(datas))]
    assert any(o % 4 for o in file_off) and all(o % 16 == 0 for o in ws_off)
    area = np.full(1 + sum(len(d) for d in datas) + GUARD, FILL, np.uint8)
    for o, d in zip(file_off, datas):
        area[o:o + len(d)] = np.frombuffer(d, np.uint8)
    files = torch.from_numpy(area).cuda()
    out = torch.full((sum(sizes) + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    ws = torch.full((ws_off[-1] + needs[-1] + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    status = torch.zeros(len(datas), dtype=torch.int32, device="cuda") if preset is None else torch.tensor(preset, dtype=torch.int32, device="cuda")
    items = ops.jpeg_batch_items(plans, file_off, out_off, ws_off)
    got = ops.jpeg_decode_batch_u8(files, items, out, bgr=bgr, status=status, workspace=ws)
    assert got.data_ptr() == status.data_ptr()
    host, wsh = out.cpu().numpy(), ws.cpu().numpy()
    intact = bool((host[:GUARD] == FILL).all() and (host[-GUARD:] == FILL).all() and np.array_equal(files.cpu().numpy(), area))
    for i in range(len(datas) + 1):                                         # the gap in front of every region and behind the last
        lo = ws_off[i] - GUARD if i < len(datas) else ws_off[-1] + needs[-1]
        intact = intact and bool((wsh[lo:lo + GUARD] == FILL).all())
    frames = [host[o:o + n].reshape(p.h, p.w, 3) for o, n, p in zip(out_off, sizes, plans)]
    return frames, status.cpu().numpy(), intact


def same(frames, names, bgr=False):
    for got, name in zip(frames, names):
        want = reference(name)[:, :, ::-1] if bgr else reference(name)
        assert got.shape == want.shape and np.array_equal(got, want), (name, int((got != want).sum()))


def test_one_batch_of_very_different_items():
    """1x1; the file with the most subsequences and the slowest re-synchronisation (it sizes the entropy block: every other item idles
    lanes); a grey file in a three-component grid; all three sampling classes; restart intervals of 1 and 16; optimised tables."""
    frames, status, intact = run_batch([C.files()[n] for n in MIXED])
    assert status.tolist() == [0] * len(MIXED)
    same(frames, MIXED)
    assert intact


@pytest.mark.parametrize("name", C.SMALLEST + C.LARGEST)
def test_a_batch_of_one_is_the_single_file_decoder(name):
    import torch
    from faster_rcnn_amd import ops
    data = C.files()[name]
    single, word = ops.jpeg_decode_u8(data)
    frames, status, intact = run_batch([data])
    assert intact and int(status[0]) == 0 == int(word.item())
    assert np.array_equal(frames[0], single.cpu().numpy())
    torch.cuda.synchronize()


def test_a_full_batch():
    """FRCNN_JPEG_DEC_BATCH_MAX items: eight files, eight times each."""
    from faster_rcnn_amd import _lib
    names = (MIXED + ("16x16_s2_q75",)) * 8
    assert len(names) == _lib.JPEG_DEC_BATCH_MAX
    frames, status, intact = run_batch([C.files()[n] for n in names])
    assert not status.any() and intact
    same(frames, names)


def test_a_damaged_item_keeps_to_itself():
    """The damaged file of the CPU tests between two sound ones: its status is the restatement's, theirs are 0 and their pixels exact,
    nothing outside the items' own bytes is touched."""
    want = D.coefficients(C.damaged())[2]
    assert want != 0
    names = ("33x65_s2_q75", "17x23_s1_q75")
    frames, status, intact = run_batch([C.files()[names[0]], C.damaged(), C.files()[names[1]]])
    assert status.tolist() == [0, want, 0]
    same([frames[0], frames[2]], names)
    assert intact


def test_channel_order():
    names = MIXED[2:6]
    frames, status, intact = run_batch([C.files()[n] for n in names], bgr=True)
    assert not status.any() and intact
    same(frames, names, bgr=True)


def test_status_words_are_sticky():
    """Words preset non-zero keep their bits behind sound files; a clear word beside them stays clear."""
    names = MIXED[3:6]
    frames, status, intact = run_batch([C.files()[n] for n in names], preset=[16, 0, 5])
    assert status.tolist() == [16, 0, 5] and intact
    same(frames, names)
