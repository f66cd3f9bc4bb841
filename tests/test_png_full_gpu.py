"""The full-format device PNG decoder on the GPU: ops.png_decode_full_batch_u8 / ops.png_decode_full_u8 against the restatement
(tests/png_full_ref.py, which tests/test_png_full_cpu.py holds to Pillow), byte for byte.  Every batch is packed as tightly as the
interface allows -- streams and palettes back to back at unaligned offsets, frames back to back between guards, workspace regions with
guard bytes between them, guard bytes behind the file area -- so that an item that reads or writes a neighbour's bytes shows.  The damaged
files run last, once each."""
import numpy as np
import pytest

from tests import png_full_cases as F
from tests import png_full_ref as ref

pytestmark = pytest.mark.gpu
GUARD = 256
FILL = 0xA7


def run_batch(datas, bgr=False, status=None):
    """-> (frames, status words, guards intact) of one ops.png_decode_full_batch_u8 over ``datas``: each file's stream and, for a palette
    file, its 768 palette bytes from byte 1 of the file area on, back to back; the frames back to back between guards; the workspace
    regions GUARD bytes apart; everything that is not an item's own is FILL before the call and must be FILL after it."""
    import torch
    from faster_rcnn_amd import ops
    plans = [ops.png_dec_full_plan(d) for d in datas]
    staged = [ops.png_dec_full_stream(d, p) for d, p in zip(datas, plans)]
    needs = [ops.png_dec_full_workspace_bytes(p) for p in plans]
    sizes = [p.h * p.w * 3 for p in plans]
    file_off, plte_off, at = [], [], 1
    for stream, palette in staged:
        file_off.append(at)
        plte_off.append(at + len(stream))
        at += len(stream) + len(palette)
    out_off = [GUARD + sum(sizes[:i]) for i in range(len(datas))]
    ws_off = [GUARD + sum(n + GUARD for n in needs[:i]) for i in range(len(datas))]
    area = np.full(at + GUARD, FILL, np.uint8)
    for o, (stream, palette) in zip(file_off, staged):
        area[o:o + len(stream) + len(palette)] = np.frombuffer(stream + palette, np.uint8)
    files = torch.from_numpy(area).cuda()
    out = torch.full((sum(sizes) + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    ws = torch.full((ws_off[-1] + needs[-1] + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    if status is None:
        status = torch.zeros(len(datas), dtype=torch.int32, device="cuda")
    items = ops.png_full_batch_items(plans, file_off, out_off, ws_off, plte_off)
    got = ops.png_decode_full_batch_u8(files[:at], items, out, bgr=bgr, status=status, workspace=ws)    # (capacity: what is staged, not the guard)
    assert got.data_ptr() == status.data_ptr()
    host, wsh = out.cpu().numpy(), ws.cpu().numpy()
    intact = bool((host[:GUARD] == FILL).all() and (host[-GUARD:] == FILL).all() and np.array_equal(files.cpu().numpy(), area))
    for i in range(len(datas) + 1):                                         # the gap in front of every region and behind the last
        lo = ws_off[i] - GUARD if i < len(datas) else ws_off[-1] + needs[-1]
        intact = intact and bool((wsh[lo:lo + GUARD] == FILL).all())
    frames = [host[o:o + n].reshape(p.h, p.w, 3) for o, n, p in zip(out_off, sizes, plans)]
    return frames, status.cpu().numpy(), intact


def test_every_case_alone_equals_the_restatement():
    wrong = []
    for name, data in F.all_sound():
        (frame,), status, intact = run_batch([data])
        want = F.expected(name)
        if not (status.tolist() == [0] and intact and frame.shape == want.shape and np.array_equal(frame, want)):
            wrong.append((name, status.tolist(), intact))
    assert not wrong, wrong


MIXED = ("sub_p1_w13_i0", "pair_c6_d8_i1", "pair_c2_d16_i0", "r1_pil_33x65_c3_l6", "photo_rgb_i1")


def test_one_batch_of_mixed_kinds():
    """A palette 1-bit file, an Adam7 RGBA file, a 16-bit RGB file, a revision-1 RGB file and the photograph in one call."""
    frames, status, intact = run_batch([F.case(n) for n in MIXED])
    assert status.tolist() == [0] * len(MIXED) and intact
    for name, got in zip(MIXED, frames):
        assert np.array_equal(got, F.expected(name)), name


def test_batch_of_one_revision_1_file_equals_revision_1():
    from faster_rcnn_amd import ops
    name = "r1_filter_mix_c4"
    (frame,), status, intact = run_batch([F.case(name)])
    assert status.tolist() == [0] and intact
    assert np.array_equal(frame, ops.png_decode_u8(F.case(name)).cpu().numpy()) and np.array_equal(frame, F.expected(name))
    assert np.array_equal(ops.png_decode_full_u8(F.case(name)).cpu().numpy(), frame)


def test_batch_of_64():
    from faster_rcnn_amd import _lib
    cases = F.sound_cases()
    order = np.random.RandomState(5).permutation(len(cases)).tolist()[:_lib.PNG_DEC_BATCH_MAX]
    assert len(order) == 64
    frames, status, intact = run_batch([cases[i][1] for i in order])
    assert status.tolist() == [0] * 64 and intact
    for i, got in zip(order, frames):
        assert np.array_equal(got, F.expected(cases[i][0])), cases[i][0]


def test_bgr_order():
    from faster_rcnn_amd import ops
    names = MIXED[:4] + ("pair_c3_d4_i1", "pair_c4_d16_i1", "pair_c0_d2_i0", "crop_adaptive_pil")
    frames, status, intact = run_batch([F.case(n) for n in names], bgr=True)
    assert status.tolist() == [0] * len(names) and intact
    for name, got in zip(names, frames):
        assert np.array_equal(got, F.expected(name)[:, :, ::-1]), name
    assert np.array_equal(ops.png_decode_full_u8(F.case(names[-1]), bgr=True).cpu().numpy(), F.expected(names[-1])[:, :, ::-1])


@pytest.mark.parametrize("kind", ("payload", "adler", "filter5"))
def test_zz_damaged_item_between_sound_neighbours(kind):
    """Run after the sound cases, once each: [sound, damaged, another sound].  The damaged item's status word is non-zero (a flipped
    Adler byte: that bit alone, its pixels still right; a filter byte of 5 in pass 4: the filter bit alone), the neighbours exact, the
    guards intact; a later sound decode into the same status words does not clear them."""
    import torch
    from faster_rcnn_amd import _lib, ops
    files = F.damaged()
    rgb = ref.decode(files["sound"])
    other = "pair_c3_d2_i1"
    status = torch.zeros(3, dtype=torch.int32, device="cuda")
    frames, words, intact = run_batch([files["sound"], files[kind], F.case(other)], status=status)
    assert intact
    assert words[0] == 0 and words[2] == 0 and words[1] != 0
    assert np.array_equal(frames[0], rgb) and np.array_equal(frames[2], F.expected(other))
    if kind == "adler":
        assert words[1] == _lib.PNG_DEC_ADLER and np.array_equal(frames[1], rgb)
    if kind == "filter5":
        assert words[1] == _lib.PNG_DEC_FILTER
    before = words.copy()
    frames, words, intact = run_batch([files["sound"]] * 3, status=status)  # sticky: ORed into, never cleared
    assert intact and words.tolist() == before.tolist()
    assert all(np.array_equal(f, rgb) for f in frames)
    if kind == "payload":
        with pytest.raises(_lib.FrcnnError, match="damaged"):
            ops.png_decode_full_u8(files[kind])
