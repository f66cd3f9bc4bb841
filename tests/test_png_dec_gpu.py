"""The device PNG decoder on the GPU: ops.png_decode_u8 / ops.png_decode_batch_u8 against Pillow, byte for byte (PNG is lossless: Pillow
is the oracle).  Every batch is packed as tightly as the interface allows -- streams back to back at unaligned offsets, frames back to
back, workspace regions with guard bytes between them -- so that an item that reads or writes a neighbour's bytes shows.  The damaged
files run last, once each."""
import functools

import numpy as np
import pytest

from tests import png_dec_cases as C

pytestmark = pytest.mark.gpu
GUARD = 256
FILL = 0xA7


def run_batch(datas, bgr=False, status=None):
    """-> (frames, status words, guards intact) of one ops.png_decode_batch_u8 over ``datas``: the staged streams from byte 1 of the
    file area on, back to back; the frames back to back between guards; the workspace regions GUARD bytes apart; everything that is not
    an item's own is FILL before the call and must be FILL after it.  ``status``: a device tensor to OR into (sticky)."""
    import torch
    from faster_rcnn_amd import ops
    plans = [ops.png_dec_plan(d) for d in datas]
    streams = [ops.png_dec_stream(d, p) for d, p in zip(datas, plans)]
    needs = [ops.png_dec_workspace_bytes(p) for p in plans]
    sizes = [p.h * p.w * 3 for p in plans]
    file_off = [1 + sum(len(s) for s in streams[:i]) for i in range(len(datas))]
    out_off = [GUARD + sum(sizes[:i]) for i in range(len(datas))]
    ws_off = [GUARD + sum(n + GUARD for n in needs[:i]) for i in range(len(datas))]
    area = np.full(1 + sum(len(s) for s in streams) + GUARD, FILL, np.uint8)
    for o, s in zip(file_off, streams):
        area[o:o + len(s)] = np.frombuffer(s, np.uint8)
    files = torch.from_numpy(area).cuda()
    out = torch.full((sum(sizes) + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    ws = torch.full((ws_off[-1] + needs[-1] + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    if status is None:
        status = torch.zeros(len(datas), dtype=torch.int32, device="cuda")
    items = ops.png_batch_items(plans, file_off, out_off, ws_off)
    got = ops.png_decode_batch_u8(files, items, out, bgr=bgr, status=status, workspace=ws)
    assert got.data_ptr() == status.data_ptr()
    host, wsh = out.cpu().numpy(), ws.cpu().numpy()
    intact = bool((host[:GUARD] == FILL).all() and (host[-GUARD:] == FILL).all() and np.array_equal(files.cpu().numpy(), area))
    for i in range(len(datas) + 1):                                         # the gap in front of every region and behind the last
        lo = ws_off[i] - GUARD if i < len(datas) else ws_off[-1] + needs[-1]
        intact = intact and bool((wsh[lo:lo + GUARD] == FILL).all())
    frames = [host[o:o + n].reshape(p.h, p.w, 3) for o, n, p in zip(out_off, sizes, plans)]
    return frames, status.cpu().numpy(), intact


@functools.lru_cache(None)
def singles():
    """Every sound case and the two photographs decoded ONE file per call, RGB: {name: frame} (shared by the tests below)."""
    from faster_rcnn_amd import ops
    return {name: ops.png_decode_u8(data).cpu().numpy() for name, data, _ in C.sound_cases() + C.photo_cases()}


def test_every_case_singly_equals_pillow():
    got = singles()
    for name, _, want in C.sound_cases() + C.photo_cases():
        assert got[name].shape == want.shape and np.array_equal(got[name], want), (name, int((got[name] != want).sum()))


def test_every_case_singly_bgr():
    from faster_rcnn_amd import ops
    for name, data, want in C.sound_cases() + C.photo_cases()[:1]:
        got = ops.png_decode_u8(data, bgr=True).cpu().numpy()
        assert np.array_equal(got, want[:, :, ::-1]), name


def test_batches_of_shuffled_mixed_sizes_equal_the_single_decodes():
    from faster_rcnn_amd import _lib
    cases = C.sound_cases() + C.photo_cases()
    order = np.random.RandomState(3).permutation(len(cases)).tolist()
    assert len(cases) > _lib.PNG_DEC_BATCH_MAX                   # (more than one batch, the first one full)
    for k in range(0, len(order), _lib.PNG_DEC_BATCH_MAX):
        part = [cases[i] for i in order[k:k + _lib.PNG_DEC_BATCH_MAX]]
        frames, status, intact = run_batch([d for _, d, _ in part], bgr=bool(k))
        assert status.tolist() == [0] * len(part) and intact
        for (name, _, _), got in zip(part, frames):
            want = singles()[name][:, :, ::-1] if k else singles()[name]
            assert np.array_equal(got, want), name


@pytest.mark.parametrize("compress", ("runs", "huffman"))
def test_round_trip_of_the_device_encoder(compress):
    """The project's own encoder's files (stored / run-length fixed blocks; per-band dynamic codes with adaptive filters) decode back to
    the frame."""
    import torch
    from faster_rcnn_amd import ops
    frames = [C.pattern(17, 23, 3, 1), C.pattern(64, 136, 3, 2), C.photo()]
    datas = [ops.png_bytes(torch.from_numpy(np.array(f)).cuda(), compress=compress) for f in frames]
    got, status, intact = run_batch(datas)
    assert status.tolist() == [0, 0, 0] and intact
    for f, g in zip(frames, got):
        assert np.array_equal(f, g)


def test_zz_damaged_items_between_sound_neighbours():
    """Run after the sound cases, once: [sound, damaged payload, sound, flipped Adler byte, sound].  The damaged items' status words are
    non-zero (the flipped one: the Adler bit alone, its pixels still right), the neighbours exact, the guards intact; a later sound decode
    into the same status words does not clear them."""
    import torch
    from faster_rcnn_amd import _lib
    sound, rgb, hurt, flipped = C.damaged()
    other = C.sound_cases()[40]
    datas = [sound, hurt, other[1], flipped, sound]
    status = torch.zeros(5, dtype=torch.int32, device="cuda")
    frames, words, intact = run_batch(datas, status=status)
    assert intact
    assert words[0] == 0 and words[2] == 0 and words[4] == 0 and words[1] != 0
    assert words[3] == _lib.PNG_DEC_ADLER
    assert np.array_equal(frames[0], rgb) and np.array_equal(frames[4], rgb) and np.array_equal(frames[2], other[2])
    assert np.array_equal(frames[3], rgb)
    before = words.copy()
    frames, words, intact = run_batch([sound] * 5, status=status)          # sticky: ORed into, never cleared
    assert intact and words.tolist() == before.tolist()
    assert all(np.array_equal(f, rgb) for f in frames)


def test_argument_validation_launches_nothing():
    """Contradictory plans, ranges beyond capacity and overlapping outputs are FRCNN_E_ARG on the host: the output keeps its fill."""
    import torch
    from faster_rcnn_amd import _lib, ops
    sound, rgb, _, _ = C.damaged()
    plan = ops.png_dec_plan(sound)
    files = torch.frombuffer(bytearray(ops.png_dec_stream(sound, plan)), dtype=torch.uint8).cuda()
    size = plan.h * plan.w * 3
    out = torch.full((2 * size,), FILL, dtype=torch.uint8, device="cuda")
    for change in (dict(out_off=[0, size - 1]), dict(out_off=[0, size + 1]), dict(ws_off=[0, 16]), dict(file_off=[0, 1])):
        args = dict(file_off=[0, 0], out_off=[0, size], ws_off=ops.png_dec_batch_layout([plan, plan])[0])
        args.update(change)
        with pytest.raises(_lib.FrcnnError, match="png_decode_batch_u8"):
            ops.png_decode_batch_u8(files, ops.png_batch_items([plan, plan], **args), out)
    bad = _lib.PngDecPlan.from_buffer_copy(bytes(plan))
    bad.inflated_len -= 1
    with pytest.raises(_lib.FrcnnError, match="contradicts"):
        ops.png_decode_batch_u8(files, ops.png_batch_items([bad], [0], [0], [0]), out, workspace=torch.empty(1 << 16, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    with pytest.raises(ops.PngUnsupported, match="palette"):
        ops.png_decode_u8(C.refusals()[0][1])
