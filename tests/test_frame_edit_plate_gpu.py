"""The plate steps of frame_edit.EditChain in a DELAYED pass, driven without a model so that the rows are known: a car that the detector
reports only from frame 4 on is followed back by the look-back into frames 3 and 2, and those BACK-FILLED rows must keep it out of the
plate and be filled from it.  Every emitted frame and the plate state against tests/plate_ref.py over the emitted buffers, byte for
byte; and against the same reference WITHOUT the back-filled rows, which must differ."""
import numpy as np
import pytest

from tests import plate_ref as P
from tests.test_frame_edit_gpu import CAP, H, NAMES, RADIUS, ROWS, SEG, W, frames_of, spec_of, staged, states_of, word
from tests.test_track_gpu import pack

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

REMOVE = (("car",), 1, 255, 1)            # S = 1, T = 255: every pixel no row touches is the plate at once
CAR = lambda f: [7 + 3 * f, 10, 23 + 3 * f, 30]      # moves with the picture, as the block match finds it
BIKE = lambda f: [40, 30 + f, 52, 44 + f]            # class 3: blocks, is never filled


def test_back_filled_rows_block_and_fill():
    from faster_rcnn_amd.frame_edit import EditChain
    frames = frames_of(3, 6)
    late = lambda f: pack([BIKE(f), CAR(f)], [3, 1], 2, ROWS) if f >= 4 else pack([BIKE(f)], [3], 1, ROWS)
    passes = [(frames[0:2], [late(0), late(1)], 2), (frames[2:4], [late(2), late(3)], 2), (frames[4:6], [late(4), late(5)], 2),
              (frames[0:2], [late(0)] * 2, -1)]                              # ... and the flush
    states = states_of()
    chain = EditChain(states, spec_of(track_motion=RADIUS, track_lookback=2, remove=REMOVE, draw=False), 2, 1, (H, W), True)
    table = np.array([n == "car" for n in NAMES], dtype=np.uint8)
    ref, bare = P.empty(H, W), P.empty(H, W)                                # ``bare``: the rule over the rows the tracker alone gave
    undelayed, emitted, extra_rows, extra_fill = {}, 0, 0, 0
    for k, (fr, packed, n) in enumerate(passes):
        buf, _ = staged(fr)
        chain.update(buf, SEG, torch.from_numpy(np.stack(packed)).cuda(), word(n))
        if n > 0:
            for i in range(2):
                undelayed[2 * k + i] = chain.track_out[i].cpu().numpy().copy()
        count = int(chain.lb_out[2][0])
        assert count == (0, 2, 2, 2)[k]
        for i in range(2):
            src, rows_buf = chain.lb_frames[i].cpu().numpy().copy(), chain.lb_out[1][i].cpu().numpy().copy()
            chain.edit(i, chain.lb_frames[i])
            if i >= count:
                continue
            f = emitted
            emitted += 1
            assert np.array_equal(src, frames[f]), f                        # the frames come out in order, untouched
            R2 = (rows_buf.size - 4) // 8
            P.update(ref, src, rows_buf, R2, *REMOVE[1:])
            want, from_plate, _ = P.fill(src.copy(), ref, rows_buf, R2, table, REMOVE[3])
            assert np.array_equal(chain.lb_frames[i].cpu().numpy(), want), f
            plain = undelayed[f]
            R1 = (plain.size - 4) // 8
            P.update(bare, src, plain, R1, *REMOVE[1:])
            _, bare_fill, _ = P.fill(src.copy(), bare, plain, R1, table, REMOVE[3])
            extra_rows += int(rows_buf[0]) - int(plain[0])
            extra_fill += int((from_plate & ~bare_fill).sum())
            if f in (2, 3):                                                 # the frames in front of the car's first detection
                x1, y1, x2, y2 = CAR(f)
                assert int(rows_buf[0]) > int(plain[0]), f                  # a back-filled row ...
                assert from_plate[y1 + 4:y2 - 3, x1 + 4:x2 - 3].all() and not bare_fill[y1:y2 + 1, x1:x2 + 1].any(), f      # ... that fills,
                assert (want[from_plate] != src[from_plate]).any()
                N, bare_N = P.unpack(ref, H, W)[3], P.unpack(bare, H, W)[3]
                assert not N[y1 + 4:y2 - 3, x1 + 4:x2 - 3].any() and bare_N[y1 + 4:y2 - 3, x1 + 4:x2 - 3].all(), f      # ... and blocks
        torch.cuda.synchronize()
        assert np.array_equal(states.plate_state(H, W, True).cpu().numpy()[:4 + 2 * H * W], ref), k
    assert emitted == 6 and ref[0] == 6 and extra_rows >= 2 and extra_fill > 0
    assert not np.array_equal(ref, bare)                                    # without the back-filled rows the car is in the plate
