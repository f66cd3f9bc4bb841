"""frame_edit.EditChain / EditStates with ``track_reid=`` on hand-made packed buffers, without a model (the inputs of
tests/test_frame_edit_gpu.py): an object that is hidden for longer than the tracker holds it comes back under its old id, its label says
so, and the count line counts it once; the same chain without the option is the statement of the gap.  Integers and bytes: no tolerance."""
import dataclasses

import numpy as np
import pytest

from tests.test_frame_edit_gpu import CAP, H, ROWS, SEG, TRACK, W, spec_of, staged, states_of, word
from tests.test_track_gpu import pack

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

COUNT = (((20, 0, 20, 47),), "all", 3)                  # a vertical line at x = 20
REID = (25, 250)
RED, BLUE = (230, 20, 20), (20, 20, 230)
HOLD = TRACK[1]
# the left edge of the 20 x 16 box per frame, None where it is hidden: it crosses the line to the right (centres 11, 17, 23), is away for
# hold + 2 frames, comes back where it left and crosses back and forth (23, 17, 23)
PATH = [2, 8, 14] + [None] * (HOLD + 2) + [14, 8, 14]
assert len(PATH) % 2 == 0


def box_at(x):
    return [x, 12, x + 19, 27]


def scene(colour_back):
    """-> [(frame, packed buffer)] along PATH: a red patch under its box; from its return on the patch is ``colour_back``."""
    out, back = [], False
    for x in PATH:
        f = np.zeros((H, W, 3), dtype=np.uint8)
        if x is None:
            back = True
            out.append((f, pack([], [], 0, ROWS)))
            continue
        x1, y1, x2, y2 = box_at(x)
        f[y1:y2 + 1, x1:x2 + 1] = colour_back if back else RED
        out.append((f, pack([box_at(x)], [1], 1, ROWS)))
    return out


def play(spec, steps, rgb=True):
    """The chain over ``steps`` in passes of two frames -> (states, chain, per frame: the live (id, cls) rows, the frame's bytes, the
    count list and the reid list -- None without the option)."""
    from faster_rcnn_amd.frame_edit import EditChain
    states = states_of()
    chain = EditChain(states, spec, 2, 1, (H, W), rgb)
    ids, pictures, counts, reids = [], [], [], []
    for at in range(0, len(steps), 2):
        buf, views = staged([s[0] for s in steps[at:at + 2]])
        chain.update(buf, SEG, torch.from_numpy(np.stack([s[1] for s in steps[at:at + 2]])).cuda(), word(2))
        for i, fr in enumerate(views):
            chain.edit(i, fr)
        torch.cuda.synchronize()
        R = (chain.tracked.shape[1] - 4) // 8
        for i in range(2):
            t = chain.tracked[i].cpu().numpy()
            ids.append([(int(t[4 + 6 * R + r]), int(t[4 + 4 * R + r])) for r in range(int(t[1]))])
            pictures.append(views[i].cpu().numpy().copy())
            counts.append(chain.count_lists[i].clone())
            reids.append(None if chain.reid_lists is None else chain.reid_lists[i].cpu().numpy())
    return states, chain, ids, pictures, counts, reids


def test_a_returning_object_keeps_its_id_its_label_and_is_counted_once():
    from faster_rcnn_amd import ops
    steps = scene(RED)
    back = len(PATH) - 3                                                    # the frame of the return
    states, chain, ids, pictures, counts, reids = play(spec_of(count=COUNT, track_reid=REID), steps)
    assert [i for i in ids if i] == [[(1, 1)]] * 6 and ids[back] == [(1, 1)]
    totals = ops.track_reid_totals(states.reid_state())
    assert totals == {"entries": 1, "frames": len(PATH), "dropped": 0, "reidentified": 1}
    # the one event: the tracker's id 2 is id 1, class 1, the same look (distance 0), last seen hold + 3 frames before
    assert [ops.track_reid_events(r) for r in reids] == [[]] * back + [[(1, 2, 1, 0, HOLD + 3)]] + [[]] * 2
    assert int(states.tracker()[1]) == 2                                    # the tracker itself issued a second id
    # once per id, line and direction: to the right (the line's - direction) once, although it crossed to the right twice; to the left once
    assert ops.count_totals(states.count_state())["totals"][0] == (1, 1)
    # the label reads car#1: the frame is the source frame with the row drawn under id 1, and not the one drawn under id 2
    for use_id, same in ((1, True), (2, False)):
        f = torch.from_numpy(steps[back][0]).cuda()
        t = ops.track_update(ops.track_state(CAP), torch.from_numpy(steps[back][1]).cuda(), word(1), chain.track_table, H, W, *TRACK)
        R = (t.shape[1] - 4) // 8
        t[0, 4 + 6 * R] = use_id
        ops.count_draw_u8(f, counts[back], COUNT[0], COUNT[2], rgb=True)
        ops.annotate_u8(f, t[0], chain.tables, tracked=True)
        assert np.array_equal(f.cpu().numpy(), pictures[back]) == same


def test_without_the_option_it_is_a_new_id_and_counted_twice():
    """The gap the option closes, stated: the same chain without ``track_reid``."""
    from faster_rcnn_amd import ops
    states, chain, ids, *_ = play(spec_of(count=COUNT), scene(RED))
    assert [i for i in ids if i] == [[(1, 1)]] * 3 + [[(2, 1)]] * 3
    assert ops.count_totals(states.count_state())["totals"][0] == (2, 1)              # (-, +): to the right is the line's - direction
    assert states._reid is None and chain.reid_out is None                  # ... and nothing of the stage ran


def test_another_object_that_appears_instead_is_a_new_id():
    from faster_rcnn_amd import ops
    states, chain, ids, *_ = play(spec_of(count=COUNT, track_reid=REID), scene(BLUE))
    assert [i for i in ids if i] == [[(1, 1)]] * 3 + [[(2, 1)]] * 3
    totals = ops.track_reid_totals(states.reid_state())
    assert totals["reidentified"] == 0 and totals["entries"] == 2
    assert ops.count_totals(states.count_state())["totals"][0] == (2, 1)              # (-, +): to the right is the line's - direction
    # B, G, R frames of the returning scene: it returns there too
    states, chain, ids, *_ = play(spec_of(count=COUNT, track_reid=REID), [(np.ascontiguousarray(f[..., ::-1]), p) for f, p in scene(RED)], rgb=False)
    assert [i for i in ids if i] == [[(1, 1)]] * 6


def test_nothing_re_identified_changes_no_byte_and_the_resets():
    from faster_rcnn_amd import ops
    from faster_rcnn_amd._lib import FrcnnError
    from faster_rcnn_amd.frame_edit import EditChain
    steps = scene(BLUE)
    states, chain, ids, with_reid, *_ = play(spec_of(count=COUNT, track_reid=REID), steps)
    _, _, _, without, *_ = play(spec_of(count=COUNT), steps)
    assert all(np.array_equal(a, b) for a, b in zip(with_reid, without))    # CONSEQUENCE, through the whole chain
    state = states.reid_state()
    assert state is states.reid_state() and int(state.numel()) == ops.track_reid_state_words(2 * CAP)
    states.reset_reid()
    assert not state.any() and int(states.tracker()[1]) == 2
    states.reid_state()[0] = 1
    states.reset_tracks()
    assert not state.any() and not states.tracker().any()
    # refused by name
    with pytest.raises(FrcnnError, match="track_reid"):
        EditChain(states_of(), spec_of(track_reid=REID, track_lookback=4), 2, 1, (H, W), True)
    with pytest.raises(FrcnnError, match="track_reid"):
        EditChain(states_of(), spec_of(track_reid=REID, track_backtrack=4, detect_every=2), 2, 2, (H, W), True)
    with pytest.raises(FrcnnError, match="track_reid"):
        EditChain(states_of(), dataclasses.replace(spec_of(track_reid=REID), track=None), 2, 1, (H, W), True)
