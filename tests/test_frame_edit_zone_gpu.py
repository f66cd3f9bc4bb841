"""frame_edit.EditChain / EditStates with ``zone=`` and every other option at once, without a model (the inputs of
tests/test_frame_edit_gpu.py): the zone lists and state against the rule (tests/zone_ref.py) from the chain's own tracked buffers, the
drawing order byte for byte, a call per frame against a call per pass, the chain captured against the eager chain, no-draw, and the
resets.  Everything is integers and bytes: torch.equal, no tolerance."""
import dataclasses

import numpy as np
import pytest

from tests import zone_ref as R
from tests.test_frame_edit_gpu import ALL_ON, ALL_ON_PASSES, CAP, COUNT, H, HEAT, NAMES, RADIUS, REDACT, SEG, TRAILS, W, frames_of, packed_of, spec_of, \
    staged, states_of, word

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# the left half and a triangle over the boxes' path, bottom anchor: the boxes of packed_of move right, 3 pixels a frame
ZONE = ((((0, 0), (32, 0), (32, 48), (0, 48)), ((20, 0), (63, 10), (30, 47))), "all", 2, 1)


def run_pass(chain, buf, views, packed, nf):
    chain.update(buf, SEG, packed, nf)
    for i, fr in enumerate(views):
        chain.edit(i, fr)


def test_every_option_at_once_the_lists_match_the_rule_and_the_zone_lies_under_every_line():
    """Two passes with every option: the zone lists and the state are the rule's over the chain's own tracked buffers; and each frame
    is the frame of the chain without ``zone=`` with ops.zone_draw_u8 slipped in behind the heat draw, in front of the trail draw."""
    from faster_rcnn_amd import ops
    from faster_rcnn_amd.frame_edit import EditChain, EditChain as Chain
    spec = spec_of(zone=ZONE, **ALL_ON)
    states = states_of()
    chain = EditChain(states, spec, 4, 2, (H, W), False)
    ref = R.Zones(H, W, ZONE[0], np.ones(len(NAMES), dtype=np.uint8), 2 * CAP, Chain.trails_expire(spec.track, 2), anchor=1)
    # the hand-written side: the chain's own steps with the zone draw in its place
    hand_states = states_of()
    hand = EditChain(hand_states, dataclasses.replace(spec, zone=None), 4, 2, (H, W), False)
    seen = 0
    for frames, pk, n in ALL_ON_PASSES:
        buf, views = staged(frames)
        packed = torch.from_numpy(np.stack(pk)).cuda()
        run_pass(chain, buf, views, packed, word(n))
        torch.cuda.synchronize()
        want_lists = ref.update(chain.tracked.cpu().numpy(), n)
        assert np.array_equal(chain.zone_lists.cpu().numpy(), want_lists) and np.array_equal(states.zone_state().cpu().numpy(), ref.words())
        seen += sum(len(R.events_of(l)) for l in want_lists)
        hbuf, hviews = staged(frames)
        hand.update(hbuf, SEG, packed, word(n))
        assert torch.equal(hand.tracked, chain.tracked)
        for i, fr in enumerate(hviews):
            sp, rows = hand.spec, hand.rows(i)
            ops.redact_u8(fr, rows, hand.redact_table, *sp.redact[1:], workspace=hand.redact_ws, tracked=True)
            ops.heat_update(hand.heat, H, W, rows, hand.heat_table, sp.heat[2], i, hand.n_frames, gate=hand.gate, tracked=True)
            ops.heat_draw_u8(fr, hand.heat, sp.heat[1])
            ops.zone_draw_u8(fr, chain.zone_lists[i], ZONE[0], ZONE[2])
            ops.track_trails_draw_u8(fr, hand.trail_lists[i], *sp.track_trails)
            ops.count_draw_u8(fr, hand.count_lists[i], sp.count[0], sp.count[2])
            ops.annotate_u8(fr, rows, hand.tables, tracked=True)
        assert torch.equal(hbuf, buf)
        plain, pviews = staged(frames)
        assert not torch.equal(plain[:SEG * n], buf[:SEG * n])
    assert seen > 0 and ref.frames == 6 and sum(ref.visitors) > 0
    assert torch.equal(hand_states.count_state(), states.count_state()) and torch.equal(hand_states.tracker(), states.tracker())


def test_the_captured_chain_replays_what_the_eager_chain_does():
    from faster_rcnn_amd.frame_edit import EditChain
    spec = spec_of(zone=ZONE, **ALL_ON)
    eager_states, states = states_of(), states_of()
    eager = EditChain(eager_states, spec, 4, 2, (H, W), False)
    chain = EditChain(states, spec, 4, 2, (H, W), False)
    buf, views = staged(ALL_ON_PASSES[0][0])
    packed, nf = torch.from_numpy(np.stack(ALL_ON_PASSES[0][1])).cuda(), word(0)
    run_pass(chain, buf, views, packed, nf)                         # the warm-up, with no real frame: it makes ``track_out``
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run_pass(chain, buf, views, packed, nf)
    states.reset_tracks()
    states.reset_heat()
    states.reset_counts()
    states.reset_zones()
    for frames, pk, n in ALL_ON_PASSES:
        buf.copy_(staged(frames)[0])
        packed.copy_(torch.from_numpy(np.stack(pk)))
        nf.fill_(n)
        graph.replay()
        ebuf, eviews = staged(frames)
        run_pass(eager, ebuf, eviews, torch.from_numpy(np.stack(pk)).cuda(), word(n))
        torch.cuda.synchronize()
        assert torch.equal(ebuf, buf) and torch.equal(eager.zone_lists, chain.zone_lists) and torch.equal(eager.count_lists, chain.count_lists)
    assert torch.equal(eager_states.zone_state(), states.zone_state()) and int(states.zone_state()[1]) == 6
    assert int(states.zone_state()[4:12].sum()) > 0


def test_a_call_per_frame_is_a_call_per_pass_and_no_draw_counts_and_draws_nothing():
    from faster_rcnn_amd.frame_edit import EditChain
    frames = frames_of(3, 3)
    spec = spec_of(redact=REDACT, track_motion=RADIUS, track_trails=TRAILS, heat=HEAT, count=COUNT, zone=ZONE)
    per_frame, per_pass, blind = states_of(), states_of(), states_of()
    for f in range(3):
        dev = torch.from_numpy(frames[f]).cuda()
        one = EditChain(per_frame, spec, 1, 1, (H, W), False)
        one.update(dev.view(-1), 0, torch.from_numpy(packed_of(f)).cuda(), per_frame.one_frame())
        one.edit(0, dev)
    packed = torch.from_numpy(np.stack([packed_of(f) for f in range(3)])).cuda()
    buf, views = staged(frames)
    chain = EditChain(per_pass, spec, 3, 1, (H, W), False)
    run_pass(chain, buf, views, packed, word(3))
    assert torch.equal(views[2], dev) and torch.equal(one.zone_lists[0], chain.zone_lists[2])
    assert torch.equal(per_frame.zone_state(), per_pass.zone_state()) and int(per_pass.zone_state()[4:12].sum()) > 0
    # no-draw: the same lists and state, and the frames of the chain without count and zone (neither is drawn)
    nbuf, nviews = staged(frames)
    nodraw = EditChain(blind, dataclasses.replace(spec, draw=False), 3, 1, (H, W), False)
    run_pass(nodraw, nbuf, nviews, packed, word(3))
    assert torch.equal(nodraw.zone_lists, chain.zone_lists) and torch.equal(blind.zone_state(), per_pass.zone_state())
    pbuf, pviews = staged(frames)
    run_pass(EditChain(states_of(), dataclasses.replace(spec, draw=False, zone=None, count=None), 3, 1, (H, W), False), pbuf, pviews, packed, word(3))
    assert torch.equal(pbuf, nbuf) and not torch.equal(nbuf, buf)


def test_the_resets_and_the_key():
    from faster_rcnn_amd import ops
    from faster_rcnn_amd.frame_edit import EditChain
    spec = spec_of(zone=ZONE)
    states = states_of()
    states.reset_tracks()                                           # (no state yet: nothing to do)
    states.reset_zones()
    chain = EditChain(states, spec, 3, 1, (H, W), False)
    buf, views = staged(frames_of(3, 3))
    run_pass(chain, buf, views, torch.from_numpy(np.stack([packed_of(f) for f in range(3)])).cuda(), word(3))
    state = states.zone_state()
    assert state is states.zone_state() and int(state.numel()) == ops.zone_state_words(2 * CAP)
    before = ops.zone_totals(state)
    assert before["entries"] > 0 and sum(before["visitors"]) > 0
    states.reset_tracks()
    assert ops.zone_totals(state) == dict(before, entries=0) and not state[ops.ZONE_HEAD:].any()
    states.reset_zones()
    assert not state.any()
    plain = spec_of().key_tail(3)
    assert spec.key_tail(3)[:len(plain)] == plain and spec.key_tail(3)[len(plain):] == ("zone",) + ZONE
    assert spec_of(count=COUNT, zone=ZONE).key_tail(3)[len(plain):] == ("count",) + COUNT + ("zone",) + ZONE
