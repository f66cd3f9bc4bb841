"""frame_edit.EditChain / EditStates driven directly, without a model: every buffer, list and state of the chain against the same
ops.* calls written out by hand in DESIGN §8's order, on copies of the same synthetic inputs; the chain captured in a graph; a call per
frame against a call per pass; and the three resets against the ops calls they stand for.  Everything is integers and bytes:
torch.equal, no tolerance."""
import numpy as np
import pytest

from tests.test_track_gpu import pack

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

H, W, ROWS, CAP = 48, 64, 8, 4
NPIX = H * W * 3
SEG = NPIX + 16                                           # the frames' distance in the staging buffer: not the frame's own size
NAMES = ["bg", "car", "person", "bike"]
TRACK, RADIUS, TRAILS, HEAT = (30, 2, 1), 4, (4, 3), ("all", 160, 1)
COUNT = (((20, 0, 20, 47),), "all", 3)
REDACT = (("car", "person"), "pixelate", 8, 2)


def frames_of(seed, n, cut_at=None):
    """n frames whose content moves 3 pixels to the right per frame (what the block match finds); from ``cut_at`` on another picture."""
    rs = np.random.RandomState(seed)
    base, other = rs.randint(0, 256, (H, W, 3)).astype(np.uint8), rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    return [np.roll(other if cut_at is not None and f >= cut_at else base, 3 * f, axis=1) for f in range(n)]


def packed_of(f):
    """Frame f's packed buffer of ROWS rows: three boxes that move with the picture, one of them across COUNT's line."""
    boxes = [[7 + 3 * f, 10, 23 + 3 * f, 30], [30 + 3 * f, 5, 44 + 3 * f, 25 + f], [2, 30 + f, 14, 44 + f]]
    return pack(boxes, [1, 2, 3], 3, ROWS)


def staged(frames):
    """The frames in one staging buffer SEG bytes apart -> (the buffer, a view per frame)."""
    buf = torch.zeros(len(frames) * SEG, dtype=torch.uint8, device="cuda")
    views = [buf[i * SEG:i * SEG + NPIX].view(H, W, 3) for i in range(len(frames))]
    for v, f in zip(views, frames):
        v.copy_(torch.from_numpy(f))
    return buf, views


def word(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


def spec_of(**kw):
    from faster_rcnn_amd.entry import PassSpec
    return PassSpec(annotate=True, track=TRACK, **kw)


def states_of():
    from faster_rcnn_amd.frame_edit import EditStates
    return EditStates(NAMES, CAP, 2 * CAP)


class Hand:
    """The states and tables of the hand-written side, made by the ops calls themselves."""

    def __init__(self):
        from faster_rcnn_amd import ops
        self.tracker, self.motion = ops.track_state(CAP), ops.track_motion_state(H, W)
        self.trails, self.count, self.heat = ops.track_trails_state(2 * CAP, TRAILS[0]), ops.count_state(2 * CAP), ops.heat_state(H, W)
        self.track_table = ops.track_table(NAMES, ["car", "person", "bike"])
        self.redact_table, self.all_table = ops.redact_table(NAMES, REDACT[0]), ops.redact_table(NAMES, "all")
        self.tables = ops.annotate_tables(NAMES)

    def same_states(self, states):
        assert torch.equal(self.tracker, states.tracker()) and torch.equal(self.motion, states.motion_state(H, W))
        assert torch.equal(self.trails, states.trails_state(TRAILS[0])) and torch.equal(self.count, states.count_state())
        assert torch.equal(self.heat, states.heat_state(H, W))
        assert len(states.motion) == len(states.trails) == len(states.heat) == 1


ALL_ON = dict(redact=REDACT, track_motion=RADIUS, detect_every=2, track_scene_cut=40, track_trails=TRAILS, heat=HEAT, count=COUNT)
# the two passes of the all-options case: (frames, the key frames' packed buffers, n_frames) -- the last frame of each is padding, and
# the third frame of the second pass is another picture
ALL_ON_PASSES = [(frames_of(1, 4), [packed_of(0), packed_of(2)], 3), (frames_of(1, 8, cut_at=6)[4:], [packed_of(4), packed_of(6)], 3)]


def hand_all_on(hand, buf, views, packed, nf, out):
    """One all-options pass (F = 4, K = 2) by hand -> (track_out, cuts, trail lists, count lists)."""
    from faster_rcnn_amd import ops
    track_out, cuts = out
    expire = (TRACK[1] + 1) * 2
    ops.track_update_cut(hand.tracker, hand.motion, buf, SEG, packed, nf, hand.track_table, H, W, *TRACK, RADIUS, 2, 40, out=track_out, cuts=cuts)
    tl = ops.track_trails_update(hand.trails, track_out, nf, TRAILS[0], expire, H, W)
    cl = ops.count_update(hand.count, track_out, nf, COUNT[0], hand.all_table, expire, H, W)
    for i, fr in enumerate(views):
        ops.redact_u8(fr, track_out[i], hand.redact_table, *REDACT[1:], tracked=True)
        ops.heat_update(hand.heat, H, W, track_out[i], hand.all_table, HEAT[2], i, nf, tracked=True)
        ops.heat_draw_u8(fr, hand.heat, HEAT[1], rgb=False)
        ops.track_trails_draw_u8(fr, tl[i], *TRAILS, rgb=False)
        ops.count_draw_u8(fr, cl[i], COUNT[0], COUNT[2], rgb=False)
        ops.annotate_u8(fr, track_out[i], hand.tables, tracked=True)
    return track_out, cuts, tl, cl


def all_on_by_hand():
    """-> (hand, [(the staging buffer, track_out, cuts, trail lists, count lists) after each pass])."""
    hand, res = Hand(), []
    out = (torch.zeros((4, 4 + 8 * (ROWS + CAP)), dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda"))
    for frames, packed, n in ALL_ON_PASSES:
        buf, views = staged(frames)
        got = hand_all_on(hand, buf, views, torch.from_numpy(np.stack(packed)).cuda(), word(n), out)
        res.append((buf,) + tuple(t.clone() for t in got))
    return hand, res


def same_pass(chain, buf, want):
    w_buf, w_track, w_cuts, w_trails, w_counts = want
    assert torch.equal(buf, w_buf), "frames"
    assert torch.equal(chain.track_out, w_track) and torch.equal(chain.cuts, w_cuts)
    assert torch.equal(chain.trail_lists, w_trails) and torch.equal(chain.count_lists, w_counts)


def test_every_option_at_once_is_the_calls_written_out():
    """(a) F = 4, K = 2 (two key buffers), n_frames = 3: the padding frame is edited too and the gates matter; two passes, so the
    states are carried."""
    from faster_rcnn_amd.frame_edit import EditChain
    hand, want = all_on_by_hand()
    states = states_of()
    chain = EditChain(states, spec_of(**ALL_ON), 4, 2, (H, W), False)
    for (frames, packed, n), w in zip(ALL_ON_PASSES, want):
        buf, views = staged(frames)
        chain.update(buf, SEG, torch.from_numpy(np.stack(packed)).cuda(), word(n))
        for i, fr in enumerate(views):
            assert chain.rows(i).data_ptr() == chain.track_out[i].data_ptr()
            chain.edit(i, fr)
        same_pass(chain, buf, w)
        assert not torch.equal(buf, staged(frames)[0])              # (the edits did paint)
    hand.same_states(states)
    assert int(states.heat_state(H, W)[0]) == 6                     # three real frames per pass


def test_a_delayed_pass_edits_the_emitted_frames():
    """(b) F = 2 with look-back 2, trails, count and heat, as two passes and the flush: the second emits the first's frames, and the
    updates read the emitted buffers and the emitted count, gated by the pass's own count."""
    from faster_rcnn_amd import _lib, ops
    from faster_rcnn_amd.frame_edit import EditChain
    frames = frames_of(2, 4)
    passes = [(frames[0:2], [packed_of(0), packed_of(1)], 2), (frames[2:4], [packed_of(2), packed_of(3)], 2), (frames[0:2], [packed_of(0)] * 2, -1)]
    hand, states = Hand(), states_of()
    chain = EditChain(states, spec_of(track_motion=RADIUS, track_lookback=2, track_trails=TRAILS, heat=HEAT, count=COUNT), 2, 1, (H, W), True)
    back = min(CAP, _lib.REDACT_MAX_ROWS - ROWS - CAP)
    window = ops.track_lookback_state(2, H, W, ROWS, CAP, back)
    track_out = torch.zeros((2, 4 + 8 * (ROWS + CAP)), dtype=torch.int32, device="cuda")
    lb_out = (torch.zeros((2, H, W, 3), dtype=torch.uint8, device="cuda"), torch.zeros((2, 4 + 8 * (ROWS + CAP + back)), dtype=torch.int32, device="cuda"),
              torch.zeros(4, dtype=torch.int32, device="cuda"))
    expire = TRACK[1] + 1
    for k, (fr, packed, n) in enumerate(passes):
        packed, nf = torch.from_numpy(np.stack(packed)).cuda(), word(n)
        buf, _ = staged(fr)
        ops.track_update_motion(hand.tracker, hand.motion, buf, SEG, packed, nf, hand.track_table, H, W, *TRACK, RADIUS, out=track_out)
        ops.track_lookback(window, buf, SEG, track_out, nf, CAP, back, H, W, 2, RADIUS, TRACK[2], out=lb_out)
        tl = ops.track_trails_update(hand.trails, lb_out[1], lb_out[2], TRAILS[0], expire, H, W, gate=nf)
        cl = ops.count_update(hand.count, lb_out[1], lb_out[2], COUNT[0], hand.all_table, expire, H, W, gate=nf)
        for i in range(2):
            ops.heat_update(hand.heat, H, W, lb_out[1][i], hand.all_table, HEAT[2], i, lb_out[2], gate=nf, tracked=True)
            ops.heat_draw_u8(lb_out[0][i], hand.heat, HEAT[1], rgb=True)
            ops.track_trails_draw_u8(lb_out[0][i], tl[i], *TRAILS, rgb=True)
            ops.count_draw_u8(lb_out[0][i], cl[i], COUNT[0], COUNT[2], rgb=True)
            ops.annotate_u8(lb_out[0][i], lb_out[1][i], hand.tables, tracked=True)
        buf2, _ = staged(fr)
        chain.update(buf2, SEG, packed.clone(), nf.clone())
        for i in range(2):
            assert chain.rows(i).data_ptr() == chain.lb_out[1][i].data_ptr()
            chain.edit(i, chain.lb_frames[i])
        assert torch.equal(buf2, buf), k                            # (a delayed pass leaves its own frames as they came)
        assert torch.equal(chain.track_out, track_out), k
        for got, w in zip(chain.lb_out, lb_out):
            assert torch.equal(got, w), k
        assert chain.lb_out[0] is chain.lb_frames and int(chain.lb_out[2][0]) == (0, 2, 2)[k]
        assert torch.equal(chain.trail_lists, tl) and torch.equal(chain.count_lists, cl), k
        if k == 1:                                                  # the emitted frames are the first pass's, edited
            assert not torch.equal(chain.lb_frames, torch.from_numpy(np.stack(frames[0:2])).cuda())
    hand.same_states(states)
    assert torch.equal(states.lookback[(H, W, 2)][0], window) and states.lookback[(H, W, 2)][1] == back
    assert int(states.heat_state(H, W)[0]) == 4                     # the four emitted frames, each once


def test_the_captured_chain_replays_what_the_eager_chain_does():
    """(c) The all-options pass captured in a graph and replayed twice from reset states, against the hand-written rounds (which (a)
    holds equal to two eager update + edit rounds)."""
    from faster_rcnn_amd.frame_edit import EditChain
    hand, want = all_on_by_hand()
    states = states_of()
    chain = EditChain(states, spec_of(**ALL_ON), 4, 2, (H, W), False)
    buf, views = staged(ALL_ON_PASSES[0][0])
    packed, nf = torch.from_numpy(np.stack(ALL_ON_PASSES[0][1])).cuda(), word(0)

    def run():
        chain.update(buf, SEG, packed, nf)
        for i, fr in enumerate(views):
            chain.edit(i, fr)
    run()                                                           # the warm-up, with no real frame: it makes ``track_out``
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    states.reset_tracks()
    states.reset_heat()
    states.reset_counts()
    for (frames, pk, n), w in zip(ALL_ON_PASSES, want):
        buf.copy_(staged(frames)[0])
        packed.copy_(torch.from_numpy(np.stack(pk)))
        nf.fill_(n)
        graph.replay()
        torch.cuda.synchronize()
        same_pass(chain, buf, w)
    hand.same_states(states)


def test_a_call_per_frame_is_a_call_per_pass():
    """(d) A one-frame chain per frame, as draw_eager builds it (F = 1, interval 1, stride 0, the one-frame count word), over frames
    0..2 against ONE chain over the three frames: the same tracker state, and the same bytes in frame 2."""
    from faster_rcnn_amd.frame_edit import EditChain
    frames = frames_of(3, 3)
    spec = spec_of(redact=REDACT, track_motion=RADIUS, track_trails=TRAILS, heat=HEAT, count=COUNT)
    per_frame, per_pass = states_of(), states_of()
    for f in range(3):
        dev = torch.from_numpy(frames[f]).cuda()
        one = EditChain(per_frame, spec, 1, 1, (H, W), False)
        one.update(dev.view(-1), 0, torch.from_numpy(packed_of(f)).cuda(), per_frame.one_frame())
        one.edit(0, dev)
    buf, views = staged(frames)
    chain = EditChain(per_pass, spec, 3, 1, (H, W), False)
    chain.update(buf, SEG, torch.from_numpy(np.stack([packed_of(f) for f in range(3)])).cuda(), word(3))
    for i, fr in enumerate(views):
        chain.edit(i, fr)
    assert torch.equal(views[2], dev) and not torch.equal(dev, torch.from_numpy(frames[2]).cuda())
    assert torch.equal(one.track_out[0], chain.track_out[2]) and torch.equal(one.count_lists[0], chain.count_lists[2])
    for name in ("tracker", "count_state"):
        assert torch.equal(getattr(per_frame, name)(), getattr(per_pass, name)()), name
    assert torch.equal(per_frame.motion_state(H, W), per_pass.motion_state(H, W))
    assert torch.equal(per_frame.trails_state(TRAILS[0]), per_pass.trails_state(TRAILS[0]))
    assert torch.equal(per_frame.heat_state(H, W), per_pass.heat_state(H, W))
    assert int(per_pass.heat_state(H, W)[0]) == 3


def test_the_resets_are_the_ops_calls_they_stand_for():
    """(e) States that passes have used (a look-back window among them), with totals written into the count state: each reset against
    the ops calls on copies; the totals survive ``reset_tracks`` and not ``reset_counts``; the tables and states are made once."""
    from faster_rcnn_amd import ops
    from faster_rcnn_amd.frame_edit import EditChain
    states = states_of()
    frames = frames_of(4, 2)
    packed = torch.from_numpy(np.stack([packed_of(0), packed_of(1)])).cuda()
    # (the delayed chain runs twice: its second pass emits the first's frames, and only emitted frames reach the trails)
    for spec, passes in ((spec_of(track_motion=RADIUS, track_trails=TRAILS, heat=HEAT, count=COUNT), 1), (spec_of(track_lookback=2, track_trails=(5, 2)), 2)):
        chain = EditChain(states, spec, 2, 1, (H, W), False)
        for _ in range(passes):
            buf, views = staged(frames)
            chain.update(buf, SEG, packed, word(2))
            for i in range(2):
                chain.edit(i, chain.lb_frames[i] if spec.delayed else views[i])
    totals = torch.arange(1, 17, dtype=torch.int32, device="cuda")
    states.count_state()[4:20] += totals
    window = states.lookback[(H, W, 2)][0]
    live = [states.tracker(), states.motion_state(H, W), window, states.trails_state(4), states.trails_state(5), states.count_state(), states.heat_state(H, W)]
    assert all(bool(t.any()) for t in live) and int(states.count_state()[0]) > 0
    tracker, motion, win, trails4, trails5, count, heat = [t.clone() for t in live]
    kept = states.count_state()[4:20].clone()

    states.reset_tracks()
    for t in (tracker, trails4, trails5):
        ops.track_reset(t)
    ops.track_motion_reset(motion)
    ops.track_lookback_reset(win)
    ops.count_reset(count, keep_totals=True)
    for got, w in zip(live, (tracker, motion, win, trails4, trails5, count, heat)):
        assert torch.equal(got, w)
    assert torch.equal(states.count_state()[4:20], kept) and int(states.count_state()[0]) == 0 and bool(states.heat_state(H, W).any())
    assert not bool(states.tracker().any()) and not bool(motion[:16].any()) and bool(motion[16:].any())

    states.reset_heat()
    assert torch.equal(states.heat_state(H, W), ops.heat_reset(heat)) and not bool(heat.any()) and torch.equal(states.count_state()[4:20], kept)
    states.reset_counts()
    assert torch.equal(states.count_state(), ops.count_reset(count)) and not bool(count.any())
    # made once: the same objects again, another for another key
    for got, w in zip([states.tracker(), states.motion_state(H, W), states.lookback_window(H, W, 2, ROWS)[0], states.trails_state(4), states.trails_state(5),
                       states.count_state(), states.heat_state(H, W)], live):
        assert got is w
    assert states.heat_state(H, W + 1) is not live[6] and states.redact_table("all") is states.redact_table("all")
    assert states.annotate_tables(True) is states.annotate_tables() and states.annotate_tables(False) is not states.annotate_tables()
    assert not bool(states.annotate_tables(False)["drawable"].any()) and states.track_table(None) is not states.track_table(("car",))
