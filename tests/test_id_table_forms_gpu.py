"""The update and draw entries of the trail, count and zone extensions as the shims over shared checks that they are (csrc/id_table.h,
csrc/overlay.h), called at the raw ABI on real device buffers of the smallest shapes: a call that breaks two rules that follow one another
in an entry's order of refusals is refused with the EARLIER rule's words, under the entry's own name; a refused call launches nothing --
state, lists and frame keep their bytes --; and a well-formed call behind the refusals runs.  The words are those the entries had before
their checks were shared."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CAP, ROWS, F, H, W, N = 2, 1, 1, 16, 16, 2                  # entries, rows of a tracked buffer, frames, the frame, points of a trail
SENTINEL = 77
BAD = 1 << 20                                               # out of every range there is

# Per entry: its rules in the order it refuses in, each (the arguments that break it, the words it is refused with).
HEAD = [(dict(state=None), "null pointer"),
        (dict(capacity=0), "capacity=0 not in [1, 128]"),
        (dict(rows=0), "rows=0 not in [1, 512]"),
        (dict(frames=65), "frames=65 not in [1, 64]"),
        (dict(frames=2, stride=11), "tracked_stride=11 under the 12 words of a tracked buffer")]
TAIL = [(dict(expire=-1), "expire=-1 not in [0, 4095]"),
        (dict(h=0), "frame 0x16 out of range (sides 1..32768)")]
LINES = (dict(n_lines=9), "n_lines=9 not in [1, 8]")
ZONES = (dict(n_zones=0), "n_zones=0 not in [1, 8]")
LENGTH = (dict(length=1), "length=1 not in [2, 64]")
DRAW_HEAD = [(dict(frame=None), "null pointer"), (dict(w=32769), "frame 16x32769 out of range (sides 1..32768)")]
WIDTH = (dict(width=10), "width=10 not in [1, 9]")
ORDERS = {
    "count_update": HEAD + [LINES, (dict(num_classes=257), "num_classes=257 not in [1, 256]")] + TAIL,
    "zone_update": HEAD + [ZONES, (dict(num_classes=0), "num_classes=0 not in [1, 256]"),
                           (dict(anchor=2), "anchor=2 is neither 0 (centre) nor 1 (bottom)")] + TAIL,
    "track_trails_update": HEAD + [LENGTH] + TAIL,
    "count_draw_u8": DRAW_HEAD + [LINES, WIDTH],
    "zone_draw_u8": DRAW_HEAD + [ZONES, WIDTH],
    "track_trails_draw_u8": DRAW_HEAD + [LENGTH, WIDTH],
}


class Buffers:
    """The device buffers of the six entries: the states zeroed, lists and frame full of the sentinel; one live row of class 1 with id 1."""

    def __init__(self):
        from faster_rcnn_amd import ops
        tracked = np.zeros((F, 4 + 8 * ROWS), dtype=np.int32)
        tracked[0, 1], tracked[0, 4:8], tracked[0, 4 + 4 * ROWS], tracked[0, 4 + 6 * ROWS] = 1, (2, 2, 10, 10), 1, 1
        self.tracked, self.nf = torch.from_numpy(tracked).cuda(), torch.full((1,), F, dtype=torch.int32, device="cuda")
        self.table = torch.tensor([0, 1], dtype=torch.uint8, device="cuda")
        self.state = {"count_update": ops.count_state(CAP), "zone_update": ops.zone_state(CAP), "track_trails_update": ops.track_trails_state(CAP, N)}
        words = {"count_update": ops.COUNT_LIST_WORDS, "zone_update": ops.ZONE_LIST_WORDS, "track_trails_update": 4 + CAP * (4 + 2 * N)}
        self.lists = {k: torch.full((F, n), SENTINEL, dtype=torch.int32, device="cuda") for k, n in words.items()}
        self.frame = torch.full((H, W, 3), SENTINEL, dtype=torch.uint8, device="cuda")
        # the lists the draws read, written by hand: one real frame; one trail of id 1 from (2, 2) to (12, 12)
        real = np.zeros(max(words.values()), dtype=np.int32)
        real[1] = 1
        trail = np.zeros(words["track_trails_update"], dtype=np.int32)
        trail[:12] = (1, 0, 0, 0, 1, 1, 2, 0, 2, 2, 12, 12)
        self.real, self.trail = torch.from_numpy(real).cuda(), torch.from_numpy(trail).cuda()
        self.line = np.array([1, 8, 14, 8], dtype=np.int32)                 # one line; one triangle
        self.verts, self.nv = np.array([1, 1, 14, 1, 8, 14], dtype=np.int32), np.array([3], dtype=np.int32)

    def call(self, entry, **over):
        """frcnn_<entry> on the null stream with well-formed arguments but for ``over`` -> its return code."""
        from faster_rcnn_amd import _lib
        host = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        v = dict(capacity=CAP, stride=4 + 8 * ROWS, rows=ROWS, frames=F, n_lines=1, n_zones=1, num_classes=2, anchor=0, length=N, expire=3, h=H, w=W,
                 width=3, frame=self.frame.data_ptr())
        if entry in self.state:
            v["state"] = self.state[entry].data_ptr()
        v.update(over)
        shape = {"count": [host(self.line), v["n_lines"]], "zone": [host(self.verts), host(self.nv), v["n_zones"]], "track": []}[entry.split("_")[0]]
        if entry.endswith("_update"):
            a = [v["state"], v["capacity"], self.tracked.data_ptr(), v["stride"], v["rows"], v["frames"], self.nf.data_ptr(), None]
            if entry == "track_trails_update":
                a += [v["length"]]
            else:
                a += shape + [self.table.data_ptr(), v["num_classes"]] + ([v["anchor"]] if entry == "zone_update" else [])
            a += [v["expire"], v["h"], v["w"], self.lists[entry].data_ptr()]
        elif entry == "track_trails_draw_u8":
            a = [v["frame"], v["h"], v["w"], self.trail.data_ptr(), v["length"], v["width"], 0]
        else:
            a = [v["frame"], v["h"], v["w"], self.real.data_ptr()] + shape + [v["width"], 0]
        return getattr(_lib.load(), "frcnn_" + entry)(*a, None)

    def untouched(self):
        torch.cuda.synchronize()
        return all(not s.cpu().numpy().any() for s in self.state.values()) and all((l.cpu().numpy() == SENTINEL).all() for l in self.lists.values()) \
            and (self.frame.cpu().numpy() == SENTINEL).all()


@pytest.mark.parametrize("entry", sorted(ORDERS))
def test_two_broken_rules_are_refused_with_the_earlier_ones_words_and_nothing_ran_and_the_next_call_runs(entry):
    from faster_rcnn_amd import _lib
    b, order = Buffers(), ORDERS[entry]
    for (first, words), (second, _) in zip(order, order[1:] + [({}, None)]):    # (the last rule alone: its words are checked too)
        code = b.call(entry, **{**second, **first})                         # (65 frames with a short stride break the stride's rule as well)
        msg = _lib.load().frcnn_last_error().decode()
        assert code == -1 and msg == "%s: %s" % (entry, words), (first, second, code, msg)
    assert b.untouched()                                                     # one synchronize behind all of them: nothing was launched
    assert b.call(entry) == 0
    torch.cuda.synchronize()
    if entry.endswith("_update"):
        state, lists = b.state[entry].cpu().numpy(), b.lists[entry].cpu().numpy()
        assert state[0] == 1 and state[1] == 1 and not (lists == SENTINEL).any()    # the row's id has its entry, the frame counted, the list written
    else:
        frame = b.frame.cpu().numpy()
        assert (frame[8, 8] != SENTINEL).any() and (frame[15, 0] == SENTINEL).all()  # the line, the triangle's label, the trail; a far corner
