"""Hand cases on tests/track_reid_ref.py, the numpy statement of the re-identify rule (DESIGN §8 "Re-identify rule"): what the rule says
at each of its edges, with numbers worked out by hand.  No GPU."""
import numpy as np

from tests import track_reid_ref as ref

H, W, R = 48, 64, 6
RED, BLUE, GREEN = (255, 0, 0), (0, 0, 255), (0, 255, 0)
CLASSES = np.array([0, 1, 1], dtype=np.uint8)          # class 0 is not tracked
BOX = (8, 8, 23, 23)                                    # 16 x 16: 256 samples, a count is worth 16
BOX2 = (40, 24, 55, 39)


def frame(*patches):
    """A black RGB frame with flat patches (box, colour[, k]): the first k samples of the box, in row order, are left black."""
    f = np.zeros((H, W, 3), dtype=np.uint8)
    for p in patches:
        (x1, y1, x2, y2), colour = p[0], p[1]
        f[y1:y2 + 1, x1:x2 + 1] = colour
        for k in range(p[2] if len(p) > 2 else 0):
            f[y1 + k // (x2 - x1 + 1), x1 + k % (x2 - x1 + 1)] = 0
    return f


def run(steps, capacity=8, pct=25, keep=250, state=None):
    """``steps``: (frame, live rows, held rows[, cut]) one call each -> (state, [out], [events])"""
    state = ref.new_state(capacity) if state is None else state
    outs, evs = [], []
    for st in steps:
        f, live, held = st[:3]
        cuts = np.array([st[3]], dtype=np.int32) if len(st) > 3 else None
        state, out, lists, _ = ref.update(state, capacity, f[None], ref.pack(R, live, held)[None], 1, CLASSES, pct, keep, True, cuts)
        outs.append(out[0])
        evs.append(ref.events(lists[0]))
    return state, outs, evs


def ids(out):
    return [int(v) for v in out[4 + 6 * R:4 + 7 * R]]


EMPTY = (frame(), [], [])


def test_signature_by_hand():
    s = ref.signature(frame((BOX, RED)), BOX, True)
    # 16 rows: bands of 6, 5 and 5 rows of 16 samples; bin of pure red = 3 << 4
    want = np.zeros(192, dtype=np.int32)
    want[48], want[64 + 48], want[128 + 48] = (96 << 12) // 256, (80 << 12) // 256, (80 << 12) // 256
    assert np.array_equal(s, want) and s.sum() == 4096
    assert np.array_equal(ref.signature(frame((BOX, RED))[:, :, ::-1], BOX, False), s)      # the same pixels as B, G, R
    assert ref.distance(s, ref.signature(frame((BOX, BLUE)), BOX, True)) == 8192
    assert ref.signature(frame(), (0, 0, 4, 2), True) is None and ref.signature(frame(), (0, 0, 3, 3), True) is not None      # 15 and 16 samples
    assert ref.signature(frame(), (70, 0, 90, 9), True) is None                              # outside the frame


def test_return_inside_and_outside_keep():
    seen = (frame((BOX, RED)), [(BOX, 1, 1)], [])
    back = lambda i: (frame((BOX2, RED)), [(BOX2, 1, i)], [])
    # keep = 3: seen in frame 1, back in frame 4: frames - last_seen == keep is taken
    state, outs, evs = run([seen, EMPTY, EMPTY, back(2)], keep=3)
    assert ids(outs[3])[0] == 1 and evs[3] == [(1, 2, 1, 0, 3)]
    table, fr, dropped, reid = ref.read_state(state, 8)
    assert (fr, dropped, reid) == (4, 0, 1) and [(e["pid"], e["tid"], e["seen"]) for e in table] == [(1, 2, 4)]
    # back in frame 5: keep + 1 is not, the entry was still there in frame 4 and leaves in frame 5
    state, outs, evs = run([seen, EMPTY, EMPTY, EMPTY], keep=3)
    assert ref.read_state(state, 8)[0][0]["pid"] == 1
    state, outs, evs = run([seen, EMPTY, EMPTY, EMPTY, back(2)], keep=3)
    assert ids(outs[4])[0] == 2 and evs[4] == []
    table, fr, dropped, reid = ref.read_state(state, 8)
    assert reid == 0 and [(e["pid"], e["tid"]) for e in table] == [(2, 2)]


def test_held_tid_is_no_candidate():
    f = frame((BOX, RED), (BOX2, RED))
    state, outs, evs = run([(f, [(BOX, 1, 1)], []), (f, [(BOX2, 1, 2)], [(BOX, 1, 1)])])
    assert ids(outs[1])[:2] == [2, 1] and evs[1] == []
    assert [(e["pid"], e["tid"]) for e in ref.read_state(state, 8)[0]] == [(1, 1), (2, 2)]
    # the held row updates nothing: last_seen of entry 1 is still frame 1
    assert ref.read_state(state, 8)[0][0]["seen"] == 1


def test_two_returns_cannot_take_one_entry():
    f = frame((BOX, RED), (BOX2, RED))
    state, outs, evs = run([(f, [(BOX, 1, 1)], []), EMPTY, (f, [(BOX, 1, 2), (BOX2, 1, 3)], [])])
    assert ids(outs[2])[:2] == [1, 3] and evs[2] == [(1, 2, 1, 0, 2)]
    assert [(e["pid"], e["tid"]) for e in ref.read_state(state, 8)[0]] == [(1, 2), (3, 3)]


def test_equal_distances_go_to_the_lowest_pid():
    f = frame((BOX, RED), (BOX2, RED))
    state, outs, evs = run([(f, [(BOX, 1, 1), (BOX2, 1, 2)], []), EMPTY, (f, [(BOX2, 1, 3)], [])])
    assert ids(outs[2])[0] == 1 and evs[2] == [(1, 3, 1, 0, 2)]


def test_nearer_beats_lower_pid():
    f = frame((BOX, RED, 32), (BOX2, RED))
    state, outs, evs = run([(f, [(BOX, 1, 1), (BOX2, 1, 2)], []), EMPTY, (f, [(BOX2, 1, 3)], [])])
    assert ids(outs[2])[0] == 2 and evs[2] == [(2, 3, 1, 0, 2)]


def test_class_mismatch_is_no_candidate():
    f = frame((BOX, RED))
    state, outs, evs = run([(f, [(BOX, 1, 1)], []), EMPTY, (f, [(BOX, 2, 2)], [])])
    assert ids(outs[2])[0] == 2 and evs[2] == []


def test_row_without_signature_never_matches_and_is_no_candidate():
    small = (8, 8, 10, 10)                                                  # 9 samples
    f = frame((BOX, RED))
    # an entry without a signature is no candidate
    state, outs, evs = run([(f, [(small, 1, 1)], []), EMPTY, (f, [(BOX, 1, 2)], [])])
    assert ids(outs[2])[0] == 2 and evs[2] == []
    assert [(e["pid"], e["has"]) for e in ref.read_state(state, 8)[0]] == [(1, 0), (2, 1)]
    # a row without a signature is never matched
    state, outs, evs = run([(f, [(BOX, 1, 1)], []), EMPTY, (f, [(small, 1, 2)], [])])
    assert ids(outs[2])[0] == 2 and evs[2] == []
    # an untracked class gets no entry at all and keeps its id
    state, outs, evs = run([(f, [(BOX, 0, 5)], [])])
    assert ids(outs[0])[0] == 5 and ref.read_state(state, 8)[0] == []


def test_pct_boundary():
    # 64 of 256 samples differ: D = 2 * 64 * 16 = 2048 and 2048 * 100 == 25 * 8192 is taken; 65 differ: 2080 is not
    for k, taken in ((64, True), (65, False)):
        state, outs, evs = run([(frame((BOX, RED)), [(BOX, 1, 1)], []), EMPTY, (frame((BOX, RED, k)), [(BOX, 1, 2)], [])], pct=25)
        assert (ids(outs[2])[0] == 1) == taken, k
        assert evs[2] == ([(1, 2, 1, 32 * k, 2)] if taken else [])
    # ... and the entry's signature is averaged: (3 * old + new + 2) >> 2
    state, outs, evs = run([(frame((BOX, RED)), [(BOX, 1, 1)], []), EMPTY, (frame((BOX, RED, 64)), [(BOX, 1, 2)], [])], pct=25)
    old, new = ref.signature(frame((BOX, RED)), BOX, True), ref.signature(frame((BOX, RED, 64)), BOX, True)
    assert np.array_equal(ref.read_state(state, 8)[0][0]["sig"], (3 * old + new + 2) >> 2)


def test_full_table_counts_dropped():
    f = frame((BOX, RED), (BOX2, BLUE))
    state, outs, evs = run([(f, [(BOX, 1, 1), (BOX2, 1, 2)], [])] * 2, capacity=1)
    assert ids(outs[1])[:2] == [1, 2]
    table, fr, dropped, reid = ref.read_state(state, 1)
    assert dropped == 2 and [e["pid"] for e in table] == [1]               # once per frame: the row has no entry in the next frame either


def test_cut_empties_the_table():
    f = frame((BOX, RED))
    state, outs, evs = run([(f, [(BOX, 1, 1)], []), EMPTY, (f, [(BOX, 1, 2)], [], 1)])
    assert ids(outs[2])[0] == 2 and evs[2] == []
    table, fr, dropped, reid = ref.read_state(state, 8)
    assert fr == 3 and [(e["pid"], e["tid"]) for e in table] == [(2, 2)]


def test_insert_keeps_pid_order_and_words_behind_are_zero():
    f = frame((BOX, RED), (BOX2, BLUE))
    state, _, _ = run([(f, [(BOX, 1, 7), (BOX2, 1, 3)], [])])
    assert [e["pid"] for e in ref.read_state(state, 8)[0]] == [3, 7]
    assert not state[4 + 2 * ref.ENTRY_WORDS:].any()
    state, _, _ = run([EMPTY] * 2, keep=1, state=state)
    assert state[0] == 0 and state[1] == 3 and not state[4:].any()


def test_consequence_byte_for_byte():
    # objects of distinct colours come and go: nothing is ever re-identified and every out buffer is the tracked buffer
    rs = np.random.RandomState(7)
    colour = lambda i: (32 + 64 * (i % 4), 32 + 64 * (i // 4 % 4), 32 + 64 * (i // 16 % 4))          # a bin of its own for every id
    boxes = [(2 + 10 * k, 4, 9 + 10 * k, 30) for k in range(6)]
    state, next_id, alive = ref.new_state(8), 1, {}
    for step in range(40):
        for k in range(6):
            if k in alive and rs.rand() < 0.2:
                del alive[k]
            elif k not in alive and rs.rand() < 0.3:
                alive[k], next_id = next_id, next_id + 1
        f = frame(*[(boxes[k], colour(alive[k])) for k in alive])
        buf = ref.pack(R, [(boxes[k], 1 + k % 2, alive[k]) for k in sorted(alive)])
        state, out, lists, _ = ref.update(state, 8, f[None], buf[None], 1, CLASSES, 10, 5, True)
        assert out.tobytes() == buf.tobytes() and lists[0, 0] == 0
    assert state[3] == 0 and state[1] == 40 and 8 < next_id <= 64


def test_one_call_of_three_frames_is_three_calls():
    f = frame((BOX, RED), (BOX2, RED))
    steps = [(f, [(BOX, 1, 1)], []), EMPTY, (f, [(BOX, 1, 2), (BOX2, 1, 3)], [])]
    state1, outs, evs = run(steps)
    tracked = np.stack([ref.pack(R, s[1], s[2]) for s in steps])
    state3, out, lists, _ = ref.update(ref.new_state(8), 8, np.stack([s[0] for s in steps]), tracked, 3, CLASSES, 25, 250, True)
    assert np.array_equal(state1, state3) and np.array_equal(out, np.stack(outs)) and ref.events(lists[2]) == evs[2]
    # n_frames = 2: the third frame is padding; n_frames = 0: nothing happens
    state2, out, lists, _ = ref.update(ref.new_state(8), 8, np.stack([s[0] for s in steps]), tracked, 2, CLASSES, 25, 250, True)
    assert state2[1] == 2 and np.array_equal(out[2], tracked[2]) and not lists[2].any()
    state0, out, lists, _ = ref.update(state1, 8, np.stack([s[0] for s in steps]), tracked, 0, CLASSES, 25, 250, True)
    assert np.array_equal(state0, state1) and np.array_equal(out, tracked) and not lists.any()
