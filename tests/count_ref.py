"""Numpy restatement of the count rule (DESIGN §8 "Count rule"; include/ext/frcnn_hip_count.h), the comparand of tests/test_count_*.py.
It follows the rule as written -- rows in row order finding or inserting their entry, the step tested against every line, a bit per line
and direction, expiry, the count list, and a draw that paints the lines in ascending order and the labels over them -- with Python ints,
not the kernels (csrc/count.hip).  Integers throughout: a sequence has one right answer.

A frame's tracked buffer is what tests/track_ref.py's ``Tracker.update`` returns (int32 [4 + 8 rows]), or a widened one."""
import numpy as np

from faster_rcnn_amd import annotate_font
from tests import track_ref, track_trails_ref

MAX_LINES, MAX_EVENTS = 8, 64
COORD = (-32768, 65535)
WIDTH = (1, 9, 3)                                # smallest, largest, default W
MAX_EXPIRE = 4095
HEAD, ENTRY = 4 + 2 * MAX_LINES, 6
LIST_WORDS = HEAD + 4 * MAX_EVENTS
PALETTE = track_trails_ref.PALETTE
CHAR_W, CHAR_H, ADVANCE, BOX_H = 10, 14, 12, 16  # a glyph at scale 2, the advance, a label's cell box


def state_words(capacity):
    return HEAD + ENTRY * capacity


def side(line, p):
    """sigma_l(P): is P on the non-negative side of the line (ax, ay, bx, by)?  A point on the line is."""
    ax, ay, bx, by = (int(v) for v in line)
    return (bx - ax) * (int(p[1]) - ay) - (by - ay) * (int(p[0]) - ax) >= 0


def crossing(line, p, q):
    """CROSSING of ``line`` by the step p -> q: None, or the direction (1: pos, 0: neg)."""
    if side(line, p) == side(line, q):
        return None
    carrier = (int(p[0]), int(p[1]), int(q[0]), int(q[1]))
    if side(carrier, line[0:2]) == side(carrier, line[2:4]):
        return None
    return 1 if side(line, q) else 0


class Counter:
    """The state and steps 1-4.  ``entries``: dicts with id, cls, last_seen, counted, pt, in ascending id order; ``totals[l]`` = [neg, pos]."""

    def __init__(self, h, w, lines, classes, capacity=64, expire=9):
        lines = [tuple(int(v) for v in ln) for ln in lines]
        assert 1 <= len(lines) <= MAX_LINES and 1 <= capacity <= track_ref.MAX and 0 <= expire <= MAX_EXPIRE
        assert all(len(ln) == 4 and ln[:2] != ln[2:] and all(COORD[0] <= v <= COORD[1] for v in ln) for ln in lines)
        assert 1 <= h <= 32768 and 1 <= w <= 32768
        self.h, self.w, self.lines, self.classes, self.capacity, self.expire = h, w, lines, np.asarray(classes), capacity, expire
        self.entries, self.frames, self.dropped, self.events_dropped = [], 0, 0, 0
        self.totals = [[0, 0] for _ in range(MAX_LINES)]

    def words(self):
        """The state as the device holds it."""
        out = np.zeros(state_words(self.capacity), dtype=np.int64)
        out[:4] = (len(self.entries), self.frames, self.dropped, self.events_dropped)
        out[4:HEAD] = np.asarray(self.totals).reshape(-1)
        for k, e in enumerate(self.entries):
            out[HEAD + ENTRY * k:HEAD + ENTRY * (k + 1)] = (e["id"], e["cls"], e["last_seen"], e["counted"], e["pt"][0], e["pt"][1])
        return out.astype(np.int32)

    def load(self, words):
        """Continue from a state as the device holds it."""
        s = np.asarray(words).astype(np.int64)
        self.frames, self.dropped, self.events_dropped = int(s[1]), int(s[2]), int(s[3])
        self.totals = [[int(s[4 + 2 * l]), int(s[5 + 2 * l])] for l in range(MAX_LINES)]
        self.entries = []
        for k in range(int(s[0])):
            e = s[HEAD + ENTRY * k:HEAD + ENTRY * (k + 1)]
            self.entries.append({"id": int(e[0]), "cls": int(e[1]), "last_seen": int(e[2]), "counted": int(e[3]), "pt": (int(e[4]), int(e[5]))})
        return self

    def frame(self, buf):
        """One real frame's tracked buffer -> its count list."""
        _, n_live, _, _, bbox, cls, _, ids, _ = track_ref.split(buf)
        self.frames += 1
        events = []
        for r in range(min(max(n_live, 0), len(ids))):
            rid = int(ids[r])
            if rid < 1:
                continue
            pt = track_trails_ref.point(bbox[r], self.h, self.w)
            c = int(cls[r])
            if pt is None or not 0 <= c < len(self.classes) or not self.classes[c]:
                continue
            entry = next((e for e in self.entries if e["id"] == rid), None)
            if entry is None:
                if len(self.entries) >= self.capacity:
                    self.dropped += 1
                    continue
                self.entries.append({"id": rid, "cls": c, "last_seen": self.frames, "counted": 0, "pt": pt})
                self.entries.sort(key=lambda e: e["id"])
                continue
            for l, line in enumerate(self.lines):
                d = crossing(line, entry["pt"], pt)
                if d is not None and not entry["counted"] >> (2 * l + d) & 1:
                    entry["counted"] |= 1 << (2 * l + d)
                    self.totals[l][d] += 1
                    events.append((l, d, rid, entry["cls"]))
            entry["pt"], entry["last_seen"] = pt, self.frames
        self.entries = [e for e in self.entries if self.frames - e["last_seen"] <= self.expire]
        self.events_dropped += max(len(events) - MAX_EVENTS, 0)
        return make_list(self.frames, self.totals, events[:MAX_EVENTS])

    def update(self, bufs, n_frames, gate=None):
        """A call over ``bufs`` (frames, words) with the device words ``n_frames`` and ``gate`` -> the workspace (frames, LIST_WORDS)."""
        bufs = np.asarray(bufs)
        nf = 0 if gate is not None and int(gate) == 0 else min(max(int(n_frames), 0), len(bufs))
        out = np.zeros((len(bufs), LIST_WORDS), dtype=np.int32)
        for f in range(nf):
            out[f] = self.frame(bufs[f])
        return out


def make_list(frames, totals, events=()):
    """A count list from the frame count, totals[l] = (neg, pos) for the first lines and [(l, dir, id, cls)]."""
    out = np.zeros(LIST_WORDS, dtype=np.int64)
    out[0], out[1] = len(events), frames
    for l, t in enumerate(totals):
        out[4 + 2 * l], out[5 + 2 * l] = t
    for k, ev in enumerate(events):
        out[HEAD + 4 * k:HEAD + 4 * k + 4] = ev
    return out.astype(np.int32)


def events_of(clist):
    c = np.asarray(clist)
    return [tuple(int(v) for v in c[HEAD + 4 * k:HEAD + 4 * k + 4]) for k in range(int(c[0]))]


def make_tracked(rows, R, n_live=None, fill=0):
    """A tracked buffer of ``R`` rows from [(id, cls, (x1, y1, x2, y2))]; the words of the rows behind them are ``fill``."""
    buf = np.full(4 + 8 * R, fill, dtype=np.int64)
    buf[:4] = (len(rows), len(rows) if n_live is None else n_live, 0, 0)
    for r, (rid, c, box) in enumerate(rows):
        buf[4 + 4 * r:8 + 4 * r] = box
        buf[4 + 4 * R + r], buf[4 + 6 * R + r] = c, rid
    return buf.astype(np.int32)


def label_text(l, totals):
    """The label of line l with totals (neg, pos); a negative total reads as 0."""
    return "L%d +%d -%d" % (l, max(int(totals[1]), 0), max(int(totals[0]), 0))


def label_box(line, text, h, w):
    """(x0, y0, bw, bh) of a label's cell box: anchored at the line's midpoint, on each axis shifted inside the frame when it fits."""
    bw, bh = ADVANCE * len(text), BOX_H
    mx, my = (int(line[0]) + int(line[2])) >> 1, (int(line[1]) + int(line[3])) >> 1
    x0 = min(max(mx, 0), w - bw) if bw <= w else mx
    y0 = min(max(my, 0), h - bh) if bh <= h else my
    return x0, y0, bw, bh


def line_mask(line, h, w, width):
    """The pixels of an h x w frame that the line covers: EVERY pixel is tested with the trail rule's inequalities (a line may be far
    longer than the frame; the frames of the tests are small)."""
    a, b = (int(line[0]), int(line[1])), (int(line[2]), int(line[3]))
    mask = np.zeros((h, w), dtype=bool)
    for y in range(h):
        for x in range(w):
            mask[y, x] = track_trails_ref.covers(a, b, x, y, width)
    return mask


def draw(frame, clist, lines, width, rgb):
    """DRAW of a count list into a copy of ``frame`` (h, w, 3) uint8: the lines painted in ascending order, then the labels in ascending
    order, so the highest one that covers a pixel is the one that stays."""
    out = np.array(frame, dtype=np.uint8, copy=True)
    h, w = out.shape[:2]
    c = np.asarray(clist)
    if int(c[1]) <= 0:
        return out
    colours = [PALETTE[l & 7] if rgb else PALETTE[l & 7][::-1] for l in range(len(lines))]
    for l, line in enumerate(lines):
        out[line_mask(line, h, w, width)] = colours[l]
    for l, line in enumerate(lines):
        text = label_text(l, (c[4 + 2 * l], c[5 + 2 * l]))
        x0, y0, bw, bh = label_box(line, text, h, w)
        for y in range(max(y0, 0), min(y0 + bh, h)):
            for x in range(max(x0, 0), min(x0 + bw, w)):
                out[y, x] = 0
        for k, ch in enumerate(text):
            rows = annotate_font.glyph(ch)
            for py in range(CHAR_H):
                for px in range(CHAR_W):
                    x, y = x0 + 1 + ADVANCE * k + px, y0 + 1 + py
                    if 0 <= x < w and 0 <= y < h and (int(rows[py >> 1]) >> (4 - (px >> 1))) & 1:
                        out[y, x] = colours[l]
    return out


# Answers written out by hand (tests/test_count_cpu.py checks the restatement against them, tests/test_count_gpu.py the kernel): name,
# (h, w), the lines, the points one id takes frame by frame, and for each frame the crossings [(line, dir)] it must give.
# V is the line x = 10 from (10, 0) down to (10, 20): s(P) = -20 (px - 10), so the non-negative side is px <= 10, ON the line included.
V = (10, 0, 10, 20)
HAND_CASES = [
    ("ends on the line, then continues", (24, 32), [V], [(5, 10), (10, 10), (15, 10)], [[], [], [(0, 0)]]),
    ("ends on the line, then turns back", (24, 32), [V], [(5, 10), (10, 10), (5, 10)], [[], [], []]),
    ("starts on the line, leaves to the negative side", (24, 32), [V], [(10, 10), (15, 10)], [[], [(0, 0)]]),
    ("starts on the line, stays on its side", (24, 32), [V], [(10, 10), (5, 10)], [[], []]),
    ("reaches the line from the negative side", (24, 32), [V], [(15, 10), (10, 10), (15, 10)], [[], [(0, 1)], [(0, 0)]]),
    # two abutting lines share (10, 10); the step's carrier puts that endpoint on its non-negative side, so exactly one of them counts
    ("through the shared endpoint, left to right", (24, 32), [(10, 0, 10, 10), (10, 10, 10, 20)], [(5, 10), (15, 10)], [[], [(0, 0)]]),
    ("through the shared endpoint, right to left", (24, 32), [(10, 0, 10, 10), (10, 10, 10, 20)], [(15, 10), (5, 10)], [[], [(1, 1)]]),
    ("through endpoint B of a single line", (24, 32), [(10, 0, 10, 10)], [(5, 10), (15, 10)], [[], [(0, 0)]]),
    ("through endpoint A of a single line", (24, 32), [(10, 10, 10, 20)], [(5, 10), (15, 10)], [[], []]),
    ("collinear with the line", (24, 32), [V], [(10, 5), (10, 15), (10, 2)], [[], [], []]),
    ("passes beyond B", (40, 32), [V], [(5, 25), (15, 25)], [[], []]),
    ("P = Q", (24, 32), [V], [(5, 5), (5, 5)], [[], []]),
    # the second line runs upwards: its non-negative side is px >= 20
    ("one step crosses two lines", (24, 32), [V, (20, 20, 20, 0)], [(5, 10), (25, 10)], [[], [(0, 0), (1, 1)]]),
    ("re-crossing in both directions counts once each", (24, 32), [V], [(5, 10), (15, 10), (5, 12), (15, 9), (5, 10)],
     [[], [(0, 0)], [(0, 1)], [], []]),
    ("a line wholly outside the frame", (20, 20), [(30, 0, 30, 19), (-9, -5, 40, -5)], [(2, 2), (19, 19), (0, 19)], [[], [], []]),
    # y = x from corner to corner of the coordinate range: s(P) = 98303 (py - px), 3.2e9 at the frame's corners -- beyond 32 bits
    ("coordinates at the ends of the range", (32768, 32768), [(-32768, -32768, 65535, 65535)], [(32767, 0), (0, 32767), (32767, 1)],
     [[], [(0, 1)], [(0, 0)]]),
]


def hand_buffers(points, R=1, rid=1, cls=1):
    """The tracked buffers of a hand case: one live row per frame, its box the point itself."""
    return np.stack([make_tracked([(rid, cls, (x, y, x, y))], R) for x, y in points])
