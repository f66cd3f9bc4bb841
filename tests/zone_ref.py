"""Numpy restatement of the zone rule (DESIGN §8 "Zone rule"; include/ext/frcnn_hip_zone.h), the comparand of tests/test_zone_*.py.  It
follows the rule as written -- rows in row order finding or inserting their entry, the point tested against every polygon edge by edge,
enter and exit zone by zone, expiry with its lost events, the occupancy, the zone list, and a draw that blends the fills, paints the
outlines in ascending order and the labels over them -- with Python ints, not the kernels (csrc/zone.hip).  Integers throughout: a
sequence has one right answer.

A frame's tracked buffer is what tests/track_ref.py's ``Tracker.update`` returns (int32 [4 + 8 rows]), or a widened one;
``count_ref.make_tracked`` makes one by hand."""
import numpy as np

from faster_rcnn_amd import annotate_font
from tests import count_ref, track_ref, track_trails_ref

MAX_ZONES, MIN_VERTS, MAX_VERTS, MAX_EVENTS = 8, 3, 16, 64
COORD = (-32768, 65535)
WIDTH = (1, 9, 3)                                # smallest, largest, default W
MAX_EXPIRE = 4095
MAX_DWELL = 1 << 30
HEAD, ENTRY = 4 + 4 * MAX_ZONES, 5 + MAX_ZONES
LIST_HEAD = 4 + 5 * MAX_ZONES
LIST_WORDS = LIST_HEAD + 5 * MAX_EVENTS
EXIT, ENTER, LOST = 0, 1, 2
PALETTE = track_trails_ref.PALETTE
make_tracked = count_ref.make_tracked


def state_words(capacity):
    return HEAD + ENTRY * capacity


def inside(poly, p):
    """INSIDE: the half-open crossing-number rule, edge by edge."""
    px, py = int(p[0]), int(p[1])
    n, odd = len(poly), False
    for i in range(n):
        (xi, yi), (xj, yj) = poly[i], poly[(i + 1) % n]
        if (yi > py) != (yj > py):
            dy = yj - yi
            t = (px - xi) * dy - (py - yi) * (xj - xi)
            if (t < 0) if dy > 0 else (t > 0):
                odd = not odd
    return odd


def inside_mask(poly, h, w):
    """INSIDE for every pixel of an h x w frame at once: the same rule edge by edge, in int64 (every product is under 2^35)."""
    ys, xs = (a.astype(np.int64) for a in np.mgrid[0:h, 0:w])
    odd = np.zeros((h, w), dtype=bool)
    n = len(poly)
    for i in range(n):
        (xi, yi), (xj, yj) = poly[i], poly[(i + 1) % n]
        dy = yj - yi
        t = (xs - xi) * dy - (ys - yi) * (xj - xi)
        odd ^= ((yi > ys) != (yj > ys)) & ((t < 0) if dy > 0 else (t > 0))
    return odd


def point(box, h, w, anchor):
    """POINT of a raw box, or None when its clipped box is empty: the centre, or with ``anchor`` 1 the bottom centre."""
    c = track_ref.clip(box, h, w)
    if track_ref.empty(c):
        return None
    return (c[0] + c[1]) >> 1, (c[3] if anchor else (c[2] + c[3]) >> 1)


class Zones:
    """The state and steps 1-5.  ``entries``: dicts with id, cls, last_seen, inside, visited, since (a list of 8), in ascending id order."""

    def __init__(self, h, w, zones, classes, capacity=64, expire=9, anchor=0):
        zones = [[(int(x), int(y)) for x, y in zn] for zn in zones]
        assert 1 <= len(zones) <= MAX_ZONES and 1 <= capacity <= track_ref.MAX and 0 <= expire <= MAX_EXPIRE and anchor in (0, 1)
        for zn in zones:
            assert MIN_VERTS <= len(zn) <= MAX_VERTS and all(COORD[0] <= v <= COORD[1] for p in zn for v in p)
            assert all(zn[i] != zn[(i + 1) % len(zn)] for i in range(len(zn)))
        assert 1 <= h <= 32768 and 1 <= w <= 32768
        self.h, self.w, self.zones, self.classes, self.capacity, self.expire, self.anchor = h, w, zones, np.asarray(classes), capacity, expire, anchor
        self.entries, self.frames, self.dropped, self.events_dropped = [], 0, 0, 0
        self.visitors, self.stays, self.dwell, self.peak = ([0] * MAX_ZONES for _ in range(4))

    def words(self):
        """The state as the device holds it."""
        out = np.zeros(state_words(self.capacity), dtype=np.int64)
        out[:4] = (len(self.entries), self.frames, self.dropped, self.events_dropped)
        out[4:HEAD] = self.visitors + self.stays + self.dwell + self.peak
        for k, e in enumerate(self.entries):
            out[HEAD + ENTRY * k:HEAD + ENTRY * (k + 1)] = [e["id"], e["cls"], e["last_seen"], e["inside"], e["visited"]] + e["since"]
        return out.astype(np.int32)

    def _close(self, z, d):
        self.stays[z] += 1
        self.dwell[z] = min(self.dwell[z] + d, MAX_DWELL)

    def frame(self, buf):
        """One real frame's tracked buffer -> its zone list."""
        _, n_live, _, _, bbox, cls, _, ids, _ = track_ref.split(buf)
        self.frames += 1
        events = []
        for r in range(min(max(n_live, 0), len(ids))):
            rid = int(ids[r])
            if rid < 1:
                continue
            pt = point(bbox[r], self.h, self.w, self.anchor)
            c = int(cls[r])
            if pt is None or not 0 <= c < len(self.classes) or not self.classes[c]:
                continue
            entry = next((e for e in self.entries if e["id"] == rid), None)
            if entry is None:
                if len(self.entries) >= self.capacity:
                    self.dropped += 1
                    continue
                entry = {"id": rid, "cls": c, "last_seen": 0, "inside": 0, "visited": 0, "since": [0] * MAX_ZONES}
                self.entries.append(entry)
                self.entries.sort(key=lambda e: e["id"])
            m = sum(1 << z for z, zn in enumerate(self.zones) if inside(zn, pt))
            for z in range(len(self.zones)):
                now, was = m >> z & 1, entry["inside"] >> z & 1
                if now and not was:
                    entry["since"][z] = self.frames
                    if not entry["visited"] >> z & 1:
                        entry["visited"] |= 1 << z
                        self.visitors[z] += 1
                    events.append((z, ENTER, rid, entry["cls"], 0))
                elif was and not now:
                    d = self.frames - entry["since"][z]
                    self._close(z, d)
                    events.append((z, EXIT, rid, entry["cls"], d))
                    entry["since"][z] = 0
            entry["inside"], entry["last_seen"] = m, self.frames
        kept = []
        for e in self.entries:                                                   # (in ascending id order)
            if self.frames - e["last_seen"] <= self.expire:
                kept.append(e)
                continue
            for z in range(MAX_ZONES):
                if e["inside"] >> z & 1:
                    d = e["last_seen"] - e["since"][z] + 1
                    self._close(z, d)
                    events.append((z, LOST, e["id"], e["cls"], d))
        self.entries = kept
        occupancy = [sum(e["inside"] >> z & 1 for e in self.entries) for z in range(MAX_ZONES)]
        self.peak = [max(p, o) for p, o in zip(self.peak, occupancy)]
        self.events_dropped += max(len(events) - MAX_EVENTS, 0)
        return make_list(self.frames, occupancy, self.visitors, self.stays, self.dwell, self.peak, events[:MAX_EVENTS])

    def update(self, bufs, n_frames, gate=None):
        """A call over ``bufs`` (frames, words) with the device words ``n_frames`` and ``gate`` -> the workspace (frames, LIST_WORDS)."""
        bufs = np.asarray(bufs)
        nf = 0 if gate is not None and int(gate) == 0 else min(max(int(n_frames), 0), len(bufs))
        out = np.zeros((len(bufs), LIST_WORDS), dtype=np.int32)
        for f in range(nf):
            out[f] = self.frame(bufs[f])
        return out


def make_list(frames, occupancy=(), visitors=(), stays=(), dwell=(), peak=(), events=()):
    """A zone list from the frame count, the five figures of the first zones and [(zone, kind, id, cls, dwell)]."""
    out = np.zeros(LIST_WORDS, dtype=np.int64)
    out[0], out[1] = len(events), frames
    for k, vals in enumerate((occupancy, visitors, stays, dwell, peak)):
        out[4 + MAX_ZONES * k:4 + MAX_ZONES * k + len(vals)] = vals
    for k, ev in enumerate(events):
        out[LIST_HEAD + 5 * k:LIST_HEAD + 5 * k + 5] = ev
    return out.astype(np.int32)


def events_of(zlist):
    c = np.asarray(zlist)
    return [tuple(int(v) for v in c[LIST_HEAD + 5 * k:LIST_HEAD + 5 * k + 5]) for k in range(int(c[0]))]


def occupancy_of(zlist, n_zones=MAX_ZONES):
    return [int(v) for v in np.asarray(zlist)[4:4 + n_zones]]


def label_text(z, occupancy, visitors):
    """The label of zone z; a negative figure reads as 0."""
    return "Z%d %d/%d" % (z, max(int(occupancy), 0), max(int(visitors), 0))


def label_box(poly, text, h, w):
    """(x0, y0, bw, bh) of a label's cell box: anchored at the centre of the vertices' bounding box, on each axis shifted inside the
    frame when it fits."""
    xs, ys = [p[0] for p in poly], [p[1] for p in poly]
    return count_ref.label_box((min(xs), min(ys), max(xs), max(ys)), text, h, w)


def draw(frame, zlist, zones, width, rgb):
    """DRAW of a zone list into a copy of ``frame`` (h, w, 3) uint8.  EVERY pixel is tested against every occupied polygon, and every
    pixel of an edge's grown bounding box against the edge: the fill of the highest occupied zone a pixel is inside, then the outlines
    in ascending order, then the labels in ascending order, so the highest one that covers a pixel is the one that stays."""
    out = np.array(frame, dtype=np.uint8, copy=True)
    h, w = out.shape[:2]
    c = np.asarray(zlist)
    if int(c[1]) <= 0:
        return out
    zones = [[(int(x), int(y)) for x, y in zn] for zn in zones]
    colours = [PALETTE[z & 7] if rgb else PALETTE[z & 7][::-1] for z in range(len(zones))]
    top = np.full((h, w), -1)
    for z, zn in enumerate(zones):
        if int(c[4 + z]) > 0:
            top[inside_mask(zn, h, w)] = z
    for z in range(len(zones)):
        sel = top == z
        out[sel] = ((3 * out[sel].astype(np.int64) + np.asarray(colours[z], dtype=np.int64) + 2) >> 2).astype(np.uint8)
    for z, zn in enumerate(zones):
        for i in range(len(zn)):
            out[track_trails_ref.segment_mask(zn[i], zn[(i + 1) % len(zn)], h, w, width)] = colours[z]
    for z, zn in enumerate(zones):
        text = label_text(z, c[4 + z], c[4 + MAX_ZONES + z])
        x0, y0, bw, bh = label_box(zn, text, h, w)
        out[max(y0, 0):max(min(y0 + bh, h), 0), max(x0, 0):max(min(x0 + bw, w), 0)] = 0
        for k, ch in enumerate(text):
            rows = annotate_font.glyph(ch)
            for py in range(count_ref.CHAR_H):
                for px in range(count_ref.CHAR_W):
                    x, y = x0 + 1 + count_ref.ADVANCE * k + px, y0 + 1 + py
                    if 0 <= x < w and 0 <= y < h and (int(rows[py >> 1]) >> (4 - (px >> 1))) & 1:
                        out[y, x] = colours[z]
    return out


def summary_figures(totals, n_zones):
    """Per zone (visitors, peak, stays, mean dwell over the completed stays or None) from ``ops.zone_totals``' form."""
    return [(totals["visitors"][z], totals["peak"][z], totals["stays"][z],
             totals["dwell"][z] / totals["stays"][z] if totals["stays"][z] else None) for z in range(n_zones)]


# Answers written out by hand (tests/test_zone_cpu.py checks the restatement against them, tests/test_zone_gpu.py the kernel).  A case:
# name, (h, w), the zones, anchor, expire, the frames -- each the rows [(id, cls, box)] of its tracked buffer, a point (x, y) standing for
# one row of id 1, class 1, whose box is the point --, for each frame the events [(zone, kind, id, dwell)] it must give, and after the last
# frame (visitors, stays, dwell, peak) of the zones the case has.
# A is the square 10 <= x < 20, 10 <= y < 20 and B the square 20 <= x < 30 beside it: they share the edge x = 20.  The rule is half-open:
# a polygon owns its left and top boundary, not its right and bottom one.
A = [(10, 10), (20, 10), (20, 20), (10, 20)]
B = [(20, 10), (30, 10), (30, 20), (20, 20)]
C = [(0, 0), (30, 0), (30, 30), (20, 30), (20, 10), (10, 10), (10, 30), (0, 30)]           # a "U" upside down: the notch 10 <= x < 20, y >= 10 is outside
BOW = [(0, 0), (20, 20), (20, 0), (0, 20)]                                                 # a bow-tie crossing itself at (10, 10): left and right triangles
E, N, L = EXIT, ENTER, LOST
HAND_CASES = [
    ("a point on the shared edge belongs to exactly one zone", (32, 40), [A, B], 0, 9, [(20, 15)], [[(1, N, 1, 0)]], ([0, 1], [0, 0], [0, 0], [0, 1])),
    ("a point on the shared vertex belongs to exactly one zone", (32, 40), [A, B], 0, 9, [(20, 10)], [[(1, N, 1, 0)]], ([0, 1], [0, 0], [0, 0], [0, 1])),
    ("the bottom vertex of the shared edge belongs to neither", (32, 40), [A, B], 0, 9, [(20, 20)], [[]], ([0, 0], [0, 0], [0, 0], [0, 0])),
    ("touches the boundary and turns back: the left edge is inside", (32, 40), [A], 0, 9, [(5, 15), (10, 15), (5, 15)],
     [[], [(0, N, 1, 0)], [(0, E, 1, 1)]], ([1], [1], [1], [1])),
    ("touches the boundary and turns back: the right edge is outside", (32, 40), [A], 0, 9, [(25, 15), (20, 15), (25, 15)], [[], [], []],
     ([0], [0], [0], [0])),
    ("flaps in and out: three stays, one visitor", (32, 40), [A], 0, 9, [(5, 15), (15, 15), (5, 15), (15, 15), (15, 16), (5, 15), (12, 12), (5, 5)],
     [[], [(0, N, 1, 0)], [(0, E, 1, 1)], [(0, N, 1, 0)], [], [(0, E, 1, 2)], [(0, N, 1, 0)], [(0, E, 1, 1)]], ([1], [3], [4], [1])),
    ("first seen inside enters in that frame", (32, 40), [A], 0, 9, [(15, 15), (15, 15), (25, 15)], [[(0, N, 1, 0)], [], [(0, E, 1, 2)]],
     ([1], [1], [2], [1])),
    # seen in frames 1..3, inside from frame 2; E = 1: it leaves behind frame 5, and its stay is frames 2..3, last_seen - since + 1 = 2
    ("lost inside: the dwell runs to last_seen", (32, 40), [A], 0, 1, [(5, 15), (15, 15), (16, 15), [], []],
     [[], [(0, N, 1, 0)], [], [], [(0, L, 1, 2)]], ([1], [1], [2], [1])),
    ("a concave zone: the notch is outside", (32, 40), [C], 0, 9, [(5, 20), (15, 20), (15, 5), (25, 20), (15, 10), (15, 9)],
     [[(0, N, 1, 0)], [(0, E, 1, 1)], [(0, N, 1, 0)], [], [(0, E, 1, 2)], [(0, N, 1, 0)]], ([1], [2], [3], [1])),
    # (the crossing point itself is the right triangle's left corner: inside)
    ("a bow-tie: both triangles are inside, above and below the crossing is not", (32, 40), [BOW], 0, 9,
     [(3, 10), (10, 3), (17, 10), (10, 17), (10, 10), (9, 10)],
     [[(0, N, 1, 0)], [(0, E, 1, 1)], [(0, N, 1, 0)], [(0, E, 1, 1)], [(0, N, 1, 0)], []], ([1], [2], [2], [1])),
    ("a zone wholly beyond the frame is never entered", (20, 20), [[(30, 0), (60, 0), (60, 19), (30, 19)], [(-9, -9), (40, -9), (40, -1), (-9, -1)]], 0, 9,
     [(2, 2), (19, 19), (19, 0)], [[], [], []], ([0, 0], [0, 0], [0, 0], [0, 0])),
    ("one step enters one zone and leaves another: events in zone order", (32, 40), [A, B], 0, 9, [(25, 15), (15, 15), (25, 15)],
     [[(1, N, 1, 0)], [(0, N, 1, 0), (1, E, 1, 1)], [(0, E, 1, 1), (1, N, 1, 0)]], ([1, 1], [1, 1], [1, 1], [1, 1])),
    # the box 12..18 x 0..14: its centre (15, 7) is above A, its foot (15, 14) inside
    ("centre: a box whose centre is outside", (32, 40), [A], 0, 9, [[(1, 1, (12, 0, 18, 14))]], [[]], ([0], [0], [0], [0])),
    ("bottom: the same box stands inside", (32, 40), [A], 1, 9, [[(1, 1, (12, 0, 18, 14))]], [[(0, N, 1, 0)]], ([1], [0], [0], [1])),
    # (a foot on the frame's last row is row h - 1: the clipped box is inclusive)
    ("bottom: a box cut by the frame stands on the last row", (20, 40), [[(10, 19), (20, 19), (20, 25), (10, 25)]], 1, 9, [[(1, 1, (12, 5, 18, 40))]],
     [[(0, N, 1, 0)]], ([1], [0], [0], [1])),
    # two ids: 2 stays while 1 comes and goes, the peak is 2; E = 0: an absent id is lost at once, 1 with the dwell 1, 2 with 3 frames
    ("two ids, peak and lost in id order", (32, 40), [A, B], 0, 0,
     [[(2, 1, (15, 15, 15, 15))], [(2, 1, (16, 15, 16, 15)), (1, 3, (11, 11, 11, 11))], [(2, 1, (15, 15, 15, 15))], []],
     [[(0, N, 2, 0)], [(0, N, 1, 0)], [(0, L, 1, 1)], [(0, L, 2, 3)]], ([2, 0], [2, 0], [4, 0], [2, 0])),
    # the triangle above the diagonal y = x from corner to corner of the coordinate range: t = -98303 (px - py) on that edge, 6.4e9 at the
    # other one -- beyond 32 bits; a point ON the diagonal is inside, one pixel below it is not
    ("coordinates at the ends of the range", (32768, 32768), [[(-32768, -32768), (65535, -32768), (65535, 65535)]], 0, 9,
     [(32767, 0), (0, 32767), (100, 100), (100, 101), (101, 100)],
     [[(0, N, 1, 0)], [(0, E, 1, 1)], [(0, N, 1, 0)], [(0, E, 1, 1)], [(0, N, 1, 0)]], ([1], [2], [2], [1])),
]


def hand_rows(frame):
    """The rows of a hand case's frame: a point stands for one row of id 1, class 1, whose box is the point."""
    if isinstance(frame, tuple):
        x, y = frame
        return [(1, 1, (x, y, x, y))]
    return list(frame)


def hand_buffers(frames, R=2):
    """The tracked buffers of a hand case."""
    return np.stack([make_tracked(hand_rows(f), R) for f in frames])
