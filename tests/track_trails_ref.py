"""Numpy restatement of the trail rule (DESIGN §8 "Trail rule"; include/ext/frcnn_hip_track_trails.h), the comparand of
tests/test_track_trails_*.py.  It follows the rule as written -- rows in row order finding or inserting their entry, a list of points per
entry, expiry, the snapshot, and a capsule test per pixel and segment painted in ascending id order -- with Python ints, not the kernels
(csrc/track_trails.hip).  Integers throughout: a sequence has one right answer.

A frame's tracked buffer is what tests/track_ref.py's ``Tracker.update`` returns (int32 [4 + 8 rows]), or a widened one."""
import numpy as np

from tests import track_ref

LENGTH = (2, 64, 16)                             # smallest, largest, default N
WIDTH = (1, 9, 3)                                # smallest, largest, default W
MAX_EXPIRE = 4095
PALETTE = ((255, 64, 64), (64, 160, 255), (255, 208, 0), (255, 0, 255), (0, 224, 224), (255, 128, 0), (160, 96, 255), (255, 255, 255))


def list_words(capacity, length):
    return 4 + capacity * (4 + 2 * length)


def point(box, h, w):
    """The point of a raw box, or None when its clipped box is empty."""
    c = track_ref.clip(box, h, w)
    if track_ref.empty(c):
        return None
    return (c[0] + c[1]) >> 1, (c[2] + c[3]) >> 1


class Trails:
    """The state and steps 1-4.  ``entries``: dicts with id, cls, last_seen, pts (a list of (x, y), oldest first), in ascending id order."""

    def __init__(self, h, w, capacity=64, length=16, expire=9):
        assert 1 <= capacity <= track_ref.MAX and LENGTH[0] <= length <= LENGTH[1] and 0 <= expire <= MAX_EXPIRE
        assert 1 <= h <= 32768 and 1 <= w <= 32768
        self.h, self.w, self.capacity, self.length, self.expire = h, w, capacity, length, expire
        self.entries, self.frames, self.dropped = [], 0, 0

    def _words(self, entries, third, fourth):
        N = self.length
        out = np.zeros(list_words(self.capacity, N), dtype=np.int64)
        for k, e in enumerate(entries):
            at = 4 + k * (4 + 2 * N)
            out[at:at + 4] = (e["id"], e["cls"], third(e), fourth(e))
            for q, (x, y) in enumerate(e["pts"]):
                out[at + 4 + 2 * q], out[at + 5 + 2 * q] = x, y
        return out

    def words(self):
        """The state as the device holds it."""
        out = self._words(self.entries, lambda e: e["last_seen"], lambda e: len(e["pts"]))
        out[:3] = (len(self.entries), self.frames, self.dropped)
        return out.astype(np.int32)

    def frame(self, buf):
        """One real frame's tracked buffer -> its point list."""
        h, w = self.h, self.w
        _, n_live, _, _, bbox, cls, _, ids, _ = track_ref.split(buf)
        self.frames += 1
        for r in range(min(max(n_live, 0), len(ids))):
            rid, pt = int(ids[r]), point(bbox[r], h, w)
            if rid < 1 or pt is None:
                continue
            entry = next((e for e in self.entries if e["id"] == rid), None)
            if entry is None:
                if len(self.entries) >= self.capacity:
                    self.dropped += 1
                    continue
                entry = {"id": rid, "cls": int(cls[r]), "last_seen": self.frames, "pts": []}
                self.entries.append(entry)
                self.entries.sort(key=lambda e: e["id"])
            entry["pts"] = (entry["pts"] + [pt])[-self.length:]
            entry["last_seen"] = self.frames
        self.entries = [e for e in self.entries if self.frames - e["last_seen"] <= self.expire]
        shown = [e for e in self.entries if e["last_seen"] == self.frames]
        out = self._words(shown, lambda e: len(e["pts"]), lambda e: 0)
        out[0] = len(shown)
        return out.astype(np.int32)

    def update(self, bufs, n_frames, gate=None):
        """A call over ``bufs`` (frames, words) with the device words ``n_frames`` and ``gate`` -> the workspace (frames, list words)."""
        bufs = np.asarray(bufs)
        nf = 0 if gate is not None and int(gate) == 0 else min(max(int(n_frames), 0), len(bufs))
        out = np.zeros((len(bufs), list_words(self.capacity, self.length)), dtype=np.int32)
        for f in range(nf):
            out[f] = self.frame(bufs[f])
        return out


def trails_of(plist, length):
    """[(id, [(x, y), ...])] of a point list."""
    plist = np.asarray(plist)
    out = []
    for t in range(int(plist[0])):
        at = 4 + t * (4 + 2 * length)
        n = int(plist[at + 2])
        out.append((int(plist[at]), [(int(plist[at + 4 + 2 * q]), int(plist[at + 5 + 2 * q])) for q in range(n)]))
    return out


def covers(a, b, px, py, width):
    """Does segment (a, b) of width ``width`` cover pixel (px, py)?  Python ints: nothing overflows."""
    dx, dy = b[0] - a[0], b[1] - a[1]
    qx, qy = px - a[0], py - a[1]
    dd, u = dx * dx + dy * dy, qx * dx + qy * dy
    if dd == 0 or u <= 0:
        return qx * qx + qy * qy <= (width * width) >> 2
    if u >= dd:
        return (px - b[0]) ** 2 + (py - b[1]) ** 2 <= (width * width) >> 2
    return (qx * dy - qy * dx) ** 2 <= (width * width * dd) >> 2


def segment_mask(a, b, h, w, width):
    """The pixels of an h x w frame that segment (a, b) covers: every pixel of the segment's grown bounding box is tested."""
    mask = np.zeros((h, w), dtype=bool)
    g = (width + 1) >> 1
    for y in range(max(min(a[1], b[1]) - g, 0), min(max(a[1], b[1]) + g, h - 1) + 1):
        for x in range(max(min(a[0], b[0]) - g, 0), min(max(a[0], b[0]) + g, w - 1) + 1):
            mask[y, x] = covers(a, b, x, y, width)
    return mask


def draw(frame, plist, length, width, rgb):
    """DRAW of a point list into a copy of ``frame`` (h, w, 3) uint8: the trails painted in ascending id order, so the highest id that
    covers a pixel is the one that stays."""
    out = np.array(frame, dtype=np.uint8, copy=True)
    h, w = out.shape[:2]
    for tid, pts in sorted(trails_of(plist, length), key=lambda t: t[0]):
        colour = PALETTE[tid & 7] if rgb else PALETTE[tid & 7][::-1]
        for a, b in zip(pts[:-1], pts[1:]):
            out[segment_mask(a, b, h, w, width)] = colour
    return out


def draw_highest(frame, plist, length, width, rgb):
    """DRAW as the rule words it: per pixel, the colour of the highest id among the trails that cover it."""
    out = np.array(frame, dtype=np.uint8, copy=True)
    h, w = out.shape[:2]
    best = np.zeros((h, w), dtype=np.int64)
    for tid, pts in trails_of(plist, length):
        for a, b in zip(pts[:-1], pts[1:]):
            m = segment_mask(a, b, h, w, width)
            best[m] = np.maximum(best[m], tid)
    for y, x in zip(*np.nonzero(best)):
        c = PALETTE[int(best[y, x]) & 7]
        out[y, x] = c if rgb else c[::-1]
    return out


def make_list(trails, capacity, length):
    """A point list from [(id, cls, [(x, y), ...])], in the order given (the rule's lists are in ascending id order)."""
    out = np.zeros(list_words(capacity, length), dtype=np.int32)
    out[0] = len(trails)
    for t, (tid, cls, pts) in enumerate(trails):
        at = 4 + t * (4 + 2 * length)
        out[at:at + 3] = (tid, cls, len(pts))
        for q, (x, y) in enumerate(pts):
            out[at + 4 + 2 * q], out[at + 5 + 2 * q] = x, y
    return out
