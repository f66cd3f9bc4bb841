"""Plain-numpy restatement of the motion rule (DESIGN §8 "Motion rule"; include/ext/frcnn_hip_track_motion.h) on top of tests/track_ref.py,
the comparand of tests/test_track_motion_*.py.  It follows the rule as written -- luma, sample grid, every candidate's cost, the
lexicographic minimum, the gate -- not the kernel (csrc/track_motion.hip).  Integers throughout: a sequence has one right answer.

Frames are (h, w, 3) uint8 arrays in any channel order; boxes given to ``search`` are clipped ones, (xa, xb, ya, yb)."""
import numpy as np

from tests import track_ref as T

RADIUS = (1, 16, 8)                              # smallest, largest, the default
GRID, MIN_SAMPLES = 32, 16


def luma(frame):
    f = np.asarray(frame).astype(np.int64)
    return (f[..., 0] + 2 * f[..., 1] + f[..., 2] + 2) >> 2


def samples(a, b):
    """The sample positions along one axis of a clipped box side [a, b]."""
    s = (b - a + 1 + GRID - 1) // GRID
    return np.arange(a + s // 2, b + 1, s)


def costs(prev, cur, box, radius):
    """-> ({(dx, dy): cost}, n) of a clipped box that is not empty."""
    xa, xb, ya, yb = box
    h, w = prev.shape[:2]
    xs, ys = samples(xa, xb), samples(ya, yb)
    lp, lc = luma(prev), luma(cur)
    t = lp[np.ix_(ys, xs)]
    out = {}
    dxs = np.arange(-radius, radius + 1)
    xx = np.clip(xs[None, :] + dxs[:, None], 0, w - 1)                    # (candidates, columns)
    for dy in range(-radius, radius + 1):
        yy = np.clip(ys + dy, 0, h - 1)
        row = np.abs(lc[yy][:, xx] - t[:, None, :]).sum(axis=(0, 2))       # (rows, candidates, columns) -> one cost per dx
        for dx, c in zip(dxs.tolist(), row.tolist()):
            out[(dx, dy)] = int(c)
    return out, len(xs) * len(ys)


def choose(cost, n):
    """The best candidate of a cost table and the gate -> (dx, dy, cost_best, cost_zero, n); (0, 0, ...) when the gate refuses."""
    best = min(cost, key=lambda d: (cost[d], d[0] * d[0] + d[1] * d[1], d[1], d[0]))
    if cost[best] + n <= cost[(0, 0)]:
        return best[0], best[1], cost[best], cost[(0, 0)], n
    return 0, 0, cost[best], cost[(0, 0)], n


def search(prev, cur, box, radius=RADIUS[2]):
    """The move of one clipped box (xa, xb, ya, yb) from ``prev`` to ``cur`` -> (dx, dy, cost_best, cost_zero, n).  (0, 0, 0, 0, n) for a
    box that is skipped: empty, or fewer than 16 samples."""
    assert RADIUS[0] <= radius <= RADIUS[1] and prev.shape == cur.shape
    if T.empty(box):
        return 0, 0, 0, 0, 0
    n = len(samples(box[0], box[1])) * len(samples(box[2], box[3]))
    if n < MIN_SAMPLES:
        return 0, 0, 0, 0, n
    return choose(*costs(prev, cur, box, radius))


class MotionTracker:
    """track_ref.Tracker plus the motion state: ``kept`` (the header's count), ``size`` (h, w) and the kept ``frame``; all None / 0 in a
    fresh or reset one."""

    def __init__(self, capacity=64):
        self.t = T.Tracker(capacity)
        self.kept, self.size, self.frame = 0, (0, 0), None
        self.moves = []                                       # (id, dx, dy) of every move taken (for the tests' own checks)

    def reset_motion(self):
        self.kept, self.size = 0, (0, 0)                      # (the kept frame's bytes stay, as on the device)

    def header(self):
        return np.array([self.kept, self.size[0], self.size[1], 0], dtype=np.int32)

    def motion_bytes(self, h, w):
        """The motion state as the device holds it, for a state made for (h, w) frames: uint8 [16 + 3hw]."""
        body = np.zeros(3 * h * w, dtype=np.uint8) if self.frame is None else self.frame.reshape(-1)
        assert body.size == 3 * h * w
        return np.concatenate([self.header().view(np.uint8), body])

    def update_call(self, frames, packed, n_frames, table, h, w, thr=30, hold=8, grow=0, radius=RADIUS[2]):
        """One call: ``frames`` a list of B frames, ``packed`` of B det_packed buffers -> the B tracked buffers."""
        nf = min(max(int(n_frames), 0), len(frames))
        rows = (np.asarray(packed[0]).size - 4) // 7
        prev = None
        if self.kept >= 1 and self.kept == self.t.frames and self.size == (h, w):
            prev = self.frame
        out = []
        for f in range(len(frames)):
            if f >= nf:
                out.append(self.t.padding(rows))
                continue
            cur = np.asarray(frames[f])
            assert cur.shape == (h, w, 3) and cur.dtype == np.uint8
            if prev is not None:
                for s in self.t.slots:
                    dx, dy = search(prev, cur, T.clip(s["bbox"], h, w), radius)[:2]
                    if dx or dy:
                        x1, y1, x2, y2 = s["bbox"]
                        s["bbox"] = [x1 + dx, y1 + dy, x2 + dx, y2 + dy]
                        self.moves.append((s["id"], dx, dy))
            out.append(self.t.update_packed(packed[f], table, h, w, thr, hold, grow))
            prev = cur
        if nf >= 1:
            self.frame, self.kept, self.size = np.array(frames[nf - 1], dtype=np.uint8), self.t.frames, (h, w)
        return out

    def track_dets(self, frame, dets, class_mapping, classes, thr=30, hold=8, grow=0, radius=RADIUS[2]):
        """track_ref.track_dets with the motion step: one frame and its host dets -> (live, held)."""
        h, w = frame.shape[:2]
        prev = self.frame if self.kept >= 1 and self.kept == self.t.frames and self.size == (h, w) else None
        if prev is not None:
            for s in self.t.slots:
                dx, dy = search(prev, frame, T.clip(s["bbox"], h, w), radius)[:2]
                if dx or dy:
                    x1, y1, x2, y2 = s["bbox"]
                    s["bbox"] = [x1 + dx, y1 + dy, x2 + dx, y2 + dy]
                    self.moves.append((s["id"], dx, dy))
        res = T.track_dets(self.t, dets, class_mapping, classes, h, w, thr, hold, grow)
        self.frame, self.kept, self.size = np.array(frame, dtype=np.uint8), self.t.frames, (h, w)
        return res


def shifted(frame, dx, dy):
    """``frame`` moved by (dx, dy) with edge replication: out[y][x] = frame[clamp(y - dy)][clamp(x - dx)]."""
    h, w = frame.shape[:2]
    return frame[np.clip(np.arange(h) - dy, 0, h - 1)][:, np.clip(np.arange(w) - dx, 0, w - 1)]
