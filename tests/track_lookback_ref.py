"""Plain-numpy restatement of the look-back rule (DESIGN §8 "Look-back rule"; include/ext/frcnn_hip_track_lookback.h) on top of
tests/track_ref.py and tests/track_motion_ref.py, the comparand of tests/test_track_lookback_*.py.  It follows the rule as written -- the
births of a call in ascending id order, each walked back frame by frame, its row appended to the frame it reaches -- not the kernels
(csrc/track_lookback.hip), which give every row its place up front.  Integers throughout: a sequence has one right answer.

The window is kept as the device keeps it (header, two halves of cells), so that ``Window.state_bytes`` can be compared byte for byte."""
import numpy as np

from tests import track_motion_ref as M
from tests import track_ref as T

LOOKBACK = (1, 16, 8)                            # smallest, largest, the default
HEADER = 32                                      # bytes in front of the cells


def widen(buf, R2):
    """A tracked buffer of R rows -> the same with R2 >= R rows; the new rows are rows behind n_rows."""
    buf = np.asarray(buf, dtype=np.int32)
    R = (buf.size - 4) // 8
    assert buf.size == 4 + 8 * R and R2 >= R
    out = np.zeros(4 + 8 * R2, dtype=np.int32)
    out[:4] = buf[:4]
    out[4:4 + 4 * R2] = -1
    out[4:4 + 4 * R] = buf[4:4 + 4 * R]
    out[4 + 4 * R2:4 + 5 * R2] = -1
    for part in range(4):
        out[4 + (4 + part) * R2:4 + (4 + part) * R2 + R] = buf[4 + (4 + part) * R:4 + (5 + part) * R]
    return out


def births(buf, first_id, capacity):
    """The rows of a (widened) tracked buffer that are births, given the next_id word of the buffer in front: live rows with id >=
    first_id, in row order (at most ``capacity``: the tracker makes no more)."""
    _, n_live, _, _, _, _, _, ids, _ = T.split(buf)
    return [r for r in range(n_live) if int(ids[r]) >= first_id][:capacity]


def step_back(prev, cur, box, radius):
    """One chain step: the raw ``box`` in frame ``prev`` (= g + 1) -> the raw box in frame ``cur`` (= g)."""
    h, w = prev.shape[:2]
    if radius == 0:
        return list(box)
    dx, dy = M.search(prev, cur, T.clip(box, h, w), radius)[:2]
    return [box[0] + dx, box[1] + dy, box[2] + dx, box[3] + dy]


def backfilled_box(box, h, w, e):
    c = T.clip(box, h, w)
    return (-1, -1, -1, -1) if T.empty(c) else (c[0] - e, c[2] - e, c[1] + e, c[3] + e)


class Window:
    """The window and the rule.  ``count``, ``half``, ``back_overflow``: the header's words; ``bufs`` (2, frames, 4 + 8 R2) int32 and
    ``pix`` (2, frames, padded frame bytes) uint8: the cells of the two halves."""

    def __init__(self, frames, h, w, max_rows, capacity, back):
        assert 1 <= frames <= 64 and 1 <= capacity <= T.MAX and 1 <= back <= 128 and max_rows >= 1
        self.B, self.h, self.w, self.capacity = frames, h, w, capacity
        self.R = max_rows + capacity
        self.R2 = self.R + back
        assert self.R2 <= 512
        self.count = self.half = self.back_overflow = 0
        self.bufs = np.zeros((2, frames, 4 + 8 * self.R2), dtype=np.int32)
        self.pix = np.zeros((2, frames, (3 * h * w + 15) // 16 * 16), dtype=np.uint8)

    def reset(self):
        self.count = self.half = self.back_overflow = 0          # (the cells stay, as on the device)

    def state_bytes(self):
        head = np.array([self.count, self.half, self.back_overflow, 0, 0, 0, 0, 0], dtype=np.int32).view(np.uint8)
        cells = [np.concatenate([self.bufs[s, i].view(np.uint8), self.pix[s, i]]) for s in range(2) for i in range(self.B)]
        return np.concatenate([head] + cells)

    def frame(self, cell):
        return self.pix[cell][:3 * self.h * self.w].reshape(self.h, self.w, 3)

    def _append(self, cell, box, cls, prob, tid, age):
        buf = self.bufs[cell]
        n, R2 = int(buf[0]), self.R2
        if n >= R2:                                               # (ascending ids: the row dropped is the highest)
            self.back_overflow += 1
            return
        buf[4 + 4 * n:8 + 4 * n] = box
        buf[4 + 4 * R2 + n], buf[4 + 5 * R2 + n], buf[4 + 6 * R2 + n], buf[4 + 7 * R2 + n] = cls, prob, tid, age
        buf[0] = n + 1

    def call(self, frames, tracked, n_frames, lookback=LOOKBACK[2], radius=0, grow=0):
        """One call: ``frames`` B frames (h, w, 3), ``tracked`` their B tracked buffers of R rows -> (the emitted frames, the emitted
        widened buffers), oldest first: what the window held before the call."""
        assert len(frames) == self.B and len(tracked) == self.B and LOOKBACK[0] <= lookback <= LOOKBACK[1] and 0 <= radius <= 16
        n_frames = int(n_frames)
        nf, c, half = min(max(n_frames, 0), self.B), self.count, self.half
        seq = [(half, i) for i in range(c)] + [(half ^ 1, f) for f in range(nf)]
        for f in range(nf):                                       # 1 join
            assert frames[f].shape == (self.h, self.w, 3) and frames[f].dtype == np.uint8
            self.bufs[half ^ 1, f] = widen(tracked[f], self.R2)
            self.pix[half ^ 1, f, :3 * self.h * self.w] = np.asarray(frames[f]).reshape(-1)
        for t in range(max(c, 1), c + nf):                        # 2 chain: the births of the call's frames, in id order
            bt = self.bufs[seq[t]]
            first_id = int(self.bufs[seq[t - 1]][2])
            _, _, _, _, t_box, t_cls, t_prob, t_id, _ = T.split(bt)
            for r in births(bt, first_id, self.capacity):
                box = [int(v) for v in t_box[r]]
                for k in range(1, lookback + 1):
                    g = t - k
                    if g < 0:
                        break
                    box = step_back(self.frame(seq[g + 1]), self.frame(seq[g]), box, radius)
                    self._append(seq[g], backfilled_box(box, self.h, self.w, grow * k), int(t_cls[r]), int(t_prob[r]), int(t_id[r]), -k)
        out = ([self.frame((half, i)).copy() for i in range(c)], [self.bufs[half, i].copy() for i in range(c)])      # 3 emit
        if n_frames < 0:                                          # 4 close
            self.count = 0
        elif n_frames > 0:
            self.count, self.half = nf, half ^ 1
        return out


# ----------------------------------------------------------------------------------------------------------- test material
def packed(dets, rows):
    """A det_packed buffer of ``rows`` rows from [(x1, y1, x2, y2, cls, prob)]: int32 [4 + 7 rows]."""
    assert len(dets) <= rows
    p = np.zeros(4 + 7 * rows, dtype=np.int32)
    p[0] = len(dets)
    for r, (x1, y1, x2, y2, cls, prob) in enumerate(dets):
        p[4 + 4 * r:8 + 4 * r] = (x1, y1, x2, y2)
        p[4 + 4 * rows + r] = cls
        p[4 + 5 * rows + r] = T.bits(prob)
    return p


def texture(h, w, seed):
    """A fixed pseudo-random (h, w, 3) uint8 frame."""
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def paste(frame, patch, x, y):
    """``frame`` with ``patch`` at (x, y), clipped to the frame."""
    out = frame.copy()
    h, w = frame.shape[:2]
    ph, pw = patch.shape[:2]
    xa, ya, xb, yb = max(x, 0), max(y, 0), min(x + pw, w), min(y + ph, h)
    if xa < xb and ya < yb:
        out[ya:yb, xa:xb] = patch[ya - y:yb - y, xa - x:xb - x]
    return out


def sequence(h, w, n, seed, rows, capacity, objects=2, hold=2, grow=1, detected=None):
    """A seeded sequence: ``objects`` textured rectangles moving over a fixed texture, each "detected" (class 1) in the frames where
    ``detected(obj, frame)`` says so (default: seeded drop-outs) -> (frames, packed buffers, tracked buffers of track_ref.Tracker).
    ``objects`` may also list the rectangles as (x, y, width, height, vx, vy)."""
    rng = np.random.RandomState(seed)
    back = texture(h, w, seed + 1000)
    objs = []
    for o in range(objects) if isinstance(objects, int) else []:
        bw, bh = int(rng.randint(8, 20)), int(rng.randint(8, 20))
        objs.append((texture(bh, bw, seed + 2000 + o), int(rng.randint(0, max(w - bw, 1))), int(rng.randint(0, max(h - bh, 1))),
                     int(rng.randint(-3, 4)), int(rng.randint(-2, 3)), rng.rand(n) < 0.6))
    for o, (x, y, bw, bh, vx, vy) in enumerate(() if isinstance(objects, int) else objects):
        objs.append((texture(bh, bw, seed + 2000 + o), x, y, vx, vy, rng.rand(n) < 0.6))
    table = np.array([0, 1, 1], dtype=np.uint8)
    tracker = T.Tracker(capacity)
    frames, packs, tracked = [], [], []
    for t in range(n):
        frame, dets = back, []
        for o, (patch, x, y, vx, vy, seen) in enumerate(objs):
            px, py = x + vx * t, y + vy * t
            frame = paste(frame, patch, px, py)
            if detected(o, t) if detected is not None else bool(seen[t]):
                dets.append((px, py, px + patch.shape[1] - 1, py + patch.shape[0] - 1, 1 + o % 2, 0.5 + 0.01 * o))
        frames.append(frame)
        packs.append(packed(dets[:rows], rows))
        tracked.append(tracker.update_packed(packs[-1], table, h, w, 30, hold, grow))
    return frames, packs, tracked


def run(window, frames, tracked, sizes, lookback, radius=0, grow=0, flush=True):
    """A whole sequence cut into calls of ``sizes`` real frames (each padded to the window's B) -> every emitted (frame, buffer), in
    order; with ``flush`` the last call is followed by a flush."""
    B, out_f, out_t, at = window.B, [], [], 0
    blank_f = np.zeros((window.h, window.w, 3), dtype=np.uint8)
    blank_t = np.zeros(4 + 8 * window.R, dtype=np.int32)
    for n in list(sizes) + ([-1] if flush else []):
        real = max(n, 0)
        fs = list(frames[at:at + real]) + [blank_f] * (B - real)
        ts = list(tracked[at:at + real]) + [blank_t] * (B - real)
        ef, et = window.call(fs, ts, n, lookback, radius, grow)
        out_f += ef
        out_t += et
        at += real
    return out_f, out_t


# ----------------------------------------------------------------------------------------------------------- host dets
def backfill_dets(frames, per_frame, lookback, radius=0, grow=0):
    """The rule over a whole sequence's host dets, as one uncut call sequence sees it (every call full, lookback <= B: the partition does
    not matter): ``per_frame`` = the (live, held) det lists of a tracking run WITHOUT look-back, frame by frame -> per frame, the
    back-filled rows as dets {"bbox", "cls_name", "prob", "track_id", "backfilled": k}, in ascending id order."""
    h, w = frames[0].shape[:2]
    out = [[] for _ in frames]
    next_id = 1                                                  # the tracker's next_id in front of frame t: ids are issued in order
    for t, (live, held) in enumerate(per_frame):
        for d in live if t > 0 else []:
            if d.get("track_id", 0) < next_id:
                continue
            box = [int(v) for v in d["bbox"]]
            for k in range(1, lookback + 1):
                g = t - k
                if g < 0:
                    break
                box = step_back(frames[g + 1], frames[g], box, radius)
                out[g].append({"bbox": np.array(backfilled_box(box, h, w, grow * k), dtype=np.int64), "cls_name": d["cls_name"],
                               "prob": d["prob"], "track_id": d["track_id"], "backfilled": k})
        next_id = max([next_id] + [d.get("track_id", 0) + 1 for d in list(live) + list(held)])
    return out
