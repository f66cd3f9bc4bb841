"""Plain-numpy restatement of the back-track rule (DESIGN §8 "Back-track rule"; include/ext/frcnn_hip_track_backtrack.h) on top of
tests/track_lookback_ref.py, tests/track_interval_ref.py, tests/track_motion_ref.py and tests/track_ref.py, the comparand of
tests/test_track_backtrack_*.py.  It follows the rule as written -- the key frames of a call in order, the sources of each in row order,
each walked back frame by frame, its row appended to the frame it reaches -- not the kernels (csrc/track_backtrack.hip), which give every
row its place up front.  Integers throughout: a sequence has one right answer."""
import numpy as np

from tests import track_interval_ref as I
from tests import track_lookback_ref as L
from tests import track_ref as T

HEADER = L.HEADER
MOVE = (3, -2)                                   # the test material's motion per frame, (dx, dy)


def sources(buf, first_id, capacity):
    """The rows of a key frame's (widened) tracked buffer that are sources, given the next_id word of the buffer in front: live rows with
    id >= 1, the first ``capacity`` in row order, each with whether it is a birth (id >= first_id) -> [(row, birth)]."""
    _, n_live, _, _, _, _, _, ids, _ = T.split(buf)
    return [(r, int(ids[r]) >= first_id) for r in range(n_live) if int(ids[r]) >= 1][:capacity]


class Window(L.Window):
    """track_lookback_ref.Window -- the same window, join, emit and close -- with the back-track rule's chain."""

    def call(self, frames, tracked, n_frames, lookback, radius=0, grow=0, interval=1):
        """One call: ``frames`` F frames (h, w, 3), ``tracked`` their F tracked buffers of R rows as the interval rule with ``interval``
        wrote them -> (the emitted frames, the emitted widened buffers), oldest first: what the window held before the call."""
        assert len(frames) == self.B and len(tracked) == self.B and L.LOOKBACK[0] <= lookback <= L.LOOKBACK[1] and 0 <= radius <= 16
        assert I.INTERVAL[0] <= interval <= I.INTERVAL[1]
        n_frames = int(n_frames)
        nf, c, half = min(max(n_frames, 0), self.B), self.count, self.half
        seq = [(half, i) for i in range(c)] + [(half ^ 1, f) for f in range(nf)]

        def key(s):                                               # the window's frames and the call's both start on a key frame
            return (s if s < c else s - c) % interval == 0

        for f in range(nf):                                       # 1 join
            assert frames[f].shape == (self.h, self.w, 3) and frames[f].dtype == np.uint8
            self.bufs[half ^ 1, f] = L.widen(tracked[f], self.R2)
            self.pix[half ^ 1, f, :3 * self.h * self.w] = np.asarray(frames[f]).reshape(-1)
        self.chained = []                                         # (t, row, birth, the frames reached) of this call, for the tests' own checks
        for t in range(max(c, 1), c + nf):                        # 2 chain: the sources of the call's key frames
            if not key(t):
                continue
            bt = self.bufs[seq[t]]
            first_id = int(self.bufs[seq[t - 1]][2])
            _, _, _, _, t_box, t_cls, t_prob, t_id, _ = T.split(bt)
            for r, birth in sources(bt, first_id, self.capacity):
                box = [int(v) for v in t_box[r]]
                reached = []
                for k in range(1, lookback + 1):
                    g = t - k
                    if g < 0 or (not birth and key(g)):           # a correction stops in front of the previous key frame
                        break
                    box = L.step_back(self.frame(seq[g + 1]), self.frame(seq[g]), box, radius)
                    self._append(seq[g], L.backfilled_box(box, self.h, self.w, grow * k), int(t_cls[r]), int(t_prob[r]), int(t_id[r]), -k)
                    reached.append(g)
                self.chained.append((t, r, birth, reached))
        out = ([self.frame((half, i)).copy() for i in range(c)], [self.bufs[half, i].copy() for i in range(c)])      # 3 emit
        if n_frames < 0:                                          # 4 close
            self.count = 0
        elif n_frames > 0:
            self.count, self.half = nf, half ^ 1
        return out


# ----------------------------------------------------------------------------------------------------------- test material
# (x, y, width, height) in frame 0: with MOVE a frame every box stays at least 4 pixels inside a 48 x 64 frame for 12 frames
OBJECTS = ((5, 27, 10, 8), (17, 36, 10, 8), (5, 36, 10, 8), (17, 27, 10, 8))


def rolled(h, w, n, seed, move=MOVE):
    """``n`` frames: one noise image rolled by ``move`` a frame (``move`` = (0, 0): identical frames)."""
    img = L.texture(h, w, seed)
    return [np.ascontiguousarray(np.roll(img, (move[1] * t, move[0] * t), axis=(0, 1))) for t in range(n)]


def object_box(o, t, move=MOVE):
    x, y, bw, bh = OBJECTS[o]
    return x + move[0] * t, y + move[1] * t, x + move[0] * t + bw - 1, y + move[1] * t + bh - 1


def sequence(h, w, n, interval, seed, rows, capacity, detected, move=MOVE, hold=2, grow=1, radius=4, per_call=None):
    """A seeded sequence of ``n`` frames (``rolled``) whose objects ride with the image; object o is "detected" (class 1 + o % 2) in key
    frame t where ``detected(o, t)`` says so -> (frames, the tracked buffers of track_interval_ref.IntervalTracker over calls of
    ``per_call`` frames, default: one call).  Every call starts on a key frame."""
    frames = rolled(h, w, n, seed, move)
    table = np.array([0, 1, 1], dtype=np.uint8)
    tracker = I.IntervalTracker(capacity)
    per_call = per_call or n
    tracked = []
    for at in range(0, n, per_call):
        part = frames[at:at + per_call]
        packs = []
        for f in range(0, len(part), interval):
            dets = [object_box(o, at + f, move) + (1 + o % 2, 0.5 + 0.01 * o) for o in range(len(OBJECTS)) if detected(o, at + f)]
            packs.append(L.packed(dets[:rows], rows))
        tracked += tracker.update_interval(part, packs, len(part), table, h, w, 30, hold, grow, radius, interval)
    return frames, tracked


def run(window, frames, tracked, sizes, lookback, radius=0, grow=0, interval=1, flush=True):
    """track_lookback_ref.run with the interval: a whole sequence cut into calls of ``sizes`` real frames (each padded to the window's
    frames) -> every emitted (frame, buffer), in order; with ``flush`` the last call is followed by a flush."""
    F, out_f, out_t, at = window.B, [], [], 0
    blank_f = np.zeros((window.h, window.w, 3), dtype=np.uint8)
    blank_t = np.zeros(4 + 8 * window.R, dtype=np.int32)
    for n in list(sizes) + ([-1] if flush else []):
        real = max(n, 0)
        fs = list(frames[at:at + real]) + [blank_f] * (F - real)
        ts = list(tracked[at:at + real]) + [blank_t] * (F - real)
        ef, et = window.call(fs, ts, n, lookback, radius, grow, interval)
        out_f += ef
        out_t += et
        at += real
    return out_f, out_t


def backfilled(buf):
    """The back-filled rows of an emitted buffer, in place order: [(id, k, bbox)]."""
    n_rows, _, _, _, bbox, _, _, ids, age = T.split(buf)
    return [(int(ids[r]), -int(age[r]), tuple(int(v) for v in bbox[r])) for r in range(n_rows) if int(age[r]) < 0]


def check_shifts(out_t, interval, h, w, margin, move=MOVE, grow=0):
    """Every back-filled row of the emitted buffers ``out_t`` (a whole sequence from its frame 0, calls of whole intervals) whose raw box
    stays ``margin`` pixels inside the (h, w) frame from its source frame to its own: its box is its source row's shifted by -k x ``move``
    (and grown by grow * k) -> how many rows were checked."""
    checked = 0
    for g, buf in enumerate(out_t):
        for tid, k, box in backfilled(buf):
            t = g + k
            assert t % interval == 0, (g, tid, k)                 # (a source sits in a key frame)
            _, n_live, _, _, bbox, _, _, ids, _ = T.split(out_t[t])
            src = [tuple(int(v) for v in bbox[r]) for r in range(n_live) if int(ids[r]) == tid]
            assert len(src) == 1, (g, tid, k)
            x1, y1, x2, y2 = src[0]
            raw = (x1 - k * move[0], y1 - k * move[1], x2 - k * move[0], y2 - k * move[1])
            if (min(x1, y1, raw[0], raw[1]) < margin or max(x2, raw[2]) > w - 1 - margin or max(y2, raw[3]) > h - 1 - margin):
                continue
            checked += 1
            e = grow * k
            assert box == (raw[0] - e, raw[1] - e, raw[2] + e, raw[3] + e), (g, tid, k, box, raw)
    return checked
