"""Plain-numpy restatement of the interval rule (DESIGN §8 "Interval rule"; include/ext/frcnn_hip_track_interval.h) on top of
tests/track_motion_ref.py and tests/track_ref.py, the comparand of tests/test_track_interval_*.py.  It follows the rule as written -- a
key frame is the motion rule's frame, a between frame moves the slots and writes them out -- not the kernel (csrc/track_interval.hip).
Integers throughout: a sequence has one right answer."""
import numpy as np

from tests import track_motion_ref as M
from tests import track_ref as T

INTERVAL = (1, 16)                               # smallest (at the ABI; the public option starts at 2), largest


def keys_of(frames, interval):
    """The key frames a call of ``frames`` frames reads detections for."""
    return (frames + interval - 1) // interval


class IntervalTracker(M.MotionTracker):
    """track_motion_ref.MotionTracker with calls whose detections come every ``interval`` frames."""

    def move(self, prev, cur, h, w, radius):
        """Step 0 of one frame: every live slot searched on its own."""
        for s in self.t.slots:
            dx, dy = M.search(prev, cur, T.clip(s["bbox"], h, w), radius)[:2]
            if dx or dy:
                x1, y1, x2, y2 = s["bbox"]
                s["bbox"] = [x1 + dx, y1 + dy, x2 + dx, y2 + dy]
                self.moves.append((s["id"], dx, dy))

    def between(self, rows, h, w, grow):
        """A between frame's OUTPUT: the slots of age 0 as live rows with their raw boxes, the held slots behind them as step 4 writes
        them; the frame counts."""
        t = self.t
        R = rows + t.capacity
        out = np.zeros(4 + 8 * R, dtype=np.int64)
        o_box, o_cls, o_prob, o_id, o_age = (out[4:4 + 4 * R].reshape(R, 4), out[4 + 4 * R:4 + 5 * R], out[4 + 5 * R:4 + 6 * R],
                                             out[4 + 6 * R:4 + 7 * R], out[4 + 7 * R:4 + 8 * R])
        o_box[:], o_cls[:] = -1, -1
        live = [s for s in t.slots if s["age"] == 0]
        held = [s for s in t.slots if s["age"] >= 1]
        for k, s in enumerate(live):
            o_box[k], o_cls[k], o_prob[k], o_id[k] = s["bbox"], s["cls"], s["prob"], s["id"]
        for k, s in enumerate(held, len(live)):
            xa, xb, ya, yb = T.clip(s["bbox"], h, w)
            g = grow * s["age"]
            o_box[k], o_cls[k], o_prob[k], o_id[k], o_age[k] = (xa - g, ya - g, xb + g, yb + g), s["cls"], s["prob"], s["id"], s["age"]
        out[:4] = (len(live) + len(held), len(live), t.next_id, t.overflow)
        t.frames += 1
        return out.astype(np.int32)

    def update_interval(self, frames, packed, n_frames, table, h, w, thr=30, hold=8, grow=0, radius=M.RADIUS[2], interval=1):
        """One call: ``frames`` a list of F frames, ``packed`` the det_packed buffers of its key frames 0, interval, ... -> the F tracked
        buffers."""
        assert INTERVAL[0] <= interval <= INTERVAL[1] and len(packed) == keys_of(len(frames), interval)
        nf = min(max(int(n_frames), 0), len(frames))
        rows = (np.asarray(packed[0]).size - 4) // 7
        prev = self.frame if self.kept >= 1 and self.kept == self.t.frames and self.size == (h, w) else None
        out = []
        for f in range(len(frames)):
            if f >= nf:
                out.append(self.t.padding(rows))
                continue
            cur = np.asarray(frames[f])
            assert cur.shape == (h, w, 3) and cur.dtype == np.uint8
            if prev is not None:
                self.move(prev, cur, h, w, radius)
            if f % interval == 0:
                out.append(self.t.update_packed(packed[f // interval], table, h, w, thr, hold, grow))
            else:
                out.append(self.between(rows, h, w, grow))
            prev = cur
        if nf >= 1:
            self.frame, self.kept, self.size = np.array(frames[nf - 1], dtype=np.uint8), self.t.frames, (h, w)
        return out

    def track_between(self, frame, class_mapping, grow=0, radius=M.RADIUS[2]):
        """``MotionTracker.track_dets`` for a between frame: one frame, no dets -> (live, held) as dets made of the tracks."""
        h, w = frame.shape[:2]
        if self.kept >= 1 and self.kept == self.t.frames and self.size == (h, w):
            self.move(self.frame, frame, h, w, radius)
        dets = between_dets(self.between(1, h, w, grow), {v: k for k, v in class_mapping.items()})
        self.frame, self.kept, self.size = np.array(frame, dtype=np.uint8), self.t.frames, (h, w)
        return [d for d in dets if "held" not in d], [d for d in dets if "held" in d]


def between_dets(buf, rev):
    """The dets a between frame's tracked buffer stands for: the live rows with "track_id" and "propagated", the held ones with "held"."""
    n_rows, n_live, _, _, bbox, cls, prob, ids, age = T.split(buf)
    dets = []
    for k in range(n_rows):
        d = {"bbox": bbox[k].astype(np.int64), "cls_name": rev[int(cls[k])], "prob": np.array([prob[k]], dtype=np.int32).view(np.float32)[0],
             "track_id": int(ids[k])}
        if k < n_live:
            d["propagated"] = True
        else:
            d["held"] = int(age[k])
        dets.append(d)
    return dets
