"""Plain-numpy restatement of the cut rule (DESIGN §8 "Cut rule"; include/ext/frcnn_hip_track_cut.h) on top of tests/track_interval_ref.py,
the comparand of tests/test_track_cut_*.py.  It follows the rule as written -- a signature of 4 x 4 regions x 32 luma bins per frame, the
sum of the counters' differences, the threshold, and step C in front of the interval rule's frame -- not the kernel (csrc/track_cut.hip).
Integers throughout: a sequence has one right answer."""
import numpy as np

from tests import track_interval_ref as I
from tests import track_motion_ref as M

REGIONS, BINS = 4, 32
PCT = (1, 100, 40)                               # smallest, largest, the default (provisional: nothing measured on real footage)


def signature(frame):
    """H_F: int64 [4][4][32], one count per pixel of the (h, w, 3) uint8 frame."""
    h, w = frame.shape[:2]
    ry = (4 * np.arange(h)) // h
    rx = (4 * np.arange(w)) // w
    sig = np.zeros((REGIONS, REGIONS, BINS), dtype=np.int64)
    np.add.at(sig, (ry[:, None].repeat(w, 1), rx[None, :].repeat(h, 0), M.luma(frame) >> 3), 1)
    return sig


def distance(ref, cur):
    """D: the sum over the 512 counters of |H_cur - H_P|, a Python int (at most 2hw)."""
    return int(np.abs(signature(cur) - signature(ref)).sum())


def is_cut(ref, cur, pct):
    """Is ``cur`` a cut behind its reference frame ``ref`` (None: no reference, never a cut)?"""
    assert PCT[0] <= pct <= PCT[1]
    if ref is None:
        return False
    h, w = cur.shape[:2]
    return distance(ref, cur) * 100 >= pct * 2 * h * w


class CutTracker(I.IntervalTracker):
    """track_interval_ref.IntervalTracker with step C in front of every frame."""

    def free_all(self):
        """Step C on a cut: no slot lives on; `issued` (next_id), `overflow` and `frames` stay."""
        self.t.slots = []

    def cut_step(self, frame, pct=PCT[2]):
        """Step C of a one-frame call (``track_dets`` / ``track_between`` then follow): the reference is the kept frame.  -> is it a cut?"""
        h, w = frame.shape[:2]
        prev = self.frame if self.kept >= 1 and self.kept == self.t.frames and self.size == (h, w) else None
        cut = is_cut(prev, frame, pct)
        if cut:
            self.free_all()
        return cut

    def update_cut(self, frames, packed, n_frames, table, h, w, thr=30, hold=8, grow=0, radius=M.RADIUS[2], interval=1, pct=PCT[2]):
        """One call -> (the F tracked buffers, cuts int32 [F])."""
        assert I.INTERVAL[0] <= interval <= I.INTERVAL[1] and len(packed) == I.keys_of(len(frames), interval)
        nf = min(max(int(n_frames), 0), len(frames))
        rows = (np.asarray(packed[0]).size - 4) // 7
        prev = self.frame if self.kept >= 1 and self.kept == self.t.frames and self.size == (h, w) else None
        out, cuts = [], np.zeros(len(frames), dtype=np.int32)
        for f in range(len(frames)):
            if f >= nf:
                out.append(self.t.padding(rows))
                continue
            cur = np.asarray(frames[f])
            assert cur.shape == (h, w, 3) and cur.dtype == np.uint8
            if is_cut(prev, cur, pct):
                cuts[f] = 1
                self.free_all()
            if prev is not None:
                self.move(prev, cur, h, w, radius)
            if f % interval == 0:
                out.append(self.t.update_packed(packed[f // interval], table, h, w, thr, hold, grow))
            else:
                out.append(self.between(rows, h, w, grow))
            prev = cur
        if nf >= 1:
            self.frame, self.kept, self.size = np.array(frames[nf - 1], dtype=np.uint8), self.t.frames, (h, w)
        return out, cuts
