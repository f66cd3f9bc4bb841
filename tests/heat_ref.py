"""Numpy restatement of the heat rule (DESIGN §8 "Heat rule"; include/ext/frcnn_hip_heat.h), the comparand of tests/test_heat_*.py.  It
follows the rule as written -- the frame's boxes, then frames, decay, add, clamp, peak; the draw pixel by pixel -- on top of
tests/redact_ref.py's clipping (``mask`` of one row) and tests/track_ref.py's buffer split, not the kernels (csrc/heat.hip).  Integers
throughout (int64 where the rule says 64 bits): a sequence has one right answer."""
import numpy as np

from tests import redact_ref, track_ref

MAX = 1 << 30                                    # FRCNN_HEAT_MAX
ALPHA, DECAY = (1, 255, 160), (0, 15, 0)         # (smallest, largest, default)
GAIN = 256


def split_packed(packed):
    """(n_dets, bbox (rows, 4), cls) of a det_packed buffer, int32 [4 + 7 rows]."""
    packed = np.asarray(packed)
    rows = (packed.size - 4) // 7
    return int(packed[0]), packed[4:4 + 4 * rows].reshape(rows, 4), packed[4 + 4 * rows:4 + 5 * rows]


def boxes_of(buf, tracked):
    """(n, bbox, cls): the rows of a frame's buffer the rule reads -- every row of a packed buffer, the LIVE rows of a tracked one --,
    the count clamped to the buffer's rows."""
    if tracked:
        _, n_live, _, _, bbox, cls, _, _, _ = track_ref.split(buf)
        n = n_live
    else:
        n, bbox, cls = split_packed(buf)
    return min(max(int(n), 0), len(cls)), bbox, cls


def coverage(h, w, buf, tracked, table):
    """(h, w) int64: how many of the frame's boxes cover each pixel.  A box is one row's redaction mask at margin 0: clipped, inclusive at
    both ends, nothing for an empty one or a class that is not set."""
    n, bbox, cls = boxes_of(buf, tracked)
    cov = np.zeros((h, w), dtype=np.int64)
    for r in range(n):
        cov += redact_ref.mask(h, w, bbox[r:r + 1], cls[r:r + 1], 1, table, 0)
    return cov


class Heat:
    """The state: ``frames``, ``peak``, ``saturated`` and the (h, w) int64 ``map``."""

    def __init__(self, h, w, words=None):
        self.h, self.w = h, w
        self.frames = self.peak = self.saturated = 0
        self.map = np.zeros((h, w), dtype=np.int64)
        if words is not None:
            words = np.asarray(words)
            self.frames, self.peak, self.saturated = int(words[0]), int(words[1]), int(words[2])
            self.map = words[4:4 + h * w].astype(np.int64).reshape(h, w)

    def words(self):
        """The state's 4 + h w int32 words."""
        return np.concatenate([[self.frames, self.peak, self.saturated, 0], self.map.reshape(-1)]).astype(np.int32)

    def update(self, buf, table, decay=0, tracked=False, frame_index=0, n_frames=1, gate=None):
        """UPDATE of one frame.  Not real: nothing changes."""
        assert DECAY[0] <= decay <= DECAY[1]
        if not frame_index < max(int(n_frames), 0) or (gate is not None and int(gate) == 0):
            return self
        self.frames += 1
        v = self.map
        if decay > 0:
            v = v - ((v + (1 << decay) - 1) >> decay)
        v = v + GAIN * coverage(self.h, self.w, buf, tracked, table)
        if (v > MAX).any():
            self.saturated = 1
        self.map = np.minimum(v, MAX)
        self.peak = int(self.map.max())
        return self

    def levels(self):
        """t of every pixel, (h, w) int64; None for a cold map."""
        if self.peak <= 0:
            return None
        return np.clip(self.map, 0, self.peak) * 255 // self.peak

    def draw(self, frame, alpha=ALPHA[2], rgb=False):
        """A copy of ``frame`` (h, w, 3) uint8 with the map blended in."""
        assert ALPHA[0] <= alpha <= ALPHA[1]
        out = np.asarray(frame, dtype=np.uint8).copy()
        t = self.levels()
        if t is None:
            return out
        ramp = np.stack([np.minimum(255, 3 * t), np.clip(3 * t - 255, 0, 255), np.clip(3 * t - 510, 0, 255)], axis=-1)      # R, G, B
        if not rgb:
            ramp = ramp[..., ::-1]
        a = (alpha * t // 255)[..., None]
        blended = (out.astype(np.int64) * (255 - a) + ramp * a + 127) // 255
        return np.where(a > 0, blended, out).astype(np.uint8)


def make_packed(rows, boxes, cls=None, n_dets=None):
    """A det_packed buffer by hand: ``boxes`` fill rows 0.., class 1 unless ``cls`` says otherwise."""
    b = np.zeros(4 + 7 * rows, dtype=np.int32)
    b[0] = len(boxes) if n_dets is None else n_dets
    for r, box in enumerate(boxes):
        b[4 + 4 * r:8 + 4 * r] = box
        b[4 + 4 * rows + r] = 1 if cls is None else cls[r]
    return b


def make_tracked(rows, n_live, boxes, cls=None):
    """A tracked buffer by hand: ``boxes`` fill rows 0.., the first ``n_live`` of them live, the rest held."""
    b = np.zeros(4 + 8 * rows, dtype=np.int32)
    b[4:4 + 5 * rows] = -1
    b[0], b[1] = len(boxes), n_live
    for r, box in enumerate(boxes):
        b[4 + 4 * r:8 + 4 * r] = box
        b[4 + 4 * rows + r] = 1 if cls is None else cls[r]
        b[4 + 6 * rows + r] = r + 1
        b[4 + 7 * rows + r] = 0 if r < n_live else 1
    return b
