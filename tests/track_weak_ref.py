"""Plain-Python restatement of the weak rule (DESIGN §8 "Weak rule"; include/ext/frcnn_hip_track_weak.h) on top of tests/track_ref.py, the
comparand of tests/test_track_weak_*.py.  It follows the rule as written -- stage A over the strong rows, stage B over the weak ones,
ageing, births from strong rows, the compacted output -- with Python ints and ONE float32 comparison per row, not the kernel
(csrc/track.hip).  ``strong=None`` is tests/track_ref.py's rule itself."""
import numpy as np

from tests import track_ref as T


def is_strong(prob_bits, strong):
    """``__int_as_float(prob) >= strong`` in float32, under the IEEE comparison: False for a NaN score."""
    p = np.array([int(prob_bits)], dtype=np.int64).astype(np.int32).view(np.float32)[0]
    with np.errstate(invalid="ignore"):
        return bool(p >= np.float32(strong))


class Tracker(T.Tracker):
    """tests/track_ref.Tracker whose ``update`` takes ``strong``."""

    def __init__(self, capacity=64):
        super().__init__(capacity)
        self.events.update({"weak_match": 0, "weak_drop": 0})

    def _match(self, rows, boxes, cls, prob, open_rows, slots, ids, hit, h, w, thr, event):
        """The slots of ``slots`` in order, each against the rows of ``open_rows`` that are still unmatched."""
        for t in slots:
            sbox = T.clip(t["bbox"], h, w)
            best = None                                       # (inter, union, row)
            for r in open_rows:
                if ids[r] or int(cls[r]) != t["cls"] or T.empty(sbox):
                    continue
                inter, union = T.inter_union(sbox, boxes[r])
                if inter <= 0 or inter * 100 < thr * union:
                    continue
                if best is None or inter * best[1] > best[0] * union:      # strictly better: ties stay with the lower row
                    best = (inter, union, r)
            if best is not None:
                r = best[2]
                ids[r] = t["id"]
                t["bbox"], t["prob"], t["age"] = rows[r], int(prob[r]), 0
                hit.add(t["id"])
                self.events[event] += 1

    def update(self, bbox, cls, prob, n_dets, max_rows, table, h, w, thr=30, hold=8, grow=0, strong=None):
        if strong is None:
            return super().update(bbox, cls, prob, n_dets, max_rows, table, h, w, thr, hold, grow)
        assert strong == strong, "a NaN strong is refused"
        assert 1 <= thr <= 100 and 0 <= hold <= 255 and 0 <= grow <= 64 and 1 <= h <= 32768 and 1 <= w <= 32768
        n = min(max(int(n_dets), 0), max_rows)
        rows = [[int(v) for v in np.asarray(bbox).reshape(-1, 4)[r]] for r in range(n)]
        boxes = [T.clip(b, h, w) for b in rows]
        eligible = [0 <= int(cls[r]) < len(table) and bool(table[int(cls[r])]) and not T.empty(boxes[r]) for r in range(n)]
        is_s = [is_strong(prob[r], strong) for r in range(n)]
        ids = [0] * n
        hit = set()
        # 1 match, stage A: the strong rows; stage B: the slots left, against the weak rows
        self._match(rows, boxes, cls, prob, [r for r in range(n) if eligible[r] and is_s[r]], self.slots, ids, hit, h, w, thr, "match")
        self._match(rows, boxes, cls, prob, [r for r in range(n) if eligible[r] and not is_s[r]],
                    [t for t in self.slots if t["id"] not in hit], ids, hit, h, w, thr, "weak_match")
        # 2 age
        kept = []
        for t in self.slots:
            if t["id"] not in hit:
                t["age"] += 1
            if t["age"] > hold:
                self.events["free"] += 1
                continue
            kept.append(t)
        self.slots = kept
        # 3 birth: strong rows only
        for r in range(n):
            if not eligible[r] or not is_s[r] or ids[r]:
                continue
            if len(self.slots) < self.capacity:
                ids[r] = self.next_id
                self.slots.append({"id": self.next_id, "cls": int(cls[r]), "bbox": rows[r], "prob": int(prob[r]), "age": 0})
                self.next_id += 1
                self.events["birth"] += 1
            else:
                self.overflow += 1
                self.events["overflow"] += 1
        self.frames += 1
        # 4 output: the strong rows and the matched weak ones move up
        R = max_rows + self.capacity
        out = np.zeros(4 + 8 * R, dtype=np.int64)
        o_box, o_cls, o_prob, o_id, o_age = (out[4:4 + 4 * R].reshape(R, 4), out[4 + 4 * R:4 + 5 * R], out[4 + 5 * R:4 + 6 * R],
                                             out[4 + 6 * R:4 + 7 * R], out[4 + 7 * R:4 + 8 * R])
        o_box[:], o_cls[:] = -1, -1
        k = 0
        for r in range(n):
            if not is_s[r] and not ids[r]:
                self.events["weak_drop"] += 1
                continue
            o_box[k], o_cls[k], o_prob[k], o_id[k] = rows[r], int(cls[r]), int(prob[r]), ids[r]
            k += 1
        n_live = k
        for t in self.slots:
            if t["age"] >= 1:
                xa, xb, ya, yb = T.clip(t["bbox"], h, w)
                g = grow * t["age"]
                o_box[k], o_cls[k], o_prob[k], o_id[k], o_age[k] = (xa - g, ya - g, xb + g, yb + g), t["cls"], t["prob"], t["id"], t["age"]
                k += 1
                self.events["hold"] += 1
        out[:4] = (k, n_live, self.next_id, self.overflow)
        return out.astype(np.int32)

    def update_packed(self, packed, table, h, w, thr=30, hold=8, grow=0, strong=None):
        packed = np.asarray(packed)
        rows = (packed.size - 4) // 7
        return self.update(packed[4:4 + 4 * rows].reshape(rows, 4), packed[4 + 4 * rows:4 + 5 * rows], packed[4 + 5 * rows:4 + 6 * rows],
                           int(packed[0]), rows, table, h, w, thr, hold, grow, strong)


def strong_only(packed, strong):
    """The packed buffer with its weak rows taken out and the strong ones moved up (dead rows behind them): what the parent sees when the
    post-process itself runs at ``strong``."""
    packed = np.asarray(packed)
    rows = (packed.size - 4) // 7
    n = min(max(int(packed[0]), 0), rows)
    keep = [r for r in range(n) if is_strong(packed[4 + 5 * rows + r], strong)]
    out = np.zeros_like(packed)
    out[0] = len(keep)
    out[4:4 + 4 * rows] = -1
    out[4 + 4 * rows:4 + 5 * rows] = -1
    for k, r in enumerate(keep):
        out[4 + 4 * k:4 + 4 * k + 4] = packed[4 + 4 * r:4 + 4 * r + 4]
        out[4 + 4 * rows + k] = packed[4 + 4 * rows + r]
        out[4 + 5 * rows + k] = packed[4 + 5 * rows + r]
    return out
