"""Plain-Python restatement of the tracking rule (DESIGN §8 "Tracking rule"; include/ext/frcnn_hip_track.h), the comparand of
tests/test_track_*.py.  It follows the rule as written -- slots in id order taking rows, ageing, births, output -- with Python ints, not
the kernel (csrc/track.hip).  Integers throughout: a sequence has one right answer.

A frame's detections are given as the kernel sees them: ``bbox`` (rows, 4) x1, y1, x2, y2, ``cls`` (rows,), ``prob`` (rows,) the
float32 BIT patterns as ints, ``n_dets``; ``table`` (num_classes,) is non-zero where a class is tracked."""
import numpy as np

from tests import annotate_ref

MAX = 128                                        # FRCNN_TRACK_MAX
DEFAULTS = (30, 8, 0)                            # thr, hold, grow


def clip(box, h, w):
    """The clipped inclusive box (xa, xb, ya, yb) of a raw (x1, y1, x2, y2): the redaction rule's with margin 0."""
    x1, y1, x2, y2 = [int(v) for v in box]
    return max(min(x1, x2), 0), min(max(x1, x2), w - 1), max(min(y1, y2), 0), min(max(y1, y2), h - 1)


def empty(c):
    return c[0] > c[1] or c[2] > c[3]


def area(c):
    return (c[1] - c[0] + 1) * (c[3] - c[2] + 1)


def inter_union(a, b):
    """(inter, union) of two clipped boxes, neither empty."""
    iw = min(a[1], b[1]) - max(a[0], b[0]) + 1
    ih = min(a[3], b[3]) - max(a[2], b[2]) + 1
    inter = iw * ih if iw > 0 and ih > 0 else 0
    return inter, area(a) + area(b) - inter


class Tracker:
    """The state and the rule.  ``slots``: the live slots, dicts with id, cls, bbox (raw), prob (bits), age, in ascending id order."""

    def __init__(self, capacity=64):
        assert 1 <= capacity <= MAX
        self.capacity, self.slots, self.next_id, self.overflow, self.frames = capacity, [], 1, 0, 0
        self.events = {"match": 0, "hold": 0, "free": 0, "birth": 0, "overflow": 0}      # what the rule did so far (for the tests' own checks)

    def words(self):
        """The state as the device holds it: int32 [4 + 8 capacity]."""
        C = self.capacity
        s = np.zeros(4 + 8 * C, dtype=np.int64)
        s[:4] = (len(self.slots), self.next_id - 1, self.overflow, self.frames)
        for i, t in enumerate(self.slots):
            s[4 + i], s[4 + C + i], s[4 + 6 * C + i], s[4 + 7 * C + i] = t["id"], t["cls"], t["prob"], t["age"]
            s[4 + 2 * C + 4 * i:4 + 2 * C + 4 * i + 4] = t["bbox"]
        return s.astype(np.int32)

    def update(self, bbox, cls, prob, n_dets, max_rows, table, h, w, thr=30, hold=8, grow=0):
        """One frame -> its tracked buffer, int32 [4 + 8R], R = max_rows + capacity."""
        assert 1 <= thr <= 100 and 0 <= hold <= 255 and 0 <= grow <= 64 and 1 <= h <= 32768 and 1 <= w <= 32768
        n = min(max(int(n_dets), 0), max_rows)
        rows = [[int(v) for v in np.asarray(bbox).reshape(-1, 4)[r]] for r in range(n)]
        boxes = [clip(b, h, w) for b in rows]
        eligible = [0 <= int(cls[r]) < len(table) and bool(table[int(cls[r])]) and not empty(boxes[r]) for r in range(n)]
        ids = [0] * n
        # 1 match
        hit = set()
        for t in self.slots:
            sbox = clip(t["bbox"], h, w)
            best = None                                       # (inter, union, row)
            for r in range(n):
                if not eligible[r] or ids[r] or int(cls[r]) != t["cls"] or empty(sbox):
                    continue
                inter, union = inter_union(sbox, boxes[r])
                if inter <= 0 or inter * 100 < thr * union:
                    continue
                if best is None or inter * best[1] > best[0] * union:      # strictly better: ties stay with the lower row
                    best = (inter, union, r)
            if best is not None:
                r = best[2]
                ids[r] = t["id"]
                t["bbox"], t["prob"], t["age"] = rows[r], int(prob[r]), 0
                hit.add(t["id"])
                self.events["match"] += 1
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
        # 3 birth
        for r in range(n):
            if not eligible[r] or ids[r]:
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
        # 4 output
        R = max_rows + self.capacity
        out = np.zeros(4 + 8 * R, dtype=np.int64)
        o_box, o_cls, o_prob, o_id, o_age = (out[4:4 + 4 * R].reshape(R, 4), out[4 + 4 * R:4 + 5 * R], out[4 + 5 * R:4 + 6 * R],
                                             out[4 + 6 * R:4 + 7 * R], out[4 + 7 * R:4 + 8 * R])
        o_box[:], o_cls[:] = -1, -1
        for r in range(n):
            o_box[r], o_cls[r], o_prob[r], o_id[r] = rows[r], int(cls[r]), int(prob[r]), ids[r]
        k = n
        for t in self.slots:
            if t["age"] >= 1:
                xa, xb, ya, yb = clip(t["bbox"], h, w)
                g = grow * t["age"]
                o_box[k], o_cls[k], o_prob[k], o_id[k], o_age[k] = (xa - g, ya - g, xb + g, yb + g), t["cls"], t["prob"], t["id"], t["age"]
                k += 1
                self.events["hold"] += 1
        out[:4] = (k, n, self.next_id, self.overflow)
        return out.astype(np.int32)

    def padding(self, max_rows):
        """The tracked buffer of a frame behind *n_frames: no rows, the state as it stands."""
        R = max_rows + self.capacity
        out = np.zeros(4 + 8 * R, dtype=np.int64)
        out[4:4 + 5 * R] = -1
        out[:4] = (0, 0, self.next_id, self.overflow)
        return out.astype(np.int32)

    def update_packed(self, packed, table, h, w, thr=30, hold=8, grow=0):
        """``update`` over a det_packed buffer (int32 [4 + 7 rows]) of the post-process."""
        packed = np.asarray(packed)
        rows = (packed.size - 4) // 7
        return self.update(packed[4:4 + 4 * rows].reshape(rows, 4), packed[4 + 4 * rows:4 + 5 * rows], packed[4 + 5 * rows:4 + 6 * rows],
                           int(packed[0]), rows, table, h, w, thr, hold, grow)


def split(buf):
    """(n_rows, n_live, next_id, overflow, bbox (R, 4), cls, prob bits, id, age) of a tracked buffer."""
    buf = np.asarray(buf)
    R = (buf.size - 4) // 8
    return (int(buf[0]), int(buf[1]), int(buf[2]), int(buf[3]), buf[4:4 + 4 * R].reshape(R, 4), buf[4 + 4 * R:4 + 5 * R],
            buf[4 + 5 * R:4 + 6 * R], buf[4 + 6 * R:4 + 7 * R], buf[4 + 7 * R:4 + 8 * R])


# ----------------------------------------------------------------------------------------------------------- host dets
def bits(p):
    return int(np.array([p], dtype=np.float32).view(np.int32)[0])


def track_dets(tracker, dets, class_mapping, classes, h, w, thr=30, hold=8, grow=0):
    """The rule over one frame's host dets (dicts with "bbox", "cls_name", "prob"; the LIVE rows of a frame, in order) -> (live, held):
    ``live`` the same dets, each with "track_id" (0: untracked), ``held`` the held rows as dets with "track_id" and "held" = age.
    ``classes``: the tracked class names."""
    C = max(class_mapping.values()) + 1
    rev = {v: k for k, v in class_mapping.items()}
    table = np.zeros(C, dtype=np.uint8)
    for name, idx in class_mapping.items():
        table[idx] = name in classes
    n = len(dets)
    bbox = np.array([[int(v) for v in d["bbox"]] for d in dets], dtype=np.int64).reshape(-1, 4)
    cls = np.array([class_mapping[d["cls_name"]] for d in dets], dtype=np.int64)
    prob = np.array([bits(d["prob"]) for d in dets], dtype=np.int64)
    n_rows, n_live, _, _, o_box, o_cls, o_prob, o_id, o_age = split(tracker.update(bbox, cls, prob, n, max(n, 1), table, h, w, thr, hold, grow))
    assert n_live == n
    live = [dict(d, track_id=int(o_id[r])) for r, d in enumerate(dets)]
    held = [{"bbox": o_box[r].astype(np.int64), "cls_name": rev[int(o_cls[r])], "prob": np.array([o_prob[r]], dtype=np.int32).view(np.float32)[0],
             "track_id": int(o_id[r]), "held": int(o_age[r])} for r in range(n_live, n_rows)]
    return live, held


def label_text(det):
    """The label of a det: "{}#{} {:6.2f}" with a track id > 0, else the drawing rule's."""
    if det.get("track_id", 0) > 0:
        return "{}#{} {:6.2f}".format(det["cls_name"], det["track_id"], det["prob"])
    return annotate_ref.label_text(det)


def annotate(frame, dets, glyphs=None):
    """tests/annotate_ref.annotate with the ids in the labels: the dets the drawing rule draws, each under the name ``cls#id`` when it
    has a track id (the rule's own filter sees the true class name first); held rows ("held") are never drawn."""
    h, w = frame.shape[:2]
    drawn = []
    for d in dets:
        if d.get("held") or not annotate_ref.is_drawn(d, w, h):
            continue
        tid = d.get("track_id", 0)
        drawn.append(dict(d, cls_name="%s#%d" % (d["cls_name"], tid)) if tid > 0 else d)
    return annotate_ref.annotate(frame, drawn, glyphs)


def mot_lines(frame_no, dets, class_mapping):
    """The MOTChallenge lines of one frame's dets: frame,id,left,top,width,height,prob,cls,-1,-1 per live tracked row, in row order;
    left / top the smaller corner, width / height the corners' distance, prob with six decimals, cls the class index."""
    out = []
    for d in dets:
        if d.get("held") or d.get("track_id", 0) <= 0:
            continue
        x1, y1, x2, y2 = [int(v) for v in d["bbox"]]
        out.append("%d,%d,%d,%d,%d,%d,%s,%s,-1,-1" % (frame_no, d["track_id"], min(x1, x2), min(y1, y2), abs(x2 - x1), abs(y2 - y1),
                                                     format(float(d["prob"]), ".6f"), class_mapping[d["cls_name"]]))
    return out
