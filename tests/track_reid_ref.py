"""The re-identify rule (include/ext/frcnn_hip_track_reid.h, DESIGN §8 "Re-identify rule") restated in plain numpy, one step at a time and
with no thought for speed: what csrc/track_reid.hip is held against, word for word.  Integers only."""
import numpy as np

SIG_WORDS, ENTRY_WORDS, LIST_WORDS, MAX_EVENTS, MAX_DISTANCE = 192, 197, 164, 32, 8192
GRID, MIN_SAMPLES = 32, 16          # the motion rule's (include/ext/frcnn_hip_track_motion.h)
WS_WORDS = 1 + SIG_WORDS


def grid(box, h, w):
    """The motion rule's GRID of a raw box -> (x0, y0, sx, sy, cols, rows), or None for an empty box."""
    x1, y1, x2, y2 = (int(v) for v in box)
    xa, xb, ya, yb = max(min(x1, x2), 0), min(max(x1, x2), w - 1), max(min(y1, y2), 0), min(max(y1, y2), h - 1)
    if xa > xb or ya > yb:
        return None
    sx, sy = (xb - xa + GRID) // GRID, (yb - ya + GRID) // GRID
    x0, y0 = xa + sx // 2, ya + sy // 2
    return x0, y0, sx, sy, (xb - x0) // sx + 1, (yb - y0) // sy + 1


def signature(frame, box, rgb):
    """SIGNATURE of ``box`` in ``frame`` (h, w, 3) uint8 -> int32[192], or None when the box has none."""
    h, w = frame.shape[:2]
    g = grid(box, h, w)
    if g is None:
        return None
    x0, y0, sx, sy, cols, rows = g
    n = cols * rows
    if n < MIN_SAMPLES:
        return None
    count = np.zeros(SIG_WORDS, dtype=np.int64)
    for j in range(rows):
        for i in range(cols):
            p = frame[y0 + j * sy, x0 + i * sx]
            r, gr, b = (int(p[0]), int(p[1]), int(p[2])) if rgb else (int(p[2]), int(p[1]), int(p[0]))
            count[64 * ((3 * j) // rows) + ((r >> 6) << 4 | (gr >> 6) << 2 | (b >> 6))] += 1
    assert count.sum() == n
    return ((count << 12) // n).astype(np.int32)


def distance(a, b):
    return int(np.abs(a.astype(np.int64) - b.astype(np.int64)).sum())


def average(entry, s):
    entry["sig"] = s.copy() if not entry["has"] else ((3 * entry["sig"].astype(np.int64) + s + 2) >> 2).astype(np.int32)
    entry["has"] = 1


def new_state(capacity):
    return np.zeros(4 + ENTRY_WORDS * capacity, dtype=np.int32)


def read_state(state, capacity):
    """-> (entries as dicts, frames, dropped, reidentified)"""
    s = np.asarray(state)
    table = []
    for e in range(min(max(int(s[0]), 0), capacity)):
        w = s[4 + ENTRY_WORDS * e:4 + ENTRY_WORDS * (e + 1)]
        table.append({"pid": int(w[0]), "tid": int(w[1]), "cls": int(w[2]), "seen": int(w[3]), "has": int(w[4]), "sig": w[5:].astype(np.int32).copy()})
    return table, int(s[1]), int(s[2]), int(s[3])


def write_state(table, frames, dropped, reid, capacity):
    s = new_state(capacity)
    s[:4] = len(table), frames, dropped, reid
    for e, t in enumerate(table):
        s[4 + ENTRY_WORDS * e:4 + ENTRY_WORDS * e + 5] = t["pid"], t["tid"], t["cls"], t["seen"], t["has"]
        s[4 + ENTRY_WORDS * e + 5:4 + ENTRY_WORDS * (e + 1)] = t["sig"]
    return s


def split(buf):
    """A tracked buffer -> (n_rows, n_live, bbox (R, 4), cls, ids), the counts clamped."""
    R = (len(buf) - 4) // 8
    n_rows = min(max(int(buf[0]), 0), R)
    return n_rows, min(max(int(buf[1]), 0), n_rows), buf[4:4 + 4 * R].reshape(R, 4), buf[4 + 4 * R:4 + 5 * R], buf[4 + 6 * R:4 + 7 * R]


def update(state, capacity, frames, tracked, n_frames, classes, pct, keep, rgb, cuts=None, ws=None):
    """The rule over the frames of a call.  ``state``: int32 words; ``frames``: (F, h, w, 3) uint8; ``tracked``: (F, 4 + 8R) int32;
    ``classes``: the per-class table; ``cuts``: None or F words; ``ws``: the workspace as the call finds it, (F, R, 193), None for
    zeros -> (state, out, lists, ws), all new arrays."""
    tracked = np.asarray(tracked, dtype=np.int32)
    F, words = tracked.shape
    R = (words - 4) // 8
    out, lists = tracked.copy(), np.zeros((F, LIST_WORDS), dtype=np.int32)
    ws = np.zeros((F, R, WS_WORDS), dtype=np.int32) if ws is None else np.array(ws, dtype=np.int32)
    nf = min(max(int(n_frames), 0), F)
    if nf == 0:
        return np.array(state, dtype=np.int32), out, lists, ws
    table, fr, dropped, reid = read_state(state, capacity)
    nc = len(classes)
    for f in range(nf):
        n_rows, n_live, bbox, cls, ids = split(tracked[f])
        tracked_cls = lambda c: 0 <= c < nc and classes[c] != 0
        # the signatures of the frame
        sigs = {}
        for r in range(R):
            s = None
            if r < n_live and ids[r] >= 1 and tracked_cls(int(cls[r])):
                s = signature(frames[f], bbox[r], rgb)
            ws[f, r, 0] = s is not None
            if s is not None:
                ws[f, r, 1:] = s
                sigs[r] = s
        if cuts is not None and cuts[f] != 0:                                # 0 CUT
            table = []
        fr += 1                                                             # 1
        present = {int(ids[r]) for r in range(n_rows) if ids[r] >= 1}       # 2 PRESENT
        for e in table:                                                     # 3 BOUND
            live = [r for r in range(n_live) if ids[r] == e["tid"] and e["tid"] >= 1]
            if live and live[0] in sigs:
                average(e, sigs[live[0]])
                e["seen"] = fr
        turn = [r for r in range(n_live) if ids[r] >= 1 and tracked_cls(int(cls[r])) and all(e["tid"] != ids[r] for e in table)]
        events = []
        for r in turn:                                                      # 4 UNBOUND
            t, c = int(ids[r]), int(cls[r])
            if any(e["tid"] == t for e in table):
                continue
            best = None
            if r in sigs:
                for k, e in enumerate(table):
                    if e["cls"] == c and e["has"] and e["tid"] not in present and fr - e["seen"] <= keep:
                        key = (distance(e["sig"], sigs[r]), k)
                        best = key if best is None or key < best else best
            if best is not None and best[0] * 100 <= pct * MAX_DISTANCE:
                e = table[best[1]]
                events.append((e["pid"], t, c, best[0], fr - e["seen"]))
                e["tid"] = t
                average(e, sigs[r])
                e["seen"] = fr
                reid += 1
            elif len(table) >= capacity:
                dropped += 1
            else:
                pos = sum(e["pid"] <= t for e in table) if table and table[-1]["pid"] > t else len(table)
                table.insert(pos, {"pid": t, "tid": t, "cls": c, "seen": fr, "has": int(r in sigs),
                                   "sig": sigs[r].copy() if r in sigs else np.zeros(SIG_WORDS, dtype=np.int32)})
        pid_of = {}
        for e in table:
            pid_of.setdefault(e["tid"], e["pid"])
        for r in range(n_rows):                                             # 5 OUT
            if ids[r] >= 1:
                out[f, 4 + 6 * R + r] = pid_of.get(int(ids[r]), int(ids[r]))
        table = [e for e in table if not (fr - e["seen"] > keep and e["tid"] not in present)]      # 6 EXPIRE
        lists[f, 0], lists[f, 1] = min(len(events), MAX_EVENTS), fr         # 7 LIST
        for k, ev in enumerate(events[:MAX_EVENTS]):
            lists[f, 4 + 5 * k:9 + 5 * k] = ev
    return write_state(table, fr, dropped, reid, capacity), out, lists, ws


def events(rlist):
    return [tuple(int(v) for v in rlist[4 + 5 * k:9 + 5 * k]) for k in range(int(rlist[0]))]


def pack(R, live, held=()):
    """A tracked buffer of R rows by hand: ``live`` and ``held`` are rows (box, cls, id); the rows behind them are the tracker's empty
    rows (bbox -1, cls -1)."""
    rows = list(live) + list(held)
    assert len(rows) <= R
    buf = np.zeros(4 + 8 * R, dtype=np.int32)
    buf[0], buf[1] = len(rows), len(live)
    buf[2] = 1 + max([r[2] for r in rows] + [0])
    buf[4:4 + 4 * R] = -1
    buf[4 + 4 * R:4 + 5 * R] = -1
    for k, (box, c, i) in enumerate(rows):
        buf[4 + 4 * k:8 + 4 * k] = box
        buf[4 + 4 * R + k] = c
        buf[4 + 5 * R + k] = np.float32(0.9).view(np.int32)
        buf[4 + 6 * R + k] = i
        buf[4 + 7 * R + k] = 0 if k < len(live) else 1
    return buf
