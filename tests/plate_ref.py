"""The plate rule (DESIGN §8 "Plate rule", include/ext/frcnn_hip_plate.h) restated in numpy: what the kernels of csrc/plate.hip must give,
bit for bit.  Integers only.  A state is an int32 array [frames, known, 0, 0 | px[h][w][2]] (the kernels' scratch words are no part of it);
a detection buffer is the packed (7 words a row) or tracked (8 words a row) int32 array the kernels read."""
import numpy as np


def empty(h, w):
    return np.zeros(4 + 2 * h * w, dtype=np.int32)


def boxes(det, rows, h, w, margin, table=None):
    """The clipped boxes (xa, xb, ya, yb) of the BLOCK set (``table`` None) or of the FILL set of ``det``, a buffer of ``rows`` rows."""
    det = np.asarray(det, dtype=np.int64)
    n = min(max(int(det[0]), 0), rows)
    out = []
    for r in range(n):
        if table is not None:
            c = int(det[4 + 4 * rows + r])
            if not (0 <= c < len(table) and table[c]):
                continue
        x1, y1, x2, y2 = (int(v) for v in det[4 + 4 * r:8 + 4 * r])
        xa, xb = max(min(x1, x2) - margin, 0), min(max(x1, x2) + margin, w - 1)
        ya, yb = max(min(y1, y2) - margin, 0), min(max(y1, y2) + margin, h - 1)
        if xa <= xb and ya <= yb:
            out.append((xa, xb, ya, yb))
    return out


def mask(det, rows, h, w, margin, table=None):
    m = np.zeros((h, w), dtype=bool)
    for xa, xb, ya, yb in boxes(det, rows, h, w, margin, table):
        m[ya:yb + 1, xa:xb + 1] = True
    return m


def unpack(state, h, w):
    """-> (P (h, w, 3), V (h, w), C (h, w, 3), N (h, w)) as int64."""
    px = np.asarray(state[4:4 + 2 * h * w]).astype(np.int64).reshape(h, w, 2) & 0xffffffff
    w0, w1 = px[:, :, 0], px[:, :, 1]
    chan = lambda v: np.stack([v & 255, (v >> 8) & 255, (v >> 16) & 255], axis=2)
    return chan(w0), w0 >> 24, chan(w1), w1 >> 24


def pack(state, h, w, P, V, C, N):
    join = lambda c, top: (c[:, :, 0] | (c[:, :, 1] << 8) | (c[:, :, 2] << 16) | (top << 24)).astype(np.uint32)
    px = np.stack([join(P, V), join(C, N)], axis=2)
    state[4:4 + 2 * h * w] = px.reshape(-1).view(np.int32)


def update(state, frame, det, rows, settle, tol, margin, frame_index=0, n_frames=1, gate=None, cut=None):
    """UPDATE, in place -> state.  ``frame`` uint8 (h, w, 3), untouched."""
    h, w = frame.shape[:2]
    if not (frame_index < max(int(n_frames), 0) and (gate is None or int(gate) != 0)):
        return state
    if cut is not None and int(cut) != 0:
        state[4:4 + 2 * h * w] = 0
    P, V, C, N = unpack(state, h, w)
    x = frame.astype(np.int64)
    blocked = mask(det, rows, h, w, margin)
    d = np.abs(x - C).max(axis=2)
    go_on = ~blocked & (N >= 1) & (d <= tol)
    restart = ~blocked & ~go_on
    N = np.where(blocked, 0, np.where(go_on, np.minimum(N + 1, 255), 1))
    C = np.where(restart[:, :, None], x, C)
    settle_now = ~blocked & (N >= settle)
    P = np.where(settle_now[:, :, None], x, P)
    V = np.where(settle_now, 1, V)
    pack(state, h, w, P, V, C, N)
    state[0] += 1
    state[1] = int((V != 0).sum())
    return state


def known(state, h, w):
    return int((unpack(state, h, w)[1] != 0).sum())


def fill(frame, state, det, rows, table, margin, keep_unknown=False):
    """FILL, in place -> (frame, the mask of the pixels filled from the plate, the mask of the FILL pixels the plate does not know)."""
    h, w = frame.shape[:2]
    P, V, _, _ = unpack(state, h, w)
    under = mask(det, rows, h, w, margin, table)
    from_plate, unknown = under & (V != 0), under & (V == 0)
    frame[from_plate] = P[from_plate].astype(np.uint8)
    if not keep_unknown:
        frame[unknown] = 0
    return frame, from_plate, unknown


def packed(rows, dets):
    """A packed buffer of ``rows`` rows from [(x1, y1, x2, y2, cls)]."""
    buf = np.zeros(4 + 7 * rows, dtype=np.int32)
    buf[0] = len(dets)
    for r, (x1, y1, x2, y2, c) in enumerate(dets[:rows]):
        buf[4 + 4 * r:8 + 4 * r] = (x1, y1, x2, y2)
        buf[4 + 4 * rows + r] = c
    return buf


def tracked(rows, dets, n_live=None):
    """A tracked buffer of ``rows`` rows from [(x1, y1, x2, y2, cls)]: the first ``n_live`` live, the others held."""
    buf = np.zeros(4 + 8 * rows, dtype=np.int32)
    buf[0], buf[1] = len(dets), len(dets) if n_live is None else n_live
    for r, (x1, y1, x2, y2, c) in enumerate(dets[:rows]):
        buf[4 + 4 * r:8 + 4 * r] = (x1, y1, x2, y2)
        buf[4 + 4 * rows + r] = c
    return buf
