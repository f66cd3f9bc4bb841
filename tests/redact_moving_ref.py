"""The moving rule (DESIGN §8 "Moving rule", include/ext/frcnn_hip_redact_moving.h) restated in numpy integers on top of
tests/plate_ref.py, which gives the plate state and the clipped boxes, and tests/redact_shape_ref.py, which gives the weight of a
distance: the comparand of tests/test_redact_moving_*.py.  It follows the rule as written -- foreground per pixel, the vote and the hold per
cell, the Chebyshev distance to the pixels of the moving cells by growing the set one pixel at a time -- not the kernels
(csrc/redact_moving.hip).

A state is (frames, cells_now, left): left a (ch, cw) uint8 array; ``empty`` is the zeroed one.
"""
import numpy as np

from tests import plate_ref as P
from tests import redact_ref as R
from tests import redact_region_ref as RR
from tests import redact_shape_ref as S

CELL = 8
DEFAULTS = {"tol": 24, "vote": 8, "hold": 4, "grow": 8, "feather": 0, "unknown": 0}       # PROVISIONAL: not measured on real footage
DEFAULT_MODE, DEFAULT_SIZE = "pixelate", 16
APPLY_TILE = (256, 16)                                                      # byte columns x rows of a tile of the apply call


def cells(h, w):
    return -(-h // CELL), -(-w // CELL)


def empty(h, w):
    return [0, 0, np.zeros(cells(h, w), dtype=np.uint8)]


def foreground(frame, plate_state, det, rows, table, margin, tol, unknown):
    """(h, w) bool: FOREGROUND of every pixel of ``frame`` against the plate state as the plate update left it for this frame."""
    h, w = frame.shape[:2]
    Pl, V, _, _ = P.unpack(plate_state, h, w)
    far = np.abs(frame.astype(np.int64) - Pl).max(axis=2) > tol
    fg = np.where(V != 0, far, bool(unknown))
    return fg & ~P.mask(det, rows, h, w, margin, table)


def cell_counts(fg):
    """-> ((ch, cw) foreground pixels of every cell, (ch, cw) pixels of every clipped cell)."""
    h, w = fg.shape
    ch, cw = cells(h, w)
    pad = np.zeros((ch * CELL, cw * CELL), dtype=np.int64)
    pad[:h, :w] = fg
    inside = np.zeros_like(pad)
    inside[:h, :w] = 1
    fold = lambda a: a.reshape(ch, CELL, cw, CELL).sum(axis=(1, 3))
    return fold(pad), fold(inside)


def vote_hold(state, fg, vote, hold, cut=None):
    """VOTE AND HOLD of a real frame, in place -> the (ch, cw) bool array of the moving cells."""
    count, pixels = cell_counts(fg)
    left = state[2].astype(np.int64)
    if cut is not None and int(cut) != 0:
        left[:] = 0
    votes = count >= np.minimum(vote, pixels)
    held = ~votes & (left > 0)
    state[2] = np.where(votes, hold, np.where(held, left - 1, left)).astype(np.uint8)
    moving = votes | held
    state[0] += 1
    state[1] = int(moving.sum())
    return moving


def hard_pixels(moving, h, w):
    """(h, w) bool: the pixels of the moving cells."""
    return np.kron(moving.astype(np.uint8), np.ones((CELL, CELL), dtype=np.uint8))[:h, :w].astype(bool)


def distance(hard, cap):
    """(h, w) ints: the Chebyshev distance of every pixel to the set ``hard``, capped at ``cap``: the set grown by one pixel in all eight
    directions, ``cap`` - 1 times."""
    h, w = hard.shape
    e0 = np.where(hard, 0, cap).astype(np.int64)
    grown = hard.copy()
    for d in range(1, cap):
        pad = np.zeros((h + 2, w + 2), dtype=bool)
        pad[1:-1, 1:-1] = grown
        nxt = np.zeros_like(grown)
        for dy in range(3):
            for dx in range(3):
                nxt |= pad[dy:dy + h, dx:dx + w]
        e0[nxt & ~grown] = d
        grown = nxt
    return e0


def weights(moving, h, w, grow, feather):
    """The (h, w) weight W of every pixel from the moving cells."""
    e0 = distance(hard_pixels(moving, h, w), grow + feather + 1)
    return np.where(e0 <= grow, 256, S.weight_of(np.maximum(e0 - grow, 1), feather)).astype(np.int64)


def dilated_mask(moving, h, w, grow):
    """The (h, w) uint8 mask "255 where e0 <= G": what the region rule is given to build the same plane."""
    return np.where(distance(hard_pixels(moving, h, w), grow + 1) <= grow, 255, 0).astype(np.uint8)


def tile_flags(W):
    """One flag per tile of the apply call: does any BYTE column of the tile belong to a pixel with W > 0."""
    h, w = W.shape
    tb, tr = APPLY_TILE
    per_byte = np.repeat(W > 0, 3, axis=1)
    ny, nx = -(-h // tr), -(-3 * w // tb)
    return np.array([[per_byte[y * tr:(y + 1) * tr, x * tb:(x + 1) * tb].any() for x in range(nx)] for y in range(ny)], dtype=np.uint8)


def build(state, frame, plate_state, det, rows, table=None, margin=8, tol=24, vote=8, hold=4, grow=8, feather=0, unknown=0, frame_index=0,
          n_frames=1, gate=None, cut=None):
    """One frame of the rule -> {"real", "header", "W" (None for a frame that is not real), "flags", "stats"}; ``state`` in place.
    ``table`` None: no class is excepted."""
    h, w = frame.shape[:2]
    tb, tr = APPLY_TILE
    if not (frame_index < max(int(n_frames), 0) and (gate is None or int(gate) != 0)):
        return {"real": False, "header": [h, w, feather, 0, 0, 1, 0, 0], "W": None,
                "flags": np.zeros((-(-h // tr), -(-3 * w // tb)), dtype=np.uint8), "stats": [0, 0, 0, 0]}
    table = np.zeros(1, dtype=np.uint8) if table is None else table
    fg = foreground(frame, plate_state, det, rows, table, margin, tol, unknown)
    moving = vote_hold(state, fg, vote, hold, cut)
    W = weights(moving, h, w, grow, feather)
    covered, full = RR.stats(W)
    return {"real": True, "header": [h, w, feather, covered, full, 1, 0, 0], "W": W, "flags": tile_flags(W), "moving": moving,
            "stats": [1, state[1], covered, full]}


def apply(current, source, W, mode=DEFAULT_MODE, size=None):
    """OUTPUT: a copy of ``current`` blended under W with R from ``source``, the untouched frame: the region rule's blend."""
    if W is None:
        return np.array(current, dtype=np.uint8)
    Wp = np.asarray(W)[:, :, None]
    C, Rep = np.asarray(current).astype(np.int64), R.replacement(np.asarray(source, dtype=np.uint8), mode, size).astype(np.int64)
    return np.where(Wp > 0, (Wp * Rep + (256 - Wp) * C + 128) >> 8, C).astype(np.uint8)


def summary_line(w, h, per_frame):
    """The line printed per frame size at the end of a list; ``per_frame``: the covered pixels of every frame of that size."""
    pct = [100.0 * c / (w * h) for c in per_frame]
    return "moving net %dx%d: %d frames, mean %.1f %% hidden, peak %.1f %%" % (w, h, len(pct), sum(pct) / max(len(pct), 1), max(pct + [0.0]))
