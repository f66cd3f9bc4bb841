"""The frames the huffman mode of the device PNG encoder is tested on (tests/test_png_huff_cpu.py runs the CPU restatement over them,
tests/test_png_huff_gpu.py holds the kernel to the restatement on them): the smallest at which each mechanism can go wrong."""
import numpy as np

from tests import png_huff_ref as R

TILE = R.TILE
ROWS = R.BAND_ROWS


def banded(h, w):
    """tests/test_png_gpu.py's pattern: flat bands with a green rectangle, what a drawn frame looks like."""
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([(x // 7 * 3) % 256, (y // 5 * 9) % 256, ((x + y) // 11 * 5) % 256], -1).astype(np.uint8)
    a[h // 5:h // 2, w // 6:w // 6 * 4] = (0, 255, 0)
    return a


def by_magnitude(k):
    """The k byte values of smallest |int8|: 0, 1, 255, 2, 254, ..."""
    return [(i + 1) // 2 if i % 2 else (256 - i // 2) % 256 for i in range(k)]


def ladder_band(counts, seed):
    """One band (ROWS rows) whose pixel bytes hold value by_magnitude(k)[i] counts[i] times, shuffled; the total is topped up to
    whole rows with the first value.  The commonest values are the smallest in magnitude, so filter None is the cheapest."""
    total = -(-sum(counts) // (3 * ROWS)) * 3 * ROWS
    counts = [counts[0] + total - sum(counts)] + list(counts[1:])
    vals = np.repeat(np.array(by_magnitude(len(counts)), np.uint8), counts)
    rs = np.random.RandomState(seed)
    rs.shuffle(vals)
    rows = vals.reshape(ROWS, -1)
    # no byte of the filtered stream (a zero in front of every row) four times in a row: three repeats would become a match and take
    # the counts off the ladder.  A byte inside such a run changes places with a random one until none is left.
    while True:
        stream = np.concatenate([np.zeros((ROWS, 1), np.uint8), rows], axis=1).reshape(-1)
        same = stream[1:] == stream[:-1]
        hit = np.flatnonzero(same[2:] & same[1:-1] & same[:-2]) + 2         # stream[hit - 2 .. hit + 1] are equal
        if not len(hit):
            return rows.reshape(ROWS, -1, 3)
        r, c = divmod(int(hit[0]) if int(hit[0]) % (rows.shape[1] + 1) else int(hit[0]) - 1, rows.shape[1] + 1)     # (a pixel byte of the run)
        r2, c2 = rs.randint(ROWS), rs.randint(rows.shape[1])
        rows[r, c - 1], rows[r2, c2] = rows[r2, c2], rows[r, c - 1]


def fibonacci_band():
    """Byte counts 1, 2, 4, 7, 12, ... (each the sum of the two before it plus one: a Fibonacci ladder that a stray symbol of count 1
    cannot fold) over 16 values, 6746 bytes, the commonest first: with end-of-block the unlimited tree is 16 deep."""
    ladder = [1, 2]
    while len(ladder) < 16:
        ladder.append(ladder[-1] + ladder[-2] + 1)
    return ladder_band(ladder[::-1], 5)


# symbols per code length of a literal/length code whose LENGTHS, counted, form a ladder of their own (1, 1, 2, 3, 5, 8, 13, 28, 55 and
# the unused symbols): the code-length code's unlimited tree is deeper than 7
CL_LADDER = {3: 5, 4: 3, 5: 2, 7: 1, 8: 8, 9: 13, 10: 55, 12: 28}


def code_length_ladder_band():
    """A value meant for length l occurs 2^(12 - l) times (4096 symbols with end-of-block, which is one of the 28 at length 12)."""
    counts = [1 << (12 - l) for l in sorted(CL_LADDER) for _ in range(CL_LADDER[l])][:-1]
    counts[0] -= ROWS + 7                       # (the filter bytes are zeros too; 4080 pixel bytes make whole rows)
    return ladder_band(counts, 1)


def five_filters():
    """Rows that make each filter the cheapest at least once: noise (None), a flat row under a different one (Sub), a repeated row
    (Up), flat rows with some noise (Average) and smooth ramps in both directions (Paeth)."""
    rs = np.random.RandomState(4)
    w = 96
    x = np.arange(w)
    rows = []
    noise = rs.randint(0, 256, (w, 3))
    rows += [np.where(rs.rand(w, 3) < 0.5, rs.randint(0, 6, (w, 3)), rs.randint(250, 256, (w, 3)))]          # small both ways: None
    rows += [np.full((w, 3), 90), np.full((w, 3), 200)]                                                    # flat, new value: Sub
    rows += [noise, noise, noise]                                                                          # repeated: Up
    rows += [100 + rs.randint(-20, 21, (w, 3)) for _ in range(4)]                                          # flat with some noise: Average
    for y in range(10):                                                                                    # a smooth 2-D ramp
        rows.append(np.stack([(3 * x + 5 * y) % 256, (2 * x + 7 * y + 40) % 256, (x * x // 64 + 3 * y * y) % 256], -1))
    for y in range(6):                                                                                     # a steep one with an edge
        rows.append(np.stack([np.where(x < 40 + y, 17 * y, 255 - 9 * y), (x * 11 + y * 13) % 256, np.minimum(x * (y + 1), 255)], -1))
    return np.stack(rows).astype(np.uint8)


def cases():
    rs = np.random.RandomState(3)
    wide = (TILE + 200) // 3                                                # a row that spans two tiles of the tokeniser
    long_band = 65535 // (3 * ROWS) + 40                                    # ROWS rows of it pass 65535 filtered bytes
    return {
        "1x1": np.array([[[1, 2, 3]]], np.uint8),
        "1x7": rs.randint(0, 256, (1, 7, 3)).astype(np.uint8),
        "7x1": rs.randint(0, 256, (7, 1, 3)).astype(np.uint8),
        "banded_plus": banded(12 * ROWS + 1, 131),
        "banded_minus": banded(12 * ROWS - 1, 131),
        "banded_two_tiles": banded(ROWS + 3, wide),
        "noise_37x53": rs.randint(0, 256, (37, 53, 3)).astype(np.uint8),
        "noise_long_band": rs.randint(0, 256, (ROWS + 1, long_band, 3)).astype(np.uint8),
        "flat_64x100": np.full((64, 100, 3), 77, np.uint8),
        "fibonacci_band": fibonacci_band(),
        "code_length_ladder_band": code_length_ladder_band(),
        "five_filters": five_filters(),
    }


CASES = cases()
