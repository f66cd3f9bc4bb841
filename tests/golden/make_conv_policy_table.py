#!/usr/bin/env python3
"""Records tests/golden/conv_policy_table.npz: the library's launch-policy answers over the descriptor grid of
tests/test_conv_policy_table_cpu.py.  Run it against a build of the commit whose policy is the reference (no GPU needed):
    python -m faster_rcnn_amd.build && python tests/golden/make_conv_policy_table.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from faster_rcnn_amd import _lib  # noqa: E402
from tests.test_conv_policy_table_cpu import CODES, COLUMNS, KNOBS, TABLE, grid, grid_digest, query  # noqa: E402

if __name__ == "__main__":
    assert not any(k in os.environ for k in KNOBS), "unset the FRCNN_* policy knobs first"
    descs = grid()
    table = query(_lib.load(), descs)
    # column-major, tile / engine codes as int8: the file stays small.  The grid itself is rebuilt by the test; only its digest is kept.
    codes = table[:, :len(CODES)]
    assert codes.min() >= -128 and codes.max() < 128
    np.savez_compressed(TABLE, codes=codes.T.astype(np.int8), bytes=table[:, len(CODES):].T.copy(), columns=np.array(COLUMNS),
                        grid_sha256=np.array(grid_digest(descs)))
    print(TABLE, descs.shape, os.path.getsize(TABLE), "bytes")
