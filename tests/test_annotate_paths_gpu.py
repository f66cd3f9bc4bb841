"""annotate_video.annotate_images against annotate_stream(directory_frames(...)) on the same frame files: the two entry points share
one loop, so the same frames must come out as the same files, with the same printed lines, through the same captured passes.  Seven
frames -- five of 96x128, then two of 128x96 -- at four images per pass: the smallest list that reaches a full pass, a one-frame pass,
a padded pass and a change of geometry."""
import os

import numpy as np
import pytest

from tests import png_dec_cases as P
from tests.test_png_entry_gpu import f32_models, quiet      # noqa: F401  (the small f32 models)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
PilImage = pytest.importorskip("PIL.Image")

RESIZE = (320, 540)
SIZES = [(96, 128)] * 5 + [(128, 96)] * 2                    # (h, w) per frame


def _files(d):
    out = []
    for name in sorted(os.listdir(d)):
        with open(os.path.join(d, name), "rb") as f:
            out.append((name, f.read()))
    return out


def test_images_and_stream_write_the_same_files(f32_models, tmp_path):
    from faster_rcnn_amd import annotate_video, entry
    mgr, det, _ = f32_models
    d_in = tmp_path / "in"
    d_in.mkdir()
    names = ["%06d.png" % k for k in range(len(SIZES))]
    for k, (name, (h, w)) in enumerate(zip(names, SIZES)):
        PilImage.fromarray(np.ascontiguousarray(P.photo()[3 * k:3 * k + h, 2 * k:2 * k + w])).save(str(d_in / name))
    eng = entry.for_models(mgr, det, 64, 16, in_flight=entry.default_in_flight("f32"))
    for encoder in ("host", "device"):
        d_files, d_stream = str(tmp_path / ("files_" + encoder)), str(tmp_path / ("stream_" + encoder))
        _, text = quiet(annotate_video.annotate_images, mgr, det, str(d_in), d_files, names, *RESIZE, png_encoder=encoder)
        captures = eng.cache.captures
        _, said = quiet(annotate_video.annotate_stream, mgr, det, annotate_video.directory_frames(str(d_in), names), d_stream, *RESIZE,
                        png_encoder=encoder)
        assert eng.cache.captures == captures, encoder               # the same passes: nothing captured anew
        assert said == text and "{'bbox'" in said, encoder           # (both label a frame by its path)
        files, stream = _files(d_files), _files(d_stream)
        assert [n for n, _ in files] == names and [n for n, _ in stream] == ["frame_%06d.png" % k for k in range(len(names))]
        assert [b for _, b in files] == [b for _, b in stream], encoder
    batches = {sl.batch for v in eng.cache._slots.values() for sl in v if sl.annotate}
    assert batches >= {4, 1}                                         # the full and the padded pass of four, the one-frame pass
