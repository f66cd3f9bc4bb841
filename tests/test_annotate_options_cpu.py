"""The options of annotate_video's entry points against the recording stub engine (no GPU): for every option, which keywords reach
``submit_batch`` through ``annotate_images``, ``annotate_stream`` and ``get_annotated_frame``, what is printed and which files are
written; which bad combination is refused by which entry point, with which words; and which keywords the command line hands on.

The expected values (tests/annotate_options_cases.py) are literals.  They were recorded by running this test's body against the code
as it was when every entry point took its options as some thirty keywords and checked them itself, so they pin that behaviour.

Only host read-backs are patched, to fixed values: ops.count_totals, ops.zone_totals, write_heatmaps, plate_summaries and
ops.redact_region_stats -- and torch.cuda.synchronize, which the heat and plate read-backs call and which needs a device."""
import contextlib
import io
import os
import types

import numpy as np
import pytest

from tests import annotate_options_cases as C
from tests.annotate_stub import MANAGER, frames, stub      # noqa: F401  (the recording stub engine)

pytest.importorskip("PIL.Image")

SIZES = [(8, 8)] * 5 + [(6, 8)] * 2                        # (h, w) per frame, as test_annotate_loop_cpu.py: A A A A A B B
RESIZE = (8, 16)
FILE_OUTPUTS = ("tracks_out",)                             # outputs the list entry points take as an open text file
PATH_OUTPUTS = ("heatmap_out", "counts_out", "zones_out", "plate_out", "reid_out", "moving_out")


@pytest.fixture
def readbacks(monkeypatch):
    """The host read-backs at the end of a list, fixed -> the paths ``write_heatmaps`` was asked for."""
    import torch
    from faster_rcnn_amd import annotate_video, ops
    heat_paths = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(ops, "count_totals", lambda state: {"totals": [(1, 2)] * 8, "events_dropped": 3})
    monkeypatch.setattr(ops, "zone_totals", lambda state: {"visitors": [4] * 8, "peak": [2] * 8, "stays": [2] * 8, "dwell": [9] * 8,
                                                           "events_dropped": 1})
    monkeypatch.setattr(annotate_video, "write_heatmaps", lambda path, states: heat_paths.append(os.path.basename(path)))
    monkeypatch.setattr(annotate_video, "plate_summaries", lambda states: {(8, 8, True): (5, 48, np.zeros((8, 8, 3), dtype=np.uint8)),
                                                                           (6, 8, True): (2, 12, np.zeros((6, 8, 3), dtype=np.uint8))})
    monkeypatch.setattr(ops, "redact_region_stats", lambda plane: {"covered": 6})
    return heat_paths


def _stated(options, d_out, single_frame=False):
    """The option set with its outputs made real: a path becomes one under ``d_out``, an open-file output a StringIO.
    ``single_frame``: ``get_annotated_frame``'s form -- its file outputs are open text files, ``moving_out`` a MovingLog, and it takes
    no ``heatmap_out`` / ``plate_out`` -> (the keywords, {output: StringIO})."""
    from faster_rcnn_amd import annotate_video
    stated, texts = dict(options), {}
    for name in options:
        if single_frame and name in ("heatmap_out", "plate_out"):
            del stated[name]
        elif single_frame and name == "moving_out":
            stated[name] = annotate_video.MovingLog(None)
        elif name in FILE_OUTPUTS or (single_frame and name in PATH_OUTPUTS):
            stated[name] = texts[name] = io.StringIO()
        elif name in PATH_OUTPUTS:
            stated[name] = os.path.join(d_out, options[name])
    return stated, texts


def _files(d_out, texts):
    """What a run left: {file name under ``d_out``: its text, None for a picture} and {output: the text written to its StringIO}."""
    left = {}
    for name in sorted(os.listdir(d_out)) if os.path.isdir(d_out) else ():
        with open(os.path.join(d_out, name), "rb") as f:
            left[name] = None if name.endswith(".png") else f.read().decode()
    left.update({name: text.getvalue() for name, text in texts.items()})
    return left


def _images(d_in, names, d_out, **opts):
    from faster_rcnn_amd import annotate_video
    annotate_video.annotate_images(MANAGER, None, d_in, d_out, names, *RESIZE, **opts)


def _stream(d_in, names, d_out, **opts):
    from faster_rcnn_amd import annotate_video
    annotate_video.annotate_stream(MANAGER, None, annotate_video.directory_frames(d_in, names), d_out, *RESIZE, **opts)


def _one_frame(**opts):
    from faster_rcnn_amd import annotate_video, shapes
    frame = np.zeros((8, 8, 3), dtype=np.uint8)
    img = shapes.InMemoryImage(data=frame, width=8, height=8)
    return annotate_video.get_annotated_frame(MANAGER, None, frame, img, *RESIZE, **opts)


def _draw_eager(redact=None, draw=True, track=None, **opts):
    from faster_rcnn_amd import annotate_video
    return annotate_video.draw_eager(np.zeros((8, 8, 3), dtype=np.uint8), [], MANAGER.class_mapping, redact, draw, track, **opts)


def list_run(run, eng, written, heat_paths, d_in, names, d_out, capsys, options):
    """One list through ``run`` -> what it did, as tests/annotate_options_cases.py records it."""
    os.makedirs(d_out)
    del eng.calls[:], eng.thresholds[:], eng.tickets[:], written[:], heat_paths[:]
    stated, texts = _stated(options, d_out)
    run(d_in, names, d_out, **stated)
    said = capsys.readouterr().out.replace(d_in + os.sep, "<in>/")
    assert all(t.collected and not t.slot.busy for t in eng.tickets)
    assert len({repr(c[3]) for c in eng.calls}) == 1           # every pass of a list takes the same keywords
    return {"passes": [c[:3] for c in eng.calls], "keywords": eng.calls[0][3], "thresholds": sorted(set(eng.thresholds)), "said": said,
            "frames": [n for n, _ in written], "heatmaps": list(heat_paths), "files": _files(d_out, texts)}


@pytest.mark.parametrize("name", list(C.OPTIONS))
def test_a_list_submits_prints_and_writes_what_it_did(stub, readbacks, tmp_path, capsys, name):
    eng, written, _ = stub
    d_in, names = frames(tmp_path, SIZES)
    got = {run.__name__: list_run(run, eng, written, readbacks, d_in, names, str(tmp_path / run.__name__), capsys, C.OPTIONS[name])
           for run in (_images, _stream)}
    want = dict(C.LISTS[name])
    frames_of = want.pop("frames")
    assert got["_images"] == dict(want, frames=frames_of[0])
    assert got["_stream"] == dict(want, frames=frames_of[1])


@pytest.mark.parametrize("name", [n for n in C.OPTIONS if n in C.ONE_FRAME])
def test_get_annotated_frame_makes_the_one_call(stub, readbacks, capsys, name):
    eng, _, _ = stub
    eng.payload = 7                                            # (what the frame is filled with)
    stated, texts = _stated(C.OPTIONS[name], "", single_frame=True)
    _one_frame(**stated)
    assert {"calls": eng.calls, "thresholds": eng.thresholds, "said": capsys.readouterr().out,
            "files": {k: t.getvalue() for k, t in texts.items()}} == C.ONE_FRAME[name]


@pytest.mark.parametrize("name", list(C.EAGER))
def test_the_eager_loop_detects_and_prints_per_frame(stub, readbacks, monkeypatch, tmp_path, capsys, name):
    """A foreign model: no engine, one ``voc_dets.get_dets`` per frame (here: no detections, so nothing reaches the device)."""
    from faster_rcnn_amd import annotate_video, voc_dets
    _, written, _ = stub
    asked = []
    monkeypatch.setattr(annotate_video, "_engine", lambda *a, **k: None)
    monkeypatch.setattr(voc_dets, "get_dets", lambda *a, **k: asked.append(sorted((k_, v) for k_, v in k.items())) or [])
    d_in, names = frames(tmp_path, SIZES[:2])
    _images(d_in, names, str(tmp_path / "out"), **C.OPTIONS[name])
    assert {"asked": asked, "said": capsys.readouterr().out.replace(d_in + os.sep, "<in>/"), "frames": [n for n, _ in written]} == C.EAGER[name]


def outcome(run, *args, **opts):
    """-> (exception type's name, its message) of a refused call, None of one that went through."""
    from faster_rcnn_amd._lib import FrcnnError
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            run(*args, **opts)
    except (ValueError, FrcnnError) as e:
        return type(e).__name__, str(e)
    return None


ENTRY_POINTS = {"annotate_images": _images, "annotate_stream": _stream, "get_annotated_frame": _one_frame, "draw_eager": _draw_eager}


@pytest.mark.parametrize("name", list(C.REFUSALS))
def test_a_bad_combination_is_refused_in_each_entry_point_s_words(stub, readbacks, tmp_path, name):
    """(An entry point that does not take one of the combination's keywords is not in its row.)"""
    eng, _, _ = stub
    eng.payload = 7
    d_in, names = frames(tmp_path, SIZES)
    for point, want in C.REFUSED[name].items():
        where = (d_in, names, str(tmp_path / point)) if point in ("annotate_images", "annotate_stream") else ()
        assert outcome(ENTRY_POINTS[point], *where, **C.REFUSALS[name]) == want, point


def test_an_unknown_keyword_is_a_type_error(stub, tmp_path):
    d_in, names = frames(tmp_path, SIZES[:1])
    for run, where in ((_images, (d_in, names, str(tmp_path / "a"))), (_stream, (d_in, names, str(tmp_path / "b"))), (_one_frame, ()), (_draw_eager, ())):
        with pytest.raises(TypeError):
            run(*where, track_motions=8)


def command_line(monkeypatch, tmp_path, line):
    """``annotate_video.main`` with the model loaders and the two list entry points replaced -> (the entry point called, its keywords:
    the models and every None left out -- None is every option's default --, an open file as "<file NAME>", a path under ``tmp_path`` as "<tmp>/...")."""
    from faster_rcnn_amd import annotate_video, det_util, resnet, y4m
    calls = []

    def plain(v):
        if isinstance(v, io.IOBase):
            return "<file %s>" % os.path.basename(v.name)
        if isinstance(v, y4m.Y4mWriter):
            return "<y4m writer %dx%d>" % (v.w, v.h)
        if isinstance(v, types.GeneratorType):
            return "<frames>"
        if isinstance(v, str):
            return v.replace(str(tmp_path), "<tmp>")
        return v

    def record(point, drop):
        def called(*args, **kwargs):
            calls.append((point, [plain(a) for a in args[drop:]], sorted((k, plain(v)) for k, v in kwargs.items() if k not in ("training_manager", "detector") and v is not None)))
        return called

    monkeypatch.setattr(annotate_video, "annotate_images", record("annotate_images", 2))
    monkeypatch.setattr(annotate_video, "annotate_stream", record("annotate_stream", 2))
    monkeypatch.setattr(resnet, "rpn_from_h5", lambda *a, **k: None)
    monkeypatch.setattr(resnet, "det_from_h5", lambda *a, **k: None)
    monkeypatch.setattr(det_util, "DetTrainingManager", lambda **k: None)
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", os.environ.get("GPU_MAX_HW_QUEUES", "8"))      # (main's setdefault then leaves no trace)
    if not (tmp_path / "in").exists():
        frames(tmp_path, SIZES[:1])
    annotate_video.main(["s3.h5", "s4.h5", str(tmp_path / "in")] + [a.replace("<tmp>", str(tmp_path)) for a in line])
    return calls


@pytest.mark.parametrize("name", list(C.COMMAND_LINES))
def test_the_command_line_hands_the_options_on(monkeypatch, tmp_path, name):
    assert command_line(monkeypatch, tmp_path, C.COMMAND_LINES[name]) == C.HANDED_ON[name]
