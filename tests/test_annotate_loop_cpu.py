"""The pipelined loop of annotate_video.annotate_images / annotate_stream against a recording stub engine (no GPU): which passes are
submitted, with which arguments and in which order, where the flush submits of the delayed passes fall, what is printed, what is
written under which name -- and that the two entry points agree on all of it.  Seven 8-pixel frames: five of one size (a full pass of
four and a short group of one), then two of another (a half-full group: one padded pass).

The expected call logs below are literals.  They were recorded by running this test's body against the two SEPARATE loops the entry
points had before they shared one driver, so they pin that behaviour, not the driver's."""
import os
import threading

import pytest

from tests.annotate_stub import MANAGER, frames as _frames, stub      # noqa: F401  (the recording stub engine)

PilImage = pytest.importorskip("PIL.Image")

SIZES = [(8, 8)] * 5 + [(6, 8)] * 2                        # (h, w) per frame: A A A A A B B
RESIZE = (8, 16)
TRACK = (30, 8, 0)
MOTION = dict(track=TRACK, track_motion=8)
OPTIONS = {"plain": {},
           "lookback": dict(MOTION, track_lookback=2),
           "interval": dict(MOTION, detect_every=2),
           "interval_backtrack": dict(MOTION, detect_every=2, track_backtrack=2)}
_T = [("annotate", True), ("track", TRACK), ("track_motion", 8)]
_LB, _EV, _BT = ("track_lookback", 2), ("detect_every", 2), ("track_backtrack", 2)
# (images, source frames, batch, the other keyword arguments sorted) per submit_batch call, in order
EXPECTED_CALLS = {
    # A A A A: a full pass; A: a short group, one one-frame pass; B B: half a pass, one padded pass
    "plain": [(4, 4, 4, [("annotate", True)]), (1, 1, 1, [("annotate", True)]), (2, 2, 4, [("annotate", True)])],
    # full passes only; a flush (no images) where the geometry changes and at the end
    "lookback": [(4, 4, 4, sorted(_T + [_LB])), (1, 1, 4, sorted(_T + [_LB])), (0, 0, 4, sorted(_T + [_LB])), (2, 2, 4, sorted(_T + [_LB])),
                 (0, 0, 4, sorted(_T + [_LB]))],
    # A x 5: three key frames, over half a pass: one pass of four images; B B: one key frame: a one-image pass of K frames
    "interval": [(3, 5, 4, sorted(_T + [_EV])), (1, 2, 1, sorted(_T + [_EV]))],
    # full passes only, and the flushes of a delayed pass
    "interval_backtrack": [(3, 5, 4, sorted(_T + [_EV, _BT])), (0, 0, 4, sorted(_T + [_EV, _BT])), (1, 2, 4, sorted(_T + [_EV, _BT])),
                           (0, 0, 4, sorted(_T + [_EV, _BT]))],
}


def _images(d_in, names, d_out, **opts):
    from faster_rcnn_amd import annotate_video
    annotate_video.annotate_images(MANAGER, None, d_in, d_out, names, *RESIZE, **opts)


def _stream(d_in, names, d_out, **opts):
    from faster_rcnn_amd import annotate_video
    annotate_video.annotate_stream(MANAGER, None, annotate_video.directory_frames(d_in, names), d_out, *RESIZE, **opts)


@pytest.mark.parametrize("options", list(OPTIONS))
def test_both_entry_points_submit_print_and_write_the_same(stub, tmp_path, capsys, options):
    eng, written, resets = stub
    d_in, names = _frames(tmp_path, SIZES)
    said = "".join("processing %s\nnum rois: 0\n" % os.path.join(d_in, n) for n in names)
    logs = []
    for run, out_names in ((_images, names), (_stream, ["frame_%06d.png" % i for i in range(len(names))])):
        del eng.calls[:], eng.thresholds[:], eng.tickets[:], written[:], resets[:]
        run(d_in, names, str(tmp_path / run.__name__), **OPTIONS[options])
        print_out = capsys.readouterr().out
        assert eng.calls == EXPECTED_CALLS[options] and eng.thresholds == [0.0] * len(eng.calls)
        assert print_out == said
        assert written == [(n, b"x") for n in out_names]
        assert len(resets) == (1 if "track" in OPTIONS[options] else 0)
        assert all(t.collected and not t.slot.busy for t in eng.tickets)
        logs.append(list(eng.calls))
    assert logs[0] == logs[1]


@pytest.mark.parametrize("run", [_images, _stream])
def test_a_failing_load_leaves_no_busy_slot_and_no_thread(stub, tmp_path, monkeypatch, run):
    """Frames A B A, then a fourth whose load raises: the exception comes out, the pass still in the window is synchronised and its slot
    released, and both executors are shut down."""
    from faster_rcnn_amd import annotate_video
    eng, written, _ = stub
    d_in, names = _frames(tmp_path, [(8, 8), (6, 8), (8, 8), (8, 8), (8, 8)])
    load = annotate_video._load_frame

    def failing(path, *a):
        if path.endswith(names[3]):
            raise ValueError("frame 3 is broken")
        return load(path, *a)

    monkeypatch.setattr(annotate_video, "_load_frame", failing)
    threads = threading.active_count()
    with pytest.raises(ValueError, match="frame 3 is broken"):
        run(d_in, names, str(tmp_path / "out"))
    assert eng.calls == [(1, 1, 1, [("annotate", True)])] * 2 and eng.thresholds == [0.0, 0.0]      # A, then B: one-frame passes; the second A never got there
    assert [t.collected for t in eng.tickets] == [True, False]      # (two in flight: the first was collected when the second went in)
    assert eng.tickets[1].slot.event.synced == 1 and not any(t.slot.busy for t in eng.tickets)
    assert threading.active_count() == threads
