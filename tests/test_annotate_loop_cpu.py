"""The pipelined loop of annotate_video.annotate_images / annotate_stream against a recording stub engine (no GPU): which passes are
submitted, with which arguments and in which order, where the flush submits of the delayed passes fall, what is printed, what is
written under which name -- and that the two entry points agree on all of it.  Seven 8-pixel frames: five of one size (a full pass of
four and a short group of one), then two of another (a half-full group: one padded pass).

The expected call logs below are literals.  They were recorded by running this test's body against the two SEPARATE loops the entry
points had before they shared one driver, so they pin that behaviour, not the driver's."""
import os
import threading
import types

import numpy as np
import pytest

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


class _Event:
    def __init__(self):
        self.synced = 0

    def synchronize(self):
        self.synced += 1


class _StubEngine:
    """What the loop asks of entry.DetectionEntry.  A frame's geometry is its resized (h, w); a pass returns one (0, [], b"x") per
    source frame, a delayed pass (``track_lookback`` / ``track_backtrack``) those of the delayed submit before it."""
    batch, in_flight = 4, 2

    def __init__(self):
        self.calls, self.tickets, self._held = [], [], 0

    def geometry_of(self, pixels):
        return pixels[1:]

    def host_pixels(self, resized):
        return ("pixels", resized.height, resized.width)

    def submit_batch(self, images, resize_ratios, det_threshold, pixels, batch=None, **kwargs):
        assert len(images) == len(resize_ratios) and det_threshold == 0.0
        # (None is submit_batch's default for every option: stating it and leaving it out are the same pass)
        self.calls.append((len(images), len(pixels), batch, sorted((k, v) for k, v in kwargs.items() if v is not None)))
        frames = len(pixels)
        if "track_lookback" in kwargs or "track_backtrack" in kwargs:
            frames, self._held = self._held, len(pixels)
        ticket = types.SimpleNamespace(frames=frames, collected=False, slot=types.SimpleNamespace(event=_Event(), busy=True))
        self.tickets.append(ticket)
        return ticket

    def collect_batch(self, ticket):
        ticket.collected, ticket.slot.busy = True, False
        return [(0, [], b"x")] * ticket.frames


@pytest.fixture
def stub(monkeypatch):
    """-> (the stub engine ``annotate_video._engine`` now returns, the (name, payload) list the file writers append to, the
    ``reset_tracks`` calls).  One writer thread: the files are then written in the order the loop hands them over."""
    from faster_rcnn_amd import annotate_video
    eng, written, resets = _StubEngine(), [], []
    monkeypatch.setattr(annotate_video, "_engine", lambda *a, **k: eng)
    monkeypatch.setattr(annotate_video, "reset_tracks", lambda *a, **k: resets.append(a))
    monkeypatch.setattr(annotate_video, "WRITE_THREADS", 1)
    for name in ("_write_png", "_write_jpg", "_write_bytes"):
        monkeypatch.setattr(annotate_video, name, lambda path, data, *a: written.append((os.path.basename(path), data)))
    return eng, written, resets


def _frames(tmp_path, sizes):
    d_in = tmp_path / "in"
    d_in.mkdir()
    names = ["f%02d.png" % i for i in range(len(sizes))]
    for i, (name, (h, w)) in enumerate(zip(names, sizes)):
        PilImage.fromarray(np.full((h, w, 3), 10 * i, dtype=np.uint8)).save(str(d_in / name))
    return str(d_in), names


MANAGER = types.SimpleNamespace(class_mapping={"bg": 0, "car": 1})


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
        del eng.calls[:], eng.tickets[:], written[:], resets[:]
        run(d_in, names, str(tmp_path / run.__name__), **OPTIONS[options])
        print_out = capsys.readouterr().out
        assert eng.calls == EXPECTED_CALLS[options]
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
    assert eng.calls == [(1, 1, 1, [("annotate", True)])] * 2      # A, then B: one-frame passes; the second A never got there
    assert [t.collected for t in eng.tickets] == [True, False]      # (two in flight: the first was collected when the second went in)
    assert eng.tickets[1].slot.event.synced == 1 and not any(t.slot.busy for t in eng.tickets)
    assert threading.active_count() == threads
