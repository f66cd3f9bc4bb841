"""A recording stub of entry.DetectionEntry for the tests of annotate_video's host side (no GPU): test_annotate_loop_cpu.py pins the
loop with it, test_annotate_options_cpu.py the options."""
import os
import types

import numpy as np
import pytest

MANAGER = types.SimpleNamespace(class_mapping={"bg": 0, "car": 1})
# what every frame's result carries behind its payload: the marks of a frame in which nothing happened
MARKS = {"crossings": [], "zones": {"occupancy": [], "events": []}, "reid": [], "moving": {"cells": 0, "covered": 0}}


class _Event:
    def __init__(self):
        self.synced = 0

    def synchronize(self):
        self.synced += 1


class _States:
    """The engine's ``edit_states`` as the end-of-list read-backs ask for them: no heat map, no plate, an empty region plane."""
    heat, plate = {}, {}

    def region_plane(self, h, w, option):
        from faster_rcnn_amd import _lib
        plane = np.zeros(4 * _lib.REDACT_REGION_HEAD_WORDS + 2 * h * w, dtype=np.uint8)
        plane[:8].view(np.int32)[:] = (h, w)
        return plane


class StubEngine:
    """What the loop asks of entry.DetectionEntry.  A frame's geometry is its resized (h, w); a pass returns one (0, [], ``payload``,
    MARKS) per source frame, a delayed pass (``track_lookback`` / ``track_backtrack``) those of the delayed submit before it.  ``calls``:
    (images, source frames, batch, the other keyword arguments sorted) per submit_batch, ``thresholds``: its det_threshold.  The
    ``*_reset`` / ``*_state`` methods do nothing: there is no state."""
    batch, in_flight = 4, 2
    payload = b"x"
    edit_states = _States()

    def __init__(self):
        self.calls, self.thresholds, self.tickets, self._held = [], [], [], 0

    def geometry_of(self, pixels):
        return pixels[1:]

    def host_pixels(self, resized):
        return ("pixels", resized.height, resized.width)

    def submit_batch(self, images, resize_ratios, det_threshold, pixels, batch=None, **kwargs):
        assert len(images) == len(resize_ratios)
        # (None is submit_batch's default for every option: stating it and leaving it out are the same pass)
        self.calls.append((len(images), len(pixels), batch, sorted((k, v) for k, v in kwargs.items() if v is not None)))
        self.thresholds.append(det_threshold)
        frames = len(pixels)
        if "track_lookback" in kwargs or "track_backtrack" in kwargs:
            frames, self._held = self._held, len(pixels)
        ticket = types.SimpleNamespace(frames=frames, collected=False, slot=types.SimpleNamespace(event=_Event(), busy=True))
        self.tickets.append(ticket)
        return ticket

    def collect_batch(self, ticket):
        ticket.collected, ticket.slot.busy = True, False
        return [(0, [], self.payload, MARKS)] * ticket.frames

    def _nothing(self, *a, **k):
        return None

    track_reset = heat_reset = plate_reset = moving_reset = count_reset = zone_reset = count_state = zone_state = _nothing


@pytest.fixture
def stub(monkeypatch):
    """-> (the stub engine ``annotate_video._engine`` now returns, the (name, payload) list the file writers append to, the
    ``reset_tracks`` calls).  One writer thread: the files are then written in the order the loop hands them over."""
    from faster_rcnn_amd import annotate_video
    eng, written, resets = StubEngine(), [], []
    monkeypatch.setattr(annotate_video, "_engine", lambda *a, **k: eng)
    monkeypatch.setattr(annotate_video, "reset_tracks", lambda *a, **k: resets.append(a))
    monkeypatch.setattr(annotate_video, "WRITE_THREADS", 1)
    for name in ("_write_png", "_write_jpg", "_write_bytes"):
        monkeypatch.setattr(annotate_video, name, lambda path, data, *a: written.append((os.path.basename(path), data)))
    return eng, written, resets


def frames(tmp_path, sizes):
    """One grey PNG per (h, w) of ``sizes`` in a new directory -> (the directory, the names)."""
    from PIL import Image
    d_in = tmp_path / "in"
    d_in.mkdir()
    names = ["f%02d.png" % i for i in range(len(sizes))]
    for i, (name, (h, w)) in enumerate(zip(names, sizes)):
        Image.fromarray(np.full((h, w, 3), 10 * i, dtype=np.uint8)).save(str(d_in / name))
    return str(d_in), names
