"""The frame-editing chain of annotate_video, stated once: ``EditStates`` owns what lives across passes for one set of
classes, ``EditChain`` makes the calls of one pass -- a captured pass of the detection entry (entry.DetectionEntry._exact_pass) and the
one-frame eager call of a foreign model (annotate_video.draw_eager) alike."""
import torch

from . import _lib, ops
from ._lib import FrcnnError


def _made(table, key, make):
    v = table.get(key)
    if v is None:
        v = table[key] = make()
    return v


class EditStates:
    """The device state of the editing rules for the classes ``class_names`` (index = class index), each piece made on first use: a
    tracker of ``track_capacity`` slots, trail, count and zone states of ``trail_capacity`` entries, a re-identify state of twice the
    tracker's slots (256 at most).  The pointers of all of them are in the captured graphs that use them: nothing here is ever replaced,
    only zeroed by the resets (on the current stream)."""

    def __init__(self, class_names, track_capacity, trail_capacity):
        self.class_names, self.track_capacity, self.trail_capacity = list(class_names), int(track_capacity), int(trail_capacity)
        self._tracker = self._count = self._zone = self._one = self._reid = None
        self.motion = {}                                 # (h, w) of the source frames -> ops.track_motion_state
        self.lookback = {}                               # (h, w, F) -> (ops.track_lookback_state: the frames tracked but not yet emitted, its back)
        self.trails = {}                                 # length N -> ops.track_trails_state
        self.heat = {}                                   # (h, w) of the source frames -> ops.heat_state
        self.plate = {}                                  # (h, w, rgb) of the source frames -> ops.plate_state
        self.region = {}                                 # (h, w) of the source frames + the option's areas and feather -> ops.redact_region_plane
        self.moving = {}                                 # (h, w, rgb) of the source frames -> ops.redact_moving_state
        self._annotate, self._redact, self._track, self._track_remove = {}, {}, {}, {}

    def tracker(self):
        """The ONE tracker state (device int32, ops.track_state)."""
        if self._tracker is None:
            self._tracker = ops.track_state(self.track_capacity)
        return self._tracker

    def one_frame(self):
        """A device word that says 1: the ``n_frames`` of a call over one real frame."""
        if self._one is None:
            self._one = torch.ones(1, dtype=torch.int32, device="cuda")
        return self._one

    def motion_state(self, h, w):
        """The motion state for source frames of (h, w): the calls with a motion step keep their last frame in it.  A sequence that
        changes its frame size has no reference on the first frame of the new size: the header of the new size's state does not carry
        the tracker's frame count."""
        return _made(self.motion, (int(h), int(w)), lambda: ops.track_motion_state(h, w))

    def lookback_window(self, h, w, F, rows):
        """-> (the look-back window for calls of F source frames of (h, w) whose packed buffers have ``rows`` rows, its ``back``: the
        tracker's capacity where the rows leave room)."""
        def make():
            cap = ops.track_capacity(self.tracker())
            back = min(cap, _lib.REDACT_MAX_ROWS - rows - cap)
            if back < 1:
                raise FrcnnError("track_lookback=: %d rows and %d tracks leave no room for back-filled rows (at most %d rows in all)"
                                 % (rows, cap, _lib.REDACT_MAX_ROWS))
            return ops.track_lookback_state(F, h, w, rows, cap, back), back
        return _made(self.lookback, (int(h), int(w), int(F)), make)

    def trails_state(self, length):
        """The trail state for trails of ``length`` points, beside the tracker state."""
        return _made(self.trails, int(length), lambda: ops.track_trails_state(self.trail_capacity, length))

    def count_state(self):
        """The ONE count state (device int32, ops.count_state; ``ops.count_totals`` reads it)."""
        if self._count is None:
            self._count = ops.count_state(self.trail_capacity)
        return self._count

    def zone_state(self):
        """The ONE zone state (device int32, ops.zone_state; ``ops.zone_totals`` reads it), sized like the count state."""
        if self._zone is None:
            self._zone = ops.zone_state(self.trail_capacity)
        return self._zone

    def reid_state(self):
        """The ONE re-identify state (device int32, ops.track_reid_state; ``ops.track_reid_totals`` reads it): 2 * ``track_capacity``
        entries, 256 at most -- the tracks there are and as many that are gone."""
        if self._reid is None:
            self._reid = ops.track_reid_state(min(2 * self.track_capacity, ops.TRACK_REID_MAX))
        return self._reid

    def heat_state(self, h, w):
        """The heat state for source frames of (h, w): one per size, whatever the other options of the calls that heat it."""
        return _made(self.heat, (int(h), int(w)), lambda: ops.heat_state(h, w))

    def plate_state(self, h, w, rgb):
        """The plate state for source frames of (h, w) whose bytes are R, G, B (``rgb``) or B, G, R: one per size and channel order --
        the plate is kept in the frames' own byte order --, whatever the other options of the calls that learn it."""
        return _made(self.plate, (int(h), int(w), bool(rgb)), lambda: ops.plate_state(h, w))

    def region_plane(self, h, w, option):
        """The plane of the region option ``option`` (ops.redact_region_option's form) for source frames of (h, w), built on first use
        on the current stream: one per size and (polygons, mask, feather) -- the mode and the size are not the plane's."""
        regions, mask_digest, _, _, feather = ops.redact_region_key(option)
        return _made(self.region, (int(h), int(w), regions, mask_digest, feather), lambda: ops.redact_region_plane(h, w, option))

    def moving_state(self, h, w, rgb):
        """The moving state (DESIGN §8 "Moving rule") for source frames of (h, w) in the channel order ``rgb``: one per size and channel
        order, beside the plate state it is compared with, whatever the other options of the calls that advance it."""
        return _made(self.moving, (int(h), int(w), bool(rgb)), lambda: ops.redact_moving_state(h, w))

    def annotate_tables(self, draw=True):
        """The drawing tables of ops.annotate_u8 (uploaded once).  ``draw`` False: the same tables with no drawable class -- the drawing
        step of a chain that only redacts paints nothing, with no branch in the chain."""
        names = self.class_names
        return _made(self._annotate, bool(draw), lambda: ops.annotate_tables(names) if draw else ops.annotate_tables(names, skip=tuple(names)))

    def redact_table(self, classes):
        """The class table of ops.redact_u8 (and of the heat and count updates) for ``classes``, "all" or a tuple of names."""
        return _made(self._redact, classes, lambda: ops.redact_table(self.class_names, classes))

    def track_table(self, redact_classes=None, remove_classes=None):
        """The class table of ops.track_update: the classes the drawing rule draws united with ``redact_classes`` and with
        ``remove_classes``.  (The tables of a chain that removes are kept apart: a key without ``remove_classes`` is what it was.)"""
        def make():
            names = self.class_names
            chosen = [n for n in names if n and n != "bg" and n not in ops.ANNOTATE_SKIP]
            for classes in (redact_classes, remove_classes):
                if classes is not None:
                    chosen += [n for n in ops.redact_class_list(names, classes) if n not in chosen]
            return ops.track_table(names, chosen)
        if remove_classes is None:
            return _made(self._track, redact_classes, make)
        return _made(self._track_remove, (redact_classes, remove_classes), make)

    def reset_tracks(self):
        """Forget every track: the ids end, and what was counted stays counted."""
        ops.track_reset(self.tracker())
        for mstate in self.motion.values():              # ... and no frame is the one in front of the next
            ops.track_motion_reset(mstate)
        for window, _ in self.lookback.values():         # ... and no frame waits to be emitted
            ops.track_lookback_reset(window)
        for trails in self.trails.values():              # ... and no path has begun
            ops.track_reset(trails)
        if self._count is not None:                      # ... and no id waits for its next step; what was counted stays
            ops.count_reset(self._count, keep_totals=True)
        if self._zone is not None:                       # ... and nobody is inside: no event is made, an open stay is not counted
            ops.zone_reset(self._zone, keep_totals=True)
        self.reset_reid()                                # ... and no look is remembered: the tracker's ids start over

    def reset_reid(self):
        """Forget every look: an object that returns is a new id.  (The tracker's own ids go on.)"""
        if self._reid is not None:
            ops.track_reid_reset(self._reid)

    def reset_heat(self):
        """A cold map for every size."""
        for state in self.heat.values():
            ops.heat_reset(state)

    def reset_plate(self):
        """An empty plate for every size and channel order."""
        for state in self.plate.values():
            ops.plate_reset(state)

    def reset_moving(self):
        """No cell held, for every size and channel order.  (The plate the net compares with is ``reset_plate``'s.)"""
        for state in self.moving.values():
            ops.redact_moving_reset(state)

    def reset_counts(self):
        """Zero totals and no entries."""
        if self._count is not None:
            ops.count_reset(self._count)

    def reset_zones(self):
        """Zero totals and no entries."""
        if self._zone is not None:
            ops.zone_reset(self._zone)


class EditChain:
    """The calls that edit the F source frames of one pass, and their workspaces.  THE ORDER, which every caller gets from
    here and nowhere else:

    ``update``, once per pass, behind the post-process and in front of every edit (the frames are still as they were uploaded):
      1. ONE tracker call over the pass's frames -- ops.track_update_cut with ``track_scene_cut``, else ops.track_update_interval with
         ``detect_every``, else ops.track_update_motion with ``track_motion``, else ops.track_update -> ``track_out``;
     1b. with ``track_reid``: ops.track_reid_update on ``track_out`` and the pass's frames (with ``track_scene_cut`` the frames' cut words
         empty its table) -> ``reid_out``, ``reid_lists``: copies of the tracked buffers in which a track that returns has its old id.
         ``tracked`` is ``reid_out`` from here on: every step below, and the host's copy, sees those ids and no other;
      2. a delayed pass: ops.track_backtrack, or ops.track_lookback: the frames and their tracked buffers join the window, and the
         frames of the pass BEFORE come out in ``lb_out`` = (frames, widened tracked buffers, their count).  Everything behind this
         point reads the EMITTED buffers and the emitted count as its ``n_frames`` word, gated by the pass's own count (a warm-up run, 0
         frames, emits what the window holds once more, and those are no new frames): ``tracked``, ``n_frames``, ``gate``;
      3. ops.track_trails_update -> ``trail_lists``;
      4. ops.count_update -> ``count_lists``; with ``track_reid`` its expire is min(max(expire, keep), 4095), so that "once per id, line
         and direction" outlives the gap an id returns over (trails and zones keep theirs: a zone entry that lingers still occupies);
      5. ops.zone_update -> ``zone_lists``: the same ``tracked`` / ``n_frames`` / ``gate``, so a delayed pass counts in emitted order.
    ``edit``, once per frame, on ``rows(i)`` -- the frame's emitted buffer, else its tracked buffer, else its packed detections:
     5b. ops.plate_update, on the frame NO edit has touched: every row blocks, the held and back-filled ones too, whatever its class;
         with ``track_scene_cut`` the frame's cut word empties the plate first;
    5b2. ops.redact_moving_build, right behind the plate update and on that same untouched frame (DESIGN §8 "Moving rule"): the frame
         against the plate as step 5b left it becomes the pass's moving plane and the frame's stats.  A chain with ``redact_moving``
         but without ``remove`` still runs step 5b, with the option's (S, T, M), and runs no fill;
     5c. ops.redact_region_prepare, on that same untouched frame: what will replace the static areas of ``redact_region`` (DESIGN §8
         "Region rule") is a function of the source frame alone, in a workspace of its own (its mode need not be the redaction's);
    5c2. ops.redact_region_prepare once more, with the moving plane, into a workspace of its own;
      6. ops.redact_u8: every tracked row, the held ones too; with ``redact_shape`` ops.redact_shaped_u8 in its place (DESIGN §8 "Shape
         rule"), and nowhere else: the plate steps on either side of it keep their rectangles;
     6b. ops.plate_fill_u8, over the redaction: the rows of the remove classes become the plate.  Where the plate is not known yet
         the redaction shows, if the chain redacts all the remove classes (``keep_unknown``); else black;
     6c. ops.redact_region_apply_u8, over the plate fill: a remove box over a static area cannot put learned background back into
         it, and everything drawn below stays legible on top of it;
     6d. ops.redact_region_apply_u8 with the moving plane, behind 6c and under everything drawn.  One plane and one workspace serve
         the frames of a pass, which are edited one after another; ``moving_stats`` is [F][4];
      7. ops.heat_update (the live rows) and ops.heat_draw_u8;
      8. ops.zone_draw_u8, unless nothing is drawn: a tinted area lies under every line;
      9. ops.track_trails_draw_u8;
     10. ops.count_draw_u8, unless nothing is drawn;
     11. ops.annotate_u8: the live rows with their ids; with the no-draw tables when nothing is drawn.
    With ``out_size`` the scale step follows (12. ops.downscale_u8, DESIGN §8 "Scale rule": the LAST edit, so labels shrink with the
    picture), then the encoders, both at the caller's: the chain itself works in source coordinates throughout.

    ``states``: an ``EditStates``; ``spec``: the normalised options, read by ``entry.PassSpec``'s field names; F source frames of ``hw``
    = (h, w), of which the detector saw every K-th; ``rgb``: the frames' bytes are R, G, B (False: B, G, R)."""

    @staticmethod
    def trails_expire(track, detect_every):
        """The frames a trail (or a count entry) outlives its last point in a chain with ``track`` = (thr, hold, grow): (hold + 1) * K,
        K = ``detect_every`` or 1 -- as long as the tracker can still re-match the id -- and at most the rule's 4095."""
        return min((track[1] + 1) * (detect_every or 1), ops.TRACK_TRAILS[2])

    def __init__(self, states, spec, F, K, hw, rgb):
        self.states, self.spec, self.F, self.K, self.hw, self.rgb = states, spec, F, K, hw, bool(rgb)
        h, w = hw
        self.lookback = spec.track_lookback or spec.track_backtrack             # (both: the delayed path is one)
        self.tables = states.annotate_tables(spec.draw)
        self.track_out = self.lb_out = self.lb_frames = self.cuts = self.trail_lists = self.count_lists = self.zone_lists = None
        self.reid_ws = self.reid_out = self.reid_lists = None
        if spec.zone and not spec.track:
            raise FrcnnError("zone= tests the tracker's ids against the zones: the chain needs track=(thr, hold, grow) too")
        if spec.track_reid:
            if not spec.track:
                raise FrcnnError("track_reid= gives the tracker's ids back: the chain needs track=(thr, hold, grow) too")
            if self.lookback:
                raise FrcnnError("track_reid= does not go with track_lookback= / track_backtrack=: their windows hold the tracked buffers of "
                                 "earlier passes, whose ids are the tracker's")
        if spec.redact_shape and not spec.redact:
            raise FrcnnError("redact_shape= shapes the redaction: the chain needs redact=(classes, mode, size, margin) too")
        if spec.redact:
            # one workspace serves the frames of a pass, which are redacted one after another
            classes, mode, size, _ = spec.redact
            self.redact_table = states.redact_table(classes)
            self.redact_ws = torch.empty(max(ops.redact_ws_bytes(h, w, mode, size), 16), dtype=torch.uint8, device="cuda")
        if spec.track:
            self.state = states.tracker()
            self.track_table = states.track_table(spec.redact[0] if spec.redact else None, spec.remove[0] if spec.remove else None)
            self.motion = states.motion_state(h, w) if spec.track_motion else None
            self.expire = self.count_expire = self.trails_expire(spec.track, spec.detect_every)
            if spec.track_reid:
                self.reid = states.reid_state()
                self.count_expire = min(max(self.expire, spec.track_reid[1]), ops.TRACK_TRAILS[2])
            if spec.track_scene_cut:
                self.cut_ws, self.cuts = ops.track_cut_workspace(F), torch.zeros(F, dtype=torch.int32, device="cuda")
            if spec.track_trails:
                self.trails = states.trails_state(spec.track_trails[0])
                self.trail_lists = ops.track_trails_workspace(F, states.trail_capacity, spec.track_trails[0])
            if spec.count:
                self.count, self.count_table = states.count_state(), states.redact_table(spec.count[1])
                self.count_lists = ops.count_workspace(F)
                self.count_lists.zero_()
            if spec.zone:
                self.zone, self.zone_table = states.zone_state(), states.redact_table(spec.zone[1])
                self.zone_lists = ops.zone_workspace(F)
                self.zone_lists.zero_()
        if spec.heat:
            self.heat, self.heat_table = states.heat_state(h, w), states.redact_table(spec.heat[0])
        if spec.remove:
            classes = spec.remove[0]
            self.plate, self.remove_table = states.plate_state(h, w, self.rgb), states.redact_table(classes)
            names = states.class_names
            # the redaction shows until the background is known where it covers the remove classes ("all" stands for its names); else black
            covered = spec.redact and set(ops.redact_class_list(names, classes)) <= set(ops.redact_class_list(names, spec.redact[0]))
            self.keep_unknown = bool(covered)
        if spec.redact_region:
            _, _, mode, size, _ = spec.redact_region
            self.region_plane = states.region_plane(h, w, spec.redact_region)
            self.region_ws = torch.empty(max(ops.redact_ws_bytes(h, w, mode, size), 16), dtype=torch.uint8, device="cuda")
        if spec.redact_moving:
            mv = spec.redact_moving
            self.plate = states.plate_state(h, w, self.rgb)
            self.moving, self.moving_table = states.moving_state(h, w, self.rgb), ops.redact_moving_table(states.class_names, mv[6])
            self.moving_plane = torch.zeros(ops.redact_region_plane_bytes(h, w), dtype=torch.uint8, device="cuda")
            self.moving_ws = torch.empty(max(ops.redact_ws_bytes(h, w, mv[7], mv[8]), 16), dtype=torch.uint8, device="cuda")
            self.moving_stats = torch.zeros((F, _lib.REDACT_MOVING_STATS_WORDS), dtype=torch.int32, device="cuda")
        if self.lookback:
            self.lb_frames = torch.zeros((F, h, w, 3), dtype=torch.uint8, device="cuda")

    def update(self, frames_u8, frame_stride, packed, n_frames):
        """Steps 1-5 (1b too).  ``frames_u8`` holds source frame f at byte ``f * frame_stride``; ``packed``: the post-process's packed buffers of
        the key frames (one buffer for one); ``n_frames``: the device word that says how many of the F frames are real."""
        sp, (h, w), K = self.spec, self.hw, self.K
        self.packed = packed
        self.tracked, self.n_frames, self.gate = None, n_frames, None
        if not sp.track:
            return
        thr, hold, grow = sp.track
        cap = ops.track_capacity(self.state)
        if self.track_out is None:                       # (the first call: the rows of a packed buffer are known now)
            self.track_out = torch.zeros((self.F, 4 + 8 * (ops.track_rows(packed) + cap)), dtype=torch.int32, device="cuda")
        common = (packed, n_frames, self.track_table, h, w, thr, hold, grow)
        strong = sp.track_strong                         # (None: the Tracking rule; else the Weak rule, whichever form the call has)
        if sp.track_scene_cut:
            ops.track_update_cut(self.state, self.motion, frames_u8, frame_stride, *common, sp.track_motion, K, sp.track_scene_cut,
                                 out=self.track_out, cuts=self.cuts, workspace=self.cut_ws, strong=strong)
        elif sp.detect_every:
            ops.track_update_interval(self.state, self.motion, frames_u8, frame_stride, *common, sp.track_motion, K, out=self.track_out,
                                      strong=strong)
        elif sp.track_motion:
            ops.track_update_motion(self.state, self.motion, frames_u8, frame_stride, *common, sp.track_motion, out=self.track_out, strong=strong)
        else:
            ops.track_update(self.state, *common, out=self.track_out, strong=strong)
        self.tracked = self.track_out
        if sp.track_reid:
            if self.reid_ws is None:
                self.reid_ws = ops.track_reid_workspace(self.F, ops.track_rows(packed) + cap)
            self.reid_out, self.reid_lists = ops.track_reid_update(self.reid, frames_u8, frame_stride, self.track_out, n_frames, self.track_table,
                                                                   h, w, *sp.track_reid, rgb=self.rgb, cuts=self.cuts, workspace=self.reid_ws)
            self.tracked = self.reid_out
        if self.lookback:
            window, back = self.states.lookback_window(h, w, self.F, ops.track_rows(packed))      # (made by the first call: the rows are known now)
            if self.lb_out is None:
                R2 = ops.track_rows(packed) + cap + back
                self.lb_out = (self.lb_frames, torch.zeros((self.F, 4 + 8 * R2), dtype=torch.int32, device="cuda"),
                               torch.zeros(4, dtype=torch.int32, device="cuda"))
            if sp.track_backtrack:
                ops.track_backtrack(window, frames_u8, frame_stride, self.track_out, n_frames, cap, back, h, w, sp.track_backtrack,
                                    sp.track_motion, grow, K, out=self.lb_out)
            else:
                ops.track_lookback(window, frames_u8, frame_stride, self.track_out, n_frames, cap, back, h, w, sp.track_lookback,
                                   sp.track_motion or 0, grow, out=self.lb_out)
            self.tracked, self.n_frames, self.gate = self.lb_out[1], self.lb_out[2], n_frames
        if sp.track_trails:
            ops.track_trails_update(self.trails, self.tracked, self.n_frames, sp.track_trails[0], self.expire, h, w, lists=self.trail_lists,
                                    gate=self.gate)
        if sp.count:
            ops.count_update(self.count, self.tracked, self.n_frames, sp.count[0], self.count_table, self.count_expire, h, w,
                             lists=self.count_lists, gate=self.gate)
        if sp.zone:
            ops.zone_update(self.zone, self.tracked, self.n_frames, sp.zone[0], self.zone_table, self.expire, h, w, anchor=sp.zone[3],
                            lists=self.zone_lists, gate=self.gate)

    @property
    def host_tracked(self):
        """The tracked buffers of the pass itself that the host copies: ``reid_out`` with ``track_reid``, else ``track_out``."""
        return self.track_out if self.reid_out is None else self.reid_out

    def rows(self, i):
        """What the edits of frame i read."""
        if self.tracked is not None:
            return self.tracked[i]
        return self.packed[i] if self.F > 1 else self.packed

    def edit(self, i, frame):
        """Steps 5b-11 (5b2, 5c, 5c2, 6c and 6d too) on ``frame``, an (h, w, 3) uint8 device tensor: frame i of the pass, or of the pass before it in a delayed pass."""
        sp, (h, w), rows, tracked = self.spec, self.hw, self.rows(i), bool(self.spec.track)
        mv = sp.redact_moving
        if sp.remove or mv:
            _, settle, tol, p_margin = sp.remove if sp.remove else (None,) + mv[9:12]
            cut = None if self.cuts is None else self.cuts[i]
            ops.plate_update(self.plate, frame, rows, settle, tol, p_margin, i, self.n_frames, gate=self.gate, cut=cut, tracked=tracked)
        if mv:
            ops.redact_moving_build(self.moving, self.moving_plane, self.moving_stats[i], frame, self.plate, rows, self.moving_table, mv, i,
                                    self.n_frames, gate=self.gate, cut=cut, tracked=tracked)
        if sp.redact_region:
            _, _, r_mode, r_size, _ = sp.redact_region
            ops.redact_region_prepare(frame, self.region_plane, r_mode, r_size, workspace=self.region_ws)
        if mv:
            ops.redact_region_prepare(frame, self.moving_plane, mv[7], mv[8], workspace=self.moving_ws)
        if sp.redact:
            _, mode, size, margin = sp.redact
            if sp.redact_shape:
                ops.redact_shaped_u8(frame, rows, self.redact_table, mode, size, margin, *sp.redact_shape, workspace=self.redact_ws,
                                     tracked=tracked)
            else:
                ops.redact_u8(frame, rows, self.redact_table, mode, size, margin, workspace=self.redact_ws, tracked=tracked)
        if sp.remove:
            ops.plate_fill_u8(frame, self.plate, rows, self.remove_table, p_margin, keep_unknown=self.keep_unknown, tracked=tracked)
        if sp.redact_region:
            ops.redact_region_apply_u8(frame, self.region_plane, r_mode, r_size, workspace=self.region_ws)
        if mv:
            ops.redact_region_apply_u8(frame, self.moving_plane, mv[7], mv[8], workspace=self.moving_ws)
        if sp.heat:
            _, alpha, decay = sp.heat
            ops.heat_update(self.heat, h, w, rows, self.heat_table, decay, i, self.n_frames, gate=self.gate, tracked=tracked)
            ops.heat_draw_u8(frame, self.heat, alpha, rgb=self.rgb)
        if sp.zone and sp.draw:
            ops.zone_draw_u8(frame, self.zone_lists[i], sp.zone[0], sp.zone[2], rgb=self.rgb)
        if sp.track_trails:
            ops.track_trails_draw_u8(frame, self.trail_lists[i], *sp.track_trails, rgb=self.rgb)
        if sp.count and sp.draw:
            ops.count_draw_u8(frame, self.count_lists[i], sp.count[0], sp.count[2], rgb=self.rgb)
        ops.annotate_u8(frame, rows, self.tables, tracked=tracked)
