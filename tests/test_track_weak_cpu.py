"""The weak rule's plain-Python restatement (tests/track_weak_ref.py) against hand-written sequences and against tests/track_ref.py at
strong = 0.0; the option, the pass spec and the command line's refusals by name.  No GPU."""
import numpy as np
import pytest

from tests import track_ref as T
from tests import track_weak_ref as WR

H, W = 120, 160
TABLE = np.array([0, 1, 1, 0, 1], dtype=np.uint8)
NAN = float("nan")


def frame(t, rows, strong=0.5, cap_rows=8, **params):
    """``rows``: [(box, cls, prob)] -> the tracked buffer split (tests/track_ref.split)."""
    bbox = np.array([r[0] for r in rows], dtype=np.int64).reshape(-1, 4)
    cls = np.array([r[1] for r in rows], dtype=np.int64)
    prob = np.array([T.bits(r[2]) for r in rows], dtype=np.int64)
    return T.split(t.update(bbox, cls, prob, len(rows), cap_rows, TABLE, H, W, strong=strong, **params))


A, A2, B = [10, 10, 29, 29], [12, 10, 31, 29], [80, 40, 99, 59]


def test_a_weak_row_continues_a_held_slot():
    t = WR.Tracker(4)
    frame(t, [(A, 1, 0.9)])
    n_rows, n_live, _, _, box, cls, prob, tid, age = frame(t, [])
    assert (n_rows, n_live) == (1, 0) and tid[0] == 1 and age[0] == 1                    # held
    n_rows, n_live, next_id, _, box, cls, prob, tid, age = frame(t, [(A2, 1, 0.3)])
    assert (n_rows, n_live, next_id) == (1, 1, 2) and tid[0] == 1 and age[0] == 0 and box[0].tolist() == A2
    assert prob[0] == T.bits(0.3) and t.slots[0]["bbox"] == A2 and t.slots[0]["prob"] == T.bits(0.3) and t.slots[0]["age"] == 0
    assert t.events["weak_match"] == 1 and t.events["weak_drop"] == 0


def test_a_weak_row_with_the_larger_iou_loses_to_a_strong_one():
    t = WR.Tracker(4)
    frame(t, [(A, 1, 0.9)])
    n_rows, n_live, next_id, _, box, cls, prob, tid, age = frame(t, [(A, 1, 0.4), (A2, 1, 0.6)])      # the weak row is the slot's own box
    assert (n_rows, n_live, next_id) == (1, 1, 2) and box[0].tolist() == A2 and tid[0] == 1 and t.slots[0]["bbox"] == A2
    assert t.events == dict(t.events, match=1, weak_match=0, weak_drop=1)


def test_a_weak_row_never_births_and_an_unmatched_one_is_dropped_and_the_later_rows_move_up():
    t = WR.Tracker(4)
    n_rows, n_live, next_id, overflow, box, cls, prob, tid, age = frame(t, [(A, 1, 0.2), (B, 2, 0.9), ([0, 0, 5, 5], 3, 0.1), (A2, 0, 0.7)])
    assert (n_rows, n_live, next_id, overflow) == (2, 2, 2, 0)
    assert box[:2].tolist() == [B, A2] and cls[:2].tolist() == [2, 0] and tid[:2].tolist() == [1, 0]      # an untracked strong row stays
    assert box[2].tolist() == [-1] * 4 and cls[2] == -1 and len(t.slots) == 1 and t.events["weak_drop"] == 2


def test_an_all_weak_frame():
    t = WR.Tracker(4)
    frame(t, [(A, 1, 0.9), (B, 2, 0.8)])
    n_rows, n_live, next_id, _, box, cls, prob, tid, age = frame(t, [(B, 2, 0.1), (A2, 1, 0.2), (A2, 1, 0.2), ([100, 90, 120, 110], 4, 0.4)])
    assert (n_rows, n_live, next_id) == (2, 2, 3) and tid[:2].tolist() == [2, 1] and box[:2].tolist() == [B, A2]      # row order; the tie: row 1
    assert [s["age"] for s in t.slots] == [0, 0] and t.events["weak_match"] == 2 and t.events["weak_drop"] == 2
    # a slot whose class has only weak rows, beside one with a strong row
    n_rows, n_live, _, _, box, cls, prob, tid, age = frame(t, [(B, 2, 0.3), (A2, 1, 0.9)])
    assert n_live == 2 and tid[:2].tolist() == [2, 1]


def test_overflow_counts_strong_rows_only():
    t = WR.Tracker(1)
    _, n_live, next_id, overflow, _, _, _, tid, _ = frame(t, [(A, 1, 0.9), (B, 2, 0.9), ([100, 90, 120, 110], 4, 0.2), ([50, 90, 70, 110], 4, 0.6)])
    assert (n_live, next_id, overflow) == (3, 2, 2) and tid[:3].tolist() == [1, 0, 0] and t.overflow == 2


def test_a_nan_score_is_weak():
    assert not WR.is_strong(T.bits(NAN), 0.0) and not WR.is_strong(T.bits(NAN), float("-inf")) and WR.is_strong(T.bits(0.5), 0.5)
    assert not WR.is_strong(T.bits(np.float32(0.5) - np.float32(2.0 ** -25)), 0.5) and WR.is_strong(T.bits(-0.0), 0.0)
    t = WR.Tracker(4)
    _, n_live, next_id, _, _, _, _, _, _ = frame(t, [(A, 1, NAN)], strong=0.0)
    assert (n_live, next_id) == (0, 1)                                       # no birth, dropped
    frame(t, [(A, 1, 0.9)])
    _, n_live, _, _, _, _, prob, tid, _ = frame(t, [(A2, 1, NAN)], strong=0.0)
    assert n_live == 1 and tid[0] == 1 and prob[0] == T.bits(NAN)            # it continues a track


@pytest.mark.parametrize("seed", range(6))
def test_strong_zero_is_the_tracking_rule_on_random_sequences(seed):
    rs = np.random.RandomState(seed)
    cap, rows = (2, 4, 16)[seed % 3], 24
    a, b = WR.Tracker(cap), T.Tracker(cap)
    pos = rs.randint(0, [W - 30, H - 30], (10, 2))
    for f in range(12):
        pos += rs.randint(-3, 4, pos.shape)
        seen = [o for o in range(10) if rs.rand() < 0.7]
        bbox = np.array([[pos[o, 0], pos[o, 1], pos[o, 0] + 20, pos[o, 1] + 25] for o in seen] + [[5, 5, 30, 30]], dtype=np.int64)
        cls = np.array([(1, 2, 4)[o % 3] for o in seen] + [3], dtype=np.int64)
        prob = np.array([T.bits(p) for p in rs.rand(len(cls))], dtype=np.int64)
        args = (bbox, cls, prob, len(cls), rows, TABLE, H, W, 30, 2, 1)
        assert np.array_equal(a.update(*args, strong=0.0), b.update(*args))
        assert np.array_equal(a.words(), b.words())
    assert a.events["weak_match"] == a.events["weak_drop"] == 0 and a.events["match"] == b.events["match"] > 0


def test_no_weak_row_in_reach_is_the_rule_on_the_strong_rows():
    a, b = WR.Tracker(4), T.Tracker(4)
    for f in range(5):
        rows = [([10 + f, 10, 29 + f, 29], 1, 0.9), ([140, 100, 155, 115], 1, 0.1), ([60, 10 + f, 79, 29 + f], 2, 0.6)]
        packed = np.zeros(4 + 7 * 8, dtype=np.int32)
        packed[0] = len(rows)
        for k, (box, c, p) in enumerate(rows):
            packed[4 + 4 * k:8 + 4 * k], packed[4 + 32 + k], packed[4 + 40 + k] = box, c, T.bits(p)
        assert np.array_equal(a.update_packed(packed, TABLE, H, W, strong=0.5), b.update_packed(WR.strong_only(packed, 0.5), TABLE, H, W))
    assert np.array_equal(a.words(), b.words()) and a.next_id == 3


# ----------------------------------------------------------------------------------------------- the option and the command line
def test_track_weak_option():
    from faster_rcnn_amd import ops
    assert ops.track_weak_option() == (0.0, None) and ops.track_weak_option(0.5) == (0.5, None)
    assert ops.track_weak_option(0.5, 0.1) == (0.5, 0.1) and ops.track_weak_option(1, 0) == (1.0, 0.0)
    assert ops.track_weak_option(0.5, None, track=False) == (0.5, None)
    for args, word in (((0.5, 0.1, False), "needs tracking"), ((0.5, 0.5), "below det threshold"), ((0.5, 0.7), "below det threshold"),
                       ((None, 0.0), "below det threshold"), ((1.5, None), "det threshold=1.5"), ((0.5, -0.1), "track low=-0.1"),
                       ((True, None), "det threshold=True"), ((NAN, None), "det threshold=nan"), ((0.5, "x"), "track low='x'")):
        with pytest.raises(ValueError, match=word):
            ops.track_weak_option(*args)


def test_the_ops_calls_take_strong():
    """(the proof against a tree without the feature: the argument does not exist there)"""
    import inspect
    from faster_rcnn_amd import ops
    for name in ("track_update", "track_update_motion", "track_update_interval", "track_update_cut"):
        assert inspect.signature(getattr(ops, name)).parameters["strong"].default is None


def parse(*extra):
    from faster_rcnn_amd import annotate_video
    return annotate_video.build_parser().parse_args(["a.h5", "b.h5", "frames"] + list(extra))


def test_the_parser_reads_the_thresholds():
    from faster_rcnn_amd import annotate_video
    both = annotate_video.det_thresholds_from_args
    assert both(parse()) == {} and both(parse("--track")) == {}
    assert both(parse("--det_threshold", "0.5")) == {"det_threshold": 0.5}
    assert both(parse("--det_threshold", "0.5", "--track", "--track_low", "0.1")) == {"det_threshold": 0.5, "track_low": 0.1}
    text = annotate_video.build_parser().format_help()
    assert "--det_threshold T" in text and "--track_low L" in text
    with pytest.raises(SystemExit):                                          # no bare form: no default has been measured
        parse("--track", "--track_low")


def test_the_parser_and_the_pipelines_refuse_with_a_reason():
    from faster_rcnn_amd import annotate_video
    both = annotate_video.det_thresholds_from_args
    for extra, word in ((["--det_threshold", "0.5", "--track_low", "0.1"], "needs tracking"),
                        (["--track", "--track_low", "0.1"], "below det threshold"),
                        (["--track", "--det_threshold", "0.3", "--track_low", "0.3"], "below det threshold"),
                        (["--det_threshold", "1.5"], "0..1"), (["--track", "--det_threshold", "0.5", "--track_low", "-1"], "0..1")):
        with pytest.raises(ValueError, match=word) as e:
            both(parse(*extra))
        assert "--det_threshold / --track_low" in str(e.value)
    check = annotate_video._det_thresholds
    assert check(None, None, None) == (0.0, None) and check(0.5, 0.1, (30, 8, 0)) == (0.5, 0.1)
    with pytest.raises(ValueError, match="needs tracking"):
        check(0.5, 0.1, None)
    with pytest.raises(ValueError, match="below det threshold"):
        check(None, 0.1, (30, 8, 0))


def test_the_pass_key_carries_the_tag_last_and_only_with_the_option():
    import dataclasses
    from faster_rcnn_amd import entry
    plain = entry.PassSpec(annotate=True, track=(30, 8, 0), track_motion=8, out_size=("scale", 2))
    weak = dataclasses.replace(plain, track_strong=0.5)
    assert weak.key_tail(4) == plain.key_tail(4) + ("weak", 0.5)
    assert entry.PassSpec(annotate=True, track=(30, 8, 0)).key_tail(1) == ("annotate", "track", 30, 8, 0)
    with pytest.raises(entry.FrcnnError, match="track_strong= tells the tracker"):
        entry.PassSpec.checked(None, 1, annotate=True, track_strong=0.5)


def test_the_eager_path_refuses_track_low_by_name(monkeypatch):
    """A foreign model has no captured pass to run the rule in: both pipelines say so, behind the pair's own check and in front of any
    work on a frame."""
    from faster_rcnn_amd import annotate_video
    monkeypatch.setattr(annotate_video, "_engine", lambda *a, **k: None)      # what a foreign model gets
    with pytest.raises(ValueError, match="track_low=0.1 runs the tracker's weak rule inside the captured passes: the eager path"):
        annotate_video.get_annotated_frame(None, None, None, None, 600, 1000, track=(30, 8, 0), det_threshold=0.5, track_low=0.1)
    with pytest.raises(ValueError, match="below det threshold"):            # (the pair's own refusal comes first)
        annotate_video.get_annotated_frame(None, None, None, None, 600, 1000, track=(30, 8, 0), det_threshold=0.1, track_low=0.5)

    class Sink:
        kwargs, closed = {}, False

        def close(self):
            self.closed = True

    sink = Sink()
    with pytest.raises(ValueError, match="track_low=0.1 runs the tracker's weak rule inside the captured passes: the eager path"):
        annotate_video._annotate(None, None, iter(()), None, lambda: sink, 600, 1000, track=(30, 8, 0), det_threshold=0.5, track_low=0.1)
    assert sink.closed
    assert annotate_video._det_thresholds(0.5, None, None, eager=True) == (0.5, None)      # det_threshold alone: the eager path takes it
