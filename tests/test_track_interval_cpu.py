"""Host-only checks of the interval rule's restatement (tests/track_interval_ref.py), of ops.track_interval_option and of
annotate_video's --detect_every parsing and refusals.  No GPU."""
import numpy as np
import pytest

from tests import track_interval_ref as I
from tests import track_motion_ref as M
from tests import track_ref as T

H, W, ROWS = 48, 64, 8
TABLE = np.array([0, 1, 1, 0, 1], dtype=np.uint8)


def pack(boxes, cls, rows=ROWS):
    p = np.zeros(4 + 7 * rows, dtype=np.int32)
    p[0] = len(cls)
    p[4:4 + 5 * rows] = -1
    for r, (b, c) in enumerate(zip(boxes, cls)):
        p[4 + 4 * r:8 + 4 * r] = b
        p[4 + 4 * rows + r] = c
        p[4 + 5 * rows + r] = T.bits(0.9 - 0.01 * r)
    return p


def noise(seed, n, step=None):
    rs = np.random.RandomState(seed)
    out = [rs.randint(0, 256, (H, W, 3)).astype(np.uint8)]
    for _ in range(n - 1):
        d = step or (int(rs.randint(-3, 4)), int(rs.randint(-3, 4)))
        out.append(np.ascontiguousarray(M.shifted(out[-1], *d)))
    return out


def random_packed(rs):
    n = int(rs.randint(0, ROWS + 1))
    xy = rs.randint(-8, [W - 8, H - 8], (n, 2))
    return pack(np.concatenate([xy, xy + rs.randint(3, 40, xy.shape)], axis=1).tolist(), rs.choice([0, 1, 2, 4], n).tolist())


@pytest.mark.parametrize("seed", range(4))
def test_interval_1_is_the_motion_rule_word_for_word(seed):
    rs = np.random.RandomState(seed)
    a, b = I.IntervalTracker(5), M.MotionTracker(5)
    frames = noise(seed, 14)
    at = 0
    for F, nf in ((1, 1), (4, 4), (3, 2), (2, 0), (4, 9)):
        packed = [random_packed(rs) for _ in range(F)]
        got = a.update_interval(frames[at:at + F], packed, nf, TABLE, H, W, 30, 2, 3, 8, 1)
        want = b.update_call(frames[at:at + F], packed, nf, TABLE, H, W, 30, 2, 3, 8)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        assert np.array_equal(a.t.words(), b.t.words()) and np.array_equal(a.motion_bytes(H, W), b.motion_bytes(H, W))
        at += F
    assert a.moves == b.moves and a.moves and a.t.events["hold"] and a.t.events["overflow"]


def test_identical_frames_leave_the_between_rows_unmoved():
    frame = noise(3, 1)[0]
    boxes, cls = [[3, 4, 42, 33], [-5, -6, 20, 18], [30, 30, 32, 32], [50, 10, 60, 40]], [1, 2, 4, 0]
    t = I.IntervalTracker(8)
    out = t.update_interval([frame] * 4, [pack(boxes, cls)], 4, TABLE, H, W, interval=4)
    key = T.split(out[0])
    tracked = [r for r in range(key[1]) if key[7][r] > 0]
    assert len(tracked) == 3 and t.moves == []
    for f in (1, 2, 3):
        n_rows, n_live, next_id, overflow, bbox, c, prob, ids, age = T.split(out[f])
        assert (n_rows, n_live, next_id, overflow) == (3, 3, 4, 0) and not age.any()
        for k, r in enumerate(tracked):                                      # the key frame's tracked rows, in id order (= row order at birth)
            assert bbox[k].tolist() == boxes[r] and c[k] == cls[r] and prob[k] == key[6][r] and ids[k] == key[7][r]
        assert (bbox[3:] == -1).all() and (c[3:] == -1).all() and not prob[3:].any() and not ids[3:].any()


def test_between_rows_follow_a_shift_of_3_2_per_frame():
    frames = noise(8, 8, step=(3, 2))
    box, lost = [5, 6, 34, 29], [36, 8, 50, 30]
    t = I.IntervalTracker(4)
    out = t.update_interval(frames, [pack([box, lost], [1, 2]), pack([[5 + 12, 6 + 8, 34 + 12, 29 + 8]], [1])], 8, TABLE, H, W, 30, 8, 2, 8, 4)
    assert [m for m in t.moves if m[0] == 1] == [(1, 3, 2)] * 7
    for f in range(1, 8):
        n_rows, n_live, _, _, bbox, _, _, ids, age = T.split(out[f])
        assert ids[0] == 1 and age[0] == 0 and n_live >= 1
        if f != 4:                                                           # (frame 4 is a key frame: the row is the detection's own)
            assert bbox[0].tolist() == [box[0] + 3 * f, box[1] + 2 * f, box[2] + 3 * f, box[3] + 2 * f], f
    # track 2 is not detected in key frame 4: held from there on with age 1, grown by grow * 1 and not more between the key frames
    for f in (5, 6, 7):
        n_rows, n_live, _, _, bbox, _, _, ids, age = T.split(out[f])
        assert (n_rows, n_live, ids[1], age[1]) == (2, 1, 2, 1)
        s = next(s for s in t.t.slots if s["id"] == 2)
        assert s["age"] == 1
    xa, xb, ya, yb = T.clip(next(s for s in t.t.slots if s["id"] == 2)["bbox"], H, W)
    assert T.split(out[7])[4][1].tolist() == [xa - 2, ya - 2, xb + 2, yb + 2]


def test_between_frames_touch_neither_ages_nor_counts_and_every_frame_counts():
    frames = noise(5, 7)
    boxes, cls = [[3, 4, 42, 33], [20, 10, 50, 40], [40, 5, 60, 30]], [1, 2, 4]
    t = I.IntervalTracker(2)                                                 # two slots for three rows: one overflow per key frame
    t.update_interval(frames[:1], [pack(boxes, cls)], 1, TABLE, H, W, 30, 1, 0, 8, 3)
    assert (t.t.frames, t.t.next_id, t.t.overflow) == (1, 3, 1)
    for nf, want_frames in ((0, 1), (1, 2), (3, 5), (6, 11)):
        seen = []
        orig = t.between

        def spy(*a, **k):
            before = ([(s["id"], s["cls"], s["prob"], s["age"]) for s in t.t.slots], t.t.next_id, t.t.overflow)
            res = orig(*a, **k)
            assert before == ([(s["id"], s["cls"], s["prob"], s["age"]) for s in t.t.slots], t.t.next_id, t.t.overflow)
            seen.append(res)
            return res

        t.between = spy
        out = t.update_interval(frames[1:], [pack([], []), pack(boxes[:1], cls[:1])], nf, TABLE, H, W, 30, 1, 0, 8, 3)
        t.between = orig
        real = min(nf, 6)
        assert t.t.frames == want_frames and len(seen) == real - I.keys_of(real, 3)
        assert t.header().tolist() == [want_frames, H, W, 0]
        for f in range(real, 6):
            assert np.array_equal(out[f], t.t.padding(ROWS))
    # hold = 1 counted in key frames: the slots survived the between frames behind their one missed key frame
    assert t.t.events["free"] >= 1


def test_track_interval_option():
    from faster_rcnn_amd import ops
    assert [ops.track_interval_option(k) for k in (2, 4, 16, np.int64(3))] == [2, 4, 16, 3]
    for bad in (1, 0, 17, -2, True, 2.0, "4", None, (4,)):
        with pytest.raises(ValueError) as e:
            ops.track_interval_option(bad)
        assert "2..16" in str(e.value)


# ----------------------------------------------------------------------------------------------------------- annotate_video
def parse(*extra):
    from faster_rcnn_amd import annotate_video
    return annotate_video.build_parser().parse_args(["a.h5", "b.h5", "frames"] + list(extra))


def test_the_parser_reads_detect_every():
    from faster_rcnn_amd import annotate_video
    assert annotate_video.detect_every_from_args(parse()) is None
    assert annotate_video.detect_every_from_args(parse("--track", "--track_motion")) is None
    assert annotate_video.detect_every_from_args(parse("--track", "--track_motion", "--detect_every", "4")) == 4
    assert annotate_video.detect_every_from_args(parse("--track", "--track_motion", "3", "--detect_every", "16")) == 16
    text = annotate_video.build_parser().format_help()
    assert "--detect_every K" in text and "DETECTED" in text                 # (the help says what --track_hold then counts)


def test_the_parser_refuses_detect_every_with_a_reason():
    from faster_rcnn_amd import annotate_video
    for extra in (["--detect_every", "4"], ["--track", "--detect_every", "4"], ["--track_motion", "8", "--detect_every", "4"]):
        with pytest.raises(ValueError) as e:
            annotate_video.detect_every_from_args(parse(*extra))
        assert "--detect_every" in str(e.value) and "needs --track --track_motion" in str(e.value)
    with pytest.raises(ValueError) as e:
        annotate_video.detect_every_from_args(parse("--track", "--track_motion", "--track_lookback", "--detect_every", "4"))
    assert "--track_lookback" in str(e.value) and "not supported" in str(e.value)
    for bad in ("1", "0", "17", "-3"):
        with pytest.raises(ValueError) as e:
            annotate_video.detect_every_from_args(parse("--track", "--track_motion", "--detect_every", bad))
        assert "--detect_every" in str(e.value) and "2..16" in str(e.value)


def test_the_one_frame_paths_and_the_pipelines_refuse_with_a_reason():
    from faster_rcnn_amd import annotate_video
    track = (30, 8, 0)
    with pytest.raises(ValueError, match="get_annotated_frame detects its one frame"):
        annotate_video.get_annotated_frame(None, None, None, None, 600, 1000, track=track, track_motion=8, detect_every=2)
    with pytest.raises(ValueError, match="eager"):                           # a foreign model: no engine
        annotate_video._detect_every(2, track, 8, None, None, None)
    for t, m in ((None, None), (track, None), (None, 8)):
        with pytest.raises(ValueError, match="track=.*track_motion="):
            annotate_video._detect_every(2, t, m, None, object(), 4)
    with pytest.raises(ValueError, match="track_lookback.*not supported"):
        annotate_video._detect_every(2, track, 8, 4, object(), 4)
    with pytest.raises(ValueError, match="2..16"):
        annotate_video._detect_every(1, track, 8, None, object(), 4)
    with pytest.raises(ValueError, match="at most 12 here"):                  # five images a pass: 5 * 13 = 65 frames in one tracker call
        annotate_video._detect_every(13, track, 8, None, object(), 5)
    assert annotate_video._detect_every(None, None, None, None, None, None) is None
    assert annotate_video._detect_every(16, track, 8, None, object(), 4) == 16


def test_a_group_is_cut_into_passes_by_its_key_frames():
    from faster_rcnn_amd import annotate_video
    g = list(range(11))
    assert annotate_video._every_parts(g[:8], 4, 2) == [(g[:8], 4)]
    assert annotate_video._every_parts(g[:3], 4, 2) == [(g[:3], 4)]          # two key frames: half a pass of four, padded
    assert annotate_video._every_parts(g[:2], 4, 2) == [(g[:2], 1)]          # one key frame: a one-image pass of two frames
    assert annotate_video._every_parts(g[:5], 8, 2) == [(g[0:2], 1), (g[2:4], 1), (g[4:5], 1)]
    assert annotate_video._every_parts(g[:4], 1, 4) == [(g[:4], 1)] and annotate_video._every_parts(g[:6], 1, 4) == [(g[:4], 1), (g[4:6], 1)]
