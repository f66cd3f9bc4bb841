"""The tracking rule (DESIGN §8 "Tracking rule") on hand-made sequences whose answers are worked out by hand, against its plain-Python
restatement tests/track_ref.py -- the comparand of the GPU tests -- and the host-only parts of the feature: annotate_video's arguments
and its MOT writer."""
import io

import numpy as np
import pytest

from tests import track_ref as T

H, W = 100, 200
TABLE = np.array([0, 1, 1, 0], dtype=np.uint8)            # classes 1 and 2 are tracked


def frame(tr, boxes, cls, max_rows=8, **kw):
    """One frame of hand-made rows through the restatement -> the split tracked buffer."""
    n = len(cls)
    bbox = np.full((max_rows, 4), -1, dtype=np.int64)
    c = np.full(max_rows, -1, dtype=np.int64)
    p = np.zeros(max_rows, dtype=np.int64)
    bbox[:n] = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    c[:n] = cls
    p[:n] = [T.bits(0.5 + 0.01 * k) for k in range(n)]
    return T.split(tr.update(bbox, c, p, n, max_rows, TABLE, H, W, **kw))


def test_an_id_persists_and_new_objects_get_new_ids():
    tr = T.Tracker(4)
    n_rows, n_live, next_id, overflow, bbox, cls, prob, ids, age = frame(tr, [[10, 10, 29, 29], [100, 50, 119, 69]], [1, 2])
    assert (n_rows, n_live, next_id, overflow) == (2, 2, 3, 0) and ids[:2].tolist() == [1, 2]
    # both move a little, in the other row order; a third appears
    out = frame(tr, [[102, 51, 121, 70], [150, 10, 160, 20], [12, 11, 31, 30]], [2, 1, 1])
    assert out[7][:3].tolist() == [2, 3, 1] and out[:4] == (3, 3, 4, 0)
    assert out[4][:3].tolist() == [[102, 51, 121, 70], [150, 10, 160, 20], [12, 11, 31, 30]]      # rows unchanged, in order
    assert [t["id"] for t in tr.slots] == [1, 2, 3] and tr.slots[0]["bbox"] == [12, 11, 31, 30]
    words = tr.words()
    assert words[:4].tolist() == [3, 3, 0, 2] and words[4:8].tolist() == [1, 2, 3, 0]


def test_a_lost_object_is_held_for_exactly_hold_frames_and_grows():
    tr = T.Tracker(4)
    frame(tr, [[10, 20, 29, 39]], [1], hold=2, grow=3)
    for age in (1, 2):
        n_rows, n_live, _, _, bbox, cls, prob, ids, ages = frame(tr, [], [], hold=2, grow=3)
        assert (n_rows, n_live) == (1, 0)
        assert bbox[0].tolist() == [10 - 3 * age, 20 - 3 * age, 29 + 3 * age, 39 + 3 * age]
        assert (cls[0], ids[0], ages[0], prob[0]) == (1, 1, age, T.bits(0.5))
    n_rows, n_live, next_id, _, bbox, cls, _, ids, _ = frame(tr, [], [], hold=2, grow=3)
    assert (n_rows, n_live, next_id) == (0, 0, 2) and tr.slots == [] and bbox[0].tolist() == [-1] * 4 and cls[0] == -1
    # a held track that is found again continues under its id, and the box it is matched on is the last SEEN one, not the grown one
    frame(tr, [[10, 20, 29, 39]], [1], hold=2, grow=3)
    frame(tr, [], [], hold=2, grow=3)
    out = frame(tr, [[12, 20, 31, 39]], [1], hold=2, grow=3)
    assert out[7][0] == 2 and out[0] == 1 and tr.slots[0]["age"] == 0
    # the held box comes from the CLIPPED box: a box across the border grows from the border
    tr = T.Tracker(4)
    frame(tr, [[-10, -5, 20, 30]], [1], hold=1, grow=2)
    assert frame(tr, [], [], hold=1, grow=2)[4][0].tolist() == [-2, -2, 22, 32]


def test_no_match_across_classes_and_untracked_classes():
    tr = T.Tracker(4)
    frame(tr, [[10, 10, 29, 29]], [1])
    out = frame(tr, [[10, 10, 29, 29], [50, 50, 60, 60], [70, 70, 80, 80], [0, 0, 5, 5]], [2, 0, 3, 7])
    assert out[7][:4].tolist() == [2, 0, 0, 0]                   # the same box in another class is a new object; classes 0, 3, 7: untracked
    assert out[0] == 5 and out[7][4] == 1 and out[8][4] == 1     # ... and track 1 is held


def test_the_threshold_edge():
    """10x10 against 10x5 sharing 50 pixels: inter 50, union 100."""
    for thr, same in ((50, True), (51, False)):
        tr = T.Tracker(4)
        frame(tr, [[0, 0, 9, 9]], [1], thr=thr)
        ids = frame(tr, [[0, 0, 9, 4]], [1], thr=thr)[7]
        assert (ids[0] == 1) == same, thr
    assert T.inter_union(T.clip([0, 0, 9, 9], H, W), T.clip([0, 0, 9, 4], H, W)) == (50, 100)


def test_both_tie_breaks():
    # equal IoU from two rows: the lower row continues the track, the other is born
    tr = T.Tracker(4)
    frame(tr, [[10, 10, 19, 19]], [1])
    assert frame(tr, [[12, 10, 21, 19], [8, 10, 17, 19]], [1, 1])[7][:2].tolist() == [1, 2]
    # two slots on one row: the lower id takes it, the other is held
    tr = T.Tracker(4)
    frame(tr, [[12, 10, 21, 19], [8, 10, 17, 19]], [1, 1])
    out = frame(tr, [[10, 10, 19, 19]], [1], thr=30)
    assert out[7][:2].tolist() == [1, 2] and out[8][:2].tolist() == [0, 1] and out[0] == 2
    # ... and a better IoU beats a lower row
    tr = T.Tracker(4)
    frame(tr, [[10, 10, 19, 19]], [1])
    assert frame(tr, [[13, 10, 22, 19], [10, 10, 19, 19]], [1, 1])[7][:2].tolist() == [2, 1]


def test_a_full_table_leaves_rows_untracked_and_counts_them():
    tr = T.Tracker(2)
    boxes = [[0, 0, 9, 9], [20, 0, 29, 9], [40, 0, 49, 9], [60, 0, 69, 9]]
    out = frame(tr, boxes, [1, 1, 1, 1])
    assert out[7][:4].tolist() == [1, 2, 0, 0] and out[3] == 2 and out[2] == 3
    out = frame(tr, boxes, [1, 1, 1, 1])
    assert out[7][:4].tolist() == [1, 2, 0, 0] and out[3] == 4      # sticky
    assert tr.words()[:4].tolist() == [2, 2, 4, 2]
    out = frame(tr, boxes[2:], [1, 1], hold=0)                     # the two tracks are freed in step 2: their slots serve step 3
    assert out[7][:2].tolist() == [3, 4] and out[3] == 4 and out[0] == 2


def test_hold_zero_assigns_ids_only():
    tr = T.Tracker(4)
    frame(tr, [[0, 0, 9, 9]], [1], hold=0)
    out = frame(tr, [], [], hold=0)
    assert out[:4] == (0, 0, 2, 0) and tr.slots == []
    assert tr.events["hold"] == 0 and tr.events["free"] == 1


def test_eligibility_boxes_and_counts():
    tr = T.Tracker(4)
    # reversed corners, across the border, wholly outside, zero live rows behind n_dets
    out = frame(tr, [[29, 29, 10, 10], [-5, -5, 3, 3], [W, 0, W + 9, 9], [0, -9, 9, -1]], [1, 1, 1, 1])
    assert out[7][:4].tolist() == [1, 2, 0, 0] and out[3] == 0
    assert frame(tr, [[10, 10, 29, 29], [3, 3, -5, -5]], [1, 1])[7][:2].tolist() == [1, 2]
    pad = T.split(tr.padding(8))
    assert pad[:4] == (0, 0, 3, 0) and (pad[4] == -1).all() and (pad[5] == -1).all() and not pad[7].any()
    # n_dets beyond max_rows is cut, a negative one is none
    tr = T.Tracker(4)
    out = T.split(tr.update(np.tile([0, 0, 9, 9], (3, 1)), [1, 1, 1], [0, 0, 0], 7, 3, TABLE, H, W))
    assert out[1] == 3
    assert T.split(tr.update(np.zeros((3, 4)), [1, 1, 1], [0, 0, 0], -2, 3, TABLE, H, W))[1] == 0


def test_products_need_int64():
    tr = T.Tracker(4)
    big = [[0, 0, 29999, 29999], [2000, 2000, 31999, 31999]]
    T.split(tr.update(big[:1], [1], [0], 1, 2, TABLE, 32768, 32768))
    inter, union = T.inter_union(T.clip(big[0], 32768, 32768), T.clip(big[1], 32768, 32768))
    assert inter * union > 2 ** 59 and inter * 100 > 2 ** 31
    assert T.split(tr.update(big[1:], [1], [0], 1, 2, TABLE, 32768, 32768, thr=77))[7][0] == 1      # 784e6 / 1016e6 = 77.2 %
    tr.slots[0]["bbox"] = big[0]
    assert T.split(tr.update(big[1:], [1], [0], 1, 2, TABLE, 32768, 32768, thr=78))[7][0] == 2


# ----------------------------------------------------------------------------------------------------------- host dets, labels, MOT
MAPPING = {"bg": 0, "car": 1, "person": 2, "Misc": 3}


def det(box, name, prob):
    return {"bbox": np.array(box, dtype=np.int64), "cls_name": name, "prob": np.float32(prob)}


def test_track_dets_and_labels():
    tr = T.Tracker(4)
    live, held = T.track_dets(tr, [det([10, 10, 29, 29], "car", 0.9), det([40, 40, 50, 50], "Misc", 0.8)], MAPPING, ("car", "person"), H, W, hold=1, grow=2)
    assert [d["track_id"] for d in live] == [1, 0] and held == []
    assert T.label_text(live[0]) == "car#1   0.90" and T.label_text(live[1]) == "Misc   0.80"
    assert T.label_text(dict(live[0], track_id=2147483647)) == "car#2147483647   0.90"
    live, held = T.track_dets(tr, [], MAPPING, ("car", "person"), H, W, hold=1, grow=2)
    assert live == [] and len(held) == 1 and held[0]["held"] == 1 and held[0]["track_id"] == 1 and held[0]["cls_name"] == "car"
    assert held[0]["bbox"].tolist() == [8, 8, 31, 31] and held[0]["prob"] == np.float32(0.9)
    # the drawing with ids: the label's pixels differ from the plain label's, held rows paint nothing
    from tests import annotate_ref
    src = np.zeros((H, W, 3), dtype=np.uint8)
    d = dict(det([10, 10, 60, 40], "car", 0.9), track_id=7)
    assert not np.array_equal(T.annotate(src, [d]), annotate_ref.annotate(src, [d]))
    assert np.array_equal(T.annotate(src, [dict(d, track_id=0)]), annotate_ref.annotate(src, [d]))
    assert np.array_equal(T.annotate(src, [dict(d, held=1)]), src)


def test_mot_writer():
    from faster_rcnn_amd import annotate_video
    dets = [dict(det([10, 12, 30, 52], "car", 0.97), track_id=3), dict(det([5, 5, 9, 9], "Misc", 0.5), track_id=0),
            dict(det([60, 40, 50, 20], "person", 0.25), track_id=11), dict(det([0, 0, 4, 4], "car", 0.9), track_id=2, held=1)]
    lines = annotate_video.mot_lines(7, dets, MAPPING)
    assert lines == ["7,3,10,12,20,40,0.970000,1,-1,-1", "7,11,50,20,10,20,0.250000,2,-1,-1"]
    assert lines == T.mot_lines(7, dets, MAPPING)
    f = io.StringIO()
    annotate_video._write_tracks(f, 7, dets, MAPPING)
    annotate_video._write_tracks(None, 7, dets, MAPPING)
    assert f.getvalue() == "".join(line + "\n" for line in lines)


def test_cli_arguments():
    from faster_rcnn_amd import annotate_video
    parse = lambda *extra: annotate_video.build_parser().parse_args(["a.h5", "b.h5", "frames"] + list(extra))
    assert annotate_video.track_from_args(parse()) is None
    assert annotate_video.track_from_args(parse("--track")) == (30, 8, 0) == T.DEFAULTS
    assert annotate_video.track_from_args(parse("--track", "--track_iou", "55", "--track_hold", "0", "--track_grow", "64")) == (55, 0, 64)
    for flag, value in (("--track_iou", "30"), ("--track_hold", "8"), ("--track_grow", "0"), ("--tracks_out", "t.txt")):
        with pytest.raises(ValueError) as e:
            annotate_video.track_from_args(parse(flag, value))
        assert flag in str(e.value) and "--track" in str(e.value)
    for flag, value in (("--track_iou", "0"), ("--track_iou", "101"), ("--track_hold", "-1"), ("--track_hold", "256"), ("--track_grow", "-1"),
                        ("--track_grow", "65")):
        with pytest.raises(ValueError) as e:
            annotate_video.track_from_args(parse("--track", flag, value))
        assert value in str(e.value)
    args = parse("--track", "--tracks_out", "t.txt")
    assert args.tracks_out == "t.txt" and annotate_video.track_from_args(args) == (30, 8, 0)


def test_option_checks_need_no_gpu():
    from faster_rcnn_amd import ops
    assert ops.track_option() == (30, 8, 0) and ops.track_option(1, 255, 64) == (1, 255, 64)
    for bad in ((0, 8, 0), (30, 256, 0), (30, 8, 65), (30.0, 8, 0), (True, 8, 0)):
        with pytest.raises(ValueError):
            ops.track_option(*bad)
    buf = np.arange(4 + 8 * 3, dtype=np.int32)
    n_rows, n_live, next_id, overflow, bbox, cls, prob, ids, age = ops.split_tracked(buf)
    assert (n_rows[0], n_live[0], next_id[0], overflow[0]) == (0, 1, 2, 3) and bbox.shape == (3, 4) and bbox[0, 0] == 4
    assert cls.tolist() == [16, 17, 18] and prob.dtype == np.float32 and ids.tolist() == [22, 23, 24] and age.tolist() == [25, 26, 27]
