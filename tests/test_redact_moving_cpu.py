"""The moving rule's restatement (tests/redact_moving_ref.py) against itself and against the region rule's (tests/redact_region_ref.py),
and the option's normalisation and refusals: no GPU."""
import numpy as np
import pytest

from faster_rcnn_amd import ops
from tests import plate_ref as P
from tests import redact_moving_ref as M
from tests import redact_region_ref as RR


def _pattern(h, w, seed, density=0.15):
    return np.random.RandomState(seed).rand(*M.cells(h, w)) < density


@pytest.mark.parametrize("G,F", [(0, 0), (8, 0), (0, 8), (32, 32)])
def test_plane_equals_region_reference_of_dilated_mask(G, F):
    for seed, (h, w) in enumerate([(37, 45), (75, 130), (9, 9)]):
        moving = _pattern(h, w, seed)
        W = M.weights(moving, h, w, G, F)
        want = RR.weights(h, w, [], M.dilated_mask(moving, h, w, G), F)
        assert np.array_equal(W, want), (h, w, G, F)


def test_weight_never_falls_when_grow_or_feather_grows():
    h, w = 37, 45
    moving = _pattern(h, w, 3, 0.05)
    base = M.weights(moving, h, w, 2, 3)
    assert (M.weights(moving, h, w, 5, 3) >= base).all() and (M.weights(moving, h, w, 2, 9) >= base).all()
    assert (M.weights(moving, h, w, 32, 32) >= base).all()


def test_every_pixel_of_a_moving_cell_is_full():
    h, w = 37, 45
    moving = _pattern(h, w, 4)
    for G, F in [(0, 0), (3, 5)]:
        W = M.weights(moving, h, w, G, F)
        assert (W[M.hard_pixels(moving, h, w)] == 256).all()
    assert (M.weights(np.zeros(M.cells(h, w), dtype=bool), h, w, 8, 8) == 0).all()


def _settled(h, w, value=100):
    """A plate state that knows every pixel as ``value``, and the frame that equals it."""
    frame = np.full((h, w, 3), value, dtype=np.uint8)
    state = P.empty(h, w)
    det = P.packed(4, [])
    P.update(state, frame, det, 4, 1, 10, 0)
    assert P.known(state, h, w) == h * w
    return state, frame, det


def test_hold_counts_down_exactly_H_frames():
    h, w, H = 16, 24, 3
    plate, still, det = _settled(h, w)
    moved = still.copy()
    moved[0:8, 8:16] = 200
    state = M.empty(h, w)
    out = M.build(state, moved, plate, det, 4, hold=H, grow=0)
    assert out["moving"].sum() == 1 and out["moving"][0, 1] and state[2][0, 1] == H
    for k in range(H):                                                      # H more frames hidden, the hold running down
        out = M.build(state, still, plate, det, 4, hold=H, grow=0)
        assert out["moving"][0, 1] and state[2][0, 1] == H - 1 - k and out["stats"] == [1, 1, 64, 64]
    out = M.build(state, still, plate, det, 4, hold=H, grow=0)
    assert not out["moving"].any() and out["stats"] == [1, 0, 0, 0] and state[0] == H + 2


def test_cut_clears_the_holds():
    h, w = 16, 24
    plate, still, det = _settled(h, w)
    moved = still.copy()
    moved[8:16, 0:8] = 0
    state = M.empty(h, w)
    M.build(state, moved, plate, det, 4, hold=9)
    assert state[2][1, 0] == 9
    out = M.build(state, still, plate, det, 4, hold=9, cut=1)
    assert not out["moving"].any() and not state[2].any() and (out["W"] == 0).all()


def test_unreal_frame_changes_nothing():
    h, w = 16, 24
    plate, still, det = _settled(h, w)
    moved = still.copy()
    moved[:8, :8] = 0
    state = M.empty(h, w)
    M.build(state, moved, plate, det, 4)
    before = [state[0], state[1], state[2].copy()]
    for kw in ({"frame_index": 1, "n_frames": 1}, {"n_frames": -1}, {"gate": 0}):
        out = M.build(state, moved, plate, det, 4, **kw)
        assert not out["real"] and out["W"] is None and out["stats"] == [0, 0, 0, 0] and not out["flags"].any()
        assert out["header"] == [h, w, 0, 0, 0, 1, 0, 0]
        assert state[0] == before[0] and state[1] == before[1] and np.array_equal(state[2], before[2])


def test_one_pixel_edge_cells_vote_with_K_64():
    h, w = 9, 9
    plate, still, det = _settled(h, w)
    moved = still.copy()
    moved[8, 8] = 0                                                         # the 1 x 1 corner cell
    moved[0, 8] = 0                                                         # one pixel of the 8 x 1 edge cell: 1 < min(64, 8)
    out = M.build(M.empty(h, w), moved, plate, det, 4, vote=64, grow=0)
    assert out["moving"].tolist() == [[False, False], [False, True]]
    assert out["stats"] == [1, 1, 1, 1]


def test_except_boxes_and_unknown():
    h, w = 16, 16
    plate, still, det0 = _settled(h, w)
    moved = still.copy()
    moved[:8, :8] = 0
    det = P.packed(4, [(0, 0, 7, 7, 2)])
    table = np.array([0, 0, 1], dtype=np.uint8)
    assert not M.build(M.empty(h, w), moved, plate, det, 4, table=table, margin=0)["moving"].any()
    assert M.build(M.empty(h, w), moved, plate, det, 4, table=np.array([0, 1, 0], dtype=np.uint8), margin=0)["moving"][0, 0]
    empty_plate = P.empty(h, w)
    assert not M.build(M.empty(h, w), moved, empty_plate, det0, 4, unknown=0)["moving"].any()
    assert M.build(M.empty(h, w), moved, empty_plate, det0, 4, unknown=1)["moving"].all()


def test_tile_flags_follow_bytes():
    W = np.zeros((17, 86), dtype=np.int64)
    W[16, 85] = 256                                                         # bytes 255..257 of row 16: both tile columns of the second tile row
    assert M.tile_flags(W).tolist() == [[0, 0], [1, 1]]


def test_option_defaults_and_normalisation():
    assert ops.redact_moving_option() == (24, 8, 4, 8, 0, "show", (), "pixelate", 16, 8, 10, 8)
    got = ops.redact_moving_option(tol=0, vote=64, hold=255, grow=32, feather=32, unknown="hide", except_classes="car", mode="blur", size=None,
                                   settle=200, plate_tol=3, margin=0)
    assert got == (0, 64, 255, 32, 32, "hide", ("car",), "blur", 12, 200, 3, 0)
    assert ops.redact_moving_option(except_classes=["all"])[6] == "all"
    assert ops.redact_moving_option(mode="fill")[7:9] == ("fill", 0)
    assert hash(got) is not None


@pytest.mark.parametrize("kw,word", [
    ({"tol": 256}, "tol"), ({"tol": -1}, "tol"), ({"tol": 1.5}, "tol"), ({"vote": 0}, "vote"), ({"vote": 65}, "vote"), ({"hold": 256}, "hold"),
    ({"hold": True}, "hold"), ({"grow": 33}, "grow"), ({"grow": -1}, "grow"), ({"feather": 33}, "feather"), ({"unknown": "maybe"}, "unknown"),
    ({"unknown": 1}, "unknown"), ({"except_classes": 5}, "except"), ({"except_classes": [""]}, "except"), ({"mode": "smear"}, "mode"),
    ({"mode": "pixelate", "size": 1}, "size"), ({"mode": "fill", "size": 3}, "size"), ({"settle": 0}, "settle"), ({"plate_tol": 256}, "plate_tol"),
    ({"margin": 65}, "margin"),
])
def test_option_refusals_by_name(kw, word):
    with pytest.raises(ValueError) as e:
        ops.redact_moving_option(**kw)
    assert "redact moving" in str(e.value) and word in str(e.value)


# ----------------------------------------------------------------------------------------------------------- the command line
NAMES = {"bg": 0, "car": 1, "person": 2}
POSITIONAL = ["rpn.h5", "det.h5", "frames"]


def _args(*flags):
    from faster_rcnn_amd import annotate_video
    return annotate_video.build_parser().parse_args(POSITIONAL + list(flags))


@pytest.mark.parametrize("flag,value", [("--moving_tol", "30"), ("--moving_min", "4"), ("--moving_hold", "2"), ("--moving_grow", "3"),
                                        ("--moving_feather", "5"), ("--moving_unknown", "hide"), ("--moving_except", "car"),
                                        ("--moving_mode", "blur"), ("--moving_size", "9"), ("--moving_out", "m.csv")])
def test_satellite_flags_are_refused_by_name_without_the_main_flag(flag, value):
    from faster_rcnn_amd import annotate_video
    with pytest.raises(ValueError) as e:
        annotate_video.redact_moving_from_args(_args(flag, value), NAMES)
    assert flag in str(e.value) and "--redact_moving" in str(e.value)
    assert annotate_video.redact_moving_from_args(_args(), NAMES) == (None, None)


def test_the_flags_become_the_option():
    from faster_rcnn_amd import annotate_video
    assert annotate_video.redact_moving_from_args(_args("--redact_moving"), NAMES) == (ops.redact_moving_option(), None)
    args = _args("--redact_moving", "--moving_tol", "30", "--moving_min", "4", "--moving_hold", "2", "--moving_grow", "3", "--moving_feather", "5",
                 "--moving_unknown", "hide", "--moving_except", "car,person", "--moving_mode", "blur", "--moving_size", "9", "--moving_out", "m.csv")
    option, out = annotate_video.redact_moving_from_args(args, NAMES)
    assert option == (30, 4, 2, 3, 5, "hide", ("car", "person"), "blur", 9, 8, 10, 8) and out == "m.csv"
    for flags, word in ((("--moving_tol", "300"), "tol"), (("--moving_min", "0"), "vote"), (("--moving_except", "unicorn"), "unicorn"),
                        (("--moving_except", ","), "--moving_except"), (("--moving_mode", "fill", "--moving_size", "3"), "size")):
        with pytest.raises(ValueError) as e:
            annotate_video.redact_moving_from_args(_args("--redact_moving", *flags), NAMES)
        assert word in str(e.value), flags


def test_the_plate_settings_go_with_either_flag():
    from faster_rcnn_amd import annotate_video
    # --remove_settle with --redact_moving alone: the removal is not asked for, the net's plate takes the setting
    args = _args("--redact_moving", "--remove_settle", "100", "--remove_tol", "5", "--remove_margin", "2")
    assert annotate_video.remove_from_args(args, NAMES) == (None, None)
    assert annotate_video.redact_moving_from_args(args, NAMES, None)[0][9:] == (100, 5, 2)
    # with --remove too the three are the removal's, and the net's option says the same
    args = _args("--redact_moving", "--remove", "car", "--remove_settle", "100")
    remove, _ = annotate_video.remove_from_args(args, NAMES)
    assert remove == (("car",), 100, 10, 8)
    assert annotate_video.redact_moving_from_args(args, NAMES, remove)[0][9:] == (100, 10, 8)
    # without either flag the refusal is what it was; --plate_out still needs --remove
    for flags in (("--remove_settle", "100"), ("--redact_moving", "--plate_out", "p.png")):
        with pytest.raises(ValueError) as e:
            annotate_video.remove_from_args(_args(*flags), NAMES)
        assert flags[-2] in str(e.value) and "--remove CLASSES" in str(e.value)
    with pytest.raises(ValueError) as e:
        ops.redact_moving_form({"settle": 9}, ("all", 8, 10, 8))
    assert "settle" in str(e.value) and "remove" in str(e.value)


def test_the_csv_and_the_printed_line(tmp_path):
    from faster_rcnn_amd import annotate_video
    assert annotate_video.moving_line(1242, 375, [0, 14904, 79177]) == M.summary_line(1242, 375, [0, 14904, 79177])
    assert M.summary_line(1242, 375, [14400] * 127 + [79177]) == "moving net 1242x375: 128 frames, mean 3.2 % hidden, peak 17.0 %"
    log = annotate_video.MovingLog(str(tmp_path / "m.csv"))
    log.add(1, 375, 1242, {"cells": 0, "covered": 0})
    log.add(2, 375, 1242, {"cells": 12, "covered": 14904})
    log.add(3, 100, 200, {"cells": 1, "covered": 64})
    log.close()
    assert (tmp_path / "m.csv").read_text() == "frame,cells,covered\n1,0,0\n2,12,14904\n3,1,64\n"
    assert log.lines() == [M.summary_line(200, 100, [64]), M.summary_line(1242, 375, [0, 14904])]
    with pytest.raises(ValueError):
        annotate_video._moving_out("m.csv", None)
