"""Host-only checks of the cut rule's restatement (tests/track_cut_ref.py) against hand-made cases, of ops.track_cut_option and of
annotate_video's --track_scene_cut parsing and refusals.  No GPU."""
import numpy as np
import pytest

from tests import track_cut_ref as C
from tests import track_interval_ref as I
from tests import track_motion_ref as M
from tests import track_ref as T

H, W, ROWS = 48, 64, 8
TABLE = np.array([0, 1, 1, 0, 1], dtype=np.uint8)
BOXES, CLS = [[3, 4, 42, 33], [20, 10, 50, 40], [40, 5, 60, 30]], [1, 2, 4]


def pack(boxes, cls, rows=ROWS):
    p = np.zeros(4 + 7 * rows, dtype=np.int32)
    p[0] = len(cls)
    p[4:4 + 5 * rows] = -1
    for r, (b, c) in enumerate(zip(boxes, cls)):
        p[4 + 4 * r:8 + 4 * r] = b
        p[4 + 4 * rows + r] = c
        p[4 + 5 * rows + r] = T.bits(0.9 - 0.01 * r)
    return p


ALL, FIRST, NONE = pack(BOXES, CLS), pack(BOXES[:1], CLS[:1]), pack([], [])


def grey(h, w, value):
    return np.full((h, w, 3), value, dtype=np.uint8)


def scene(seed, n, lo, hi, h=H, w=W):
    """``n`` frames of one scene: noise with every channel, and so the luma, in lo..hi, each frame the last moved one pixel right."""
    rs = np.random.RandomState(seed)
    out = [rs.randint(lo, hi + 1, (h, w, 3)).astype(np.uint8)]
    for _ in range(n - 1):
        out.append(np.ascontiguousarray(M.shifted(out[-1], 1, 0)))
    return out


def scene_a(seed, n, **kw):
    return scene(seed, n, 0, 120, **kw)


def scene_b(seed, n, **kw):
    return scene(seed, n, 136, 255, **kw)


# ----------------------------------------------------------------------------------------------------------- the signature
@pytest.mark.parametrize("h,w", [(16, 24), (8, 8), (40, 64)])
def test_the_threshold_edge(h, w):
    """Half of every region's pixels move from bin 2 to bin 12: D = hw exactly, a cut at 50 and none at 51; every pixel moves: D = 2hw, a
    cut at 100."""
    a, half, b = grey(h, w, 20), grey(h, w, 20), grey(h, w, 100)
    half[:, 1::2] = 100                                                      # (w / 4 is even: half of every region's columns)
    assert M.luma(a)[0, 0] >> 3 == 2 and M.luma(b)[0, 0] >> 3 == 12
    assert C.distance(a, half) == h * w
    assert C.is_cut(a, half, 50) and not C.is_cut(a, half, 51) and C.is_cut(a, half, 1)
    assert C.distance(a, b) == 2 * h * w
    assert C.is_cut(a, b, 100) and C.is_cut(b, a, 100)
    assert C.distance(a, a) == 0 and not C.is_cut(a, a, 1)
    for pct, want in ((50, 1), (51, 0)):
        t = C.CutTracker(4)
        assert t.update_cut([a, half], [pack([], [])] * 2, 2, TABLE, h, w, pct=pct)[1].tolist() == [0, want]


def test_region_boundaries_at_sizes_that_are_no_multiple_of_4():
    h, w = 37, 53
    f = grey(h, w, 0)
    f[0, 13] = f[0, 14] = 255                                                # (4 * 13) / 53 = 0, (4 * 14) / 53 = 1
    f[9, 0] = f[10, 0] = 255                                                 # (4 * 9) / 37 = 0, (4 * 10) / 37 = 1
    f[h - 1, w - 1] = 255
    sig = C.signature(f)
    assert sig.sum() == h * w and sig.shape == (4, 4, 32)
    assert sig[..., 31].tolist() == [[1 + 1, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]]
    # every region's size is what the two divisions say
    want = np.zeros((4, 4), dtype=np.int64)
    for y in range(h):
        for x in range(w):
            want[(4 * y) // h, (4 * x) // w] += 1
    assert np.array_equal(sig.sum(axis=2), want) and want.min() >= 9 * 13 and want.max() <= 10 * 14
    rs = np.random.RandomState(0)
    noise = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    assert C.signature(noise).sum() == h * w and np.array_equal(C.signature(noise).sum(axis=2), want)
    # an object that moves INSIDE a region changes nothing; one that crosses a boundary counts twice
    g = grey(h, w, 0)
    g[0, 12] = g[0, 14] = 255
    g[9, 0] = g[10, 0] = g[h - 1, w - 1] = 255
    assert C.distance(f, g) == 0
    g[0, 12], g[0, 15] = 0, 255
    assert C.distance(f, g) == 4


def test_without_a_reference_frame_0_is_never_a_cut():
    a, b = grey(H, W, 20), grey(H, W, 100)
    t = C.CutTracker(4)
    assert t.header().tolist() == [0, 0, 0, 0]
    out, cuts = t.update_cut([a, a], [ALL, ALL], 2, TABLE, H, W, pct=1)
    assert cuts.tolist() == [0, 0] and t.header().tolist() == [2, H, W, 0]
    # the kept frame is the reference of the next call's frame 0 ...
    assert t.update_cut([b], [ALL], 1, TABLE, H, W, pct=100)[1].tolist() == [1]
    # ... unless the header was reset, ...
    t.reset_motion()
    assert t.update_cut([a], [ALL], 1, TABLE, H, W, pct=1)[1].tolist() == [0]
    # ... counts another frame than the tracker's last, ...
    t.kept -= 1
    assert t.update_cut([b], [ALL], 1, TABLE, H, W, pct=1)[1].tolist() == [0]
    # ... or the kept frame has another size
    h2, w2 = H // 2, W
    assert t.header().tolist() == [t.t.frames, H, W, 0]
    ids = [s["id"] for s in t.t.slots]
    assert t.update_cut([grey(h2, w2, 20)], [ALL], 1, TABLE, h2, w2, pct=1)[1].tolist() == [0]
    assert [s["id"] for s in t.t.slots][:1] == ids[:1]                      # (no cut: the track lives on)


# ----------------------------------------------------------------------------------------------------------- the effect
def test_a_cut_ends_every_track():
    a, b = scene_a(1, 4), scene_b(2, 4)
    for x, y in zip(a[:-1] + b[:-1], a[1:] + b[1:]):                          # inside a scene: far from the decision
        assert C.distance(x, y) * 100 * 4 < 40 * 2 * H * W
    assert C.distance(a[-1], b[0]) == 2 * H * W
    t = C.CutTracker(2)                                                      # two slots for three rows: an overflow per full frame
    # frames 0-1 see everything, frames 2-3 the first box only: track 2 is HELD when the cut arrives
    out, cuts = t.update_cut(a + b, [ALL, ALL, FIRST, FIRST, ALL, FIRST, FIRST, FIRST], 8, TABLE, H, W, 30, 3, 0, 8, 1, 40)
    assert cuts.tolist() == [0, 0, 0, 0, 1, 0, 0, 0]
    ids_before = {int(i) for f in range(4) for i in T.split(out[f])[7] if i > 0}
    assert ids_before == {1, 2} and T.split(out[3])[0] - T.split(out[3])[1] == 1          # a held row in front of the cut
    overflow_before, next_before = T.split(out[3])[3], T.split(out[3])[2]
    assert overflow_before == 2 and next_before == 3
    n_rows, n_live, next_id, overflow, _, _, _, ids, age = T.split(out[4])
    assert n_rows == n_live == 3 and sorted(ids[:3].tolist()) == [0, 3, 4]                # new ids only, no held row
    assert next_id == 5 and overflow == overflow_before + 1                               # `issued` and `overflow` are carried
    for f in range(4, 8):
        n_rows, n_live, _, _, _, _, _, ids, age = T.split(out[f])
        assert all(i == 0 or i > max(ids_before) for i in ids[:n_rows].tolist())
        held = ids[n_live:n_rows].tolist()
        assert held == ([] if f == 4 else [4]) and all(i > max(ids_before) for i in held)  # only the new scene's own tracks age
    assert t.t.frames == 8 and t.header().tolist() == [8, H, W, 0]
    # the same frames with the cut rule switched off (pct can not be reached: D = 2hw is needed at 100, so compare with the interval rule)
    u = I.IntervalTracker(2)
    plain = u.update_interval(a + b, [ALL, ALL, FIRST, FIRST, ALL, FIRST, FIRST, FIRST], 8, TABLE, H, W, 30, 3, 0, 8, 1)
    assert T.split(plain[4])[7][0] == 1                                      # without the rule the id carries over


def test_a_cut_on_a_between_frame_leaves_empty_outputs_until_the_next_key_frame():
    a, b = scene_a(3, 4), scene_b(4, 5)
    t = C.CutTracker(4)
    frames = a + b                                                           # key frames 0, 3, 6; the cut is frame 4
    out, cuts = t.update_cut(frames, [ALL, ALL, ALL], 9, TABLE, H, W, 30, 3, 0, 8, 3, 40)
    assert cuts.tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0]
    for f in (1, 2, 3):
        assert T.split(out[f])[0] == 3
    for f in (4, 5):
        n_rows, n_live, next_id, overflow, bbox, cls, prob, ids, age = T.split(out[f])
        assert (n_rows, n_live, next_id, overflow) == (0, 0, 4, 0)
        assert (bbox == -1).all() and (cls == -1).all() and not prob.any() and not ids.any() and not age.any()
    assert T.split(out[6])[7][:3].tolist() == [4, 5, 6]
    for f in (7, 8):
        assert T.split(out[f])[7][:3].tolist() == [4, 5, 6] and T.split(out[f])[0] == 3
    assert t.t.frames == 9                                                   # every real frame counts, the empty ones too


@pytest.mark.parametrize("interval", [1, 3])
def test_without_a_cut_every_byte_is_the_interval_rule_s(interval):
    frames = scene_a(5, 8)
    c, i = C.CutTracker(2), I.IntervalTracker(2)
    at = 0
    for F, nf in ((1, 1), (4, 4), (3, 2)):
        packed = [(ALL, NONE, FIRST)[k % 3] for k in range(I.keys_of(F, interval))]
        got, cuts = c.update_cut(frames[at:at + F], packed, nf, TABLE, H, W, 30, 2, 3, 8, interval, 40)
        want = i.update_interval(frames[at:at + F], packed, nf, TABLE, H, W, 30, 2, 3, 8, interval)
        assert not cuts.any() and cuts.dtype == np.int32 and cuts.shape == (F,)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        assert np.array_equal(c.t.words(), i.t.words()) and np.array_equal(c.motion_bytes(H, W), i.motion_bytes(H, W))
        at += F
    assert c.moves == i.moves and c.moves


def test_frames_behind_n_frames_are_untouched_and_no_cut():
    a, b = scene_a(6, 2), scene_b(7, 2)
    t = C.CutTracker(4)
    t.update_cut(a[:1], [ALL], 1, TABLE, H, W)
    words, kept = t.t.words(), t.motion_bytes(H, W)
    out, cuts = t.update_cut([b[0], a[1]], [ALL, ALL], 0, TABLE, H, W)       # nothing is real: the cut at frame 0 is not seen
    assert cuts.tolist() == [0, 0] and np.array_equal(t.t.words(), words) and np.array_equal(t.motion_bytes(H, W), kept)
    assert all(np.array_equal(o, t.t.padding(ROWS)) for o in out)
    out, cuts = t.update_cut([a[1], b[0], a[0]], [ALL, ALL, ALL], 1, TABLE, H, W)
    assert cuts.tolist() == [0, 0, 0] and t.t.frames == 2 and [s["id"] for s in t.t.slots] == [1, 2, 3]
    assert all(np.array_equal(o, t.t.padding(ROWS)) for o in out[1:])
    assert np.array_equal(t.frame, a[1])
    out, cuts = t.update_cut([b[0], b[1], a[0]], [ALL, ALL, ALL], 2, TABLE, H, W)
    assert cuts.tolist() == [1, 0, 0] and t.t.frames == 4 and [s["id"] for s in t.t.slots] == [4, 5, 6]


# ----------------------------------------------------------------------------------------------------------- the option
def test_track_cut_option():
    from faster_rcnn_amd import ops
    assert ops.TRACK_CUT_PCT == C.PCT == (1, 100, 40)
    assert [ops.track_cut_option(p) for p in (None, 1, 40, 100, np.int64(55))] == [40, 1, 40, 100, 55]
    assert ops.track_cut_option() == 40
    for bad in (0, 101, -1, True, 40.0, "40", (40,)):
        with pytest.raises(ValueError) as e:
            ops.track_cut_option(bad)
        assert "1..100" in str(e.value)


def parse(*extra):
    from faster_rcnn_amd import annotate_video
    return annotate_video.build_parser().parse_args(["a.h5", "b.h5", "frames"] + list(extra))


def test_the_parser_reads_track_scene_cut():
    from faster_rcnn_amd import annotate_video
    cut = annotate_video.track_scene_cut_from_args
    assert cut(parse()) is None and cut(parse("--track", "--track_motion")) is None
    assert cut(parse("--track", "--track_motion", "--track_scene_cut")) == 40             # bare: the default
    assert cut(parse("--track", "--track_motion", "--track_scene_cut", "55")) == 55
    assert cut(parse("--track", "--track_motion", "4", "--detect_every", "3", "--track_scene_cut", "100")) == 100
    text = annotate_video.build_parser().format_help()
    assert "--track_scene_cut [PCT]" in text and "provisional" in text


def test_the_parser_refuses_track_scene_cut_with_a_reason():
    from faster_rcnn_amd import annotate_video
    cut = annotate_video.track_scene_cut_from_args
    for extra in (["--track_scene_cut"], ["--track", "--track_scene_cut", "40"], ["--track_motion", "8", "--track_scene_cut"]):
        with pytest.raises(ValueError) as e:
            cut(parse(*extra))
        assert "--track_scene_cut" in str(e.value) and "needs --track --track_motion" in str(e.value)
    with pytest.raises(ValueError) as e:
        cut(parse("--track", "--track_motion", "--track_lookback", "--track_scene_cut"))
    assert "--track_lookback" in str(e.value) and "not supported" in str(e.value)
    with pytest.raises(ValueError) as e:
        cut(parse("--track", "--track_motion", "--detect_every", "4", "--track_backtrack", "--track_scene_cut"))
    assert "--track_backtrack" in str(e.value) and "not supported" in str(e.value)
    for bad in ("0", "101", "-3"):
        with pytest.raises(ValueError) as e:
            cut(parse("--track", "--track_motion", "--track_scene_cut", bad))
        assert "--track_scene_cut" in str(e.value) and "1..100" in str(e.value)


def test_the_pipelines_refuse_with_a_reason():
    from faster_rcnn_amd import annotate_video
    track = (30, 8, 0)
    check = annotate_video._track_scene_cut
    assert check(None, None, None, None, None) is None
    assert check(40, track, 8, None, None) == 40 and check(np.int64(7), track, 8, None, None) == 7
    for t, m in ((None, None), (track, None), (None, 8)):
        with pytest.raises(ValueError, match="track=.*track_motion="):
            check(40, t, m, None, None)
    with pytest.raises(ValueError, match="track_lookback.*not supported"):
        check(40, track, 8, 4, None)
    with pytest.raises(ValueError, match="track_backtrack.*not supported"):
        check(40, track, 8, None, 4)
    with pytest.raises(ValueError, match="1..100"):
        check(0, track, 8, None, None)
