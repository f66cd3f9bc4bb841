"""The plane-reading ring with its rows assigned to tiles by padding class (csrc/conv_h3.hip h3_ring_tile<.., ROWMAP>,
include/ext/frcnn_hip_rowmap.h; ``ops.conv2d(..., rowmap=)``) against the unmapped launch of the same layer on the same planes, BIT FOR
BIT (torch.equal on integer views), after asserting that the mapped entry point was the one called.

  RoIs     1, 5 (every class a partial tile), 6 (294 rows: a RoI straddles the unmapped launch's tile boundary), 256 (one full super-group:
           49 full tiles, nothing padded), 257 (one RoI past it: nine more tiles of one RoI's rows), 300 (a partial last group).
  depth    Cin = 64 and 128 (two and four 32-channel groups: 8 / 16 chunks in a corner tile, 18 / 36 in an interior one).
  columns  Cout = 128 and 192 (a partial second column tile).
  output   f32 and fp16 planes; with and without a ReLU; the magnitude record and the planes' exponent equal too.
Each mapped launch runs twice into buffers of its own, poisoned with NaN beforehand where the allocator hands the block back.
One case is captured and replayed twice with the cached map; one MUTATION: a tap bit dropped from an interior tile's word must break the
equality (or the comparison would prove nothing); and the batched head with the knob on and off, eager and replayed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POOL, TILE = 7, 86
N_ROIS = [1, 5, 6, 256, 257, 300]


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


@pytest.fixture(scope="module")
def data():
    from faster_rcnn_amd import ops
    rs = np.random.RandomState(33)
    d = {"x": {}, "pc0": {}, "pc": {}}
    for cin in (64, 128):
        d["x"][cin] = torch.from_numpy(rs.randn(max(N_ROIS), POOL, POOL, cin).astype(np.float32)).cuda()
        d["pc0"][cin] = ops.PackedConv((rs.randn(1, 1, cin, cin) * np.sqrt(2.0 / cin)).astype(np.float32))
        for cout in (128, 192):
            wt = (rs.randn(3, 3, cin, cout) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
            d["pc"][cin, cout] = ops.PackedConv(wt, (1 + 0.1 * rs.randn(cout)).astype(np.float32), (0.1 * rs.randn(cout)).astype(np.float32))
    return d


def planes_of(data, n, cin, x=None):
    from faster_rcnn_amd import ops
    x = data["x"][cin][:n].contiguous() if x is None else x
    p = ops.conv2d(x, data["pc0"][cin], 1, "valid", "relu", tile=TILE, planes_out=True)
    assert isinstance(p, ops.PlaneTensor)
    return p


def poison(shape, planes):
    """A NaN-filled block of the result's size, freed again: the next allocation of that size is likely to be it, so a row the mapped
    launch failed to store would not compare equal by accident."""
    t = torch.full(((2,) + tuple(shape)) if planes else tuple(shape), float("nan"), dtype=torch.float16 if planes else torch.float32, device="cuda")
    del t


def same(got, want, planes):
    from faster_rcnn_amd import ops
    if planes:
        assert isinstance(got, ops.PlaneTensor) and isinstance(want, ops.PlaneTensor)
        ok = torch.equal(bits(got.planes), bits(want.planes)) and torch.equal(got.exponent, want.exponent)
    else:
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape)
        ok = torch.equal(bits(got), bits(want))
    # the magnitude record: a maximum over the same values (whichever slots they landed in), status word clean
    ga, wa = got._amax.view(-1, 32), want._amax.view(-1, 32)
    return ok and float(ga[:, 0].max()) == float(wa[:, 0].max()) and int(bits(got._amax)[1].item()) == int(bits(want._amax)[1].item()) == 0


def run_pair(x, pc, act, planes_out, times=2):
    """-> (unmapped result, [mapped results]); asserts which entry point each launch took."""
    from faster_rcnn_amd import ops
    ops.CONV_PROFILE = rec = []
    try:
        want = ops.conv2d(x, pc, 1, "same", act, tile=TILE, planes_out=planes_out)
        gots = []
        for _ in range(times):
            poison(want.shape, planes_out)
            gots.append(ops.conv2d(x, pc, 1, "same", act, tile=TILE, planes_out=planes_out, rowmap="force"))
    finally:
        ops.CONV_PROFILE = None
    torch.cuda.synchronize()
    assert len(rec) == 1 + times and not rec[0].get("rowmap") and all(r.get("rowmap") for r in rec[1:])
    n = x.shape[0]
    assert all(r["shape"] == (n * 49, pc.cout, 9 * pc.cin, 1, "rowmap") and r["kernel"] == "k_conv_igemm_h3_db<2,1,4,4,planes>" for r in rec[1:])
    return want, gots


@pytest.mark.parametrize("cout", [128, 192])
@pytest.mark.parametrize("cin", [64, 128])
@pytest.mark.parametrize("n", N_ROIS)
def test_mapped_launch_equals_the_unmapped_launch(data, n, cin, cout):
    from faster_rcnn_amd import ops
    pc = data["pc"][cin, cout]
    with ops.f32_engine("f16x3"), ops.conv_workspace(ops.NO_SPLIT_K):
        x = planes_of(data, n, cin)
        assert ops.conv_takes_rowmap(x, pc, 1, "same", "relu", 0, TILE)
        for planes_out in (False, True):
            for act in ("relu", None):
                want, gots = run_pair(x, pc, act, planes_out)
                v = want.float() if planes_out else want
                assert tuple(v.shape) == (n, POOL, POOL, cout) and bool(torch.isfinite(v).all())
                assert bool((v == 0).any()) == (act == "relu") and bool((v > 0).any())
                for got in gots:
                    if not planes_out:
                        print("n %d cin %d cout %d act %s: max |mapped - unmapped| = %g" % (n, cin, cout, act, float((got - want).abs().max())))
                    assert same(got, want, planes_out), (n, cin, cout, planes_out, act)
                assert (gots[0].planes if planes_out else gots[0]).data_ptr() != (gots[1].planes if planes_out else gots[1]).data_ptr()


def test_request_is_declined_where_the_map_does_not_pay_or_the_launch_cannot(data):
    """rowmap=True (the head's request): five RoIs' map saves nothing -> the plain launch; 256 RoIs' pays -> the mapped one; f32 input, a
    residual or another tile -> the plain launch, same results."""
    from faster_rcnn_amd import ops
    pc = data["pc"][64, 128]
    with ops.f32_engine("f16x3"), ops.conv_workspace(ops.NO_SPLIT_K):
        for n, mapped in ((5, False), (256, True)):
            x = planes_of(data, n, 64)
            ops.CONV_PROFILE = rec = []
            try:
                got = ops.conv2d(x, pc, 1, "same", "relu", tile=TILE, rowmap=True)
                want = ops.conv2d(x, pc, 1, "same", "relu", tile=TILE)
                res = torch.zeros_like(want)
                with_res = ops.conv2d(x, pc, 1, "same", "relu", residual=res, tile=TILE, rowmap=True)
                other_tile = ops.conv2d(x, pc, 1, "same", "relu", tile=82, rowmap=True)
                f32_in = ops.conv2d(data["x"][64][:n].contiguous(), pc, 1, "same", "relu", tile=TILE, rowmap=True)
            finally:
                ops.CONV_PROFILE = None
            assert [bool(r.get("rowmap")) for r in rec] == [mapped, False, False, False, False]
            assert torch.equal(bits(got), bits(want)) and torch.equal(bits(with_res), bits(want)) and torch.equal(bits(other_tile), bits(want))
            assert tuple(f32_in.shape) == tuple(want.shape)
        assert not ops.conv_takes_rowmap(data["x"][64][:5].contiguous(), pc, 1, "same", "relu", 0, TILE)
        assert not ops.conv_takes_rowmap(planes_of(data, 5, 64), pc, 1, "same", "relu", 0, 85)


def test_captured_graph_replays_with_the_cached_map(data):
    from faster_rcnn_amd import ops
    n, cin, cout = 257, 64, 192
    pc = data["pc"][cin, cout]
    rs = np.random.RandomState(5)
    a = data["x"][cin][:n].contiguous()
    b = torch.from_numpy(rs.randn(n, POOL, POOL, cin).astype(np.float32)).cuda()
    static = a.clone()
    arena = ops.AmaxArena()
    with ops.f32_engine("f16x3"), ops.conv_workspace(ops.NO_SPLIT_K), ops.amax_arena(arena):
        wants = []
        for src in (a, b):
            ops.amax_begin()
            wants.append(ops.conv2d(planes_of(data, n, cin, src), pc, 1, "same", "relu", tile=TILE).clone())
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                       # the warm-up pass uploads the map: a capture cannot
            ops.amax_begin()
            warm = ops.conv2d(planes_of(data, n, cin, static), pc, 1, "same", "relu", tile=TILE, rowmap="force")
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert torch.equal(bits(warm), bits(wants[0]))
        cached = len(ops._ROWMAP_CACHE)
        g = torch.cuda.CUDAGraph()
        ops.CONV_PROFILE = rec = []
        try:
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                ops.amax_begin()
                out = ops.conv2d(planes_of(data, n, cin, static), pc, 1, "same", "relu", tile=TILE, rowmap="force")
        finally:
            ops.CONV_PROFILE = None
        assert rec[-1].get("rowmap") and len(ops._ROWMAP_CACHE) == cached
        for src, want in ((a, wants[0]), (b, wants[1]), (a, wants[0])):
            static.copy_(src)
            out.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(bits(out), bits(want))
        assert int(arena.status().item()) == 0
        g.reset()
    assert not torch.equal(bits(wants[0]), bits(wants[1]))


def test_mutation_a_dropped_tap_bit_breaks_the_equality(data):
    """One tap bit cleared in ONE interior tile's word: that tile's rows lose the products of one tap, and the comparison above fails."""
    from faster_rcnn_amd import ops
    n, cin, cout = 256, 64, 128
    pc = data["pc"][cin, cout]
    with ops.f32_engine("f16x3"), ops.conv_workspace(ops.NO_SPLIT_K):
        x = planes_of(data, n, cin)
        want = ops.conv2d(x, pc, 1, "same", "relu", tile=TILE)
        d = ops._conv_desc(tuple(x.shape), 3, 3, cout, 1, "same", ops.ACT["relu"], 0, TILE)
        row_map, taps = ops._conv_rowmap(d, force=True)
        words = taps.cpu().numpy().view(np.uint32)
        interior = int(np.flatnonzero(words == 0x1ff)[3])
        clean = ops._conv2d_h3_planes(d, x, pc, None, tuple(want.shape), False, "relu", (row_map, taps))
        mutated = taps.clone()
        mutated[interior] = int(words[interior]) & ~(1 << 4)                  # the centre tap: it meets the image for every row
        broken = ops._conv2d_h3_planes(d, x, pc, None, tuple(want.shape), False, "relu", (row_map, mutated))
        torch.cuda.synchronize()
    assert torch.equal(bits(clean), bits(want))
    assert not torch.equal(bits(broken), bits(want))
    rows = row_map.cpu().numpy()[interior * 256:(interior + 1) * 256]
    differ = (bits(broken) != bits(want)).reshape(n * 49, cout).any(dim=1).cpu().numpy()
    print("mutation: %d rows differ, all %d of them in tile %d" % (int(differ.sum()), int(differ[rows].sum()), interior))
    assert differ.sum() > 0 and set(np.flatnonzero(differ)) <= set(int(r) for r in rows)       # and only that tile's rows


# ---- the batched head, knob on and off
H, W = 160, 192


@pytest.fixture(scope="module")
def models():
    from faster_rcnn_amd import resnet, util
    from faster_rcnn_amd.weights import synthetic_resnet
    anchors = util.get_anchors([128, 256, 512])
    w = synthetic_resnet(50, anchors_per_loc=9, num_classes=21, seed=4)
    base = resnet.resnet50_base(weights=w)
    rpn = resnet.resnet50_rpn(base, include_conv=True, anchors_per_loc=9)
    det = resnet.resnet50_classifier(300, 21, weights=w)
    return rpn, det, anchors


def flat(res):
    out = {}
    for k, v in res.items():
        for i, t in enumerate(v if isinstance(v, (list, tuple)) else [v]):
            t = t.clone()
            if k == "det_packed":                            # header words nobody writes (tests/test_head_roi_res_gpu.py)
                t[1], t[3] = 0, 0
                if i > 0:
                    t[2] = 0
            out["%s[%d]" % (k, i)] = t
    return out


def test_batched_head_is_bit_equal_with_and_without(models, monkeypatch):
    """Two images of 128 proposals: 256 RoIs, 12 544 rows -- the 3x3 layers run the 256x128 form under the shared-chip policy and the map
    pays, so those of the three that read planes (res5b / res5c always; res5a where the conv4 pair left a magnitude record for the crops)
    take the mapped entry with the knob on, none with it off; every output of the pass equal."""
    from faster_rcnn_amd import nets, ops
    from faster_rcnn_amd.pipeline import BatchedInferencePipeline
    rpn, det, anchors = models
    rs = np.random.RandomState(9)
    x = torch.from_numpy(rs.randint(0, 256, (2, H, W, 3)).astype(np.float32) - np.array([103.939, 116.779, 123.68], np.float32)).cuda()
    got, mapped = {}, {}
    for knob in (True, False):
        monkeypatch.setattr(nets, "HEAD_ROWMAP", knob)
        pipe = BatchedInferencePipeline(rpn, det, anchors, 2, max_proposals=128)
        ops.CONV_PROFILE = rec = []
        try:
            with ops.conv_workspace(ops.NO_SPLIT_K), ops.tile_policy(True), ops.f32_engine("f16x3"), ops.amax_arena(ops.AmaxArena()):
                eager = flat(pipe.forward_dev(x))
        finally:
            ops.CONV_PROFILE = None
        three = [r for r in rec if r["shape"][0] == 256 * 49 and r["shape"][2] == 9 * 512]
        plane_in = [r for r in three if r["kernel"].endswith(",planes>")]
        assert len(three) == 3 and len(plane_in) >= 2
        assert all(bool(r.get("rowmap")) == knob for r in plane_in) and not any(r.get("rowmap") for r in rec if r not in plane_in)
        mapped[knob] = sum(1 for r in rec if r.get("rowmap"))
        pipe.capture(H, W, split_k=False, throughput=True, f32_engine="f16x3")
        first = flat(pipe.replay(x))
        second = flat(pipe.replay(x))
        torch.cuda.synchronize()
        pipe.close()
        got[knob] = (eager, first, second)
    assert mapped[True] >= 2 and mapped[False] == 0
    for a, b in zip(got[True], got[False]):
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    for k in got[True][1]:
        assert torch.equal(got[True][1][k], got[True][2][k]), k
    assert int(got[True][0]["n_rois[0]"].item()) > 0
