"""The detector head with res5a's shortcut gathered in branch2c's epilogue (nets.HEAD_ROI_RES, FRCNN_HEAD_ROI_RES=1) against the head that
resamples it into a tensor (=0): every output tensor of a pass bit-equal, eager and captured + replayed twice, for the batched pass
([roi][7][7] rows, two images) and the one-image pass (position-major rows).  Shapes small enough for seconds, large enough that the
shared-chip tile policy puts the head's 1x1 layers on the 256x128 form (>= 128 tiles of 128x128), which the tests assert."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

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


def images(n):
    rs = np.random.RandomState(9)
    x = rs.randint(0, 256, (n, H, W, 3)).astype(np.float32) - np.array([103.939, 116.779, 123.68], np.float32)
    return torch.from_numpy(x).cuda()


def flat(res):
    out = {}
    for k, v in res.items():
        for i, t in enumerate(v if isinstance(v, (list, tuple)) else [v]):
            t = t.clone()
            if k == "det_packed":                            # header words nobody writes (ops.detections allocates with torch.empty): 1 and 3,
                t[1], t[3] = 0, 0                            # and 2 except in the first image's, where the pass's status word lands
                if i > 0:                                    # (pipeline._pass_status; it is compared there and as "h3_status")
                    t[2] = 0
            out["%s[%d]" % (k, i)] = t
    return out


def run_both(monkeypatch, make_pipe, x):
    """-> {knob: (eager outputs, first replay, second replay)} and the number of gathered residuals each setting built."""
    from faster_rcnn_amd import nets, ops
    got, built = {}, {}
    real = ops.RoiResidual
    for knob in (True, False):
        count = [0]

        class counting(real):
            def __init__(self, *a, _count=count, **kw):
                _count[0] += 1
                super().__init__(*a, **kw)
        monkeypatch.setattr(nets, "HEAD_ROI_RES", knob)
        monkeypatch.setattr(ops, "RoiResidual", counting)
        pipe = make_pipe()
        with ops.conv_workspace(ops.NO_SPLIT_K), ops.tile_policy(True), ops.f32_engine("f16x3"), ops.amax_arena(ops.AmaxArena()):
            eager = flat(pipe.forward_dev(x))
        pipe.capture(H, W, split_k=False, throughput=True, f32_engine="f16x3")
        first = flat(pipe.replay(x))
        second = flat(pipe.replay(x))
        torch.cuda.synchronize()
        pipe.close()
        got[knob], built[knob] = (eager, first, second), count[0]
        monkeypatch.setattr(ops, "RoiResidual", real)
    return got, built


def check(got, built):
    assert built[True] >= 4 and built[False] == 0           # eager, two warm-up passes and the capture gathered; the other setting never did
    on, off = got[True], got[False]
    for a, b in zip(on, off):
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    for k in on[1]:
        assert torch.equal(on[1][k], on[2][k]), k           # two replays agree
    assert int(on[0]["n_rois[0]"].item()) > 0


def test_batched_pass_is_bit_equal_with_and_without(models, monkeypatch):
    from faster_rcnn_amd.pipeline import BatchedInferencePipeline
    rpn, det, anchors = models
    got, built = run_both(monkeypatch, lambda: BatchedInferencePipeline(rpn, det, anchors, 2, max_proposals=16), images(2))
    check(got, built)


def test_one_image_pass_is_bit_equal_with_and_without(models, monkeypatch):
    from faster_rcnn_amd.pipeline import InferencePipeline
    rpn, det, anchors = models
    # 32 proposals: 1 568 rows x 2 048 columns = 208 tiles of 128x128, like the batched pass above
    got, built = run_both(monkeypatch, lambda: InferencePipeline(rpn, det, anchors, max_proposals=32), images(1))
    check(got, built)
