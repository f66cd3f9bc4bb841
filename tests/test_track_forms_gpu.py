"""The eight tracker update entries (frcnn_track_update, its motion, interval and cut forms and their _weak twins) as the shims over one
argument record, one check and one frame walk that they are (csrc/track_call.h), called at the raw ABI: every entry refuses under its
own name, the refusals come in one order whatever the form, a refused call launches nothing, and the wider forms with their extras
switched off leave the bytes of the narrower one."""
import numpy as np
import pytest

from tests import track_cut_ref as C
from tests.test_track_gpu import pack

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CAP, ROWS, F, H, W = 4, 8, 2, 32, 48                        # slots, rows of a packed buffer, frames (= key buffers at interval 1), the frame
TABLE = np.array([0, 1, 1], dtype=np.uint8)
SENTINEL = 77
NAN, ALL_STRONG = float("nan"), float("-inf")
FORMS = ("", "_motion", "_interval", "_cut")


def film():
    """Two frames of one texture, the second moved by two pixels, and a box on a bright patch that moves with it."""
    rs = np.random.RandomState(11)
    first = rs.randint(0, 64, (H, W, 3)).astype(np.uint8)
    first[8:20, 10:26] += 150
    frames = np.stack([first, np.roll(first, 2, axis=1)])
    packed = np.stack([pack([[10 + 2 * f, 8, 25 + 2 * f, 19], [30, 20, 44, 30]], [1, 2], 2, ROWS, prob=[0.9, 0.6]) for f in range(F)])
    return frames, packed


class Buffers:
    """A call's device buffers: ``state`` and ``mstate`` zeroed, ``out`` full of the sentinel."""

    def __init__(self):
        from faster_rcnn_amd import ops
        frames, packed = film()
        self.frames, self.packed = torch.from_numpy(frames).cuda(), torch.from_numpy(packed).cuda()
        self.state, self.mstate = ops.track_state(CAP), ops.track_motion_state(H, W)
        self.out = torch.full((F, 4 + 8 * (ROWS + CAP)), SENTINEL, dtype=torch.int32, device="cuda")
        self.table = torch.from_numpy(TABLE).cuda()
        self.nf = torch.full((1,), F, dtype=torch.int32, device="cuda")
        self.ws, self.cuts = ops.track_cut_workspace(F), torch.full((F,), SENTINEL, dtype=torch.int32, device="cuda")

    def call(self, form, weak, **over):
        """frcnn_track_update<form>[_weak] on the null stream with well-formed arguments but for ``over`` -> (its name, its return code)."""
        from faster_rcnn_amd import _lib
        v = dict(thr=30, hold=2, grow=1, radius=4, interval=1, strong=ALL_STRONG, pct=100, workspace=self.ws.data_ptr(), cuts=self.cuts.data_ptr())
        v.update(over)
        a = [self.state.data_ptr(), CAP]
        if form:
            a += [self.mstate.data_ptr(), self.frames.data_ptr(), 3 * H * W]
        a += [self.packed.data_ptr(), 4 + 7 * ROWS, F, self.nf.data_ptr(), ROWS, self.table.data_ptr(), len(TABLE), v["thr"], v["hold"], v["grow"]]
        if form:
            a += [v["radius"]]
        if form in ("_interval", "_cut"):
            a += [v["interval"]]
        a += [H, W] + ([v["strong"]] if weak else []) + [self.out.data_ptr(), int(self.out.shape[1])]
        if form == "_cut":
            a += [v["pct"], v["workspace"], v["cuts"]]
        name = "track_update" + form + ("_weak" if weak else "")
        return name, getattr(_lib.load(), "frcnn_" + name)(*a, None)

    def refused(self, form, weak, **over):
        """The call is refused with FRCNN_E_ARG -> the message."""
        from faster_rcnn_amd import _lib
        name, code = self.call(form, weak, **over)
        assert code == -1, (name, over, code)
        return name, _lib.load().frcnn_last_error().decode()

    def untouched(self):
        torch.cuda.synchronize()
        return (self.out.cpu().numpy() == SENTINEL).all() and not self.state.cpu().numpy().any() and not self.mstate.cpu().numpy().any() \
            and (self.cuts.cpu().numpy() == SENTINEL).all()

    def ran(self, form, weak, **over):
        """The well-formed call -> the bytes it left in (state, mstate, out)."""
        name, code = self.call(form, weak, **over)
        assert code == 0, (name, code)
        torch.cuda.synchronize()
        return self.state.cpu().numpy(), self.mstate.cpu().numpy(), self.out.cpu().numpy()


def test_every_entry_refuses_under_its_own_name_and_in_one_order_and_nothing_ran():
    b = Buffers()
    for form in FORMS:
        for weak in (False, True):
            name, msg = b.refused(form, weak, thr=0)
            assert msg.startswith(name + ": thr=0"), msg
    # the order of the checks: interval, the tracking arguments, the motion ones, pct, workspace and cuts, strong
    for form, over, word in (("_cut", dict(interval=0, thr=0, pct=0), "interval"),
                             ("_cut", dict(thr=0, radius=17), "thr"),
                             ("_cut", dict(radius=17, pct=0), "radius"),
                             ("_cut", dict(pct=0, workspace=None), "pct"),
                             ("_cut", dict(cuts=None, strong=NAN), "null pointer"),
                             ("_motion", dict(radius=17, strong=NAN), "radius")):
        name, msg = b.refused(form, True, **over)
        assert msg.startswith(name + ": " + word), (over, msg)
    assert b.untouched()                                                     # one synchronize behind all of them: nothing was launched


def test_the_wider_forms_with_their_extras_off_are_the_motion_form_byte_for_byte():
    frames, _ = film()
    assert not C.is_cut(frames[0], frames[1], 100)                           # (frame 0 has no reference: the motion state starts zeroed)
    want = Buffers().ran("_motion", False)
    assert want[0][3] == F and want[2][0, 1] == 2 and want[1][:16].copy().view(np.int32)[0] == F    # both frames counted, two live rows, frame 1 kept
    cut = Buffers()
    for got, ref in zip(cut.ran("_cut", True, interval=1, strong=ALL_STRONG, pct=100), want):
        assert np.array_equal(got, ref)
    assert not cut.cuts.cpu().numpy().any()
    for got, ref in zip(Buffers().ran("_interval", True, interval=1, strong=ALL_STRONG), want):
        assert np.array_equal(got, ref)
