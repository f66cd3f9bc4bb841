"""Mirror of the reference's args_util.py flag grammar (args_util.py:7-77)."""
from .data.voc_data_helpers import extract_img_data, get_img_names_from_set
from .train import optimizer_from_str  # noqa: F401  ('sgd' -> SGD(momentum 0.9), else Adam; args_util.py:48-59)


def base_paths_to_imgs(base_path_str, img_set="trainval", do_flip=True):
    """args_util.py:7-27: comma-separated VOC roots -> Image list (+ horizontally flipped copies)."""
    imgs = []
    for path in base_path_str.split(","):
        imgs.extend(extract_img_data(path, name) for name in get_img_names_from_set(path, img_set))
    if do_flip:
        imgs += [img.horizontal_flip() for img in imgs]
    return imgs


def phases_from_str(phases_str):
    """'60000:1e-3,20000:1e-4' -> [[60000, 1e-3], [20000, 1e-4]] (args_util.py:30-45)."""
    return [[int(p.split(":")[0]), float(p.split(":")[1])] for p in phases_str.split(",")]


def resize_dims_from_str(resize_dims_str):
    return [int(d) for d in resize_dims_str.split(",")]


def anchor_scales_from_str(anchor_scales_str):
    return [int(d) for d in anchor_scales_str.split(",")]


from ._lib import DETECT_POST_MODES as NMS_MODES          # (one list: the C ABI's mode numbers are its indices)


def add_post_arguments(p):
    """The five post-process arguments voc_dets and annotate_video share (DESIGN §8 "Post-process rule")."""
    p.add_argument("--nms", dest="nms", choices=NMS_MODES, default=None,
                   help="the detection post-process's NMS: hard (the reference's, the default), soft_linear or soft_gaussian (Soft-NMS: an "
                        "overlapped box loses score instead of being deleted; the written prob is the decayed score)")
    p.add_argument("--nms_thresh", dest="nms_thresh", type=float, default=None, help="IoU above which hard deletes and soft_linear decays (0.5)")
    p.add_argument("--nms_sigma", dest="nms_sigma", type=float, default=None,
                   help="soft_gaussian's sigma (0.5, provisional: not tuned on a dataset); only with --nms soft_gaussian")
    p.add_argument("--nms_min_score", dest="nms_min_score", type=float, default=None,
                   help="a soft mode stops a class when its best decayed score falls under this (default: the detection threshold; "
                        "provisional); not with --nms hard")
    p.add_argument("--box_vote", dest="box_vote", type=float, nargs="?", const=0.5, default=None, metavar="IOU",
                   help="box voting: a detection's box becomes the score-weighted mean of its class's boxes that overlap it by at least "
                        "IOU (bare: 0.5, provisional)")


def post_from_args(args):
    """The post-process option of a parsed command line -> None when none of the five arguments was given (nothing changes then), else
    ops.det_post_option's tuple.  Arguments that depend on another are refused by name: ValueError with the reason."""
    given = [getattr(args, k, None) for k in ("nms", "nms_thresh", "nms_sigma", "nms_min_score", "box_vote")]
    if all(v is None for v in given):
        return None
    mode = args.nms or "hard"
    if args.nms_sigma is not None and mode != "soft_gaussian":
        raise ValueError("--nms_sigma needs --nms soft_gaussian (it is the gaussian weight's sigma; the mode here is %s)" % mode)
    if args.nms_min_score is not None and mode == "hard":
        raise ValueError("--nms_min_score needs --nms soft_linear or soft_gaussian (hard NMS decays no score)")
    from . import ops
    return ops.det_post_option((mode, args.nms_thresh, args.nms_sigma, args.nms_min_score, args.box_vote))
