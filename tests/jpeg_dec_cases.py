"""The files the device JPEG decoder is tested on (tests/test_jpeg_dec_cpu.py holds the CPU restatement to Pillow on them,
tests/test_jpeg_dec_gpu.py the kernels to the restatement): written by Pillow from the frames of tests/jpeg_cases.py, at the smallest
sizes at which each edge rule can go wrong (1x1; one block; a chroma plane of width 2 or less; odd sides with 2x1 and 2x2 sampling;
more than one MCU row; the encoder's long-file case), plus the golden VOC image."""
import functools
import io
import os

import numpy as np

from tests import jpeg_cases as J

GOLDEN = os.path.join(J.ROOT, "tests", "golden", "VOC_test", "JPEGImages", "000005.jpg")
SIZES = [(1, 1), (8, 8), (7, 9), (16, 16), (17, 23), (33, 65), (64, 136)]
LONG = ((0, 100), (1, 75), (2, 10))     # (subsampling, quality) at 64x136: sampling and quality are crossed in full at the smaller sizes
DAMAGE_OF = "33x65_s2_q75"


def write(frame, mode="RGB", **kw):
    from PIL import Image
    out = io.BytesIO()
    Image.fromarray(frame if mode == "RGB" else np.ascontiguousarray(frame[:, :, 0])).save(out, "JPEG", **kw)
    return out.getvalue()


def frame(h, w):
    return J.CASES["noise_64x136"] if (h, w) == (64, 136) else J.noise(h, w, 100 * h + w)


@functools.lru_cache(None)
def files():
    """name -> the file's bytes."""
    out = {"golden_000005": open(GOLDEN, "rb").read()}
    for h, w in SIZES:
        for ss in (0, 1, 2):
            for q in (10, 75, 100):
                if (h, w) == (64, 136) and (ss, q) not in LONG:
                    continue
                out["%dx%d_s%d_q%d" % (h, w, ss, q)] = write(frame(h, w), quality=q, subsampling=ss)
    photo = J.CASES["photo_96x128"]
    out["photo_s2_q75_optimize"] = write(photo, quality=75, subsampling=2, optimize=True)
    out["photo_s1_q90_optimize_rst16"] = write(photo[:41, :77], quality=90, subsampling=1, optimize=True, restart_marker_blocks=16)
    out["17x23_s2_q75_rst1"] = write(frame(17, 23), quality=75, subsampling=2, restart_marker_blocks=1)
    out["33x65_s0_q100_rst16"] = write(frame(33, 65), quality=100, subsampling=0, restart_marker_blocks=16)
    out["33x65_s2_q10_optimize_rst1"] = write(frame(33, 65), quality=10, subsampling=2, optimize=True, restart_marker_blocks=1)
    out["grey_17x23_q75"] = write(frame(17, 23), mode="L", quality=75)
    out["grey_33x65_q100_optimize"] = write(frame(33, 65), mode="L", quality=100, optimize=True)
    return out


SMALLEST = ("1x1_s0_q75", "1x1_s2_q75", "7x9_s1_q100", "7x9_s2_q75", "17x23_s1_q75", "17x23_s2_q100")
LARGEST = ("golden_000005", "64x136_s0_q100")


def damaged():
    """A supported file with a stretch of its scan overwritten: the headers stand, the block total does not."""
    from tests import jpeg_dec_ref as D
    data = bytearray(files()[DAMAGE_OF])
    p = D.plan(bytes(data))
    at = p.scan_off + p.scan_len // 3
    data[at:at + 96] = bytes([0x5A, 0x00, 0xA5, 0x0F] * 24)
    return bytes(data)


def patch_sof(data, component, value):
    """The file with one component's sampling byte (component None: the precision byte) of its frame header replaced: what lies
    outside the supported set is decided from the headers alone."""
    at = data.index(b"\xFF\xC0") + 4
    data = bytearray(data)
    data[at if component is None else at + 7 + 3 * component] = value
    return bytes(data)


def unsupported():
    """name -> (bytes, a word of the reason): every kind outside the supported set that Pillow writes here (progressive, CMYK, R G B
    kept as it is: Adobe transform 0), and, since every ``subsampling`` Pillow offers lies inside the set ("4:1:1" is its old name for
    4:2:0), frame headers patched to other sampling factors and to 12 bits."""
    f = frame(17, 23)
    from PIL import Image
    cmyk = io.BytesIO()
    Image.fromarray(f).convert("CMYK").save(cmyk, "JPEG", quality=75)
    return {
        "progressive": (write(f, quality=75, progressive=True), "progressive"),
        "cmyk": (cmyk.getvalue(), "CMYK"),
        "sampling_1x2": (patch_sof(write(f, quality=75, subsampling=1), 0, 0x12), "sampling"),
        "sampling_chroma_2x1": (patch_sof(write(f, quality=75, subsampling=1), 1, 0x21), "sampling"),
        "12_bit": (patch_sof(write(f, quality=75), None, 12), "12-bit"),
        "rgb_ids": (write(f, quality=75, keep_rgb=True), "Adobe transform 0"),
    }
