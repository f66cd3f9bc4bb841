/* Frames scaled DOWN on the device by an exact area mean, the last step of the editing chain in front of every encoder: an EXTENSION of
 * the C ABI of libfrcnn_hip.so (include/frcnn_hip.h and the other extension headers stay as they are, and so do their entry points).
 * Same library, same conventions (int status, message via the library's last-error call, `stream` = hipStream_t or NULL), a revision of
 * its own: a host that uses these entry points checks frcnn_scale_version() == FRCNN_SCALE_VERSION.
 *   1 = frcnn_downscale_u8.
 *
 * The rule (DESIGN §8 "Scale rule"; tests/scale_ref.py restates it in numpy).  Integers only: a frame has one right answer.
 *   INPUTS  a frame S[h][w][3] uint8, any channel order, and an output size (H, W) with 1 <= H <= h, 1 <= W <= w, h <= 16 H and
 *           w <= 16 W (FRCNN_SCALE_MAX_RATIO); sides 1..FRCNN_REDACT_MAX_SIDE.
 *   COLUMNS cx(X, x) = max(0, min((X + 1) w, (x + 1) W) - max(X w, x W)): the overlap of source pixel x and output pixel X on a line of
 *           w W units.  For every X the weights sum to w; they are non-zero for at most ceil(w / W) + 1 consecutive x.
 *   ROWS    ry(Y, y) is the same with h, H; for every Y the weights sum to h.
 *   OUTPUT  out[Y][X][c] = (sum_y sum_x ry(Y, y) cx(X, x) S[y][x][c] + (h w) / 2) / (h w), floor division.  The numerator is below 2^38
 *           and is held in 64 bits; the horizontal partial sum sum_x cx(X, x) S[y][x][c] is below 2^23.
 *   SO      (H, W) == (h, w) is the identity; h = N H and w = N W is the N x N box mean rounded half up; a constant frame stays what it
 *           is; and the double sum is separable without intermediate rounding, which is how the kernel works.
 *   ORDER   in a frame: behind redaction, plate fill, heat, trails, lines, boxes and labels -- labels shrink with the picture --, in
 *           front of every encoder.  Boxes that are reported stay in SOURCE coordinates. */
#ifndef FRCNN_HIP_SCALE_H
#define FRCNN_HIP_SCALE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_SCALE_VERSION 1
#define FRCNN_SCALE_MAX_RATIO 16           /* h <= 16 H and w <= 16 W */
int frcnn_scale_version(void);

/* `frames` frames scaled in ONE launch on `stream`; the grid's third dimension is the frame.  Frame f, uint8 [h][w][3] contiguous at any
 * alignment, is read at src + f * src_stride; output f, uint8 [H][W][3] contiguous, is written at dst + f * dst_stride (strides in bytes;
 * with one frame they are not read).  Frames f >= min(max(*n_frames, 0), frames) are not written; a NULL n_frames means all frames.  A
 * workgroup owns 256 output byte columns x 4 output rows: it stages the source rows of its footprint in LDS with aligned 16-byte loads,
 * forms the 32-bit horizontal sums once per source row and adds them up vertically in 64 bits; one division per output byte.  Every byte
 * has one writer, plain vector stores, no atomics, no floats.  Everything but the scalars is DEVICE memory; src and dst do not overlap.
 * No allocation, no synchronisation, nothing read on the host: the count is read by the kernel, so the call can be captured in a graph and
 * replayed.
 * FRCNN_E_ARG, with nothing launched: a null src or dst; frames outside 1..FRCNN_TRACK_MAX_FRAMES; a side of the source or of the output
 * outside 1..FRCNN_REDACT_MAX_SIDE; H > h, W > w, h > 16 H or w > 16 W; with frames > 1, src_stride < 3 h w or dst_stride < 3 H W. */
int frcnn_downscale_u8(const uint8_t* src, long long src_stride, int frames, const int32_t* n_frames, int h, int w, uint8_t* dst,
                       long long dst_stride, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_SCALE_H */
