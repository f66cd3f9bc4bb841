/* Detected objects hidden in a uint8 frame on the device: an EXTENSION of the C ABI of libfrcnn_hip.so (include/frcnn_hip.h and the
 * other extension headers stay as they are).  Same library, same conventions (int status, message via frcnn_last_error, `stream` =
 * hipStream_t or NULL), a revision of its own: a host that uses these entry points checks frcnn_redact_version() == FRCNN_REDACT_VERSION.
 *   1 = frcnn_redact_ws_bytes, frcnn_redact_u8.
 *
 * The rule (DESIGN §8 "Redaction rule"; tests/redact_ref.py restates it in numpy).  S is the frame, [h][w][3] uint8 in any channel order.
 *   MASK    pixel (x, y) is masked when a row r < *n_dets has 0 <= det_cls[r] < num_classes, redact[det_cls[r]] != 0 and
 *           xa <= x <= xb, ya <= y <= yb with xa = max(min(x1, x2) - margin, 0), xb = min(max(x1, x2) + margin, w - 1), ya and yb
 *           likewise from y1, y2 and h.  A box that crosses the frame's border is redacted where it lies inside (the drawing rule drops
 *           such a box); one with xa > xb or ya > yb is empty.
 *   OUTPUT  out = masked ? R : S, with R a function of S alone:
 *     FILL      R = 0.
 *     PIXELATE  size = P: cell (i, j) of the grid anchored at the origin covers rows [iP, min((i + 1)P, h)) and columns
 *               [jP, min((j + 1)P, w)), n pixels; per channel R = (sum of S over the cell + n / 2) / n.
 *     BLUR      size = r, k = 2r + 1, coordinates clamped to the frame:
 *               H[y][x][c] = (sum over d = -r..r of S[y][clamp(x + d, 0, w - 1)][c] + k / 2) / k,
 *               R[y][x][c] = (sum over d = -r..r of H[clamp(y + d, 0, h - 1)][x][c] + k / 2) / k, both rounded to uint8 as written.
 *   Integer arithmetic with integer division: one right answer per frame, whatever the order of the rows. */
#ifndef FRCNN_HIP_REDACT_H
#define FRCNN_HIP_REDACT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_REDACT_VERSION 1
#define FRCNN_REDACT_MAX_ROWS 512
#define FRCNN_REDACT_MAX_SIDE 32768
int frcnn_redact_version(void);

/* modes, and the range of `size` in each */
#define FRCNN_REDACT_FILL 0       /* size must be 0 */
#define FRCNN_REDACT_PIXELATE 1   /* size = the cell's side P, 2..64 */
#define FRCNN_REDACT_BLUR 2       /* size = the radius r, 1..32 */
#define FRCNN_REDACT_PIXELATE_MIN 2
#define FRCNN_REDACT_PIXELATE_MAX 64
#define FRCNN_REDACT_BLUR_MIN 1
#define FRCNN_REDACT_BLUR_MAX 32

/* Bytes of workspace frcnn_redact_u8 needs for a frame of h x w: the cell means (PIXELATE: ceil(h / P) * ceil(w / P) * 3) or H (BLUR:
 * h * w * 3); 0 for FILL -- and 0 for a side outside 1..FRCNN_REDACT_MAX_SIDE, an unknown mode or a size outside the mode's range. */
size_t frcnn_redact_ws_bytes(int h, int w, int mode, int size);

/* frame ([h][w][3] uint8, contiguous, DEVICE) is edited in place.  det_bbox ([max_rows][4] int32: x1, y1, x2, y2), det_cls ([max_rows]
 * int32) and n_dets (one int32) are what frcnn_detections(_dyn) wrote, on the device; rows >= *n_dets are never read.  redact: uint8
 * [num_classes] on the device.  Two launches on `stream`: the first reads the frame and writes the workspace (nothing for FILL), the
 * second replaces the masked pixels from the workspace alone.  No allocation, no synchronisation, nothing read on the host: *n_dets is
 * read by the kernels, so the call can be captured in a graph and replayed with other detections.  With *n_dets <= 0 no byte of the
 * frame is written.  `workspace` needs no alignment and may be NULL for FILL.
 * FRCNN_E_ARG, with nothing launched: a null pointer; a side outside 1..FRCNN_REDACT_MAX_SIDE; max_rows outside
 * 1..FRCNN_REDACT_MAX_ROWS; num_classes outside 1..256; an unknown mode; a size outside the mode's range; margin < 0; ws_bytes smaller
 * than frcnn_redact_ws_bytes(h, w, mode, size). */
int frcnn_redact_u8(uint8_t* frame, int h, int w, const int32_t* det_bbox, const int32_t* det_cls, const int32_t* n_dets, int max_rows,
                    const uint8_t* redact, int num_classes, int mode, int size, int margin, void* workspace, size_t ws_bytes,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_REDACT_H */
