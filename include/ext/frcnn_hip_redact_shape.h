/* Shaped redaction -- an elliptical mask and a soft edge for the redaction extension's call: an EXTENSION of the C ABI of libfrcnn_hip.so
 * (include/frcnn_hip.h, include/ext/frcnn_hip_redact.h and the other extension headers stay as they are).  Same library, same
 * conventions (int status, message via frcnn_last_error, `stream` = hipStream_t or NULL), a revision of its own: a host that uses these
 * entry points checks frcnn_redact_shape_version() == FRCNN_REDACT_SHAPE_VERSION.
 *   1 = frcnn_redact_shaped_u8.
 *
 * The rule (DESIGN §8 "Shape rule"; tests/redact_shape_ref.py restates it in Python integers).  S is the frame, [h][w][3] uint8.  Beside
 * the Redaction rule's (classes, mode, size, margin) there are `shape` (BOX, ELLIPSE) and `feather` F, 0..FRCNN_REDACT_FEATHER_MAX pixels.
 *   ROWS     the eligible rows are the Redaction rule's: r < *n_dets, 0 <= det_cls[r] < num_classes, redact[det_cls[r]] != 0.
 *   GROWN    the grown box of a row is NOT clipped to the frame: X0 = min(x1, x2) - margin, X1 = max(x1, x2) + margin, Y0 and Y1
 *            likewise, A = X1 - X0 + 1, B = Y1 - Y0 + 1.  An ellipse that crosses the border stays the ellipse of the whole box; pixels
 *            exist only inside the frame.  A row whose grown box has a side above FRCNN_REDACT_SHAPE_MAX_SIDE counts as a BOX row.
 *   DISTANCE e_r(x, y) is the smallest e >= 0 for which the pixel lies inside the row's shape grown by e:
 *     BOX      e = max(X0 - x, x - X1, Y0 - y, y - Y1, 0).
 *     ELLIPSE  with u = 2x - (X0 + X1), v = 2y - (Y0 + Y1) the pixel lies inside the ellipse grown by e when
 *              u^2 (B + 2e)^2 + v^2 (A + 2e)^2 <= (A + 2e)^2 (B + 2e)^2, evaluated exactly (the products pass 2^64: the comparison is made
 *              in 128 bits).  The ellipses are nested, so the condition is monotone in e.
 *   WEIGHT   W_r = 256 where e_r = 0, (256 (F + 1 - e_r)) / (F + 1) where 1 <= e_r <= F, 0 beyond F; the pixel's W is the maximum of
 *            W_r over the eligible rows.  The feather goes OUTWARDS: what the hard shape hides stays fully hidden.
 *   OUTPUT   per byte out = (W R + (256 - W) S + 128) >> 8, R exactly the Redaction rule's R for the mode, a function of S alone.  Bytes
 *            with W = 0 are not written; W = 256 gives R exactly.
 *   BOX with F = 0 is the Redaction rule byte for byte; the masked set of ELLIPSE is a subset of BOX's at the same F; W never falls when F
 *   grows.  Integer arithmetic throughout: one right answer per frame, whatever the order of the rows. */
#ifndef FRCNN_HIP_REDACT_SHAPE_H
#define FRCNN_HIP_REDACT_SHAPE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_REDACT_SHAPE_VERSION 1
int frcnn_redact_shape_version(void);

#define FRCNN_REDACT_SHAPE_BOX 0
#define FRCNN_REDACT_SHAPE_ELLIPSE 1
#define FRCNN_REDACT_FEATHER_MAX 32
#define FRCNN_REDACT_SHAPE_MAX_SIDE 131072   /* a grown box with a larger side is a BOX row whatever `shape` says */

/* The redaction call of include/ext/frcnn_hip_redact.h (the same buffers, modes, sizes and margin) with `shape` and `feather`.  The
 * workspace is as large as that header's workspace function says for (h, w, mode, size).  Two launches on `stream`: the first is that
 * call's (it reads the frame and writes the workspace; nothing for FILL), the second blends every byte with W > 0 from the workspace and
 * the byte itself.  No
 * allocation, no synchronisation, nothing read on the host: *n_dets is read by the kernels, so the call can be captured in a graph and
 * replayed with other detections.  With *n_dets <= 0 no byte of the frame is written.
 * FRCNN_E_ARG, with nothing launched: everything that call refuses; a shape that is neither BOX nor ELLIPSE; a feather outside
 * 0..FRCNN_REDACT_FEATHER_MAX. */
int frcnn_redact_shaped_u8(uint8_t* frame, int h, int w, const int32_t* det_bbox, const int32_t* det_cls, const int32_t* n_dets,
                           int max_rows, const uint8_t* redact, int num_classes, int mode, int size, int margin, int shape, int feather,
                           void* workspace, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_REDACT_SHAPE_H */
