/* Static areas hidden in a uint8 frame on the device -- polygons and a painted mask, with no detection row anywhere: an EXTENSION of the
 * C ABI of libfrcnn_hip.so (include/frcnn_hip.h, include/ext/frcnn_hip_redact.h, include/ext/frcnn_hip_redact_shape.h,
 * include/ext/frcnn_hip_zone.h and the other extension headers stay as they are, and so do their entry points).  Same library, same
 * conventions (int status, message via the library's last-error call, `stream` = hipStream_t or NULL), a revision of its own: a host
 * that uses these entry points checks frcnn_redact_region_version() == FRCNN_REDACT_REGION_VERSION.
 *   1 = frcnn_redact_region_plane_bytes, frcnn_redact_region_build, frcnn_redact_region_prepare, frcnn_redact_region_apply_u8.
 *
 * The rule (DESIGN §8 "Region rule"; tests/redact_region_ref.py restates it in Python integers).  Integers only: a frame has one right
 * answer.  S is the UNTOUCHED source frame, C the frame as the steps in front left it, both [h][w][3] uint8.
 *   PARAMETERS  n_regions, 0..FRCNN_REDACT_REGION_MAX (8); a region is a polygon in exactly the grammar and limits of the polygons of
 *           include/ext/frcnn_hip_zone.h: 3..16 vertices, every coordinate in -32768..65535 in source-frame pixels, no two consecutive
 *           vertices equal (the last and the first are consecutive), convex or not, simple or not.  An optional mask, [h][w] uint8.  At
 *           least one of the two.  feather F, 0..FRCNN_REDACT_REGION_FEATHER_MAX (32).  mode and size: those of
 *           include/ext/frcnn_hip_redact.h, with its ranges.
 *   HARD    an integer point (x, y) with -F <= x < w + F and -F <= y < h + F is hard when INSIDE_z(x, y) holds for any region z --
 *           INSIDE is frcnn_hip_zone.h's half-open crossing-number test, in int64, unchanged: a polygon owns its left and top boundary --;
 *           a point inside the frame is also hard when mask[y][x] >= 128.  The domain is padded by F so that a polygon that extends beyond
 *           the frame feathers as an unclipped box does under frcnn_hip_redact_shape.h.
 *   DISTANCE  e(x, y), the Chebyshev distance from the pixel to the hard set, capped at F + 1, computed separably:
 *             d1(x, y') = min |x - x'| over the hard points (x', y') of row y' (F + 1 when there is none within F),
 *             e(x, y)   = min over |y - y'| <= F of max(d1(x, y'), |y - y'|), F + 1 when that is larger.
 *   WEIGHT  frcnn_hip_redact_shape.h's: W = 256 where e = 0, (256 (F + 1 - e)) / (F + 1) where 1 <= e <= F, 0 beyond F.  The feather goes
 *           OUTWARDS: what the hard set hides stays fully hidden.
 *   OUTPUT  per byte out = (W R + (256 - W) C + 128) >> 8, R exactly frcnn_hip_redact.h's R for (mode, size) taken from S: grid and blur
 *           anchored at the frame's origin, edge replication.  Bytes with W = 0 are not written; W = 256 gives R exactly.
 *   The polygon (x0, y0), (x1 + 1, y0), (x1 + 1, y1 + 1), (x0, y1 + 1) on an untouched frame gives, byte for byte, what frcnn_hip_redact.h
 *   gives at F = 0 and what frcnn_hip_redact_shape.h gives with BOX and feather F for one eligible row (x0, y0, x1, y1), margin 0, the same
 *   mode and size -- boxes that cross the border included.  W never falls when F grows; a plane with no hard point writes no byte.
 *
 *   PLANE   device memory of the caller's, frcnn_redact_region_plane_bytes(h, w) bytes, 16-byte aligned:
 *             int32 [8]         [h, w, F, covered, full, 1, 0, 0]: covered = the pixels with W > 0, full = those with W = 256; word 5
 *                               is always 1;
 *             uint16 W[h][w]    the weights, at byte 32;
 *             uint8 [tiles]     at the next multiple of 16: one flag per tile of the apply kernel (private layout);
 *             ...               at the next multiple of 16: what the build kernels hand each other (private). */
#ifndef FRCNN_HIP_REDACT_REGION_H
#define FRCNN_HIP_REDACT_REGION_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_REDACT_REGION_VERSION 1
#define FRCNN_REDACT_REGION_MAX 8
#define FRCNN_REDACT_REGION_FEATHER_MAX 32
#define FRCNN_REDACT_REGION_HEAD_WORDS 8
int frcnn_redact_region_version(void);

/* Bytes of a plane for frames of h x w, whatever the feather; 0 for a side outside 1..FRCNN_REDACT_MAX_SIDE. */
size_t frcnn_redact_region_plane_bytes(int h, int w);

/* The plane of (polygons, mask, feather) for frames of h x w: ONCE per frame size, three launches on `stream` -- the HARD set over the
 * padded domain (a thread per point, the edge tests from LDS), d1, then e, W and the tile flags; covered and full are summed with
 * integer atomics.  No floats, nothing read on the host but `verts` and `nv`.
 *   plane      DEVICE, frcnn_redact_region_plane_bytes(h, w) bytes; every byte of header, W and flags is written.
 *   verts, nv  HOST memory, as frcnn_hip_zone.h passes its polygons: nv is int32 [n_regions], verts int32 (x, y) pairs, region 0's
 *              nv[0] vertices, then region 1's, and so on: read before the call returns.  Both may be NULL with n_regions = 0.
 *   mask       DEVICE uint8 [h][w], or NULL for none.
 * FRCNN_E_ARG, with nothing launched: a null plane; a side outside 1..FRCNN_REDACT_MAX_SIDE; n_regions outside
 * 0..FRCNN_REDACT_REGION_MAX; n_regions = 0 and no mask; null verts / nv with n_regions > 0; an nv outside 3..16; a coordinate out of
 * range; two equal consecutive vertices; a feather outside 0..FRCNN_REDACT_REGION_FEATHER_MAX. */
int frcnn_redact_region_build(void* plane, int h, int w, const int32_t* verts, const int32_t* nv, int n_regions, const uint8_t* mask,
                              int feather, void* stream);

/* Phase one of frcnn_hip_redact.h's call run UNCONDITIONALLY on `frame`, which must be the frame NO edit has touched: the cell means
 * (PIXELATE) or the horizontal blur stage (BLUR) of the whole frame into `workspace`, which is as large as that header's workspace
 * function says for (h, w, mode, size); no launch for FILL.  Its kernels are that call's own, unchanged: they read the plane's word 5
 * as their count word on the device, so a zeroed plane, which nobody has built, writes nothing; the frame is never written here, and
 * whether the plane is this size's is the apply kernel's to check.  Captured and replayed like every call here.
 * FRCNN_E_ARG, with nothing launched: a null frame or plane; a side outside 1..FRCNN_REDACT_MAX_SIDE; an unknown mode; a size outside
 * the mode's range; a null or short workspace where the mode needs one. */
int frcnn_redact_region_prepare(const uint8_t* frame, int h, int w, const void* plane, int mode, int size, void* workspace, size_t ws_bytes,
                                void* stream);

/* OUTPUT, in ONE launch on `stream`: frame ([h][w][3] uint8, contiguous, DEVICE) is edited in place from the plane and the workspace
 * frcnn_redact_region_prepare filled.  Tiles of 256 byte columns x 16 rows, threads are bytes: a workgroup reads its tile's flag and
 * returns when it is 0; else every thread walks its byte column, loads W for its pixel and blends, the vertical blur sum sliding from
 * one byte with W > 0 to the next.  One writer per byte, plain vector stores, no atomics, no floats, no detection rows, no allocation, no
 * synchronisation.  A plane whose header is not (h, w) writes nothing (checked on the device).
 * FRCNN_E_ARG, with nothing launched: as frcnn_redact_region_prepare. */
int frcnn_redact_region_apply_u8(uint8_t* frame, int h, int w, const void* plane, int mode, int size, const void* workspace,
                                 size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_REDACT_REGION_H */
