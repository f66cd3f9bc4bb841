/* Whatever differs from the learned background hidden in a uint8 frame on the device -- a safety net under the detector, with no
 * detection row needed: an EXTENSION of the C ABI of libfrcnn_hip.so (include/frcnn_hip.h, include/ext/frcnn_hip_plate.h,
 * include/ext/frcnn_hip_redact_region.h and the other extension headers stay as they are, and so do their entry points).  Same library,
 * same conventions (int status, message via the library's last-error call, `stream` = hipStream_t or NULL), a revision of its own: a
 * host that uses these entry points checks frcnn_redact_moving_version() == FRCNN_REDACT_MOVING_VERSION.
 *   1 = frcnn_redact_moving_state_bytes, frcnn_redact_moving_build.
 *
 * The rule (DESIGN §8 "Moving rule"; tests/redact_moving_ref.py restates it in numpy).  Integers only: a sequence has one right answer.
 *   PARAMETERS  tolerance D, 0..255; vote K, 1..64; hold H, 0..255 frames; grow G, 0..32 pixels; feather F, 0..32 pixels; unknown, 0
 *           (show) or 1 (hide); an EXCEPT table, a per-class byte table in the redaction's form; the margin M of frcnn_hip_plate.h.  The
 *           defaults (D 24, K 8, H 4, G 8) are PROVISIONAL: nobody has measured them on real footage.
 *   CELLS   a cell is 8 x 8 pixels anchored at the frame's origin: cw = ceil(w / 8) by ch = ceil(h / 8) of them, the edge cells clipped to
 *           the frame.
 *   STATE   device, one per frame size and channel order as the plate: int32 [frames, cells_now, 0, 0], then uint8 left[ch][cw], padded to
 *           16 bytes.  A zeroed buffer is the empty state.  (The BUFFER is longer: behind `left` it carries one byte per cell -- is it
 *           moving in the last real frame -- and one word per tile of the first kernel, which the launches hand each other:
 *           frcnn_redact_moving_state_bytes says how long.  Those are scratch: every real build writes them all before it reads them.)
 *   FOREGROUND  of a pixel of frame f = frame_index, from the UNTOUCHED frame bytes x and the plate state (P, V of frcnn_hip_plate.h) as
 *           that header's update call left it for this same frame: the plate update comes first.
 *             under an EXCEPT box: never.  The EXCEPT set is the rows of the plate rule's BLOCK set whose class c has 0 <= c < num_classes
 *               and table[c] != 0, each box clipped exactly as the plate rule clips at margin M;
 *             otherwise, with V != 0: foreground iff the maximum over the three channels of |x_c - P_c| is > D;
 *             otherwise (V = 0): foreground iff unknown = 1.
 *   VOTE AND HOLD  a cell VOTES when it has at least min(K, the pixels of the clipped cell) foreground pixels.  With a `cut` word that is
 *           non-zero every `left` counts as 0 first.  A cell that votes sets left = H and is MOVING; a cell that does not vote with
 *           left > 0 gets left -= 1 and is MOVING; any other cell is not.  Then frames += 1 and cells_now = the number of moving cells.
 *   REAL    the frame is real under the plate update's conditions exactly: f < max(*n_frames, 0) and, with a gate word, *gate != 0.
 *           For a frame that is not real no word of the state buffer is written; the plane's header is written with covered = full = 0
 *           and every tile flag as 0, so the apply call writes nothing; the frame's stats are all 0.
 *   WEIGHT  the hard set is the pixels of the moving cells; e0(x, y) is the Chebyshev distance from the pixel to it, capped at G + F + 1;
 *           W = 256 where e0 <= G; with e = e0 - G, W = (256 (F + 1 - e)) / (F + 1) where 1 <= e <= F; 0 beyond.  The feather goes
 *           OUTWARDS, as everywhere else here.
 *   PLANE   exactly frcnn_hip_redact_region.h's: header [h, w, F, covered, full, 1, 0, 0], uint16 W[h][w] at byte 32, the tile flags;
 *           as many bytes as that header's plane-size call says for (h, w), 16-byte aligned.  Every word of header, W and flags is written on every real
 *           frame, and equals what that header's build call writes for no polygons, the same F and the mask "255 where e0 <= G".
 *   OUTPUT  that header's prepare call on the untouched frame and its apply call, both unchanged, with a workspace of
 *           their own and any (mode, size) of frcnn_hip_redact.h.
 *   STATS   per frame int32 [real, cells_now, covered, full].
 *   LIMITS  an object that stands still and is never detected becomes background after the plate's S frames: that is the plate's own
 *           limit, and this net does not block learning -- use a large settle.  A lighting change hides everything until the plate
 *           settles again.  Moving cameras are out of scope.  Until a pixel's background is known it is SHOWN (unknown = 0), or the start
 *           of a sequence is blanked (unknown = 1): either way the first S frames are not protected by the net under the default. */
#ifndef FRCNN_HIP_REDACT_MOVING_H
#define FRCNN_HIP_REDACT_MOVING_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_REDACT_MOVING_VERSION 1
#define FRCNN_REDACT_MOVING_CELL 8
#define FRCNN_REDACT_MOVING_VOTE_MAX 64
#define FRCNN_REDACT_MOVING_HOLD_MAX 255
#define FRCNN_REDACT_MOVING_GROW_MAX 32
#define FRCNN_REDACT_MOVING_FEATHER_MAX 32
#define FRCNN_REDACT_MOVING_DEFAULT_TOL 24      /* PROVISIONAL, as the three below: not measured on real footage */
#define FRCNN_REDACT_MOVING_DEFAULT_VOTE 8
#define FRCNN_REDACT_MOVING_DEFAULT_HOLD 4
#define FRCNN_REDACT_MOVING_DEFAULT_GROW 8
#define FRCNN_REDACT_MOVING_STATS_WORDS 4
int frcnn_redact_moving_version(void);

/* Bytes of a state BUFFER for frames of h x w: 16 + ch cw of state padded to 16, then the scratch (see STATE); 0 for a side outside
 * 1..FRCNN_REDACT_MAX_SIDE. */
size_t frcnn_redact_moving_state_bytes(int h, int w);

/* The plane of one frame, three launches on `stream`: the cells (tiles of 128 x 8 pixels as the plate update's, a thread owns 4
 * consecutive pixels, the EXCEPT boxes staged in LDS 256 rows a round, one writer per `left` byte), the counts (one workgroup), the
 * weights (the apply call's tiles of 256 byte columns x 16 rows; the cells within reach G + F of a tile staged in LDS as bits, the
 * distance separably at cell granularity; covered and full summed with integer atomics).  No floats, no allocation, no
 * synchronisation, nothing read on the host: every count and guard is read by the kernels, so the call can be captured in a graph and
 * replayed.  Everything but the scalars is DEVICE memory.
 *   state        frcnn_redact_moving_state_bytes(h, w) bytes, 16-byte aligned, read and written.
 *   plane        a plane of the region extension's size for (h, w), 16-byte aligned, written.
 *   stats        int32 [4], written: see STATS.
 *   frame        uint8 [h][w][3] contiguous, any alignment, read only: the frame NO edit has touched.
 *   plate        the plate state of frcnn_hip_plate.h for (h, w), 16-byte aligned, read only, already updated with this frame.
 *   det, rows, tracked   the frame's packed or tracked buffer, as the plate update takes it.  `tracked` is IGNORED, as it is there: both
 *                kinds of buffer count their rows in word 0, so no value of it is refused.
 *   table, num_classes   the EXCEPT table, uint8 [num_classes].
 *   margin, tol, vote, hold, grow, feather, unknown   M, D, K, H, G, F and unknown of the rule.
 *   frame_index, n_frames, gate, cut   as the plate update's; gate and cut may be NULL.
 * FRCNN_E_ARG, with nothing launched: a null pointer (but gate and cut); a state, plane or plate state that is not 16-byte aligned; a
 * side outside 1..FRCNN_REDACT_MAX_SIDE; rows outside 1..FRCNN_REDACT_MAX_ROWS; num_classes outside 1..256; margin outside
 * 0..FRCNN_PLATE_MAX_MARGIN; tol outside 0..255; vote outside 1..64; hold outside 0..255; grow or feather outside 0..32; unknown other
 * than 0 or 1; frame_index outside 0..FRCNN_PLATE_MAX_FRAMES - 1. */
int frcnn_redact_moving_build(void* state, void* plane, int32_t* stats, int h, int w, const uint8_t* frame, const int32_t* plate,
                              const int32_t* det, int rows, int tracked, const uint8_t* table, int num_classes, int margin, int tol,
                              int vote, int hold, int grow, int feather, int unknown, int frame_index, const int32_t* n_frames,
                              const int32_t* gate, const int32_t* cut, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_REDACT_MOVING_H */
