/* Objects painted out with a learned background: a per-pixel background PLATE learned over the frames of a fixed-camera sequence and
 * copied into the boxes of chosen classes, on the device: an EXTENSION of the C ABI of libfrcnn_hip.so (include/frcnn_hip.h and the other
 * extension headers stay as they are, and so do their entry points).  Same library, same conventions (int status, message via the
 * library's last-error call, `stream` = hipStream_t or NULL), a revision of its own: a host that uses these entry points checks
 * frcnn_plate_version() == FRCNN_PLATE_VERSION.
 *   1 = frcnn_plate_state_bytes, frcnn_plate_update, frcnn_plate_fill_u8.
 *
 * The rule (DESIGN §8 "Plate rule"; tests/plate_ref.py restates it in numpy).  Integers only: a sequence has one right answer.
 *   PARAMETERS  settle S, 1..FRCNN_PLATE_MAX_SETTLE (255); tolerance T, 0..255; margin M, 0..FRCNN_PLATE_MAX_MARGIN (64); a per-class byte
 *           table, the redaction's form.  The defaults (8, 10, 8) are PROVISIONAL: nobody has measured them on real footage.
 *   STATE   device int32 [frames, known, 0, 0 | px[h][w][2]]: 16 + 8hw bytes, sides 1..FRCNN_REDACT_MAX_SIDE.  Per pixel, word 0 is the
 *           bytes P0, P1, P2, V (lowest first): the plate in the frame's own byte order, V = 1 when it is known; word 1 is the bytes C0,
 *           C1, C2, N: a candidate and the length of its run.  A zeroed buffer is the empty state.  (The BUFFER is longer: behind the
 *           pixels it carries one word per tile of the update kernel, its partial `known` counts -- frcnn_plate_state_bytes says how long.
 *           Those words are scratch: every real update writes them all before it reads them, they belong to no rule, and a reader of
 *           the state stops at the pixels.)
 *   BOXES   of a frame, from a packed detection buffer (tracked = 0: int32 [n_dets, 0, 0, 0 | bbox[rows][4] | cls[rows] | ...]) or a
 *           tracked buffer (tracked = 1: int32 [n_rows, n_live, ., . | bbox[rows][4] | cls[rows] | ...], plain or widened).
 *           BLOCK set: every row r < n_dets, or r < n_rows of a tracked buffer -- the held and back-filled rows too --, WHATEVER its class:
 *           anything any detection touches is not background.  FILL set: the rows of the BLOCK set whose class c has 0 <= c < num_classes
 *           and table[c] != 0.  Counts are clamped to 0..rows.  Each box is clipped as the redaction rule clips at margin M (in 64 bits):
 *           xa = max(min(x1, x2) - M, 0), xb = min(max(x1, x2) + M, w - 1), ya and yb likewise from y1, y2 and h, both ends inclusive; a
 *           box with xa > xb or ya > yb is empty and skipped.  FILL is a subset of BLOCK at the same margin: a filled pixel is never
 *           learned in the same frame, and the two steps do not depend on each other's order within a frame.
 *   UPDATE  of frame f = frame_index from the UNTOUCHED frame bytes x.  The frame is REAL when f < max(*n_frames, 0) and, with a gate word,
 *           *gate != 0.  If it is not, no word of the buffer is written.  With a `cut` word that is non-zero every pixel's two words count
 *           as 0 before the steps below: the plate of the old scene is gone, in the same launch.  Then frames += 1, and per pixel:
 *             under a BLOCK box: N = 0; P and V stay (and C).
 *             otherwise, with d = the maximum over the three channels of |x_c - C_c|:
 *               N >= 1 and d <= T: N = min(N + 1, 255), C stays -- C is an anchor: slow drift beyond T restarts the run;
 *               else: C = x, N = 1;
 *               then, if N >= S: P = x, V = 1.
 *           known = the number of pixels with V != 0.
 *   FILL    of a frame, uint8 [h][w][3] in place.  A pixel under a FILL box becomes P if V != 0; otherwise 0 (black) with keep_unknown = 0,
 *           or it is left as it is with keep_unknown = 1.  Pixels outside the FILL boxes are never written.
 *   LIMIT   an object that stands still and is never detected becomes background after S frames.  That is the rule.
 *   ORDER   in a frame: the update reads the frame in front of every edit; the fill lies over the redaction, under everything drawn. */
#ifndef FRCNN_HIP_PLATE_H
#define FRCNN_HIP_PLATE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_PLATE_VERSION 1
#define FRCNN_PLATE_MAX_SETTLE 255
#define FRCNN_PLATE_DEFAULT_SETTLE 8       /* PROVISIONAL, as the two below: not measured on real footage */
#define FRCNN_PLATE_DEFAULT_TOL 10
#define FRCNN_PLATE_DEFAULT_MARGIN 8
#define FRCNN_PLATE_MAX_MARGIN 64
#define FRCNN_PLATE_MAX_FRAMES 65536       /* frame_index is 0..FRCNN_PLATE_MAX_FRAMES - 1 */
#define FRCNN_PLATE_TILE_W 128             /* the update kernel's tile: one scratch word each */
#define FRCNN_PLATE_TILE_H 8
int frcnn_plate_version(void);

/* Bytes of a state BUFFER for frames of h x w: 16 + 8hw of state, then 4 per tile of FRCNN_PLATE_TILE_W x FRCNN_PLATE_TILE_H pixels
 * (ceil(w / 128) x ceil(h / 8) of them); 0 for a side outside 1..FRCNN_REDACT_MAX_SIDE. */
size_t frcnn_plate_state_bytes(int h, int w);

/* UPDATE of one frame, two launches on `stream`.  The first is one pass over the pixels in tiles of 128 x 8: a workgroup stages the
 * frame's boxes that meet its tile in LDS, 256 candidate rows a round; a thread owns 4 consecutive pixels of a row -- 32 bytes of state,
 * moved as two 16-byte accesses where the run starts on an even pixel, and 12 bytes of frame, read as the aligned words that hold them --
 * and the tile's count of known pixels goes to its scratch word; the second, one workgroup, adds those in a fixed order and writes frames
 * and known.  One writer per word, plain vector stores, no atomics on memory, no floats.  Everything but the scalars is DEVICE memory.
 *   state        frcnn_plate_state_bytes(h, w) bytes, 16-byte aligned, read and written.
 *   frame        uint8 [h][w][3] contiguous, any alignment, read only.
 *   det, rows    the frame's packed (int32 [4 + 7 rows]) or tracked (int32 [4 + 8 rows]) buffer, see BOXES; `tracked` says which.
 *   frame_index, n_frames, gate   see UPDATE; gate may be NULL.  (A caller whose n_frames word is a COUNT another kernel wrote -- the
 *                frames a delayed pass emitted -- passes as gate the word that says whether the pass itself is real.)
 *   cut          one int32, may be NULL: see UPDATE.
 * No allocation, no synchronisation, nothing read on the host: every count and guard is read by the kernels, so the call can be captured
 * in a graph and replayed.
 * FRCNN_E_ARG, with nothing launched: a null pointer (but gate and cut); a state that is not 16-byte aligned; a side outside
 * 1..FRCNN_REDACT_MAX_SIDE; rows outside 1..FRCNN_REDACT_MAX_ROWS; margin outside 0..FRCNN_PLATE_MAX_MARGIN; settle outside
 * 1..FRCNN_PLATE_MAX_SETTLE; tol outside 0..255; frame_index outside 0..FRCNN_PLATE_MAX_FRAMES - 1. */
int frcnn_plate_update(int32_t* state, int h, int w, const uint8_t* frame, const int32_t* det, int rows, int tracked, int margin,
                       int settle, int tol, int frame_index, const int32_t* n_frames, const int32_t* gate, const int32_t* cut,
                       void* stream);

/* FILL of one frame, uint8 [h][w][3] contiguous, edited in place, in ONE launch on `stream`.  A workgroup owns a tile of 256 byte columns
 * x 16 rows and threads are bytes, as in the heat extension's draw call; it stages the FILL boxes that meet its tile as the update does and leaves
 * at once where there is none.  Every byte has one writer; the counts are read by the kernel, so the call can be captured and replayed.
 * FRCNN_E_ARG, with nothing launched: a null pointer; a side outside 1..FRCNN_REDACT_MAX_SIDE; rows outside 1..FRCNN_REDACT_MAX_ROWS;
 * num_classes outside 1..256; margin outside 0..FRCNN_PLATE_MAX_MARGIN; keep_unknown other than 0 or 1. */
int frcnn_plate_fill_u8(uint8_t* frame, int h, int w, const int32_t* state, const int32_t* det, int rows, int tracked,
                        const uint8_t* table, int num_classes, int margin, int keep_unknown, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_PLATE_H */
