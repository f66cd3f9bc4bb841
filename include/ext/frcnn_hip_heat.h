/* Where objects have been: an occupancy ("dwell") heat map accumulated over the frames of a sequence and blended into them, on the
 * device: an EXTENSION of the C ABI of libfrcnn_hip.so (include/frcnn_hip.h and the other extension headers stay as they are, and so do
 * their entry points).  Same library, same conventions (int status, message via the library's last-error call, `stream` = hipStream_t or
 * NULL), a revision of its own: a host that uses these entry points checks frcnn_heat_version() == FRCNN_HEAT_VERSION.
 *   1 = frcnn_heat_state_bytes, frcnn_heat_update, frcnn_heat_draw_u8.
 *
 * The rule (DESIGN §8 "Heat rule"; tests/heat_ref.py restates it in numpy).  Integers only: a sequence has one right answer.
 *   PARAMETERS  decay S, 0..FRCNN_HEAT_MAX_DECAY (15), 0 = none; alpha A, 1..255; a per-class byte table, the redaction's form.
 *   STATE   device int32 [frames, peak, saturated, 0 | map[h][w]]: 16 + 4hw bytes, sides 1..FRCNN_REDACT_MAX_SIDE.  A zeroed buffer is the
 *           empty state.  (The BUFFER is longer: behind the map it carries one word per tile of the update kernel, its partial maxima --
 *           frcnn_heat_state_bytes says how long.  Those words are scratch: every real update writes them all before it reads them, they
 *           belong to no rule, and a reader of the state stops at the map.)
 *   BOXES   of a frame.  From a packed detection buffer (tracked = 0: int32 [n_dets, 0, 0, 0 | bbox[rows][4] | cls[rows] | ...]): every
 *           row r < n_dets whose class c has 0 <= c < num_classes and table[c] != 0.  From a tracked buffer (tracked = 1: int32 [n_rows,
 *           n_live, ., . | bbox[rows][4] | cls[rows] | ...], plain or widened): the LIVE rows r < n_live only, same class test -- held and
 *           back-filled rows are guesses, not observations.  Counts are clamped to 0..rows.  Each box is clipped to the frame as the
 *           redaction rule clips at margin 0: xa = max(min(x1, x2), 0), xb = min(max(x1, x2), w - 1), ya and yb likewise from y1, y2 and
 *           h, both ends inclusive; a box with xa > xb or ya > yb is empty and skipped; one that crosses the border counts with the part
 *           inside.
 *   UPDATE  of frame f = frame_index.  The frame is REAL when f < max(*n_frames, 0) and, with a gate word, *gate != 0.  If it is not, no
 *           word of the buffer is written.  Otherwise, in this order:
 *     1 frames += 1.
 *     2 DECAY, if S > 0: every v becomes v - ((v + 2^S - 1) >> S): every positive value loses at least 1, so the map can return to 0.
 *     3 ADD   every pixel gains 256 x (the number of the frame's boxes that cover it); the result is clamped to FRCNN_HEAT_MAX (2^30);
 *             saturated becomes 1 when any pixel was clamped -- sticky, and all writers store the same value.  No int32 can overflow: a
 *             frame adds at most 256 x FRCNN_REDACT_MAX_ROWS.
 *     4 peak = the maximum of the map.
 *   DRAW    into a frame, uint8 [h][w][3].  With p = peak: p <= 0 writes nothing.  Otherwise for a pixel of value v (read as 0 below 0 and
 *           as p above p, which an update never leaves): t = (v x 255) / p, in 64 bits, rounded down; the colour is the ramp
 *           R = min(255, 3t), G = clamp(3t - 255, 0, 255), B = clamp(3t - 510, 0, 255); the weight a = (A x t) / 255, rounded down; each
 *           channel becomes out = (src x (255 - a) + C x a + 127) / 255.  `rgb` says which order the frame's bytes are in (non-zero:
 *           R, G, B; zero: B, G, R).  With a == 0 the byte is not written: every pixel with v == 0 among them.
 *   ORDER   in a frame: over the redaction, under the trails, the boxes and the labels. */
#ifndef FRCNN_HIP_HEAT_H
#define FRCNN_HIP_HEAT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_HEAT_VERSION 1
#define FRCNN_HEAT_MAX_DECAY 15
#define FRCNN_HEAT_DEFAULT_ALPHA 160
#define FRCNN_HEAT_MAX 1073741824          /* 2^30: where a pixel's value stops */
#define FRCNN_HEAT_MAX_FRAMES 65536        /* frame_index is 0..FRCNN_HEAT_MAX_FRAMES - 1 */
#define FRCNN_HEAT_TILE_W 64               /* the update kernel's tile: one scratch word each */
#define FRCNN_HEAT_TILE_H 16
int frcnn_heat_version(void);

/* Bytes of a state BUFFER for frames of h x w: 16 + 4hw of state, then 4 per tile of FRCNN_HEAT_TILE_W x FRCNN_HEAT_TILE_H pixels
 * (ceil(w / 64) x ceil(h / 16) of them); 0 for a side outside 1..FRCNN_REDACT_MAX_SIDE. */
size_t frcnn_heat_state_bytes(int h, int w);

/* UPDATE of one frame, two launches on `stream`.  The first is one pass over the map in tiles of 64 x 16 pixels: a workgroup stages the
 * frame's boxes that meet its tile in LDS, 256 candidate rows a round, decays and adds its pixels (a thread owns 4 of them) and leaves its
 * tile's maximum in the scratch words; the second, one workgroup, reduces those in a fixed order and writes frames and peak.  One writer
 * per word but for the same-value `saturated` store, plain vector stores, no atomics on memory, no floats.  Everything but the scalars
 * is DEVICE memory.
 *   state        frcnn_heat_state_bytes(h, w) bytes, read and written.
 *   det, rows    the frame's packed (int32 [4 + 7 rows]) or tracked (int32 [4 + 8 rows]) buffer, see BOXES; `tracked` says which.
 *   table        uint8 [num_classes].
 *   frame_index, n_frames, gate   see UPDATE; gate may be NULL.  (A caller whose n_frames word is a COUNT another kernel wrote -- the
 *                frames a delayed pass emitted -- passes as gate the word that says whether the pass itself is real.)
 * No allocation, no synchronisation, nothing read on the host: every count and guard is read by the kernels, so the call can be captured
 * in a graph and replayed.
 * FRCNN_E_ARG, with nothing launched: a null pointer (but gate); a side outside 1..FRCNN_REDACT_MAX_SIDE; rows outside
 * 1..FRCNN_REDACT_MAX_ROWS; num_classes outside 1..256; decay outside 0..FRCNN_HEAT_MAX_DECAY; frame_index outside
 * 0..FRCNN_HEAT_MAX_FRAMES - 1. */
int frcnn_heat_update(int32_t* state, int h, int w, const int32_t* det, int rows, int tracked, const uint8_t* table, int num_classes,
                      int decay, int frame_index, const int32_t* n_frames, const int32_t* gate, void* stream);

/* DRAW of the state into one frame, uint8 [h][w][3] contiguous, edited in place, in ONE launch on `stream`.  A workgroup owns a tile of
 * 256 byte columns x 16 rows and threads are bytes (64 lanes on 64 consecutive bytes are one coalesced access wherever a row of 3-byte
 * pixels starts); every byte has one writer, and `peak` is read by the kernel, so the call can be captured and replayed.
 * FRCNN_E_ARG, with nothing launched: a null pointer; a side outside 1..FRCNN_REDACT_MAX_SIDE; alpha outside 1..255. */
int frcnn_heat_draw_u8(uint8_t* frame, int h, int w, const int32_t* state, int alpha, int rgb, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_HEAT_H */
