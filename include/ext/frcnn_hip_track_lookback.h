/* New tracks hidden in the frames BEFORE their first detection: an EXTENSION of the C ABI of libfrcnn_hip.so (include/frcnn_hip.h,
 * include/ext/frcnn_hip_track.h, include/ext/frcnn_hip_track_motion.h and the other extension headers stay as they are, and so do their
 * entry points).  Same library, same conventions, a revision of its own: a host that uses these entry points checks
 * frcnn_track_lookback_version() == FRCNN_TRACK_LOOKBACK_VERSION.
 *   1 = frcnn_track_lookback_state_bytes, frcnn_track_lookback.
 *
 * The rule (DESIGN §8 "Look-back rule"; tests/track_lookback_ref.py restates it in numpy).  Integers only: a sequence has one right answer.
 *   PARAMETERS  lookback L, 1..FRCNN_TRACK_LOOKBACK_MAX; radius 0..16 (0: the box stands still, nothing is searched); grow 0..64 as in the
 *           tracker; back 1..128, the back-filled rows a frame with every live and held row in use can still take.
 *   WIDENED  a tracked buffer of frcnn_hip_track.h with R2 = max_rows + capacity + back rows instead of R = max_rows + capacity:
 *           int32[4 + 8 R2] = [n_rows, n_live, next_id, overflow | bbox[R2][4] | cls[R2] | prob[R2] | id[R2] | age[R2]]; rows R..R2 - 1
 *           start as the rows behind n_rows do (bbox -1, cls -1, prob, id, age 0).  R2 <= FRCNN_REDACT_MAX_ROWS.
 *   WINDOW  device memory of the caller's, frcnn_track_lookback_state_bytes(...) bytes: the frames that have been tracked but not
 *           emitted, each as its UNTOUCHED bytes [h][w][3] and its widened tracked buffer.  Layout: a header int32[8] =
 *           [count, half, back_overflow, 0, 0, 0, 0, 0], then two halves of `frames` cells, a cell = [widened buffer, 16 + 32 R2 bytes |
 *           frame, 3hw bytes padded to 16].  Window frame i < count is cell i of half `half`.  A zeroed header is an empty window.
 *   SEQUENCE of a call, with nf = min(max(*n_frames, 0), frames) and c = the window's count: S = the c window frames, oldest first,
 *           then frames 0..nf - 1 of the call.
 *   BIRTH   in frame t of the call (never in a window frame: those were chained when they were a call's): a live row (index < n_live) of
 *           frame t's tracked buffer with id >= first_id(t), first_id(t) = the next_id word of the buffer in front of t in S.  The first
 *           frame of S has no frame in front of it and no births to fill: there is nothing to fill into.
 *   CHAIN   for a birth with raw box b_t, for k = 1..L while g = t - k is still in S:
 *             the motion rule's search (frcnn_hip_track_motion.h LUMA, GRID, COST, BEST, GATE) with REFERENCE P = frame g + 1, the box
 *             b_{g+1}, and "current" = frame g; skipped, the box unchanged, when radius = 0, the clipped box is empty or n < 16;
 *             b_g = b_{g+1} shifted by the taken (dx, dy);
 *             frame g receives one BACK-FILLED row: bbox = (xa - e, ya - e, xb + e, yb + e) from b_g's clipped box with e = grow * k, or
 *             (-1, -1, -1, -1) when the clipped box is empty; cls, prob and id those of the birth row; age = -k.
 *           The chain never stops early: a row's place does not depend on the pixels.
 *   PLACE   frame g's back-filled rows follow its held rows in ascending id order (births of later frames have larger ids, so the rows
 *           of a call follow those of the call before).  n_rows counts them, n_live does not move: the redaction hides them, the drawing
 *           step never draws them.  Rows that would pass R2 are dropped, highest ids first, and counted in back_overflow (sticky).
 *   PER CALL
 *     1 JOIN  with nf >= 1: the call's nf frames and their tracked buffers, widened, go into the cells of the OTHER half.
 *     2 CHAIN their births, into earlier frames of this call and into the window's frames.
 *     3 EMIT  the c window frames, oldest first: bytes and widened buffers are copied to out_frames / out_tracked, *out_count = c; of
 *             out_tracked[e], e >= c, the four count words are written 0 and nothing else; out_frames[e], e >= c, is not written.
 *     4 CLOSE with nf >= 1: half ^= 1, count = nf (the window holds this call's frames).
 *   *n_frames == 0 (warm-up, capture): step 3 alone; no byte of the window or its header is written.
 *   *n_frames < 0 (flush): step 3, then count = 0.
 *   CONSEQUENCE  with every call full (nf = frames = B) and L <= B, every back-filled row the rule can produce is in place before its
 *           frame is emitted: the emitted sequence does not depend on how the sequence was cut into calls. */
#ifndef FRCNN_HIP_TRACK_LOOKBACK_H
#define FRCNN_HIP_TRACK_LOOKBACK_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_TRACK_LOOKBACK_VERSION 1
#define FRCNN_TRACK_LOOKBACK_MAX 16        /* frames a birth is chained back over, at most */
#define FRCNN_TRACK_LOOKBACK_MAX_BACK 128  /* `back`, at most */
#define FRCNN_TRACK_LOOKBACK_HEADER 32     /* bytes in front of the window's cells */
int frcnn_track_lookback_version(void);

/* Bytes of a window for calls of `frames` frames of h x w: 32 + 2 * frames * (16 + 32 R2 + (3hw + 15) / 16 * 16); 0 for an argument
 * frcnn_track_lookback refuses. */
size_t frcnn_track_lookback_state_bytes(int frames, int h, int w, int max_rows, int capacity, int back);

/* One call of the rule.  Everything but the scalars is DEVICE memory.
 *   window        frcnn_track_lookback_state_bytes(...) bytes, 16-byte aligned, read and written.
 *   frames_u8     frame f of the call at frames_u8 + f * frame_stride (bytes): [h][w][3] uint8 as uploaded, read only.
 *   tracked       frame f's tracked buffer (frcnn_track_update's `out`) at tracked + f * tracked_stride (4-byte words), R rows, read only.
 *   n_frames      one int32, see above.
 *   out_frames    emitted frame e at out_frames + e * out_frame_stride (bytes); out_tracked: its widened buffer at
 *                 out_tracked + e * out_tracked_stride (words); out_count: one int32.
 * Five launches on `stream` (join, chain: one workgroup per birth, counts, emit, close).  No allocation, no synchronisation, nothing
 * read on the host: *n_frames, the window's count and the births are device values, so the call can be captured in a graph and replayed.
 * FRCNN_E_ARG, with nothing launched: a null pointer; a window that is not 16-byte aligned; frames outside 1..FRCNN_TRACK_MAX_FRAMES;
 * max_rows < 1; capacity outside 1..FRCNN_TRACK_MAX; back outside 1..128; R2 > FRCNN_REDACT_MAX_ROWS; lookback outside
 * 1..FRCNN_TRACK_LOOKBACK_MAX; radius outside 0..16; grow outside 0..64; a side outside 1..FRCNN_REDACT_MAX_SIDE; with frames > 1,
 * frame_stride or out_frame_stride < 3hw, tracked_stride < 4 + 8R or out_tracked_stride < 4 + 8 R2. */
int frcnn_track_lookback(uint8_t* window, const uint8_t* frames_u8, long long frame_stride, const int32_t* tracked, long long tracked_stride,
                         int frames, const int32_t* n_frames, int max_rows, int capacity, int back, int lookback, int radius, int grow,
                         int h, int w, uint8_t* out_frames, long long out_frame_stride, int32_t* out_tracked, long long out_tracked_stride,
                         int32_t* out_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_TRACK_LOOKBACK_H */
