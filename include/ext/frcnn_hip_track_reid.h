/* A returning object given its old id back: an appearance memory behind the tracker, on the device: an EXTENSION of the C ABI of
 * libfrcnn_hip.so (include/frcnn_hip.h, include/ext/frcnn_hip_track.h and the other extension headers stay as they are, and so do the
 * tracker's entry points).  Same library, same conventions (int status, message via the library's last-error call, `stream` = hipStream_t
 * or NULL), a revision of its own: a host that uses these entry points checks frcnn_track_reid_version() == FRCNN_TRACK_REID_VERSION.
 *   1 = frcnn_track_reid_state_bytes, frcnn_track_reid_workspace_bytes, frcnn_track_reid_update.
 *
 * The rule (DESIGN §8 "Re-identify rule"; tests/track_reid_ref.py restates it in numpy).  Integers only: a sequence has one right answer.
 * It is a stage behind a tracker call: it reads the tracked buffers of frcnn_hip_track.h and writes copies of them whose id column it has
 * rewritten.  The tracker's ids are called tid, the ids in the copies -- what everything downstream sees -- pid.
 *   PARAMETERS  pct, 1..100; keep, 1..FRCNN_TRACK_REID_MAX_KEEP (4095) frames; a per-class byte table, the tracker's `tracked`; rgb: 1 when
 *           byte 0 of a pixel is R, 0 when it is B.  The defaults (25, 250) are PROVISIONAL: nobody has measured them on real footage.
 *   ROWS    of frame f's tracked buffer int32 [n_rows, n_live, ., . | bbox[R][4] | cls[R] | prob[R] | id[R] | age[R]]: n_rows is clamped to
 *           0..R and n_live to 0..n_rows; a row r < n_live is LIVE, a row n_live <= r < n_rows is HELD.
 *   SIGNATURE  of a live row with id >= 1 and a class c with 0 <= c < num_classes and classes[c] != 0, in the frame as it was uploaded.
 *           The row's clipped box and sample grid are exactly the motion rule's (frcnn_hip_track_motion.h BOX, GRID): xa = max(min(x1, x2),
 *           0), xb = min(max(x1, x2), w - 1), ya, yb likewise; sx = (xb - xa + 32) / 32, x0 = xa + sx / 2, cols = (xb - x0) / sx + 1; sy, y0,
 *           rows likewise; n = cols * rows <= 1024.  An empty box, or n < FRCNN_TRACK_MOTION_MIN_SAMPLES (16): the row has NO signature.
 *           Sample (i, j), 0 <= i < cols, 0 <= j < rows, is the pixel (x0 + i sx, y0 + j sy); its band is (3 j) / rows, its bin
 *           (R >> 6) << 4 | (G >> 6) << 2 | (B >> 6): 3 bands x 64 bins = FRCNN_TRACK_REID_SIG_WORDS (192) counters, index 64 band + bin,
 *           that sum to n.  Each is normalised: v = (count << 12) / n, floor.  Every other row has no signature.
 *   DISTANCE  of two signatures: the sum over the 192 words of |a - b|, at most 8192.
 *   AVERAGE   of an entry's signature with a row's s: sig = s when has_sig == 0, else sig[k] = (3 sig[k] + s[k] + 2) >> 2; has_sig = 1.
 *   STATE   device int32 [n_entries, frames, dropped, reidentified | entry[capacity][FRCNN_TRACK_REID_ENTRY_WORDS]], an entry = [pid, tid,
 *           cls, last_seen, has_sig, sig[192]] (197 words); capacity 1..FRCNN_TRACK_REID_MAX (256).  The live entries are compacted in
 *           ascending pid order, their tids are distinct, and every word behind them is 0.  A zeroed buffer is the empty state.
 *   PER FRAME  for the real frames f < nf = min(max(*n_frames, 0), frames) of a call, in order:
 *     0 CUT      with a `cuts` array and cuts[f] != 0 the table is emptied (n_entries = 0; the three counters stay).
 *     1          frames += 1.
 *     2 PRESENT  = the ids >= 1 of all rows r < n_rows, the held ones too.
 *     3 BOUND    for every entry whose tid is the id of a live row: with r the LOWEST such row (a tracker's ids are distinct in a frame),
 *                if r has a signature s: AVERAGE with s, last_seen = frames.  Held rows update nothing.
 *     4 UNBOUND  the live rows r in ascending order with id t >= 1 and a class as SIGNATURE asks, whose t is no entry's tid WHEN THE ROW'S
 *                TURN COMES (an earlier row of the frame with the same t may just have bound it: then nothing more happens):
 *                CANDIDATES are the entries with cls == the row's, has_sig == 1, tid not in PRESENT -- the tracker has given that id up
 *                and can never issue it again; an entry taken earlier in this frame has a tid that IS present --, and frames - last_seen <=
 *                keep.  If the row has a signature s and there is a candidate, take the one with the least DISTANCE D, the lowest pid
 *                (the first in the table) among equals.  If D * 100 <= pct * 8192: gap = frames - last_seen; tid = t, AVERAGE with s,
 *                last_seen = frames, reidentified += 1, and the event (pid, t, cls, D, gap) is appended.  Otherwise, and for a row
 *                without a signature: with n_entries == capacity, dropped += 1; else a new entry [t, t, cls, frames, has, s or zeros] is
 *                inserted behind the last entry whose pid <= t.
 *     5 OUT      frame f's tracked buffer copied word for word, but for the ids of the rows r < n_rows with id t >= 1: the pid of the entry
 *                whose tid == t, if there is one, else t.
 *     6 EXPIRE   the entries with frames - last_seen > keep whose tid is not in PRESENT are removed, the rest compacted, order kept.
 *     7 LIST     frame f's reid list int32 [n_events, frames, 0, 0 | event[FRCNN_TRACK_REID_MAX_EVENTS][5]] (164 words): the first 32 events of
 *                the frame in row order, n_events = min(events, 32), zeros behind them.  Events beyond 32 still happen.
 *   (OUT stands in front of EXPIRE here; either order gives the same words: an entry that expires has a tid that is on no row.)
 *   A frame f >= nf: its tracked buffer is copied unchanged and its list is all zeros.  With nf == 0 no word of the state is written.
 *   CONSEQUENCE  while nothing is re-identified every pid equals its tid, and `out` is byte for byte `tracked`. */
#ifndef FRCNN_HIP_TRACK_REID_H
#define FRCNN_HIP_TRACK_REID_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_TRACK_REID_VERSION 1
#define FRCNN_TRACK_REID_MAX 256             /* entries of a state, at most */
#define FRCNN_TRACK_REID_BANDS 3
#define FRCNN_TRACK_REID_BINS 64
#define FRCNN_TRACK_REID_SIG_WORDS 192       /* bands x bins */
#define FRCNN_TRACK_REID_ENTRY_WORDS 197     /* pid, tid, cls, last_seen, has_sig, sig[192] */
#define FRCNN_TRACK_REID_MAX_DISTANCE 8192   /* two normalised signatures differ by at most this */
#define FRCNN_TRACK_REID_MAX_KEEP 4095
#define FRCNN_TRACK_REID_DEFAULT_PCT 25      /* PROVISIONAL, as the one below: not measured on real footage */
#define FRCNN_TRACK_REID_DEFAULT_KEEP 250
#define FRCNN_TRACK_REID_MAX_EVENTS 32       /* events a frame's list holds */
#define FRCNN_TRACK_REID_LIST_WORDS 164      /* 4 + 5 * 32 */
int frcnn_track_reid_version(void);

/* Bytes of a state of `capacity` entries: 4 * (4 + 197 * capacity); 0 for a capacity outside 1..FRCNN_TRACK_REID_MAX. */
size_t frcnn_track_reid_state_bytes(int capacity);

/* Bytes of the workspace of a call over `frames` frames whose tracked buffers have max_rows rows: 4 * 193 * frames * max_rows -- per
 * (frame, row) a has-signature word and the 192 normalised words; 0 for frames outside 1..FRCNN_TRACK_MAX_FRAMES or max_rows outside
 * 1..FRCNN_REDACT_MAX_ROWS.  Of a real frame the call writes the has word of every row and the 192 words of the rows that have a signature;
 * it writes nothing else. */
size_t frcnn_track_reid_workspace_bytes(int frames, int max_rows);

/* The rule over the frames of one pass, TWO launches on `stream`.  Signatures: one workgroup per (row, frame), which leaves at once for a
 * row that gets none; threads are samples, the 192 counters are in LDS under integer LDS atomics (integer sums do not depend on order).
 * Step: ONE workgroup walks the frames in order -- frame f + 1 needs frame f's table --, the entries' five head words in LDS, their
 * signatures in the state itself; the parallelism is inside a frame: threads over rows x entries for PRESENT, BOUND and OUT, a wave per
 * (row, candidate) pair for the 192-term distance with a shuffle sum, and one packed key D << 32 | place under a 64-bit minimum (the
 * table is in pid order, so the place stands for the pid).  One writer per word, no atomics on memory, no floats.  Everything but the
 * scalars is DEVICE memory.
 *   state        int32[4 + 197 * capacity], read and written.
 *   frames_u8    frame f at frames_u8 + f * frame_stride (bytes): [h][w][3] uint8 as uploaded, read only; `rgb` says which byte is R.
 *   tracked      frame f's tracked buffer at tracked + f * tracked_stride (words), int32[4 + 8 * max_rows] (frcnn_track_update's `out`,
 *                PLAIN: a delayed pass's widened buffers are not taken), read only.
 *   n_frames     one int32, see PER FRAME.      cuts   int32[frames], or NULL: see CUT.
 *   classes      uint8[num_classes], the tracker's `tracked` table.
 *   workspace    frcnn_track_reid_workspace_bytes(frames, max_rows) bytes, 4-byte aligned.
 *   out          frame f's copy at out + f * out_stride (words), int32[4 + 8 * max_rows]; must not overlap `tracked`.
 *   lists        int32[frames][FRCNN_TRACK_REID_LIST_WORDS].
 * No allocation, no synchronisation, nothing read on the host: *n_frames, the cut words and the row counts are read by the kernels, so the
 * call can be captured in a graph and replayed.
 * FRCNN_E_ARG, with nothing launched: a null pointer (but cuts); capacity outside 1..FRCNN_TRACK_REID_MAX; frames outside
 * 1..FRCNN_TRACK_MAX_FRAMES; max_rows outside 1..FRCNN_REDACT_MAX_ROWS; a side outside 1..FRCNN_REDACT_MAX_SIDE; frame_stride < 3hw, or
 * tracked_stride or out_stride < 4 + 8 * max_rows, with frames > 1; num_classes outside 1..256; pct outside 1..100; keep outside
 * 1..FRCNN_TRACK_REID_MAX_KEEP; rgb other than 0 or 1. */
int frcnn_track_reid_update(int32_t* state, int capacity, const uint8_t* frames_u8, long long frame_stride, int h, int w, int rgb,
                            const int32_t* tracked, long long tracked_stride, int max_rows, int frames, const int32_t* n_frames,
                            const int32_t* cuts, const uint8_t* classes, int num_classes, int pct, int keep, int32_t* workspace, int32_t* out,
                            long long out_stride, int32_t* lists, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_TRACK_REID_H */
