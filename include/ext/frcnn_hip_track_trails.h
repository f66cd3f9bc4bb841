/* The path of every track drawn into the frames: an EXTENSION of the C ABI of libfrcnn_hip.so (include/frcnn_hip.h,
 * include/ext/frcnn_hip_track.h and the other extension headers stay as they are, and so do their entry points).  Same library, same
 * conventions, a revision of its own: a host that uses these entry points checks frcnn_track_trails_version() == FRCNN_TRACK_TRAILS_VERSION.
 *   1 = frcnn_track_trails_state_bytes, frcnn_track_trails_list_words, frcnn_track_trails_update, frcnn_track_trails_draw_u8.
 *
 * The rule (DESIGN §8 "Trail rule"; tests/track_trails_ref.py restates it in numpy).  Integers only: a sequence has one right answer.
 *   PARAMETERS  length N, FRCNN_TRACK_TRAILS_MIN_LENGTH..FRCNN_TRACK_TRAILS_MAX_LENGTH (2..64): the points a trail keeps; width W, 1..9;
 *           expire E, 0..4095, in frames; capacity, 1..FRCNN_TRACK_MAX.
 *   STATE   device int32 [n_entries, frames, dropped, 0 | per entry: id, cls, last_seen, n, pts[N][2]], an entry 4 + 2N words, `capacity`
 *           of them.  The entries are compacted, in ascending id order; pts[0..n) are the trail's points (x, y), oldest first; every word
 *           behind them and behind the entries is 0.  A zeroed buffer is the empty state.  `frames` counts the real frames seen, `dropped`
 *           is sticky.
 *   POINT   of a row: the centre of the Tracking rule's clipped box (frcnn_hip_track.h BOX, margin 0): cx = (xa + xb) >> 1,
 *           cy = (ya + yb) >> 1.  It always lies inside the frame.
 *   PER FRAME  for the real frames f < nf of a call, in order; nf = min(max(*n_frames, 0), frames), and 0 when the call has a `gate`
 *           word that is 0:
 *     1 frames += 1.
 *     2 APPEND  the live rows r < n_live of the frame's tracked buffer with id >= 1 and a box that is not empty, in row order: the entry
 *               with that id is found; if there is none, one is inserted (n = 0, the row's cls), keeping id order; when the table is full
 *               the row gets no trail and dropped += 1.  The point is appended; beyond N points the oldest leaves, order kept (a ring in
 *               the kernel's memory, oldest to newest in the rule and in the state).  last_seen = frames.  Held rows (index >= n_live),
 *               back-filled rows and rows with id 0 are never read.  (The tracker's live rows have distinct ids; rows that share one
 *               append one point each, in row order.)
 *     3 EXPIRE  entries with frames - last_seen > E are removed and the rest compacted.
 *     4 SNAPSHOT  the frame's POINT LIST, int32 [n_trails, 0, 0, 0 | per trail: id, cls, n, 0, pts[N][2]], `capacity` trails of 4 + 2N
 *               words: the entries with last_seen == frames, in ascending id order, points oldest first, every word behind them 0.  It is
 *               written to list f of a workspace of `frames` such lists.
 *           Frames f >= nf get an empty list (every word 0).  With nf <= 0 no word of the state is written.
 *   DRAW    a trail with n points has the n - 1 segments (p_i, p_{i+1}); a trail with one point has none.  With A, B a segment's ends,
 *           P a pixel, d = B - A, p = P - A, dd = d.d, u = p.d, all int64, the segment COVERS P when
 *             dd == 0 or u <= 0:   |p|^2 <= (W W) >> 2;
 *             else u >= dd:        |P - B|^2 <= (W W) >> 2;
 *             otherwise:           (p.x d.y - p.y d.x)^2 <= (W W dd) >> 2
 *           -- the capsule of radius W / 2 around the segment; with sides up to FRCNN_REDACT_MAX_SIDE the square stays below 2^63
 *           (4 cross^2 would not), and W = 1 already gives a connected line.  A covered pixel of the frame takes the colour of the HIGHEST
 *           id among the trails that cover it, so the result does not depend on any order of execution.  The colour is PALETTE[id & 7], in
 *           R, G, B: (255,64,64) (64,160,255) (255,208,0) (255,0,255) (0,224,224) (255,128,0) (160,96,255) (255,255,255); `rgb` says
 *           which channel order the frame's bytes are in (non-zero: R, G, B; zero: B, G, R).  Pixels outside the frame are clipped, and
 *           nothing else of the frame is written. */
#ifndef FRCNN_HIP_TRACK_TRAILS_H
#define FRCNN_HIP_TRACK_TRAILS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_TRACK_TRAILS_VERSION 1
#define FRCNN_TRACK_TRAILS_MIN_LENGTH 2
#define FRCNN_TRACK_TRAILS_MAX_LENGTH 64
#define FRCNN_TRACK_TRAILS_MAX_WIDTH 9
#define FRCNN_TRACK_TRAILS_MAX_EXPIRE 4095
int frcnn_track_trails_version(void);

/* Bytes of a state: 4 * (4 + capacity * (4 + 2 * length)); 0 for a capacity outside 1..FRCNN_TRACK_MAX or a length out of range. */
size_t frcnn_track_trails_state_bytes(int capacity, int length);

/* 4-byte words of one point list: 4 + capacity * (4 + 2 * length), a state's words; 0 as above.  A workspace is `frames` lists. */
size_t frcnn_track_trails_list_words(int capacity, int length);

/* Steps 1-4 over the frames of one call, in order, in ONE launch on `stream` (one workgroup: frame f + 1 needs frame f's table, which it
 * keeps in LDS; the parallelism is over rows and entries inside a frame: wave64 ballots and prefixes for the ranks, one writer per word,
 * plain vector stores, no atomics).  Everything but the scalars is DEVICE memory.
 *   state        frcnn_track_trails_state_bytes(capacity, length) bytes, read and written.
 *   tracked      frame f's tracked buffer at tracked + f * tracked_stride (4-byte words): int32[4 + 8 * rows] as frcnn_track_update
 *                (rows = max_rows + capacity) or the look-back (rows = R2) writes it; bbox, id and cls of the rows r < n_live are read.
 *   n_frames     one int32, see above.
 *   gate         NULL, or one int32: with *gate == 0 no frame of the call is real.  (A caller whose n_frames word is a COUNT another
 *                kernel wrote -- the frames a look-back emitted -- passes the word that says whether the pass itself is real: the
 *                look-back emits the same frames again when a pass is replayed with no frames of its own.)
 *   h, w         the frame's sides: the POINT's clipped box.
 *   lists        `frames` point lists of frcnn_track_trails_list_words(capacity, length) words, every word written by one thread.
 * No allocation, no synchronisation, nothing read on the host, so the call can be captured in a graph and replayed.
 * FRCNN_E_ARG, with nothing launched: a null pointer (but gate); capacity outside 1..FRCNN_TRACK_MAX; rows outside 1..FRCNN_REDACT_MAX_ROWS; frames
 * outside 1..FRCNN_TRACK_MAX_FRAMES; tracked_stride < 4 + 8 * rows with frames > 1; length or expire out of range; a side outside
 * 1..FRCNN_REDACT_MAX_SIDE. */
int frcnn_track_trails_update(int32_t* state, int capacity, const int32_t* tracked, long long tracked_stride, int rows, int frames,
                              const int32_t* n_frames, const int32_t* gate, int length, int expire, int h, int w, int32_t* lists,
                              void* stream);

/* DRAW of one point list into one frame, uint8 [h][w][3], in ONE launch on `stream`: a gather.  A workgroup owns a tile of 256 byte
 * columns x 16 rows (threads are bytes: 64 lanes on 64 consecutive bytes are one coalesced access wherever a row of 3-byte pixels
 * starts); it stages the segments whose bounding box, grown by (W + 1) >> 1, meets the tile in LDS, in chunks when they do not fit, and
 * returns without touching a pixel when none does; otherwise each thread tests its pixels against the staged segments, keeps the highest
 * id and stores.  No atomics, one writer per byte: the bytes are deterministic.  *list (n_trails) is read by the kernel, so the call can
 * be captured and replayed; n_trails above FRCNN_TRACK_MAX and n above `length` are read as those bounds.
 * FRCNN_E_ARG, with nothing launched: a null pointer; a side outside 1..FRCNN_REDACT_MAX_SIDE; length or width out of range. */
int frcnn_track_trails_draw_u8(uint8_t* frame, int h, int w, const int32_t* list, int length, int width, int rgb, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_TRACK_TRAILS_H */
