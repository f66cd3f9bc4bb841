/* How many went past: tracks counted as they cross lines, on the device, and the lines and their totals drawn into the frames: an
 * EXTENSION of the C ABI of libfrcnn_hip.so (include/frcnn_hip.h, include/ext/frcnn_hip_track.h and the other extension headers stay as
 * they are, and so do their entry points).  Same library, same conventions (int status, message via the library's last-error call,
 * `stream` = hipStream_t or NULL), a revision of its own: a host that uses these entry points checks frcnn_count_version() ==
 * FRCNN_COUNT_VERSION.
 *   1 = frcnn_count_state_bytes, frcnn_count_list_words, frcnn_count_update, frcnn_count_draw_u8.
 *
 * The rule (DESIGN §8 "Count rule"; tests/count_ref.py restates it in numpy).  Integers only: everything is compared exactly in int64,
 * nothing is divided, and the result never depends on an order of execution.
 *   PARAMETERS  n_lines, 1..FRCNN_COUNT_MAX_LINES (8); line l = (ax, ay, bx, by), A != B, every coordinate in FRCNN_COUNT_MIN_COORD..
 *           FRCNN_COUNT_MAX_COORD (-32768..65535): a line may extend beyond the frame; width W, 1..9 (default 3); expire E, 0..4095, in
 *           frames; capacity, 1..FRCNN_TRACK_MAX; classes, uint8 [num_classes], non-zero where a class counts (the redaction's form).
 *   POINT   of a row: the trail rule's (frcnn_hip_track_trails.h POINT): the centre of the clipped box, cx = (xa + xb) >> 1,
 *           cy = (ya + yb) >> 1.  It always lies inside the frame.
 *   SIDE    s_l(P) = (bx - ax)(py - ay) - (by - ay)(px - ax), sigma_l(P) = (s_l(P) >= 0): a point ON the line belongs to the non-negative
 *           side, so a track that touches the line and turns back is neither missed nor counted twice.
 *   CROSSING  a step P -> Q of one id crosses line l when both hold:
 *             sigma_l(P) != sigma_l(Q) (which also means P != Q);
 *             the step's carrier line separates A from B under the same half-open convention:
 *             tau(X) = ((qx - px)(xy - py) - (qy - py)(xx - px) >= 0), tau(A) != tau(B).
 *           The direction is pos (1) when sigma_l(Q) is 1, otherwise neg (0).
 *   ONCE    an id counts at most once per line and direction: its entry carries a 16-bit `counted` mask, bit 2 l + dir.  Jitter about a
 *           line cannot inflate a total.
 *   STATE   device int32 [n_entries, frames, dropped, events_dropped | totals[8][2] | per entry: id, cls, last_seen, counted, px, py]:
 *           20 + 6 capacity words.  The entries are compacted, in ascending id order; every word behind the live entries is 0.  A zeroed
 *           buffer is the empty state.  `frames` counts the real frames seen; `dropped` and `events_dropped` are sticky sums.
 *   PER FRAME  for the real frames f < nf of a call, in order; nf = min(max(*n_frames, 0), frames), and 0 when the call has a `gate`
 *           word that is 0:
 *     1 frames += 1.
 *     2 the live rows r < n_live of the frame's tracked buffer with id >= 1, a box that is not empty and a class c with 0 <= c <
 *       num_classes and classes[c] != 0, in row order: the entry of the id is found.  If there is none, one is inserted, keeping id
 *       order (counted = 0, the row's cls), with no crossing; when the table is full dropped += 1 and the row is skipped.  Otherwise the
 *       step from (px, py) to the row's point is tested against every line in ascending l, and for each crossing whose bit is not yet
 *       set: the bit is set, totals[l][dir] += 1, and the event (l, dir, id, cls) is appended, cls the ENTRY's.  Then (px, py) becomes
 *       the row's point and last_seen = frames.  Held rows (index >= n_live), back-filled rows and rows with id 0 are never read.  (The
 *       tracker's live rows have distinct ids; rows that share one step one after another, in row order.)
 *     3 entries with frames - last_seen > E are removed and the rest compacted.
 *     4 the frame's COUNT LIST, int32 [FRCNN_COUNT_LIST_WORDS] = [n_events, frames, 0, 0 | totals[8][2] as they stand behind this
 *       frame | events[64][4]], is written to list f of a workspace of `frames` lists: the events in (row, line) order, (l, dir, id, cls)
 *       each, n_events of them and every word behind them 0.  Events beyond FRCNN_COUNT_MAX_EVENTS (64) are left out of the list and
 *       summed into events_dropped; the totals are exact regardless.
 *     Frames f >= nf get a list of zeros.  With nf <= 0 no word of the state is written.
 *   DRAW    of one count list into one frame.  A list whose `frames` word is <= 0 (the list of a frame that is not real) draws nothing.
 *     LINES   line l is the trail rule's capsule of radius W / 2 around A-B: with P a pixel, d = B - A, p = P - A, dd = d.d, u = p.d,
 *             all int64, the line COVERS P when
 *               dd == 0 or u <= 0:   |p|^2 <= (W W) >> 2;
 *               else u >= dd:        |P - B|^2 <= (W W) >> 2;
 *               otherwise:           (p.x d.y - p.y d.x)^2 <= (W W dd) >> 2
 *             (frcnn_hip_track_trails.h DRAW; with coordinates beyond the frame the last square can pass 2^63, so the kernel first
 *             compares |cross| with 2^31, above which no W <= 9 can cover: the same answer in whole numbers).  The colour is
 *             PALETTE[l & 7] of that header; the HIGHEST l wins a shared pixel.
 *     LABELS  above all lines, one label per line: the text "L{l} +{pos} -{neg}", l, pos = totals[l][1] and neg = totals[l][0] in
 *             decimal (a negative total reads as 0), in the 5x7 glyphs at the scale and advance of frcnn_annotate_u8: a character is
 *             10 x 14 pixels, the advance 12.  A text of n characters has the cell box of bw = 12 n by bh = 16 pixels; character k's
 *             glyph has its top left pixel at (x0 + 1 + 12 k, y0 + 1).  The anchor is the line's midpoint, mx = (ax + bx) >> 1,
 *             my = (ay + by) >> 1 (arithmetic shifts); on each axis on its own, a box that fits the frame (bw <= w; bh <= h) is
 *             shifted inside it, x0 = min(max(mx, 0), w - bw), and one that does not stays at the anchor, x0 = mx, and is clipped; y0
 *             likewise from my, bh and h.  Glyph pixels take the line's colour, every other pixel of the box is black (0, 0, 0); the
 *             HIGHEST l wins a pixel that two boxes share, and any box wins over any line.
 *             `rgb` says which channel order the frame's bytes are in (non-zero: R, G, B; zero: B, G, R).  Nothing else of the frame is
 *             written, and every byte has one writer. */
#ifndef FRCNN_HIP_COUNT_H
#define FRCNN_HIP_COUNT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_COUNT_VERSION 1
#define FRCNN_COUNT_MAX_LINES 8
#define FRCNN_COUNT_MAX_EVENTS 64
#define FRCNN_COUNT_MIN_COORD (-32768)
#define FRCNN_COUNT_MAX_COORD 65535
#define FRCNN_COUNT_MAX_WIDTH 9
#define FRCNN_COUNT_DEFAULT_WIDTH 3
#define FRCNN_COUNT_MAX_EXPIRE 4095
#define FRCNN_COUNT_MAX_CLASSES 256
#define FRCNN_COUNT_LIST_WORDS (4 + 2 * FRCNN_COUNT_MAX_LINES + 4 * FRCNN_COUNT_MAX_EVENTS)
int frcnn_count_version(void);

/* Bytes of a state: 4 * (20 + 6 * capacity); 0 for a capacity outside 1..FRCNN_TRACK_MAX. */
size_t frcnn_count_state_bytes(int capacity);

/* 4-byte words of one count list: FRCNN_COUNT_LIST_WORDS (276).  A workspace is `frames` lists. */
size_t frcnn_count_list_words(void);

/* Steps 1-4 over the frames of one call, in order, in ONE launch on `stream` (one workgroup: frame f + 1 needs frame f's table, which
 * it keeps in LDS; the parallelism is over rows and entries inside a frame: wave64 ballots and prefixes for the ranks, one writer per
 * word, plain vector stores, no atomics).  Everything but the scalars and `lines` is DEVICE memory.
 *   state        frcnn_count_state_bytes(capacity) bytes, read and written.
 *   tracked      frame f's tracked buffer at tracked + f * tracked_stride (4-byte words): int32[4 + 8 * rows] as frcnn_track_update
 *                (rows = max_rows + capacity) or the look-back (rows = R2) writes it; bbox, id and cls of the rows r < n_live are read.
 *   n_frames, gate   see PER FRAME; gate may be NULL.  (A caller whose n_frames word is a COUNT another kernel wrote -- the frames a
 *                look-back emitted -- passes as gate the word that says whether the pass itself is real.)
 *   lines        HOST memory, int32 [n_lines][4]: read before the call returns, passed to the kernel by value.
 *   classes      uint8 [num_classes].
 *   h, w         the frame's sides: the POINT's clipped box.
 *   lists        `frames` count lists, every word written by one thread.
 * No allocation, no synchronisation, nothing read on the host but `lines`, so the call can be captured in a graph and replayed.
 * FRCNN_E_ARG, with nothing launched: a null pointer (but gate); capacity outside 1..FRCNN_TRACK_MAX; rows outside
 * 1..FRCNN_REDACT_MAX_ROWS; frames outside 1..FRCNN_TRACK_MAX_FRAMES; tracked_stride < 4 + 8 * rows with frames > 1; n_lines outside
 * 1..FRCNN_COUNT_MAX_LINES; a coordinate out of range; A = B; num_classes outside 1..FRCNN_COUNT_MAX_CLASSES; expire out of range; a side
 * outside 1..FRCNN_REDACT_MAX_SIDE. */
int frcnn_count_update(int32_t* state, int capacity, const int32_t* tracked, long long tracked_stride, int rows, int frames,
                       const int32_t* n_frames, const int32_t* gate, const int32_t* lines, int n_lines, const uint8_t* classes,
                       int num_classes, int expire, int h, int w, int32_t* lists, void* stream);

/* DRAW of one count list into one frame, uint8 [h][w][3] contiguous, edited in place, in ONE launch on `stream`: a gather.  A workgroup
 * owns a tile of 256 byte columns x 16 rows (threads are bytes: 64 lanes on 64 consecutive bytes are one coalesced access wherever a row
 * of 3-byte pixels starts); it stages in LDS the lines whose bounding box, grown by (W + 1) >> 1, meets the tile and the label boxes that
 * do, their texts formatted on the device, and returns without touching a pixel when nothing meets it.  No atomics, one writer per byte.
 * The list's words are read by the kernel, so the call can be captured and replayed.  `lines`: HOST memory, as above.
 * FRCNN_E_ARG, with nothing launched: a null pointer; a side outside 1..FRCNN_REDACT_MAX_SIDE; n_lines, a coordinate or width out of
 * range; A = B. */
int frcnn_count_draw_u8(uint8_t* frame, int h, int w, const int32_t* list, const int32_t* lines, int n_lines, int width, int rgb,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_COUNT_H */
