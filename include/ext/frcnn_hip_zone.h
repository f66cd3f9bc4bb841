/* Who is in a region, how many have been and how long they stayed: polygon zones over the tracker's stable ids, on the device, and the
 * zones and their figures drawn into the frames: an EXTENSION of the C ABI of libfrcnn_hip.so (include/frcnn_hip.h,
 * include/ext/frcnn_hip_count.h and the other extension headers stay as they are, and so do their entry points).  Same library, same
 * conventions (int status, message via the library's last-error call, `stream` = hipStream_t or NULL), a revision of its own: a host that
 * uses these entry points checks frcnn_zone_version() == FRCNN_ZONE_VERSION.
 *   1 = frcnn_zone_state_bytes, frcnn_zone_list_words, frcnn_zone_update, frcnn_zone_draw_u8.
 *
 * The rule (DESIGN §8 "Zone rule"; tests/zone_ref.py restates it in numpy).  Integers only: everything is compared exactly in int64,
 * nothing is divided, and the result never depends on an order of execution.
 *   PARAMETERS  n_zones, 1..FRCNN_ZONE_MAX_ZONES (8); zone z is a polygon of nv[z] vertices, FRCNN_ZONE_MIN_VERTS..FRCNN_ZONE_MAX_VERTS
 *           (3..16), every coordinate in FRCNN_ZONE_MIN_COORD..FRCNN_ZONE_MAX_COORD (-32768..65535), in source-frame pixels: a zone may
 *           extend beyond the frame.  No two consecutive vertices are equal, the last and the first counting as consecutive.  The
 *           polygon need not be convex or simple: the even-odd rule below defines its interior either way.  Width W, 1..9 (default 3);
 *           anchor, 0 = centre, 1 = bottom; expire E, 0..4095, in frames; capacity, 1..FRCNN_TRACK_MAX; classes, uint8 [num_classes],
 *           non-zero where a class counts (the redaction's form).
 *   POINT   of a row, from its clipped box (xa, xb, ya, yb), inclusive on all four sides (frcnn_hip_track_trails.h POINT):
 *             anchor 0: the trail rule's point, cx = (xa + xb) >> 1, cy = (ya + yb) >> 1;
 *             anchor 1: the same cx with y = yb, the lowest pixel row the clipped box covers (yb is INCLUSIVE: the row itself, not the
 *                       one below it).  A person stands where their feet are.
 *           It always lies inside the frame.
 *   INSIDE  INSIDE_z(P), the half-open crossing-number rule.  For each edge (V_i, V_j), j = i + 1 mod nv, with dy = y_j - y_i: the edge
 *           COUNTS when (y_i > py) != (y_j > py) and, with t = (px - x_i) dy - (py - y_i)(x_j - x_i), t < 0 if dy > 0, else t > 0.  P is
 *           inside when an odd number of edges count.  A point on a boundary that two zones share belongs to exactly one of them.  Every
 *           product is under 2^35: int64 suffices.
 *   STATE   device int32 [n_entries, frames, dropped, events_dropped | visitors[8] | stays[8] | dwell[8] | peak[8] | per entry: id, cls,
 *           last_seen, inside, visited, since[8]]: 36 + 13 capacity words.  `inside` and `visited` are masks, bit z for zone z; since[z]
 *           is the value of `frames` at which the open stay in zone z began, 0 when there is none.  The entries are compacted, in
 *           ascending id order; every word behind the live entries is 0.  A zeroed buffer is the empty state.  `dropped` and
 *           `events_dropped` are sticky sums.
 *   PER FRAME  for the real frames f < nf of a call, in order; nf = min(max(*n_frames, 0), frames), and 0 when the call has a `gate`
 *           word that is 0 (both exactly as the count extension's update call has them):
 *     1 frames += 1.
 *     2 the live rows r < n_live of the frame's tracked buffer with id >= 1, a box that is not empty and a class c with 0 <= c <
 *       num_classes and classes[c] != 0, in row order: the entry of the id is found, or one is inserted, keeping id order (the row's cls,
 *       inside = visited = 0, since[] = 0); when the table is full dropped += 1 and the row is skipped.  m = the mask of the zones z with
 *       INSIDE_z(POINT).  For z in ascending order:
 *         ENTER, bit z in m and not in inside: since[z] = frames; if bit z of visited is clear it is set and visitors[z] += 1 (an id is
 *                a visitor of a zone once: jitter on a boundary cannot inflate it); the event (z, 1, id, cls, 0) is appended.
 *         EXIT,  bit z in inside and not in m: d = frames - since[z]; stays[z] += 1; dwell[z] = min(dwell[z] + d, 2^30); the event
 *                (z, 0, id, cls, d) is appended; since[z] = 0.
 *       Then inside = m and last_seen = frames.  An id first seen inside a zone enters it in that frame.  Rows that share an id step one
 *       after another, in row order.  cls in events is the ENTRY's.  Held rows (index >= n_live), back-filled rows and rows with id 0
 *       are never read.
 *     3 entries with frames - last_seen > E leave, in ascending id order: for each bit z of inside in ascending order the event
 *       (z, 2, id, cls, d) with d = last_seen - since[z] + 1 is appended (LOST), stays[z] += 1 and dwell[z] = min(dwell[z] + d, 2^30).
 *       LOST events follow the frame's row events.  The rest of the table is compacted.
 *     4 occupancy[z] = the number of remaining entries with bit z of inside (an entry not seen this frame but not yet expired still
 *       occupies); peak[z] = max(peak[z], occupancy[z]).
 *     5 the frame's ZONE LIST, int32 [FRCNN_ZONE_LIST_WORDS] = [n_events, frames, 0, 0 | occupancy[8] | visitors[8] | stays[8] |
 *       dwell[8] | peak[8] as they stand behind this frame | events[64][5]], is written to list f of a workspace of `frames` lists: the
 *       events (zone, kind, id, cls, dwell) in the order above, n_events of them and every word behind them 0.  Events beyond
 *       FRCNN_ZONE_MAX_EVENTS (64) are left out of the list and summed into events_dropped; the totals are exact regardless.
 *     Frames f >= nf get a list of zeros.  With nf <= 0 no word of the state is written.
 *   DRAW    of one zone list into one frame.  A list whose `frames` word is <= 0 (the list of a frame that is not real) draws nothing.
 *           Three layers, bottom to top:
 *     FILL    for every zone with occupancy[z] > 0, every frame pixel P with INSIDE_z(P) has each channel byte b replaced by
 *             (3 b + c + 2) >> 2, c that channel of PALETTE[z & 7] (frcnn_hip_track_trails.h); a pixel inside several occupied zones is
 *             blended ONCE, with the highest z.
 *     OUTLINE every edge of every zone is the count rule's capsule of radius W / 2 (frcnn_hip_count.h DRAW LINES, its COVER inequalities
 *             and its comparison of |cross| with 2^31 word for word), in PALETTE[z & 7]; the HIGHEST z wins a shared pixel.
 *     LABEL   one per zone, the text "Z{z} {occupancy}/{visitors}" in decimal (a negative figure reads as 0), in the glyph geometry and
 *             with the box placement of the count rule's LABELS: a cell box of 12 n by 16 pixels, on each axis shifted inside the frame
 *             when it fits, else left at the anchor and clipped.  The anchor is the centre of the vertices' bounding box,
 *             ((minx + maxx) >> 1, (miny + maxy) >> 1) (arithmetic shifts).  Glyph pixels take the zone's colour, every other pixel of
 *             the box is black; the HIGHEST z wins among boxes, and any box wins over any outline.
 *             `rgb` says which channel order the frame's bytes are in (non-zero: R, G, B; zero: B, G, R).  Nothing else of the frame is
 *             written, and every byte has one writer. */
#ifndef FRCNN_HIP_ZONE_H
#define FRCNN_HIP_ZONE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_ZONE_VERSION 1
#define FRCNN_ZONE_MAX_ZONES 8
#define FRCNN_ZONE_MIN_VERTS 3
#define FRCNN_ZONE_MAX_VERTS 16
#define FRCNN_ZONE_MAX_EVENTS 64
#define FRCNN_ZONE_MIN_COORD (-32768)
#define FRCNN_ZONE_MAX_COORD 65535
#define FRCNN_ZONE_MAX_WIDTH 9
#define FRCNN_ZONE_DEFAULT_WIDTH 3
#define FRCNN_ZONE_MAX_EXPIRE 4095
#define FRCNN_ZONE_MAX_CLASSES 256
#define FRCNN_ZONE_MAX_DWELL (1 << 30)
#define FRCNN_ZONE_HEAD_WORDS (4 + 4 * FRCNN_ZONE_MAX_ZONES)
#define FRCNN_ZONE_ENTRY_WORDS (5 + FRCNN_ZONE_MAX_ZONES)
#define FRCNN_ZONE_LIST_WORDS (4 + 5 * FRCNN_ZONE_MAX_ZONES + 5 * FRCNN_ZONE_MAX_EVENTS)
int frcnn_zone_version(void);

/* Bytes of a state: 4 * (36 + 13 * capacity); 0 for a capacity outside 1..FRCNN_TRACK_MAX. */
size_t frcnn_zone_state_bytes(int capacity);

/* 4-byte words of one zone list: FRCNN_ZONE_LIST_WORDS (364).  A workspace is `frames` lists. */
size_t frcnn_zone_list_words(void);

/* Steps 1-5 over the frames of one call, in order, in ONE launch on `stream` (one workgroup: frame f + 1 needs frame f's table, which
 * it keeps in LDS; the parallelism is over rows and entries inside a frame: a row's mask of zones is computed by the row's thread,
 * wave64 ballots and prefixes give the ranks, one writer per word, plain vector stores, no atomics).  Everything but the scalars, `verts`
 * and `nv` is DEVICE memory.
 *   state        frcnn_zone_state_bytes(capacity) bytes, read and written.
 *   tracked, tracked_stride, rows, frames, n_frames, gate   as the count extension's update call takes them.
 *   verts, nv    HOST memory: nv is int32 [n_zones], verts int32 (x, y) pairs, zone 0's nv[0] vertices, then zone 1's, and so on: read
 *                before the call returns, passed to the kernel by value.
 *   classes      uint8 [num_classes].
 *   anchor       0 or 1, see POINT.
 *   h, w         the frame's sides: the POINT's clipped box.
 *   lists        `frames` zone lists, every word written by one thread.
 * No allocation, no synchronisation, nothing read on the host but `verts` and `nv`, so the call can be captured in a graph and replayed.
 * FRCNN_E_ARG, with nothing launched: a null pointer (but gate); capacity outside 1..FRCNN_TRACK_MAX; rows outside
 * 1..FRCNN_REDACT_MAX_ROWS; frames outside 1..FRCNN_TRACK_MAX_FRAMES; tracked_stride < 4 + 8 * rows with frames > 1; n_zones outside
 * 1..FRCNN_ZONE_MAX_ZONES; an nv outside 3..16; a coordinate out of range; two equal consecutive vertices; num_classes outside
 * 1..FRCNN_ZONE_MAX_CLASSES; anchor not 0 or 1; expire out of range; a side outside 1..FRCNN_REDACT_MAX_SIDE. */
int frcnn_zone_update(int32_t* state, int capacity, const int32_t* tracked, long long tracked_stride, int rows, int frames,
                      const int32_t* n_frames, const int32_t* gate, const int32_t* verts, const int32_t* nv, int n_zones,
                      const uint8_t* classes, int num_classes, int anchor, int expire, int h, int w, int32_t* lists, void* stream);

/* DRAW of one zone list into one frame, uint8 [h][w][3] contiguous, edited in place, in ONE launch on `stream`: a gather.  A workgroup
 * owns a tile of 256 byte columns x 16 rows (threads are bytes); its first threads stage per zone in LDS the edges, whether the zone's
 * bounding box (for the fill, and only when the zone is occupied) and its box grown by (W + 1) >> 1 (for the outline) meet the tile, and
 * the label's text, formatted on the device, with its box; it returns without touching a pixel when nothing meets it.  The pixel tests
 * are exact, in int64.  No atomics, one writer per byte.  The list's words are read by the kernel, so the call can be captured and
 * replayed.  `verts`, `nv`: HOST memory, as above.
 * FRCNN_E_ARG, with nothing launched: a null pointer; a side outside 1..FRCNN_REDACT_MAX_SIDE; n_zones, an nv, a coordinate or width out
 * of range; two equal consecutive vertices. */
int frcnn_zone_draw_u8(uint8_t* frame, int h, int w, const int32_t* list, const int32_t* verts, const int32_t* nv, int n_zones, int width,
                       int rgb, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_ZONE_H */
