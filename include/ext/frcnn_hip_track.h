/* Detections of consecutive frames joined into tracks on the device: an EXTENSION of the C ABI of libfrcnn_hip.so (include/frcnn_hip.h and
 * the other extension headers stay as they are).  Same library, same conventions (int status, message via frcnn_last_error, `stream` =
 * hipStream_t or NULL), a revision of its own: a host that uses these entry points checks frcnn_track_version() == FRCNN_TRACK_VERSION.
 *   1 = frcnn_track_state_bytes, frcnn_track_update, frcnn_annotate_ids_u8.
 *
 * The rule (DESIGN §8 "Tracking rule"; tests/track_ref.py restates it in plain Python).  Integers only: a sequence has one right answer.
 *   STATE   `capacity` slots, 1 <= capacity <= FRCNN_TRACK_MAX, a count of ids issued (next_id = issued + 1, so ids start at 1), a sticky
 *           `overflow` count and a count of the frames seen.  A live slot holds id (int32 >= 1), cls, the raw bbox of the row it last
 *           matched, that row's prob bits, and age = frames since that match (0: matched in this frame).  Live slots are compacted, in
 *           ascending id order, at all times.  A zeroed buffer is the empty state.  In 4-byte words:
 *             [n_slots, issued, overflow, frames | id[capacity] | cls[capacity] | bbox[capacity][4] | prob[capacity] | age[capacity]],
 *           every word behind the live slots 0.
 *   BOX     of a row or a slot, for matching: the redaction rule's clipped box with margin 0 (frcnn_hip_redact.h): xa = max(min(x1, x2), 0),
 *           xb = min(max(x1, x2), w - 1), ya and yb likewise from y1, y2 and h; inclusive; empty when xa > xb or ya > yb.  area =
 *           (xb - xa + 1)(yb - ya + 1); inter = the area of the intersection of two such boxes (0 when they do not meet), union = area_a +
 *           area_b - inter.  Everything is compared exactly in int64 and nothing is divided: "IoU at least thr percent" is inter > 0 and
 *           inter * 100 >= thr * union; "a better than b" is inter_a * union_b > inter_b * union_a.  Sides are at most FRCNN_REDACT_MAX_SIDE.
 *   ELIGIBLE  row r < n = min(max(*n_dets, 0), max_rows) with 0 <= cls < num_classes, tracked[cls] != 0 and a box that is not empty.
 *   PER FRAME, in this order:
 *     1 MATCH   the live slots in ascending id order: each takes the still unmatched eligible row of its own class with the best IoU among
 *               those with IoU at least thr percent, the lowest row among equals; it takes the row's raw bbox and prob, age = 0.
 *     2 AGE     every unmatched live slot: age += 1; freed when age > hold.  The rest is compacted, order kept.
 *     3 BIRTH   the unmatched eligible rows in ascending row order: each takes a free slot with id = next_id++ (age 0); when none is free
 *               the row stays untracked and overflow += 1.
 *     4 OUTPUT  the n input rows first, order, bbox, cls and prob unchanged, each with its id (0 = untracked) and age 0; then the held
 *               slots (age >= 1) in id order: bbox = (xa - g, ya - g, xb + g, yb + g) with g = grow * age from the slot's clipped box, the
 *               slot's cls, prob, id and age.  n_live = n, n_rows = n + held.  Rows behind n_rows: bbox -1, cls -1, prob, id, age 0.
 *   thr 1..100, hold 0..255 (0: nothing is ever held, ids only), grow 0..64. */
#ifndef FRCNN_HIP_TRACK_H
#define FRCNN_HIP_TRACK_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_TRACK_VERSION 1
#define FRCNN_TRACK_MAX 128          /* slots of a state, at most */
#define FRCNN_TRACK_MAX_FRAMES 64    /* frames of one call, at most */
#define FRCNN_TRACK_MAX_HOLD 255
#define FRCNN_TRACK_MAX_GROW 64
int frcnn_track_version(void);

/* Bytes of a state of `capacity` slots: 4 * (4 + 8 * capacity); 0 for a capacity outside 1..FRCNN_TRACK_MAX. */
size_t frcnn_track_state_bytes(int capacity);

/* The rule over the frames of one pass, in order, in ONE launch on `stream` (one workgroup: frame i + 1 needs frame i's state; the
 * parallelism is inside a frame).  Everything but the scalars is DEVICE memory.
 *   state        int32[4 + 8 * capacity], read and written.
 *   det_packed   frame f's detections at det_packed + f * det_stride (4-byte words): the packed buffer of frcnn_detections(_dyn) with
 *                max_rows rows, [n_dets, 3 words | bbox[max_rows][4] | cls[max_rows] | prob[max_rows] | ...]; rows >= *n_dets are never read.
 *   n_frames     one int32: frames f >= *n_frames (a short pass's padding) neither change the state nor count as a frame; their tracked
 *                buffer is [0, 0, next_id, overflow] and no rows.  With *n_frames <= 0 no word of the state is written.
 *   tracked      uint8[num_classes], non-zero where a class is tracked.
 *   out          frame f's tracked buffer at out + f * out_stride: int32[4 + 8R], R = max_rows + capacity,
 *                [n_rows, n_live, next_id, overflow | bbox[R][4] | cls[R] | prob[R] | id[R] | age[R]], every word written by one thread;
 *                bbox, cls and &n_rows are what the redaction (frcnn_hip_redact.h) takes as det_bbox, det_cls, n_dets with max_rows = R; bbox, cls, prob, id
 *                and &n_live what frcnn_annotate_ids_u8 takes.
 * No allocation, no synchronisation, nothing read on the host: *n_dets and *n_frames are read by the kernel, so the call can be captured in
 * a graph and replayed.  The same state and detections give the same bytes.
 * FRCNN_E_ARG, with nothing launched: a null pointer; capacity outside 1..FRCNN_TRACK_MAX; frames outside 1..FRCNN_TRACK_MAX_FRAMES;
 * max_rows < 1 or max_rows + capacity > FRCNN_REDACT_MAX_ROWS (512); det_stride < 4 + 7 * max_rows or out_stride < 4 + 8R with frames > 1;
 * num_classes outside 1..256; thr outside 1..100; hold outside 0..255; grow outside 0..64; a side outside 1..FRCNN_REDACT_MAX_SIDE. */
int frcnn_track_update(int32_t* state, int capacity, const int32_t* det_packed, long long det_stride, int frames, const int32_t* n_frames,
                       int max_rows, const uint8_t* tracked, int num_classes, int thr, int hold, int grow, int h, int w, int32_t* out,
                       long long out_stride, void* stream);

/* frcnn_annotate_u8 (include/frcnn_hip.h) with the rows' track ids: a row with det_id[r] > 0 is labelled
 * "{}#{} {:6.2f}".format(cls_name, id, prob), any other row as frcnn_annotate_u8 labels it; det_id NULL is frcnn_annotate_u8 exactly (the
 * two share one kernel).  det_id: int32[max_rows] on the device.  Errors as frcnn_annotate_u8. */
int frcnn_annotate_ids_u8(uint8_t* frame, int height, int width, const int32_t* det_bbox, const int32_t* det_cls, const float* det_prob,
                          const int32_t* det_id, const int32_t* n_dets, int max_rows, const uint8_t* drawable, const char* labels,
                          int label_stride, int num_classes, const uint8_t* glyphs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_TRACK_H */
