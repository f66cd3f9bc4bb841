/* The detector on every K-th frame, the block match alone in between: an EXTENSION of the C ABI of libfrcnn_hip.so (include/frcnn_hip.h,
 * include/ext/frcnn_hip_track.h, include/ext/frcnn_hip_track_motion.h and the other extension headers stay as they are, and so do
 * frcnn_track_update and frcnn_track_update_motion).  Same library, same conventions, a revision of its own: a host that uses these entry
 * points checks frcnn_track_interval_version() == FRCNN_TRACK_INTERVAL_VERSION.
 *   1 = frcnn_track_update_interval.
 *
 * The rule (DESIGN §8 "Interval rule"; tests/track_interval_ref.py restates it in numpy).  Integers only: a sequence has one right answer.
 *   With nf = min(max(*n_frames, 0), frames), frame f < nf of the call is a KEY frame when f % interval == 0, otherwise a BETWEEN frame.
 *   DETECTIONS  det_packed holds one packed buffer per KEY frame: key frame f reads det_packed + (f / interval) * det_stride.  A between
 *           frame reads no detections.
 *   KEY FRAME   exactly frcnn_hip_track_motion.h's step 0 followed by frcnn_hip_track.h's steps 1-4, unchanged.
 *   BETWEEN FRAME
 *     0 MOTION  exactly frcnn_hip_track_motion.h's step 0: every live slot, the same REFERENCE (frame f - 1 of the call; a between frame is
 *               never frame 0), LUMA, GRID, COST, BEST and GATE.
 *     No MATCH, no AGE, no BIRTH: ages, ids, cls, prob, `issued` and `overflow` are untouched.  `hold` is therefore counted in KEY frames,
 *               and a held box does not grow between two key frames.
 *     OUTPUT    the tracked buffer of frcnn_hip_track.h, R = max_rows + capacity: first the slots of age 0 in id order as live rows, bbox =
 *               the slot's RAW (moved) bbox, the slot's cls, prob and id, age 0; n_live = their count.  Then the held slots (age >= 1) in
 *               id order, exactly as step 4 writes held rows (the clipped box grown by grow * age).  n_rows = n_live + held; words [2] and
 *               [3] are next_id and overflow; rows behind n_rows: bbox -1, cls -1, prob, id, age 0.
 *   FRAMES SEEN  the state's `frames` word (state[3]) counts every real frame, key or between.  The kept frame and its header are written
 *           after the last real frame, as in the Motion rule: frame nf - 1's bytes and [state[3] after the call, h, w, 0].
 *   With nf <= 0 no byte of the state, the motion state or the kept frame is written; the `out` buffers of padding frames (f >= nf) are
 *   written as frcnn_track_update writes them.
 *   CONSEQUENCES
 *     with interval == 1 every byte of `state`, `motion_state` and `out` is what frcnn_track_update_motion produces;
 *     with identical consecutive frames a between frame's live rows are the tracked rows of the frame before, unmoved (the gate). */
#ifndef FRCNN_HIP_TRACK_INTERVAL_H
#define FRCNN_HIP_TRACK_INTERVAL_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_TRACK_INTERVAL_VERSION 1
#define FRCNN_TRACK_INTERVAL_MIN 1
#define FRCNN_TRACK_INTERVAL_MAX 16  /* frames from one key frame to the next, at most */
int frcnn_track_interval_version(void);

/* frcnn_track_update_motion with the detector's frames `interval` apart.  Everything but the scalars is DEVICE memory; the arguments
 * frcnn_track_update_motion has mean what they mean there, except
 *   det_packed   key frame f's detections at det_packed + (f / interval) * det_stride: (frames + interval - 1) / interval buffers;
 *   frames       the frames of the call, key and between, 1..FRCNN_TRACK_MAX_FRAMES; frames_u8 and `out` hold one entry per FRAME;
 *   interval     FRCNN_TRACK_INTERVAL_MIN..FRCNN_TRACK_INTERVAL_MAX.
 * Per frame at most two launches on `stream` (the search: one workgroup per slot; then a key frame's steps 1-4, frcnn_track_update's kernel
 * on that one frame, or a between frame's output, one small workgroup), and one more per call that keeps frame nf - 1.  No allocation, no
 * synchronisation, nothing read on the host: *n_dets, *n_frames and the slot count are read by the kernels, so the call can be captured in
 * a graph and replayed.
 * FRCNN_E_ARG, with nothing launched: everything frcnn_track_update_motion refuses, its det_stride check apart; interval out of range;
 * det_stride < 4 + 7 * max_rows with (frames + interval - 1) / interval > 1. */
int frcnn_track_update_interval(int32_t* state, int capacity, uint8_t* motion_state, const uint8_t* frames_u8, long long frame_stride,
                                const int32_t* det_packed, long long det_stride, int frames, const int32_t* n_frames, int max_rows,
                                const uint8_t* tracked, int num_classes, int thr, int hold, int grow, int radius, int interval, int h, int w,
                                int32_t* out, long long out_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_TRACK_INTERVAL_H */
