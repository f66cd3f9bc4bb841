/* Low-score rows that keep a track alive: an EXTENSION of the C ABI of libfrcnn_hip.so (include/frcnn_hip.h, include/ext/frcnn_hip_track.h,
 * include/ext/frcnn_hip_track_motion.h, include/ext/frcnn_hip_track_interval.h, include/ext/frcnn_hip_track_cut.h and the other extension
 * headers stay as they are, and so do frcnn_track_update, frcnn_track_update_motion, frcnn_track_update_interval and
 * frcnn_track_update_cut).  Same library, same conventions, a revision of its own: a host that uses these entry points checks
 * frcnn_track_weak_version() == FRCNN_TRACK_WEAK_VERSION.
 *   1 = frcnn_track_update_weak, frcnn_track_update_motion_weak, frcnn_track_update_interval_weak, frcnn_track_update_cut_weak.
 *
 * The rule (DESIGN §8 "Weak rule"; tests/track_weak_ref.py restates it in plain Python).  The detector is run with a LOW score threshold
 * and the tracker is told the one the user asked for, `strong`: the rows between the two may continue a track and do nothing else (the
 * second association of ByteTrack, Zhang et al., ECCV 2022).
 *   STRONG  a row whose prob, read as a float32, satisfies prob >= strong under the IEEE comparison; every other row is WEAK, a row with a
 *           NaN score among them.  This is the rule's one float operation; everything else is frcnn_hip_track.h's integers.
 *   The Tracking rule (frcnn_hip_track.h) holds as written but for:
 *     1 MATCH, stage A   the live slots in ascending id order against the eligible STRONG rows only: the Tracking rule's step, word for word.
 *     1 MATCH, stage B   the slots stage A left unmatched go again, in ascending id order: each takes the still unmatched eligible WEAK row
 *               of its own class with the best IoU among those with IoU at least thr percent, the lowest row among equals; it takes the
 *               row's raw bbox and prob, age = 0.  Stage A ends before stage B starts: a strong row beats a weak one that overlaps more.
 *     2 AGE     unchanged; a slot matched in either stage is matched.
 *     3 BIRTH   from the unmatched eligible STRONG rows only; overflow counts those alone.  A weak row never starts a track.
 *     4 OUTPUT  the live part is every strong row, eligible or not, and every weak row stage B matched, in ascending row order, moved up
 *               over the dropped rows, each with its bbox, cls, prob, id (0 = untracked) and age 0.  Every unmatched weak row is dropped,
 *               the ineligible ones included.  n_live = the rows kept; the held rows and the dead rows follow as in the Tracking rule,
 *               n_rows = n_live + held.  The buffer's format is frcnn_hip_track.h's.
 *   CONSEQUENCES  with strong <= every score (and no NaN score) every byte of `state` and `out` is the parent entry point's; with no weak
 *           row within any slot's reach the result is the parent's on the strong rows alone. */
#ifndef FRCNN_HIP_TRACK_WEAK_H
#define FRCNN_HIP_TRACK_WEAK_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_TRACK_WEAK_VERSION 1
int frcnn_track_weak_version(void);

/* Each entry point is the one it is named after -- same arguments, same launches, same states, capturable alike -- with the Weak rule in
 * the place of the Tracking rule's steps 1-4 (the tracker's kernel in its second instantiation; the block match, the between frames and
 * the cut step are untouched), and `strong`, a host scalar, in front of `out`.
 * FRCNN_E_ARG, with nothing launched: everything the parent refuses; a NaN `strong`. */
int frcnn_track_update_weak(int32_t* state, int capacity, const int32_t* det_packed, long long det_stride, int frames, const int32_t* n_frames,
                            int max_rows, const uint8_t* tracked, int num_classes, int thr, int hold, int grow, int h, int w, float strong,
                            int32_t* out, long long out_stride, void* stream);

int frcnn_track_update_motion_weak(int32_t* state, int capacity, uint8_t* motion_state, const uint8_t* frames_u8, long long frame_stride,
                                   const int32_t* det_packed, long long det_stride, int frames, const int32_t* n_frames, int max_rows,
                                   const uint8_t* tracked, int num_classes, int thr, int hold, int grow, int radius, int h, int w, float strong,
                                   int32_t* out, long long out_stride, void* stream);

int frcnn_track_update_interval_weak(int32_t* state, int capacity, uint8_t* motion_state, const uint8_t* frames_u8, long long frame_stride,
                                     const int32_t* det_packed, long long det_stride, int frames, const int32_t* n_frames, int max_rows,
                                     const uint8_t* tracked, int num_classes, int thr, int hold, int grow, int radius, int interval, int h,
                                     int w, float strong, int32_t* out, long long out_stride, void* stream);

int frcnn_track_update_cut_weak(int32_t* state, int capacity, uint8_t* motion_state, const uint8_t* frames_u8, long long frame_stride,
                                const int32_t* det_packed, long long det_stride, int frames, const int32_t* n_frames, int max_rows,
                                const uint8_t* tracked, int num_classes, int thr, int hold, int grow, int radius, int interval, int h, int w,
                                float strong, int32_t* out, long long out_stride, int pct, int32_t* workspace, int32_t* cuts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_TRACK_WEAK_H */
