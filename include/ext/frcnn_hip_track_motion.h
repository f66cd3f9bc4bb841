/* The tracker's held boxes moved with the pixels under them: an EXTENSION of the C ABI of libfrcnn_hip.so (include/frcnn_hip.h,
 * include/ext/frcnn_hip_track.h and the other extension headers stay as they are, and so does frcnn_track_update).  Same library, same
 * conventions, a revision of its own: a host that uses these entry points checks frcnn_track_motion_version() == FRCNN_TRACK_MOTION_VERSION.
 *   1 = frcnn_track_motion_state_bytes, frcnn_track_update_motion.
 *
 * The rule (DESIGN §8 "Motion rule"; tests/track_motion_ref.py restates it in numpy).  Integers only: a sequence has one right answer.
 *   MOTION STATE  device memory of frcnn_track_motion_state_bytes(h, w) = 16 + 3hw bytes: a header int32[4] = [kept, h, w, 0] and one kept
 *           frame uint8[h][w][3].  A zeroed header means "no reference".
 *   With nf = min(max(*n_frames, 0), frames), for each frame f < nf in order, STEP 0 in front of frcnn_hip_track.h's steps 1-4:
 *     0 MOTION
 *       REFERENCE P  for f > 0 frame f - 1 of this call.  For f = 0 the kept frame, if and only if header[0] >= 1, header[0] == the
 *               state's `frames` word (state[3]) as it was when the call began, header[1] == h and header[2] == w; otherwise there is no
 *               reference and step 0 is skipped for this frame.
 *       LUMA    L(F, x, y) = (F[y][x][0] + 2 F[y][x][1] + F[y][x][2] + 2) >> 2: symmetric in channels 0 and 2, so BGR and RGB frames
 *               give the same result.
 *       Every live slot, those of age 0 included, is searched independently:
 *       BOX     (xa, xb, ya, yb) = the slot's clipped box (frcnn_hip_track.h BOX); an empty box is skipped.
 *       GRID    bw = xb - xa + 1, sx = (bw + 31) / 32; the sample columns are x = xa + sx / 2 + i sx while x <= xb; rows likewise with
 *               sy from yb - ya + 1.  n = columns * rows, at most 32 * 32.  The slot is skipped when n < 16.
 *       COST    cost(dx, dy) = the sum over the grid of |L(cur, clamp(x + dx, 0, w - 1), clamp(y + dy, 0, h - 1)) - L(P, x, y)| for every
 *               |dx| <= radius and |dy| <= radius (edge replication, as in the blur); at most 1024 * 255.
 *       BEST    the smallest (cost, dx^2 + dy^2, dy, dx), compared lexicographically.
 *       GATE    the move is taken only when cost(best) + n <= cost(0, 0) (an average gain of one grey level per sample: a flat or
 *               unchanged region does not move).  Then the slot's RAW bbox becomes (x1 + dx, y1 + dy, x2 + dx, y2 + dy); id, cls, prob
 *               and age are untouched.
 *     1-4       exactly frcnn_hip_track.h's, on the moved slots: a match compares against the moved box, and a held row's output box is
 *               the moved box grown by grow * age.
 *   AFTER the last real frame (nf >= 1): the kept frame becomes frame nf - 1's bytes and the header [state[3] after the call, h, w, 0].
 *   With nf <= 0 no byte of the state, the motion state or the kept frame is written; the `out` buffers of padding frames are written as
 *   frcnn_track_update writes them.
 *   CONSEQUENCE  with a zeroed motion header and frames = 1, `state` and `out` are byte for byte what frcnn_track_update produces. */
#ifndef FRCNN_HIP_TRACK_MOTION_H
#define FRCNN_HIP_TRACK_MOTION_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_TRACK_MOTION_VERSION 1
#define FRCNN_TRACK_MOTION_MIN_RADIUS 1
#define FRCNN_TRACK_MOTION_MAX_RADIUS 16
#define FRCNN_TRACK_MOTION_GRID 32         /* sample columns, and rows, of a slot at most */
#define FRCNN_TRACK_MOTION_MIN_SAMPLES 16  /* a slot with fewer samples is not searched */
int frcnn_track_motion_version(void);

/* Bytes of a motion state for h x w frames: 16 + 3hw; 0 for a side outside 1..FRCNN_REDACT_MAX_SIDE. */
size_t frcnn_track_motion_state_bytes(int h, int w);

/* frcnn_track_update with step 0.  Everything but the scalars is DEVICE memory; the arguments frcnn_track_update has mean what they
 * mean there, and `out` has its layout (the redaction and frcnn_annotate_ids_u8 consume it unchanged).
 *   motion_state  frcnn_track_motion_state_bytes(h, w) bytes, 4-byte aligned, read and written.
 *   frames_u8     frame f of the call at frames_u8 + f * frame_stride (bytes): [h][w][3] uint8 in any channel order, read only.
 *   radius        FRCNN_TRACK_MOTION_MIN_RADIUS..FRCNN_TRACK_MOTION_MAX_RADIUS.
 * Per frame at most two launches on `stream` (the search: one workgroup per slot; steps 1-4: frcnn_track_update's kernel on that one
 * frame), and one more per call that keeps frame nf - 1.  No allocation, no synchronisation, nothing read on the host: *n_dets, *n_frames
 * and the slot count are read by the kernels, so the call can be captured in a graph and replayed.
 * FRCNN_E_ARG, with nothing launched: everything frcnn_track_update refuses; a null motion_state or frames_u8; radius out of range;
 * frame_stride < 3hw with frames > 1. */
int frcnn_track_update_motion(int32_t* state, int capacity, uint8_t* motion_state, const uint8_t* frames_u8, long long frame_stride,
                              const int32_t* det_packed, long long det_stride, int frames, const int32_t* n_frames, int max_rows,
                              const uint8_t* tracked, int num_classes, int thr, int hold, int grow, int radius, int h, int w, int32_t* out,
                              long long out_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_TRACK_MOTION_H */
