/* Every track ended at a hard cut of the footage: an EXTENSION of the C ABI of libfrcnn_hip.so (include/frcnn_hip.h,
 * include/ext/frcnn_hip_track.h, include/ext/frcnn_hip_track_motion.h, include/ext/frcnn_hip_track_interval.h and the other extension
 * headers stay as they are, and so do frcnn_track_update, frcnn_track_update_motion and frcnn_track_update_interval).  Same library, same
 * conventions, a revision of its own: a host that uses these entry points checks frcnn_track_cut_version() == FRCNN_TRACK_CUT_VERSION.
 *   1 = frcnn_track_cut_workspace_bytes, frcnn_track_update_cut.
 *
 * The rule (DESIGN §8 "Cut rule"; tests/track_cut_ref.py restates it in numpy).  Integers only: a sequence has one right answer.
 *   LUMA and REFERENCE  L(F, x, y) and the reference frame P of frame f are frcnn_hip_track_motion.h's: for f > 0 frame f - 1 of the call, for
 *           f = 0 the kept frame under exactly that header's conditions (header[0] >= 1, header[0] == state[3] as it was when the call
 *           began, header[1] == h, header[2] == w); otherwise frame f has no reference and is never a cut.
 *   SIGNATURE  of a frame F: 4 x 4 regions x 32 bins = 512 counters.  Pixel (x, y) belongs to region (ry, rx) = ((4 y) / h, (4 x) / w), its
 *           bin is L(F, x, y) >> 3, and H_F[ry][rx][bin] counts the frame's pixels, every one of them: the counters sum to hw.
 *   DISTANCE   D(f) = the sum over the 512 counters of |H_cur - H_P|, at most 2hw.
 *   DECISION   with nf = min(max(*n_frames, 0), frames), frame f < nf is a CUT when it has a reference and D * 100 >= pct * 2 * h * w,
 *           compared in 64 bits.  cuts[f] = 1 on a cut and 0 otherwise, frames f >= nf included.
 *           The regions keep a pan, or an object that moves inside a region, from counting as a change.  A fade or a dissolve changes the
 *           signature a little per frame and is NOT detected.
 *   EFFECT     a step C in front of step 0 of the Interval rule (frcnn_hip_track_interval.h), on every frame f < nf, key and between alike:
 *           on a cut every live slot is freed -- n_slots = 0 and the slot words are zeroed; `issued`, `overflow` and `frames` stay.  Step 0
 *           then finds no slot to search, steps 1-4 of a key frame give every eligible row a new id, and a between frame emits no rows
 *           until the next key frame: ids never continue across a cut and no held row crosses it.
 *   The kept frame and its header after the call are the Interval rule's, unchanged.
 *   CONSEQUENCE  with no cut in a call every byte of `state`, `motion_state` and `out` is what frcnn_track_update_interval produces. */
#ifndef FRCNN_HIP_TRACK_CUT_H
#define FRCNN_HIP_TRACK_CUT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_TRACK_CUT_VERSION 1
#define FRCNN_TRACK_CUT_REGIONS 4    /* regions along each side of a frame */
#define FRCNN_TRACK_CUT_BINS 32      /* luma bins of a region: L >> 3 */
#define FRCNN_TRACK_CUT_MIN_PCT 1
#define FRCNN_TRACK_CUT_MAX_PCT 100
int frcnn_track_cut_version(void);

/* Bytes of the workspace of a call of `frames` frames: (frames + 1) signatures of 512 int32 counters (the kept frame's and one per
 * frame); 0 for frames outside 1..FRCNN_TRACK_MAX_FRAMES. */
size_t frcnn_track_cut_workspace_bytes(int frames);

/* frcnn_track_update_interval with step C.  Everything but the scalars is DEVICE memory; the arguments frcnn_track_update_interval has
 * mean what they mean there (interval 1 is the motion form), and
 *   pct        FRCNN_TRACK_CUT_MIN_PCT..FRCNN_TRACK_CUT_MAX_PCT: the share of 2hw at which a frame is a cut;
 *   workspace  frcnn_track_cut_workspace_bytes(frames) bytes, 4-byte aligned, written by every call (nothing is carried in it);
 *   cuts       int32[frames], written by every call.
 * Three launches on `stream` in front of the frames (the workspace cleared; the frames + 1 signatures: workgroups over row bands of every
 * frame, a histogram in LDS per wave with integer LDS atomics, flushed with integer global atomics -- integer sums do not depend on their
 * order --; the decisions), then per frame one small launch that frees the slots where cuts[f] is set in front of
 * frcnn_track_update_interval's own launches.  No allocation, no synchronisation, nothing read on the host: *n_dets, *n_frames, the motion
 * state's header and the slot count are read by the kernels, so the call can be captured in a graph and replayed.
 * FRCNN_E_ARG, with nothing launched: everything frcnn_track_update_interval refuses; pct out of range; a null workspace or cuts. */
int frcnn_track_update_cut(int32_t* state, int capacity, uint8_t* motion_state, const uint8_t* frames_u8, long long frame_stride,
                           const int32_t* det_packed, long long det_stride, int frames, const int32_t* n_frames, int max_rows,
                           const uint8_t* tracked, int num_classes, int thr, int hold, int grow, int radius, int interval, int h, int w,
                           int32_t* out, long long out_stride, int pct, int32_t* workspace, int32_t* cuts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_TRACK_CUT_H */
