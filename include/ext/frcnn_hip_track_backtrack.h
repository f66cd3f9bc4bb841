/* Tracks hidden on the frames BETWEEN two detections, from both sides: an EXTENSION of the C ABI of libfrcnn_hip.so (include/frcnn_hip.h,
 * include/ext/frcnn_hip_track_lookback.h, include/ext/frcnn_hip_track_interval.h and the other extension headers stay as they are, and so
 * do their entry points).  Same library, same conventions, a revision of its own: a host that uses these entry points checks
 * frcnn_track_backtrack_version() == FRCNN_TRACK_BACKTRACK_VERSION.
 *   1 = frcnn_track_backtrack.
 *
 * The rule (DESIGN §8 "Back-track rule"; tests/track_backtrack_ref.py restates it in numpy).  Integers only: a sequence has one right
 * answer.  It is the look-back rule of frcnn_hip_track_lookback.h over the tracked buffers of frcnn_track_update_interval, with more rows
 * chained.  PARAMETERS, WIDENED, WINDOW (the same bytes: frcnn_track_lookback_state_bytes), SEQUENCE S, JOIN, EMIT, CLOSE, *n_frames == 0
 * and *n_frames < 0 are that header's, word for word; `frames` is the F source frames of a call, key and between.  New or changed:
 *   KEY     with `interval` K: frame f of the call is a KEY frame iff f % K == 0; window frame i is a key frame iff i % K == 0 (every call
 *           starts on a key frame).  Every other frame is a BETWEEN frame.
 *   SOURCE  in KEY frame t of the call, t >= 1 in S: a live row (index < n_live) with id >= 1; the first `capacity` of them in row order
 *           (the tracker has no more slots).  A source is a BIRTH when id >= first_id(t), the next_id word of the buffer in front of t in
 *           S (the look-back's definition), otherwise a CORRECTION.  Rows with id 0 and all rows of between frames are not sources.
 *   CHAIN   the look-back's step, unchanged: REFERENCE P = frame g + 1, "current" = frame g, b_g = b_{g+1} shifted by the taken move; the
 *           BACK-FILLED row in frame g has bbox = the clipped b_g grown by grow * k, or -1s when empty, cls, prob and id of the source
 *           row, age = -k.  A birth walks k = 1..L while g = t - k is in S.  A correction walks k = 1..L while g is in S AND g is a
 *           between frame: it stops in front of the previous key frame, where the track's box came from a detection.  Neither stops
 *           early because of pixels.
 *   PLACE   frame g's back-filled rows follow its held rows, ordered by source frame t ascending, then by source row ascending.  A row's
 *           place = g's n_rows as joined (or as the calls before left it) + the sources of the call's key frames strictly between g and
 *           t that reach g + the row's rank among t's sources that reach g.  Rows that would pass R2 are dropped from the end of that
 *           order and counted in back_overflow (sticky).  n_live never moves.
 *   CONSEQUENCES
 *     with interval == 1 every byte of the window, the emitted frames and the emitted buffers is frcnn_track_lookback's;
 *     with every call full and L <= frames the emitted sequence does not depend on how the sequence was cut into calls;
 *     with L >= K - 1 every between frame carries a row tracked back from the next key frame for every track that key frame sees. */
#ifndef FRCNN_HIP_TRACK_BACKTRACK_H
#define FRCNN_HIP_TRACK_BACKTRACK_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_TRACK_BACKTRACK_VERSION 1
int frcnn_track_backtrack_version(void);

/* One call of the rule: frcnn_track_lookback's arguments, which mean what they mean there, and
 *   interval      K, 1..FRCNN_TRACK_INTERVAL_MAX (16): the `interval` frcnn_track_update_interval made `tracked` with.
 * Five launches on `stream` (join, chain: one workgroup per source of a key frame, counts, emit, close; join, emit and close are the
 * look-back's kernels).  No allocation, no synchronisation, nothing read on the host: the call can be captured in a graph and replayed.
 * FRCNN_E_ARG, with nothing launched: everything frcnn_track_lookback refuses; interval outside 1..16. */
int frcnn_track_backtrack(uint8_t* window, const uint8_t* frames_u8, long long frame_stride, const int32_t* tracked, long long tracked_stride,
                          int frames, const int32_t* n_frames, int max_rows, int capacity, int back, int lookback, int radius, int grow,
                          int interval, int h, int w, uint8_t* out_frames, long long out_frame_stride, int32_t* out_tracked,
                          long long out_tracked_stride, int32_t* out_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_TRACK_BACKTRACK_H */
