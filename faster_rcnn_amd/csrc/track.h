// What csrc/track_motion.hip and csrc/track_interval.hip share with csrc/track.hip: frcnn_track_update's argument checks and the launch of its kernel on a part of
// a call's frames (a kernel is launched from the translation unit that defines it).
#pragma once
#include "common.h"

namespace frcnn {

// FRCNN_OK, or FRCNN_E_ARG with the message set under the name ``who``: everything frcnn_track_update refuses
int track_check(const char* who, const int32_t* state, int capacity, const int32_t* det_packed, long long det_stride, int frames,
                const int32_t* n_frames, int max_rows, const uint8_t* tracked, int num_classes, int thr, int hold, int grow, int h, int w,
                const int32_t* out, long long out_stride);

// ``strong``, here and below: null for the Tracking rule; else a HOST value, the Weak rule's threshold (frcnn_hip_track_weak.h), read
// before the call returns.
// Steps 1-4 over frames [first, first + frames) of a call of ``total`` frames, in one launch; det_packed and out are the CALL's
void track_launch(int32_t* state, int capacity, const int32_t* det_packed, long long det_stride, int first, int frames, int total,
                  const int32_t* n_frames, int max_rows, const uint8_t* tracked, int num_classes, int thr, int hold, int grow, int h, int w,
                  int32_t* out, long long out_stride, hipStream_t stream, const float* strong = nullptr);

// The same with the buffers of frame ``first`` given as they lie: ``det`` and ``out`` are THAT frame's (the interval extension, whose
// detections are not one buffer per frame)
void track_launch_at(int32_t* state, int capacity, const int32_t* det, long long det_stride, int first, int frames, int total,
                     const int32_t* n_frames, int max_rows, const uint8_t* tracked, int num_classes, int thr, int hold, int grow, int h, int w,
                     int32_t* out, long long out_stride, hipStream_t stream, const float* strong = nullptr);

// What the _weak entries (include/ext/frcnn_hip_track_weak.h) refuse on top of their parents: FRCNN_E_ARG for a NaN ``strong``
int weak_check(const char* who, float strong);

}  // namespace frcnn
