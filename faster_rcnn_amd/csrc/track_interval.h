// What csrc/track_cut.hip shares with csrc/track_interval.hip: the interval extension's argument checks and the launch of its between-frame
// kernel (a kernel is launched from the translation unit that defines it).
#pragma once
#include "common.h"

namespace frcnn {

// FRCNN_OK, or FRCNN_E_ARG with the message set under the name ``who``: everything frcnn_track_update_interval refuses
int interval_check(const char* who, const int32_t* state, int capacity, const uint8_t* motion_state, const uint8_t* frames_u8,
                   long long frame_stride, const int32_t* det_packed, long long det_stride, int frames, const int32_t* n_frames, int max_rows,
                   const uint8_t* tracked, int num_classes, int thr, int hold, int grow, int radius, int interval, int h, int w,
                   const int32_t* out, long long out_stride);

// Between frame ``f`` of a call of ``total`` frames: its tracked buffer ``o`` from the slots as they stand; the frame counts
void interval_between_launch(int32_t* state, int capacity, int f, int total, const int32_t* n_frames, int max_rows, int grow, int h, int w,
                             int32_t* o, hipStream_t stream);

}  // namespace frcnn
