// What csrc/track_interval.hip shares with csrc/track_motion.hip: the motion extension's own argument checks and the launches of its two
// kernels (a kernel is launched from the translation unit that defines it).
#pragma once
#include "common.h"

namespace frcnn {

// FRCNN_OK, or FRCNN_E_ARG with the message set under the name ``who``: what frcnn_track_update_motion refuses beyond frcnn_track_update
int motion_check(const char* who, const uint8_t* motion_state, const uint8_t* frames_u8, long long frame_stride, int frames, int radius, int h,
                 int w);

// Step 0 of frame ``f`` of a call of ``frames`` frames: one workgroup per slot of the state
void motion_search_launch(int32_t* state, int capacity, const uint8_t* motion_state, const uint8_t* frames_u8, long long frame_stride, int f,
                          int frames, const int32_t* n_frames, int radius, int h, int w, hipStream_t stream);

// Behind a call's last frame: frame nf - 1 and the header into the motion state
void motion_keep_launch(const int32_t* state, uint8_t* motion_state, const uint8_t* frames_u8, long long frame_stride, int frames,
                        const int32_t* n_frames, int h, int w, hipStream_t stream);

}  // namespace frcnn
