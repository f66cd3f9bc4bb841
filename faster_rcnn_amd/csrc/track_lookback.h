// What csrc/track_backtrack.hip shares with csrc/track_lookback.hip: the window's geometry and cells, the look-back extension's argument
// checks and the launches of its join, emit and close kernels (a kernel is launched from the translation unit that defines it).
#pragma once
#include "common.h"
#include "../../include/ext/frcnn_hip_redact.h"
#include "../../include/ext/frcnn_hip_track.h"
#include "../../include/ext/frcnn_hip_track_lookback.h"

namespace frcnn {

constexpr int LB_HEADER = FRCNN_TRACK_LOOKBACK_HEADER;
constexpr int LB_MAX_ROWS = FRCNN_REDACT_MAX_ROWS;

struct LbGeom {
    int frames, R, R2, cap, h, w;
    long long tracked_bytes, cell;                      // a widened buffer; a cell (buffer + padded frame)
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// cell ``s`` of the call's sequence: the c window frames in half ``half``, then the call's frames in the other half
__device__ __forceinline__ uint8_t* lb_cell(uint8_t* window, const LbGeom& g, int c, int half, int s) {
    const int at = s < c ? half * g.frames + s : (half ^ 1) * g.frames + (s - c);
    return window + LB_HEADER + (long long)at * g.cell;
}

// the geometry of a window, or false for an argument out of range (``why`` says which)
bool lb_geom(int frames, int h, int w, int max_rows, int capacity, int back, LbGeom& g, const char*& why);

// FRCNN_OK with ``g`` set, or FRCNN_E_ARG with the message set under the name ``who``: everything frcnn_track_lookback refuses
int lookback_check(const char* who, const uint8_t* window, const uint8_t* frames_u8, long long frame_stride, const int32_t* tracked,
                   long long tracked_stride, int frames, const int32_t* n_frames, int max_rows, int capacity, int back, int lookback, int radius,
                   int grow, int h, int w, const uint8_t* out_frames, long long out_frame_stride, const int32_t* out_tracked,
                   long long out_tracked_stride, const int32_t* out_count, LbGeom& g);

// JOIN: the call's frames and their tracked buffers, widened, into the cells of the window's other half
void lookback_join_launch(uint8_t* window, const LbGeom& g, const uint8_t* frames_u8, long long frame_stride, const int32_t* tracked,
                          long long tracked_stride, const int32_t* n_frames, hipStream_t stream);

// EMIT: the window's frames copied out
void lookback_emit_launch(uint8_t* window, const LbGeom& g, uint8_t* out_frames, long long out_frame_stride, int32_t* out_tracked,
                          long long out_tracked_stride, int32_t* out_count, hipStream_t stream);

// CLOSE: the header behind a call
void lookback_close_launch(uint8_t* window, const LbGeom& g, const int32_t* n_frames, hipStream_t stream);

}  // namespace frcnn
