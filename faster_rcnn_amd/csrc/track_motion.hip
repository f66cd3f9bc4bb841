// The tracker's slots moved with the pixels under them (include/ext/frcnn_hip_track_motion.h states the rule, DESIGN §8 "Motion rule"): an
// integer block match per live slot between two frames, in front of csrc/track.hip's steps 1-4.  gfx950 (CDNA4) only.
// A call's frames are walked one by one by csrc/track.hip's track_walk (csrc/track_call.h) -- the search of frame f + 1 needs the boxes
// after frame f --: k_motion_search (one workgroup per slot of the state; one past n_slots, read on the device, returns at once) and then
// track.hip's kernel on that frame; k_motion_keep closes the call.  This file defines the two kernels, their launches and the entries.  The
// search itself is csrc/track_motion_search.h's (shared with csrc/track_lookback.hip).  One writer per slot word; no atomics.
#include "common.h"
#include "../../include/ext/frcnn_hip_redact.h"
#include "../../include/ext/frcnn_hip_track.h"
#include "../../include/ext/frcnn_hip_track_motion.h"
#include "../../include/ext/frcnn_hip_track_weak.h"
#include "track_call.h"
#include "track_motion_search.h"

namespace frcnn {

constexpr int TM_HEADER = 16;                                               // bytes in front of the kept frame

// Step 0 for frame ``f`` of the call, slot blockIdx.x.
__global__ void __launch_bounds__(TM_THREADS) k_motion_search(int32_t* state, int cap, const uint8_t* motion_state, const uint8_t* frames_u8,
                                                                long long frame_stride, int f, int frames, const int32_t* n_frames,
                                                                int radius, int h, int w) {
    __shared__ TmShared sh;
    const int slot = blockIdx.x, lane = threadIdx.x & 63;
    if (f >= min(max(*n_frames, 0), frames)) return;                        // padding
    if (slot >= min(max(state[0], 0), cap)) return;
    const uint8_t* ref;
    if (f > 0) {
        ref = frames_u8 + (long long)(f - 1) * frame_stride;
    } else {                                                                // the kept frame, when it is the frame in front of this one
        const int32_t* hd = reinterpret_cast<const int32_t*>(motion_state);
        if (hd[0] < 1 || hd[0] != state[3] || hd[1] != h || hd[2] != w) return;
        ref = motion_state + TM_HEADER;
    }
    const uint8_t* cur = frames_u8 + (long long)f * frame_stride;
    int32_t* raw = state + 4 + 2 * cap + 4 * slot;
    const int x1 = raw[0], y1 = raw[1], x2 = raw[2], y2 = raw[3];
    int dx = 0, dy = 0;
    if (!tm_search(ref, cur, x1, y1, x2, y2, radius, h, w, sh, dx, dy)) return;      // (true in wave 0 alone)
    if (lane < 4) raw[lane] = (lane == 0 ? x1 : lane == 1 ? y1 : lane == 2 ? x2 : y2) + ((lane & 1) ? dy : dx);
}

// Behind the last frame: frame nf - 1 becomes the kept frame, the header [state[3], h, w, 0]; nothing with nf <= 0.
__global__ void __launch_bounds__(256) k_motion_keep(const int32_t* state, uint8_t* motion_state, const uint8_t* frames_u8, long long frame_stride,
                                                      int frames, const int32_t* n_frames, int h, int w) {
    const int nf = min(max(*n_frames, 0), frames);
    if (nf <= 0) return;
    const uint8_t* src = frames_u8 + (long long)(nf - 1) * frame_stride;
    uint8_t* dst = motion_state + TM_HEADER;
    const size_t bytes = (size_t)3 * h * w, at = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
        const size_t quads = bytes / 16;
        for (size_t i = at; i < quads; i += step) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
        for (size_t i = quads * 16 + at; i < bytes; i += step) dst[i] = src[i];
    } else {
        for (size_t i = at; i < bytes; i += step) dst[i] = src[i];
    }
    if (at < 4) {
        int32_t* hd = reinterpret_cast<int32_t*>(motion_state);
        hd[at] = at == 0 ? state[3] : at == 1 ? h : at == 2 ? w : 0;
    }
}

void motion_search_launch(const TrackCall& c, int f, hipStream_t stream) {
    k_motion_search<<<c.capacity, TM_THREADS, 0, stream>>>(c.state, c.capacity, c.motion_state, c.frames_u8, c.frame_stride, f, c.frames, c.n_frames,
                                                           c.radius, c.h, c.w);
}

void motion_keep_launch(const TrackCall& c, hipStream_t stream) {
    const long long frame_bytes = 3LL * c.h * c.w;
    const int blocks = (int)((frame_bytes / 16 + 255) / 256 < 1024 ? (frame_bytes / 16 + 255) / 256 : 1024);
    k_motion_keep<<<blocks < 1 ? 1 : blocks, 256, 0, stream>>>(c.state, c.motion_state, c.frames_u8, c.frame_stride, c.frames, c.n_frames, c.h, c.w);
}

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_track_motion_version(void) { return FRCNN_TRACK_MOTION_VERSION; }

extern "C" size_t frcnn_track_motion_state_bytes(int h, int w) {
    if (h < 1 || h > FRCNN_REDACT_MAX_SIDE || w < 1 || w > FRCNN_REDACT_MAX_SIDE) return 0;
    return TM_HEADER + (size_t)3 * h * w;
}

extern "C" int frcnn_track_update_motion(int32_t* state, int capacity, uint8_t* motion_state, const uint8_t* frames_u8, long long frame_stride,
                                         const int32_t* det_packed, long long det_stride, int frames, const int32_t* n_frames, int max_rows,
                                         const uint8_t* tracked, int num_classes, int thr, int hold, int grow, int radius, int h, int w,
                                         int32_t* out, long long out_stride, void* stream) {
    TrackCall c{};
    c.form = TRACK_MOTION; c.state = state; c.capacity = capacity; c.motion_state = motion_state; c.frames_u8 = frames_u8;
    c.frame_stride = frame_stride; c.det_packed = det_packed; c.det_stride = det_stride; c.frames = frames; c.n_frames = n_frames;
    c.max_rows = max_rows; c.tracked = tracked; c.num_classes = num_classes; c.thr = thr; c.hold = hold; c.grow = grow; c.radius = radius;
    c.interval = 1; c.h = h; c.w = w; c.out = out; c.out_stride = out_stride;
    const int bad = track_call_check("track_update_motion", c);
    return bad ? bad : track_walk("track_update_motion", c, as_stream(stream));
}

extern "C" int frcnn_track_update_motion_weak(int32_t* state, int capacity, uint8_t* motion_state, const uint8_t* frames_u8,
                                              long long frame_stride, const int32_t* det_packed, long long det_stride, int frames,
                                              const int32_t* n_frames, int max_rows, const uint8_t* tracked, int num_classes, int thr, int hold,
                                              int grow, int radius, int h, int w, float strong, int32_t* out, long long out_stride,
                                              void* stream) {
    TrackCall c{};
    c.form = TRACK_MOTION; c.state = state; c.capacity = capacity; c.motion_state = motion_state; c.frames_u8 = frames_u8;
    c.frame_stride = frame_stride; c.det_packed = det_packed; c.det_stride = det_stride; c.frames = frames; c.n_frames = n_frames;
    c.max_rows = max_rows; c.tracked = tracked; c.num_classes = num_classes; c.thr = thr; c.hold = hold; c.grow = grow; c.radius = radius;
    c.interval = 1; c.h = h; c.w = w; c.strong = &strong; c.out = out; c.out_stride = out_stride;
    const int bad = track_call_check("track_update_motion_weak", c);
    return bad ? bad : track_walk("track_update_motion_weak", c, as_stream(stream));
}
