// The detector on every K-th frame of a call, the block match alone in between (include/ext/frcnn_hip_track_interval.h states the rule,
// DESIGN §8 "Interval rule").  gfx950 (CDNA4) only.  csrc/track.hip's track_walk (csrc/track_call.h) walks a call's frames one by one:
// csrc/track_motion.hip's search, then on a key frame track.hip's kernel with that key frame's detections, on a between frame
// k_interval_between, defined here, which writes the frame's tracked buffer from the slots as the search left them and counts the frame;
// track_motion.hip's keep kernel closes the call.  The motion form is this one with interval 1: no frame is a between frame.  k_interval_between
// is one workgroup with a thread per slot: a row's place is a prefix count of the slots in front of it (a ballot per wave, the waves'
// counts through LDS), so places do not depend on which thread runs when.  One writer per word; no atomics.
#include "common.h"
#include "../../include/ext/frcnn_hip_redact.h"
#include "../../include/ext/frcnn_hip_track.h"
#include "../../include/ext/frcnn_hip_track_interval.h"
#include "../../include/ext/frcnn_hip_track_weak.h"
#include "track_call.h"

namespace frcnn {

constexpr int TI_THREADS = FRCNN_TRACK_MAX;                                 // a thread per slot
constexpr int TI_WAVES = TI_THREADS / 64;
static_assert(TI_THREADS % 64 == 0, "whole waves");

// Frame ``f`` of a call of ``total`` frames, a between frame (or padding): ``o`` is that frame's tracked buffer.
__global__ void __launch_bounds__(TI_THREADS) k_interval_between(int32_t* state, int cap, int f, int total, const int32_t* n_frames, int max_rows,
                                                                   int grow, int h, int w, int32_t* o) {
    __shared__ int s_live[TI_WAVES], s_held[TI_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = max_rows + cap;
    int32_t *o_box = o + 4, *o_cls = o + 4 + 4 * R, *o_prob = o + 4 + 5 * R, *o_id = o + 4 + 6 * R, *o_age = o + 4 + 7 * R;
    int rows = 0;                                                           // rows written in front of the dead ones
    if (f < min(max(*n_frames, 0), total)) {
        const int n_slots = min(max(state[0], 0), cap);
        const bool some = tid < n_slots;
        const int age = some ? state[4 + 7 * cap + tid] : 0;
        const bool live = some && age == 0, held = some && age >= 1;
        const unsigned long long m_live = __ballot(live), m_held = __ballot(held), below = (1ull << lane) - 1;
        if (lane == 0) { s_live[wave] = __popcll(m_live); s_held[wave] = __popcll(m_held); }
        __syncthreads();
        int n_live = 0, n_held = 0, at_live = __popcll(m_live & below), at_held = __popcll(m_held & below);
        for (int k = 0; k < TI_WAVES; ++k) {
            n_live += s_live[k]; n_held += s_held[k];
            at_live += k < wave ? s_live[k] : 0;
            at_held += k < wave ? s_held[k] : 0;
        }
        rows = n_live + n_held;                                             // (<= cap <= R)
        if (some) {
            const int32_t* raw = state + 4 + 2 * cap + 4 * tid;
            const int x1 = raw[0], y1 = raw[1], x2 = raw[2], y2 = raw[3];
            const int r = live ? at_live : n_live + at_held;
            if (live) {
                o_box[4 * r] = x1; o_box[4 * r + 1] = y1; o_box[4 * r + 2] = x2; o_box[4 * r + 3] = y2;
            } else {                                                        // step 4's held row: the clipped box, grown
                const int g = grow * age;
                o_box[4 * r] = max(min(x1, x2), 0) - g; o_box[4 * r + 1] = max(min(y1, y2), 0) - g;
                o_box[4 * r + 2] = min(max(x1, x2), w - 1) + g; o_box[4 * r + 3] = min(max(y1, y2), h - 1) + g;
            }
            o_cls[r] = state[4 + cap + tid]; o_prob[r] = state[4 + 6 * cap + tid]; o_id[r] = state[4 + tid]; o_age[r] = age;
        }
        if (tid == 0) {
            o[0] = rows; o[1] = n_live; o[2] = state[1] + 1; o[3] = state[2];
            state[3] += 1;                                                  // the frame counts (this thread alone reads and writes the word)
        }
    } else if (tid == 0) {                                                  // a short pass's padding: no frame at all
        o[0] = 0; o[1] = 0; o[2] = state[1] + 1; o[3] = state[2];
    }
    for (int r = rows + tid; r < R; r += TI_THREADS) {
        for (int c = 0; c < 4; ++c) o_box[4 * r + c] = -1;
        o_cls[r] = -1; o_prob[r] = 0; o_id[r] = 0; o_age[r] = 0;
    }
}

void interval_between_launch(const TrackCall& c, int f, int32_t* out, hipStream_t stream) {
    k_interval_between<<<1, TI_THREADS, 0, stream>>>(c.state, c.capacity, f, c.frames, c.n_frames, c.max_rows, c.grow, c.h, c.w, out);
}

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_track_interval_version(void) { return FRCNN_TRACK_INTERVAL_VERSION; }

extern "C" int frcnn_track_update_interval(int32_t* state, int capacity, uint8_t* motion_state, const uint8_t* frames_u8, long long frame_stride,
                                           const int32_t* det_packed, long long det_stride, int frames, const int32_t* n_frames, int max_rows,
                                           const uint8_t* tracked, int num_classes, int thr, int hold, int grow, int radius, int interval, int h,
                                           int w, int32_t* out, long long out_stride, void* stream) {
    TrackCall c{};
    c.form = TRACK_MOTION; c.state = state; c.capacity = capacity; c.motion_state = motion_state; c.frames_u8 = frames_u8;
    c.frame_stride = frame_stride; c.det_packed = det_packed; c.det_stride = det_stride; c.frames = frames; c.n_frames = n_frames;
    c.max_rows = max_rows; c.tracked = tracked; c.num_classes = num_classes; c.thr = thr; c.hold = hold; c.grow = grow; c.radius = radius;
    c.interval = interval; c.h = h; c.w = w; c.out = out; c.out_stride = out_stride;
    const int bad = track_call_check("track_update_interval", c);
    return bad ? bad : track_walk("track_update_interval", c, as_stream(stream));
}

extern "C" int frcnn_track_update_interval_weak(int32_t* state, int capacity, uint8_t* motion_state, const uint8_t* frames_u8,
                                                long long frame_stride, const int32_t* det_packed, long long det_stride, int frames,
                                                const int32_t* n_frames, int max_rows, const uint8_t* tracked, int num_classes, int thr,
                                                int hold, int grow, int radius, int interval, int h, int w, float strong, int32_t* out,
                                                long long out_stride, void* stream) {
    TrackCall c{};
    c.form = TRACK_MOTION; c.state = state; c.capacity = capacity; c.motion_state = motion_state; c.frames_u8 = frames_u8;
    c.frame_stride = frame_stride; c.det_packed = det_packed; c.det_stride = det_stride; c.frames = frames; c.n_frames = n_frames;
    c.max_rows = max_rows; c.tracked = tracked; c.num_classes = num_classes; c.thr = thr; c.hold = hold; c.grow = grow; c.radius = radius;
    c.interval = interval; c.h = h; c.w = w; c.strong = &strong; c.out = out; c.out_stride = out_stride;
    const int bad = track_call_check("track_update_interval_weak", c);
    return bad ? bad : track_walk("track_update_interval_weak", c, as_stream(stream));
}
