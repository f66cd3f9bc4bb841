// Every track ended at a hard cut (include/ext/frcnn_hip_track_cut.h states the rule, DESIGN §8 "Cut rule").  gfx950 (CDNA4) only.
// A frame's signature is 4 x 4 regions x 32 luma bins; two consecutive frames whose signatures differ by `pct` percent of the largest
// distance there is are a cut.  A call clears its workspace (k_cut_clear), builds the signatures of the kept frame and of every frame
// (k_cut_signatures: a workgroup per row band of a frame, each wave counting whole rows into a histogram of its own in LDS with integer LDS
// atomics; the workgroup's sums go out with integer global atomics, so the result does not depend on any order), decides (k_cut_decide: a
// workgroup per frame; the reference of frame 0 is read from the motion state's header here) and then hands its frames to the one walk
// every form has (csrc/track.hip's track_walk, csrc/track_call.h), which puts k_cut_apply in front of each frame's search: it frees the
// slots where cuts[f] is set, and the search, which returns behind n_slots, the tracker's kernel and the between-frame kernel are the
// interval form's, unchanged.
#include "common.h"
#include "../../include/ext/frcnn_hip_redact.h"
#include "../../include/ext/frcnn_hip_track.h"
#include "../../include/ext/frcnn_hip_track_cut.h"
#include "../../include/ext/frcnn_hip_track_interval.h"
#include "../../include/ext/frcnn_hip_track_weak.h"
#include "track_call.h"

namespace frcnn {

constexpr int TC_REGIONS = FRCNN_TRACK_CUT_REGIONS, TC_BINS = FRCNN_TRACK_CUT_BINS;
constexpr int TC_WORDS = TC_REGIONS * TC_REGIONS * TC_BINS;                 // counters of a signature: 512
constexpr int TC_THREADS = 256, TC_WAVES = TC_THREADS / 64;
constexpr int TC_BANDS = 64;                                                // row bands of a frame, at most
constexpr int TC_HEADER = 16;                                               // bytes in front of the motion state's kept frame
static_assert(TC_REGIONS == 4 && TC_BINS == 32 && TC_WORDS % TC_THREADS == 0, "the region of a pixel is three comparisons");

// Has frame 0 of the call the kept frame for its reference (frcnn_hip_track_motion.h REFERENCE)?  state[3] is the word as the call found it:
// every launch that reads this runs in front of the call's first tracker launch.
__device__ inline bool tc_kept_is_reference(const int32_t* state, const uint8_t* motion_state, int h, int w) {
    const int32_t* hd = reinterpret_cast<const int32_t*>(motion_state);
    return hd[0] >= 1 && hd[0] == state[3] && hd[1] == h && hd[2] == w;
}

__global__ void __launch_bounds__(TC_THREADS) k_cut_clear(int32_t* workspace, int words) {
    for (int i = blockIdx.x * TC_THREADS + threadIdx.x; i < words; i += gridDim.x * TC_THREADS) workspace[i] = 0;
}

// Signature blockIdx.y (0: the kept frame; f + 1: frame f of the call), rows [blockIdx.x * band, ... + band) of it.
__global__ void __launch_bounds__(TC_THREADS) k_cut_signatures(const int32_t* state, const uint8_t* motion_state, const uint8_t* frames_u8,
                                                                 long long frame_stride, int frames, const int32_t* n_frames, int h, int w,
                                                                 int band, int32_t* workspace) {
    __shared__ int s_hist[TC_WAVES][TC_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sig = blockIdx.y;
    const uint8_t* src;
    if (sig == 0) {
        if (!tc_kept_is_reference(state, motion_state, h, w)) return;       // (the whole workgroup)
        src = motion_state + TC_HEADER;
    } else {
        if (sig - 1 >= min(max(*n_frames, 0), frames)) return;              // padding
        src = frames_u8 + (long long)(sig - 1) * frame_stride;
    }
    const int y0 = blockIdx.x * band, y1 = min(y0 + band, h);
    if (y0 >= h) return;
    for (int i = tid; i < TC_WAVES * TC_WORDS; i += TC_THREADS) (&s_hist[0][0])[i] = 0;
    __syncthreads();
    // (4 x) / w >= k  <=>  x >= ceil(k w / 4)
    const int xb1 = (w + 3) / 4, xb2 = (2 * w + 3) / 4, xb3 = (3 * w + 3) / 4;
    const int yb1 = (h + 3) / 4, yb2 = (2 * h + 3) / 4, yb3 = (3 * h + 3) / 4;
    int* hist = s_hist[wave];
    for (int y = y0 + wave; y < y1; y += TC_WAVES) {
        const int ry = (y >= yb1) + (y >= yb2) + (y >= yb3);
        const uint8_t* row = src + (size_t)3 * y * w;
        for (int x = lane; x < w; x += 64) {
            const int rx = (x >= xb1) + (x >= xb2) + (x >= xb3);
            const int luma = (row[3 * x] + 2 * row[3 * x + 1] + row[3 * x + 2] + 2) >> 2;
            atomicAdd(&hist[(ry * TC_REGIONS + rx) * TC_BINS + (luma >> 3)], 1);
        }
    }
    __syncthreads();
    int32_t* out = workspace + (size_t)sig * TC_WORDS;
    for (int c = tid; c < TC_WORDS; c += TC_THREADS) {
        int v = 0;
        for (int k = 0; k < TC_WAVES; ++k) v += s_hist[k][c];
        if (v) atomicAdd(&out[c], v);
    }
}

// cuts[blockIdx.x]: frame f against its reference.
__global__ void __launch_bounds__(TC_THREADS) k_cut_decide(const int32_t* state, const uint8_t* motion_state, int frames, const int32_t* n_frames,
                                                             int h, int w, int pct, const int32_t* workspace, int32_t* cuts) {
    __shared__ unsigned long long s_sum[TC_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, f = blockIdx.x;
    const bool real = f < min(max(*n_frames, 0), frames) && (f > 0 || tc_kept_is_reference(state, motion_state, h, w));
    unsigned long long d = 0;
    if (real) {                                                             // (uniform in the workgroup)
        const int32_t *ref = workspace + (size_t)f * TC_WORDS, *cur = ref + TC_WORDS;
        for (int c = tid; c < TC_WORDS; c += TC_THREADS) d += (unsigned long long)abs(cur[c] - ref[c]);
    }
    for (int off = 32; off > 0; off >>= 1) d += __shfl_down(d, off, 64);
    if (lane == 0) s_sum[wave] = d;
    __syncthreads();
    if (tid == 0) {
        long long D = 0;
        for (int k = 0; k < TC_WAVES; ++k) D += (long long)s_sum[k];
        cuts[f] = real && D * 100 >= (long long)pct * 2 * h * w ? 1 : 0;
    }
}

// Step C of frame ``f``: on a cut every slot is freed.
__global__ void __launch_bounds__(TC_THREADS) k_cut_apply(int32_t* state, int cap, const int32_t* cuts, int f) {
    if (!cuts[f]) return;
    if (threadIdx.x == 0) state[0] = 0;
    for (int i = threadIdx.x; i < 8 * cap; i += TC_THREADS) state[4 + i] = 0;
}

void cut_apply_launch(const TrackCall& c, int f, hipStream_t stream) {
    k_cut_apply<<<1, TC_THREADS, 0, stream>>>(c.state, c.capacity, c.cuts, f);
}

// In front of the walk: cuts[f] of every frame of the call, through the workspace
static void cut_decide_launch(const TrackCall& c, hipStream_t st) {
    const int words = (c.frames + 1) * TC_WORDS;
    k_cut_clear<<<(words + TC_THREADS - 1) / TC_THREADS, TC_THREADS, 0, st>>>(c.workspace, words);
    const int band = (c.h + TC_BANDS - 1) / TC_BANDS, bands = (c.h + band - 1) / band;
    k_cut_signatures<<<dim3(bands, c.frames + 1), TC_THREADS, 0, st>>>(c.state, c.motion_state, c.frames_u8, c.frame_stride, c.frames, c.n_frames,
                                                                       c.h, c.w, band, c.workspace);
    k_cut_decide<<<c.frames, TC_THREADS, 0, st>>>(c.state, c.motion_state, c.frames, c.n_frames, c.h, c.w, c.pct, c.workspace, c.cuts);
}

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_track_cut_version(void) { return FRCNN_TRACK_CUT_VERSION; }

extern "C" size_t frcnn_track_cut_workspace_bytes(int frames) {
    if (frames < 1 || frames > FRCNN_TRACK_MAX_FRAMES) return 0;
    return (size_t)(frames + 1) * TC_WORDS * sizeof(int32_t);
}

extern "C" int frcnn_track_update_cut(int32_t* state, int capacity, uint8_t* motion_state, const uint8_t* frames_u8, long long frame_stride,
                                      const int32_t* det_packed, long long det_stride, int frames, const int32_t* n_frames, int max_rows,
                                      const uint8_t* tracked, int num_classes, int thr, int hold, int grow, int radius, int interval, int h, int w,
                                      int32_t* out, long long out_stride, int pct, int32_t* workspace, int32_t* cuts, void* stream) {
    TrackCall c{};
    c.form = TRACK_CUT; c.state = state; c.capacity = capacity; c.motion_state = motion_state; c.frames_u8 = frames_u8;
    c.frame_stride = frame_stride; c.det_packed = det_packed; c.det_stride = det_stride; c.frames = frames; c.n_frames = n_frames;
    c.max_rows = max_rows; c.tracked = tracked; c.num_classes = num_classes; c.thr = thr; c.hold = hold; c.grow = grow; c.radius = radius;
    c.interval = interval; c.h = h; c.w = w; c.out = out; c.out_stride = out_stride; c.pct = pct; c.workspace = workspace; c.cuts = cuts;
    const int bad = track_call_check("track_update_cut", c);
    if (bad) return bad;
    cut_decide_launch(c, as_stream(stream));
    return track_walk("track_update_cut", c, as_stream(stream));
}

extern "C" int frcnn_track_update_cut_weak(int32_t* state, int capacity, uint8_t* motion_state, const uint8_t* frames_u8, long long frame_stride,
                                           const int32_t* det_packed, long long det_stride, int frames, const int32_t* n_frames, int max_rows,
                                           const uint8_t* tracked, int num_classes, int thr, int hold, int grow, int radius, int interval, int h,
                                           int w, float strong, int32_t* out, long long out_stride, int pct, int32_t* workspace, int32_t* cuts,
                                           void* stream) {
    TrackCall c{};
    c.form = TRACK_CUT; c.state = state; c.capacity = capacity; c.motion_state = motion_state; c.frames_u8 = frames_u8;
    c.frame_stride = frame_stride; c.det_packed = det_packed; c.det_stride = det_stride; c.frames = frames; c.n_frames = n_frames;
    c.max_rows = max_rows; c.tracked = tracked; c.num_classes = num_classes; c.thr = thr; c.hold = hold; c.grow = grow; c.radius = radius;
    c.interval = interval; c.h = h; c.w = w; c.strong = &strong; c.out = out; c.out_stride = out_stride; c.pct = pct; c.workspace = workspace;
    c.cuts = cuts;
    const int bad = track_call_check("track_update_cut_weak", c);
    if (bad) return bad;
    cut_decide_launch(c, as_stream(stream));
    return track_walk("track_update_cut_weak", c, as_stream(stream));
}
