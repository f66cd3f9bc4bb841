// The tracker's slots moved with the pixels under them (include/ext/frcnn_hip_track_motion.h states the rule, DESIGN §8 "Motion rule"): an
// integer block match per live slot between two frames, in front of csrc/track.hip's steps 1-4.  gfx950 (CDNA4) only.
// A call walks its frames one by one -- the search of frame f + 1 needs the boxes after frame f --: k_motion_search (one workgroup per
// slot of the state; one past n_slots, read on the device, returns at once) and then track.hip's kernel on that frame; k_motion_keep
// closes the call.  A search workgroup stages the slot's <= 1024 template lumas once; a wave takes a candidate at a time, its lanes the
// samples (16 each, in registers), and reads the current frame where it lies: the window of a strided grid does not tile into LDS, and a
// whole search is <= 1.1 M pixel reads that L2 serves.  A candidate's cost is a shuffle sum; a wave keeps the minimum of ONE packed key
// per candidate, cost << 22 | norm << 12 | dy + 16 << 6 | dx + 16 (18 + 10 + 6 + 6 bits): a uint64 minimum IS the lexicographic rule.  The
// waves' keys meet in LDS and wave 0 shuffles them down.  One writer per slot word; no atomics.
#include "common.h"
#include "../../include/ext/frcnn_hip_redact.h"
#include "../../include/ext/frcnn_hip_track.h"
#include "../../include/ext/frcnn_hip_track_motion.h"
#include "track.h"

namespace frcnn {

constexpr int TM_THREADS = 1024;
constexpr int TM_WAVES = TM_THREADS / 64;
constexpr int TM_GRID = FRCNN_TRACK_MOTION_GRID;
constexpr int TM_PER_LANE = TM_GRID * TM_GRID / 64;                         // samples of a lane
constexpr int TM_HEADER = 16;                                               // bytes in front of the kept frame
static_assert(TM_GRID * TM_GRID <= TM_THREADS, "a thread stages one template luma");
static_assert(TM_WAVES <= 64, "wave 0 reduces the waves' keys");

__device__ __forceinline__ int luma(const uint8_t* p) { return ((int)p[0] + 2 * (int)p[1] + (int)p[2] + 2) >> 2; }

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int off) {
    const unsigned lo = __shfl_xor((unsigned)v, off), hi = __shfl_xor((unsigned)(v >> 32), off);
    return ((unsigned long long)hi << 32) | lo;
}

// Step 0 for frame ``f`` of the call, slot blockIdx.x.
__global__ void __launch_bounds__(TM_THREADS) k_motion_search(int32_t* state, int cap, const uint8_t* motion_state, const uint8_t* frames_u8,
                                                                long long frame_stride, int f, int frames, const int32_t* n_frames,
                                                                int radius, int h, int w) {
    __shared__ uint8_t s_t[TM_GRID * TM_GRID];
    __shared__ unsigned long long s_key[TM_WAVES];
    __shared__ int s_zero;
    const int slot = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
    const int xa = max(min(x1, x2), 0), xb = min(max(x1, x2), w - 1), ya = max(min(y1, y2), 0), yb = min(max(y1, y2), h - 1);
    if (xa > xb || ya > yb) return;
    const int sx = (xb - xa + 1 + TM_GRID - 1) / TM_GRID, sy = (yb - ya + 1 + TM_GRID - 1) / TM_GRID;
    const int x0 = xa + sx / 2, y0 = ya + sy / 2;                           // (sx / 2 < the box's width: the first sample is inside)
    const int cols = (xb - x0) / sx + 1, rows = (yb - y0) / sy + 1, n = cols * rows;
    if (n < FRCNN_TRACK_MOTION_MIN_SAMPLES) return;                         // (the whole workgroup, as every return above)
    if (tid < n) {
        const int x = x0 + (tid % cols) * sx, y = y0 + (tid / cols) * sy;
        s_t[tid] = (uint8_t)luma(ref + ((size_t)y * w + x) * 3);
    }
    __syncthreads();
    // ---- this lane's samples lane, lane + 64, ...: place and template luma
    int px[TM_PER_LANE], py[TM_PER_LANE], pt[TM_PER_LANE];
#pragma unroll
    for (int k = 0; k < TM_PER_LANE; ++k) {
        const int i = lane + 64 * k;
        const bool some = i < n;
        px[k] = some ? x0 + (i % cols) * sx : -1;
        py[k] = some ? y0 + (i / cols) * sy : 0;
        pt[k] = some ? s_t[i] : 0;
    }
    const int side = 2 * radius + 1, cands = side * side;
    unsigned long long best = ~0ull;
    for (int c = wave; c < cands; c += TM_WAVES) {                          // (wave-uniform: the shuffles below see all 64 lanes)
        const int dy = c / side - radius, dx = c % side - radius;
        int cost = 0;
#pragma unroll
        for (int k = 0; k < TM_PER_LANE; ++k) {
            if (px[k] < 0) continue;
            const int xx = min(max(px[k] + dx, 0), w - 1), yy = min(max(py[k] + dy, 0), h - 1);
            cost += abs(luma(cur + ((size_t)yy * w + xx) * 3) - pt[k]);
        }
        for (int off = 32; off > 0; off >>= 1) cost += __shfl_xor(cost, off);
        const unsigned long long key = ((unsigned long long)cost << 22) | ((unsigned long long)(dx * dx + dy * dy) << 12) |
                                       ((unsigned long long)(dy + 16) << 6) | (unsigned long long)(dx + 16);
        best = key < best ? key : best;
        if (dx == 0 && dy == 0 && lane == 0) s_zero = cost;
    }
    if (lane == 0) s_key[wave] = best;
    __syncthreads();
    if (wave != 0) return;
    best = lane < TM_WAVES ? s_key[lane] : ~0ull;
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = shfl_xor_u64(best, off);
        best = o < best ? o : best;
    }
    const int cost = (int)(best >> 22), dy = (int)((best >> 6) & 63) - 16, dx = (int)(best & 63) - 16;
    if (cost + n > s_zero) return;                                          // the gate: a flat or unchanged region does not move
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
    const char* who = "track_update_motion";
    const int bad = track_check(who, state, capacity, det_packed, det_stride, frames, n_frames, max_rows, tracked, num_classes, thr, hold, grow,
                                h, w, out, out_stride);
    if (bad) return bad;
    if (!motion_state || !frames_u8) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (reinterpret_cast<uintptr_t>(motion_state) & 3) return fail(FRCNN_E_ARG, "%s: motion_state is not 4-byte aligned", who);
    if (radius < FRCNN_TRACK_MOTION_MIN_RADIUS || radius > FRCNN_TRACK_MOTION_MAX_RADIUS)
        return fail(FRCNN_E_ARG, "%s: radius=%d not in [%d, %d]", who, radius, FRCNN_TRACK_MOTION_MIN_RADIUS, FRCNN_TRACK_MOTION_MAX_RADIUS);
    const long long frame_bytes = 3LL * h * w;
    if (frames > 1 && frame_stride < frame_bytes)
        return fail(FRCNN_E_ARG, "%s: frame_stride=%lld bytes, a %dx%d frame has %lld", who, frame_stride, h, w, frame_bytes);
    hipStream_t st = as_stream(stream);
    for (int f = 0; f < frames; ++f) {
        k_motion_search<<<capacity, TM_THREADS, 0, st>>>(state, capacity, motion_state, frames_u8, frame_stride, f, frames, n_frames, radius, h, w);
        track_launch(state, capacity, det_packed, det_stride, f, 1, frames, n_frames, max_rows, tracked, num_classes, thr, hold, grow, h, w, out,
                     out_stride, st);
    }
    const int blocks = (int)((frame_bytes / 16 + 255) / 256 < 1024 ? (frame_bytes / 16 + 255) / 256 : 1024);
    k_motion_keep<<<blocks < 1 ? 1 : blocks, 256, 0, st>>>(state, motion_state, frames_u8, frame_stride, frames, n_frames, h, w);
    return check_launch(who);
}
