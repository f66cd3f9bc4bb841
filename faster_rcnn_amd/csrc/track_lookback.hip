// New tracks hidden in the frames before their first detection (include/ext/frcnn_hip_track_lookback.h states the rule, DESIGN §8
// "Look-back rule"): a window of tracked, not yet emitted frames on the device, and from every birth a block match BACKWARDS through it.
// gfx950 (CDNA4) only.  Five launches per call, all guarded by device words (*n_frames, the window's count), so a captured call replays:
//   k_lb_join    the call's frames and their tracked buffers, widened to R2 rows, into the cells of the window's other half;
//   k_lb_chain   one workgroup per (birth, frame of the call): it finds its birth row, then walks its L steps itself -- step k needs step
//                k - 1's box -- each a search of csrc/track_motion_search.h (shared with csrc/track_motion.hip), and writes one row a step.
//                A row's place is the frame's n_rows as it was + the births of the call's frames in between + the birth's rank: every
//                workgroup counts those for itself, so nothing is handed from one workgroup to another;
//   k_lb_counts  one workgroup: every frame's n_rows moved behind its new rows, the dropped rows summed into back_overflow;
//   k_lb_emit    the window's older frames copied out;
//   k_lb_close   the header: the halves change places (no overlapping shift), or the window empties on a flush.
// One writer per word; no atomics.  The chain writes rows at and behind a frame's n_rows only and reads rows in front of n_live only.
// The geometry, the cells, the argument checks and the launches of join, emit and close are shared with csrc/track_backtrack.hip through
// csrc/track_lookback.h.
#include "track_lookback.h"
#include "track_motion_search.h"

namespace frcnn {

static_assert(LB_MAX_ROWS <= TM_THREADS, "a thread of the chain's workgroup looks at one live row");
static_assert(2 * FRCNN_TRACK_MAX_FRAMES <= TM_THREADS, "a thread of k_lb_counts takes one frame of the sequence");

__device__ __forceinline__ void lb_copy(uint8_t* dst, const uint8_t* src, size_t bytes, size_t at, size_t step) {
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
        const size_t quads = bytes / 16;
        for (size_t i = at; i < quads; i += step) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
        for (size_t i = quads * 16 + at; i < bytes; i += step) dst[i] = src[i];
    } else {
        for (size_t i = at; i < bytes; i += step) dst[i] = src[i];
    }
}

// is row ``row`` of sequence frame ``t`` >= 1 a birth: a live row whose id the frame in front had not yet issued?
__device__ __forceinline__ bool lb_is_birth(uint8_t* window, const LbGeom& g, int c, int half, int t, int row) {
    const int32_t* bt = reinterpret_cast<const int32_t*>(lb_cell(window, g, c, half, t));
    const int32_t* bp = reinterpret_cast<const int32_t*>(lb_cell(window, g, c, half, t - 1));
    return row < clampi(bt[1], 0, g.R2) && bt[4 + 6 * g.R2 + row] >= bp[2];
}

// grid (blocks, frames): frame blockIdx.y of the call joins the window's other half
__global__ void __launch_bounds__(256) k_lb_join(uint8_t* window, LbGeom g, const uint8_t* frames_u8, long long frame_stride, const int32_t* tracked,
                                                  long long tracked_stride, const int32_t* n_frames) {
    const int f = blockIdx.y;
    if (f >= clampi(*n_frames, 0, g.frames)) return;
    const int32_t* hd = reinterpret_cast<const int32_t*>(window);
    const int c = clampi(hd[0], 0, g.frames), half = hd[1] & 1;
    uint8_t* cell = lb_cell(window, g, c, half, c + f);
    const size_t at = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
    int32_t* dst = reinterpret_cast<int32_t*>(cell);
    const int32_t* src = tracked + (long long)f * tracked_stride;
    const int R = g.R, R2 = g.R2;
    for (size_t i = at; i < (size_t)(4 + 8 * R2); i += step) {
        int32_t v;
        if (i < 4) {
            v = src[i];
        } else if (i < (size_t)(4 + 4 * R2)) {
            const int r = (int)(i - 4) >> 2;
            v = r < R ? src[i] : -1;
        } else {                                        // cls, prob, id, age: one word a row
            const int part = (int)(i - 4 - 4 * R2) / R2, r = (int)(i - 4 - 4 * R2) % R2;
            v = r < R ? src[4 + (4 + part) * R + r] : (part == 0 ? -1 : 0);
        }
        dst[i] = v;
    }
    lb_copy(cell + g.tracked_bytes, frames_u8 + (long long)f * frame_stride, (size_t)3 * g.h * g.w, at, step);
}

// grid (capacity, frames): birth blockIdx.x of the call's frame blockIdx.y, chained back over at most ``L`` frames
__global__ void __launch_bounds__(TM_THREADS) k_lb_chain(uint8_t* window, LbGeom g, const int32_t* n_frames, int L, int radius, int grow) {
    __shared__ TmShared sh;
    __shared__ uint8_t s_flag[LB_MAX_ROWS];
    __shared__ int s_row, s_mv[2];
    const int j = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    if (f >= clampi(*n_frames, 0, g.frames)) return;
    const int32_t* hd = reinterpret_cast<const int32_t*>(window);
    const int c = clampi(hd[0], 0, g.frames), half = hd[1] & 1, t = c + f, R2 = g.R2;
    if (t == 0) return;                                                     // no frame in front of it: nothing to fill into
    const bool mine = tid < LB_MAX_ROWS && lb_is_birth(window, g, c, half, t, tid);
    if (tid < LB_MAX_ROWS) s_flag[tid] = mine;
    const int births = min(__syncthreads_count(mine), g.cap);
    if (j >= births) return;                                                // (the whole workgroup)
    if (mine) {
        int rank = 0;
        for (int r = 0; r < tid; ++r) rank += s_flag[r];
        if (rank == j) s_row = tid;
    }
    __syncthreads();
    const int row = s_row;
    const int32_t* bt = reinterpret_cast<const int32_t*>(lb_cell(window, g, c, half, t));
    int x1 = bt[4 + 4 * row], y1 = bt[4 + 4 * row + 1], x2 = bt[4 + 4 * row + 2], y2 = bt[4 + 4 * row + 3];
    const int cls = bt[4 + 4 * R2 + row], prob = bt[4 + 5 * R2 + row], id = bt[4 + 6 * R2 + row];
    int between = 0;                                                        // births of the frames between g and t: their rows lie in front
    for (int k = 1; k <= L; ++k) {
        const int gi = t - k;
        if (gi < 0) break;
        if (k >= 2 && gi + 1 >= c)                                          // (a window frame has no births of this call)
            between += min(__syncthreads_count(tid < LB_MAX_ROWS && lb_is_birth(window, g, c, half, gi + 1, tid)), g.cap);
        uint8_t* cell = lb_cell(window, g, c, half, gi);
        int dx = 0, dy = 0;
        const bool took = radius > 0 && tm_search(lb_cell(window, g, c, half, gi + 1) + g.tracked_bytes, cell + g.tracked_bytes, x1, y1, x2, y2,
                                                  radius, g.h, g.w, sh, dx, dy);
        if (tid == 0) {                                                     // (wave 0 holds the result)
            s_mv[0] = took ? dx : 0;
            s_mv[1] = took ? dy : 0;
        }
        __syncthreads();
        x1 += s_mv[0], x2 += s_mv[0], y1 += s_mv[1], y2 += s_mv[1];
        int32_t* bg = reinterpret_cast<int32_t*>(cell);
        const int place = clampi(bg[0], 0, R2) + between + j;
        if (place < R2 && tid < 8) {
            const int xa = max(min(x1, x2), 0), xb = min(max(x1, x2), g.w - 1), ya = max(min(y1, y2), 0), yb = min(max(y1, y2), g.h - 1);
            const bool none = xa > xb || ya > yb;
            const int e = grow * k;
            if (tid < 4) bg[4 + 4 * place + tid] = none ? -1 : tid == 0 ? xa - e : tid == 1 ? ya - e : tid == 2 ? xb + e : yb + e;
            else bg[4 + (tid) * R2 + place] = tid == 4 ? cls : tid == 5 ? prob : tid == 6 ? id : -k;
        }
        __syncthreads();                                                    // s_mv and sh are written again
    }
}

// one workgroup: n_rows of every frame of the sequence behind its new rows; what did not fit is counted
__global__ void __launch_bounds__(TM_THREADS) k_lb_counts(uint8_t* window, LbGeom g, const int32_t* n_frames, int L) {
    __shared__ int s_births[FRCNN_TRACK_MAX_FRAMES], s_drop[2 * FRCNN_TRACK_MAX_FRAMES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nf = clampi(*n_frames, 0, g.frames);
    if (nf <= 0) return;
    int32_t* hd = reinterpret_cast<int32_t*>(window);
    const int c = clampi(hd[0], 0, g.frames), half = hd[1] & 1, total = c + nf;
    for (int f = wave; f < nf; f += TM_WAVES) {
        int n = 0;
        if (c + f >= 1)
            for (int r = lane; r < LB_MAX_ROWS; r += 64) n += lb_is_birth(window, g, c, half, c + f, r);
        for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
        if (lane == 0) s_births[f] = min(n, g.cap);
    }
    __syncthreads();
    if (tid < 2 * FRCNN_TRACK_MAX_FRAMES) {
        int drop = 0;
        if (tid < total) {
            int added = 0;
            for (int t = max(tid + 1, c); t <= min(tid + L, total - 1); ++t) added += s_births[t - c];
            int32_t* b = reinterpret_cast<int32_t*>(lb_cell(window, g, c, half, tid));
            const int rows = clampi(b[0], 0, g.R2) + added;
            drop = max(rows - g.R2, 0);
            if (added) b[0] = rows - drop;
        }
        s_drop[tid] = drop;
    }
    __syncthreads();
    if (tid == 0) {
        int sum = 0;
        for (int s = 0; s < total; ++s) sum += s_drop[s];
        if (sum) hd[2] += sum;
    }
}

// grid (blocks, frames): window frame blockIdx.y copied out; behind the window's count the four count words of the buffer are zeroed
__global__ void __launch_bounds__(256) k_lb_emit(uint8_t* window, LbGeom g, uint8_t* out_frames, long long out_frame_stride, int32_t* out_tracked,
                                                  long long out_tracked_stride, int32_t* out_count) {
    const int e = blockIdx.y;
    const int32_t* hd = reinterpret_cast<const int32_t*>(window);
    const int c = clampi(hd[0], 0, g.frames), half = hd[1] & 1;
    const size_t at = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
    if (e == 0 && at == 0) *out_count = c;
    int32_t* ot = out_tracked + (long long)e * out_tracked_stride;
    if (e >= c) {
        if (at < 4) ot[at] = 0;
        return;
    }
    const uint8_t* cell = lb_cell(window, g, c, half, e);
    const int32_t* src = reinterpret_cast<const int32_t*>(cell);
    for (size_t i = at; i < (size_t)(4 + 8 * g.R2); i += step) ot[i] = src[i];
    lb_copy(out_frames + (long long)e * out_frame_stride, cell + g.tracked_bytes, (size_t)3 * g.h * g.w, at, step);
}

__global__ void k_lb_close(uint8_t* window, int frames, const int32_t* n_frames) {
    if (threadIdx.x != 0) return;
    int32_t* hd = reinterpret_cast<int32_t*>(window);
    const int raw = *n_frames;
    if (raw == 0) return;
    if (raw < 0) {
        hd[0] = 0;
    } else {
        hd[0] = min(raw, frames);
        hd[1] = (hd[1] & 1) ^ 1;
    }
}

// the geometry of a window, or false for an argument out of range (``why`` says which)
bool lb_geom(int frames, int h, int w, int max_rows, int capacity, int back, LbGeom& g, const char*& why) {
    why = nullptr;
    if (frames < 1 || frames > FRCNN_TRACK_MAX_FRAMES) why = "frames";
    else if (h < 1 || h > FRCNN_REDACT_MAX_SIDE || w < 1 || w > FRCNN_REDACT_MAX_SIDE) why = "frame side";
    else if (max_rows < 1 || max_rows > FRCNN_REDACT_MAX_ROWS) why = "max_rows";
    else if (capacity < 1 || capacity > FRCNN_TRACK_MAX) why = "capacity";
    else if (back < 1 || back > FRCNN_TRACK_LOOKBACK_MAX_BACK) why = "back";
    else if (max_rows + capacity + back > FRCNN_REDACT_MAX_ROWS) why = "max_rows + capacity + back";
    if (why) return false;
    g.frames = frames, g.R = max_rows + capacity, g.R2 = g.R + back, g.cap = capacity, g.h = h, g.w = w;
    g.tracked_bytes = 4LL * (4 + 8 * g.R2);
    g.cell = g.tracked_bytes + (3LL * h * w + 15) / 16 * 16;
    return true;
}

int lookback_check(const char* who, const uint8_t* window, const uint8_t* frames_u8, long long frame_stride, const int32_t* tracked,
                   long long tracked_stride, int frames, const int32_t* n_frames, int max_rows, int capacity, int back, int lookback, int radius,
                   int grow, int h, int w, const uint8_t* out_frames, long long out_frame_stride, const int32_t* out_tracked,
                   long long out_tracked_stride, const int32_t* out_count, LbGeom& g) {
    if (!window || !frames_u8 || !tracked || !n_frames || !out_frames || !out_tracked || !out_count) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (reinterpret_cast<uintptr_t>(window) & 15) return fail(FRCNN_E_ARG, "%s: window is not 16-byte aligned", who);
    const char* why;
    if (!lb_geom(frames, h, w, max_rows, capacity, back, g, why))
        return fail(FRCNN_E_ARG, "%s: %s out of range (frames=%d, %dx%d, max_rows=%d, capacity=%d, back=%d; at most %d rows in all)", who, why, frames,
                    h, w, max_rows, capacity, back, FRCNN_REDACT_MAX_ROWS);
    if (lookback < 1 || lookback > FRCNN_TRACK_LOOKBACK_MAX)
        return fail(FRCNN_E_ARG, "%s: lookback=%d not in [1, %d]", who, lookback, FRCNN_TRACK_LOOKBACK_MAX);
    if (radius < 0 || radius > FRCNN_TRACK_MOTION_MAX_RADIUS)
        return fail(FRCNN_E_ARG, "%s: radius=%d not in [0, %d]", who, radius, FRCNN_TRACK_MOTION_MAX_RADIUS);
    if (grow < 0 || grow > FRCNN_TRACK_MAX_GROW) return fail(FRCNN_E_ARG, "%s: grow=%d not in [0, %d]", who, grow, FRCNN_TRACK_MAX_GROW);
    const long long frame_bytes = 3LL * h * w;
    if (frames > 1 && (frame_stride < frame_bytes || out_frame_stride < frame_bytes))
        return fail(FRCNN_E_ARG, "%s: frame_stride=%lld, out_frame_stride=%lld bytes, a %dx%d frame has %lld", who, frame_stride, out_frame_stride, h,
                    w, frame_bytes);
    if (frames > 1 && (tracked_stride < 4 + 8 * g.R || out_tracked_stride < 4 + 8 * g.R2))
        return fail(FRCNN_E_ARG, "%s: tracked_stride=%lld (a buffer has %d words), out_tracked_stride=%lld (%d)", who, tracked_stride, 4 + 8 * g.R,
                    out_tracked_stride, 4 + 8 * g.R2);
    return FRCNN_OK;
}

// the blocks a frame's bytes are copied by
static unsigned lb_blocks(const LbGeom& g) {
    const long long quads = 3LL * g.h * g.w / 16 + 1;
    return (unsigned)((quads + 255) / 256 < 256 ? (quads + 255) / 256 : 256);
}

void lookback_join_launch(uint8_t* window, const LbGeom& g, const uint8_t* frames_u8, long long frame_stride, const int32_t* tracked,
                          long long tracked_stride, const int32_t* n_frames, hipStream_t stream) {
    k_lb_join<<<dim3(lb_blocks(g), g.frames), 256, 0, stream>>>(window, g, frames_u8, frame_stride, tracked, tracked_stride, n_frames);
}

void lookback_emit_launch(uint8_t* window, const LbGeom& g, uint8_t* out_frames, long long out_frame_stride, int32_t* out_tracked,
                          long long out_tracked_stride, int32_t* out_count, hipStream_t stream) {
    k_lb_emit<<<dim3(lb_blocks(g), g.frames), 256, 0, stream>>>(window, g, out_frames, out_frame_stride, out_tracked, out_tracked_stride, out_count);
}

void lookback_close_launch(uint8_t* window, const LbGeom& g, const int32_t* n_frames, hipStream_t stream) {
    k_lb_close<<<1, 64, 0, stream>>>(window, g.frames, n_frames);
}

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_track_lookback_version(void) { return FRCNN_TRACK_LOOKBACK_VERSION; }

extern "C" size_t frcnn_track_lookback_state_bytes(int frames, int h, int w, int max_rows, int capacity, int back) {
    LbGeom g;
    const char* why;
    if (!lb_geom(frames, h, w, max_rows, capacity, back, g, why)) return 0;
    return LB_HEADER + (size_t)2 * frames * g.cell;
}

extern "C" int frcnn_track_lookback(uint8_t* window, const uint8_t* frames_u8, long long frame_stride, const int32_t* tracked,
                                    long long tracked_stride, int frames, const int32_t* n_frames, int max_rows, int capacity, int back,
                                    int lookback, int radius, int grow, int h, int w, uint8_t* out_frames, long long out_frame_stride,
                                    int32_t* out_tracked, long long out_tracked_stride, int32_t* out_count, void* stream) {
    const char* who = "track_lookback";
    LbGeom g;
    const int bad = lookback_check(who, window, frames_u8, frame_stride, tracked, tracked_stride, frames, n_frames, max_rows, capacity, back, lookback,
                                   radius, grow, h, w, out_frames, out_frame_stride, out_tracked, out_tracked_stride, out_count, g);
    if (bad != FRCNN_OK) return bad;
    hipStream_t st = as_stream(stream);
    lookback_join_launch(window, g, frames_u8, frame_stride, tracked, tracked_stride, n_frames, st);
    k_lb_chain<<<dim3(capacity, frames), TM_THREADS, 0, st>>>(window, g, n_frames, lookback, radius, grow);
    k_lb_counts<<<1, TM_THREADS, 0, st>>>(window, g, n_frames, lookback);
    lookback_emit_launch(window, g, out_frames, out_frame_stride, out_tracked, out_tracked_stride, out_count, st);
    lookback_close_launch(window, g, n_frames, st);
    return check_launch(who);
}
