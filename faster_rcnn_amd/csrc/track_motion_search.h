// The integer block match of the motion rule (include/ext/frcnn_hip_track_motion.h: LUMA, GRID, COST, BEST, GATE) as device code, shared
// by csrc/track_motion.hip (a tracker slot between two frames of a call) and csrc/track_lookback.hip (a new track's box, backwards).
// One workgroup of TM_THREADS threads searches one box: it stages the box's <= 1024 template lumas once; a wave takes a candidate at a
// time, its lanes the samples (16 each, in registers), and reads the current frame where it lies: the window of a strided grid does not
// tile into LDS, and a whole search is <= 1.1 M pixel reads that L2 serves.  A candidate's cost is a shuffle sum; a wave keeps the minimum
// of ONE packed key per candidate, cost << 22 | norm << 12 | dy + 16 << 6 | dx + 16 (18 + 10 + 6 + 6 bits): a uint64 minimum IS the
// lexicographic rule.  The waves' keys meet in LDS and wave 0 shuffles them down.
#pragma once
#include "common.h"
#include "../../include/ext/frcnn_hip_track_motion.h"

namespace frcnn {

constexpr int TM_THREADS = 1024;
constexpr int TM_WAVES = TM_THREADS / 64;
constexpr int TM_GRID = FRCNN_TRACK_MOTION_GRID;
constexpr int TM_PER_LANE = TM_GRID * TM_GRID / 64;                         // samples of a lane
static_assert(TM_GRID * TM_GRID <= TM_THREADS, "a thread stages one template luma");
static_assert(TM_WAVES <= 64, "wave 0 reduces the waves' keys");

// the LDS of one search
struct TmShared {
    uint8_t t[TM_GRID * TM_GRID];
    unsigned long long key[TM_WAVES];
    int zero;
};

__device__ __forceinline__ int luma(const uint8_t* p) { return ((int)p[0] + 2 * (int)p[1] + (int)p[2] + 2) >> 2; }

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int off) {
    const unsigned lo = __shfl_xor((unsigned)v, off), hi = __shfl_xor((unsigned)(v >> 32), off);
    return ((unsigned long long)hi << 32) | lo;
}

// The move of the raw box (x1, y1, x2, y2) from frame ``ref`` to frame ``cur``, both [h][w][3]: true, with (dx, dy) set, in the lanes of
// WAVE 0 when a move passes the gate; false in every other thread, and in all of them for a box that is not searched (empty, or fewer
// than 16 samples).  Called by all TM_THREADS threads of a workgroup with the same arguments: every path crosses the same barriers (two
// when the box is searched, none otherwise).  ``sh`` may be used again behind a barrier of the caller's.
__device__ __forceinline__ bool tm_search(const uint8_t* ref, const uint8_t* cur, int x1, int y1, int x2, int y2, int radius, int h, int w,
                                          TmShared& sh, int& dx_out, int& dy_out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int xa = max(min(x1, x2), 0), xb = min(max(x1, x2), w - 1), ya = max(min(y1, y2), 0), yb = min(max(y1, y2), h - 1);
    if (xa > xb || ya > yb) return false;
    const int sx = (xb - xa + 1 + TM_GRID - 1) / TM_GRID, sy = (yb - ya + 1 + TM_GRID - 1) / TM_GRID;
    const int x0 = xa + sx / 2, y0 = ya + sy / 2;                           // (sx / 2 < the box's width: the first sample is inside)
    const int cols = (xb - x0) / sx + 1, rows = (yb - y0) / sy + 1, n = cols * rows;
    if (n < FRCNN_TRACK_MOTION_MIN_SAMPLES) return false;                   // (the whole workgroup, as every return above)
    if (tid < n) {
        const int x = x0 + (tid % cols) * sx, y = y0 + (tid / cols) * sy;
        sh.t[tid] = (uint8_t)luma(ref + ((size_t)y * w + x) * 3);
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
        pt[k] = some ? sh.t[i] : 0;
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
        if (dx == 0 && dy == 0 && lane == 0) sh.zero = cost;
    }
    if (lane == 0) sh.key[wave] = best;
    __syncthreads();
    if (wave != 0) return false;
    best = lane < TM_WAVES ? sh.key[lane] : ~0ull;
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = shfl_xor_u64(best, off);
        best = o < best ? o : best;
    }
    const int cost = (int)(best >> 22);
    if (cost + n > sh.zero) return false;                                   // the gate: a flat or unchanged region does not move
    dy_out = (int)((best >> 6) & 63) - 16;
    dx_out = (int)(best & 63) - 16;
    return true;
}

}  // namespace frcnn
