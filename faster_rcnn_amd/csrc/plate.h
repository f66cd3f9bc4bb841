// What csrc/redact_moving.hip shares with csrc/plate.hip: the update kernel's tile and run, the test for a real frame, the round that
// stages a frame's boxes in LDS, and the aligned word of the frame.
#pragma once
#include "common.h"
#include "../../include/ext/frcnn_hip_redact.h"
#include "../../include/ext/frcnn_hip_plate.h"

namespace frcnn {

constexpr int PL_THREADS = 256, PL_WAVES = PL_THREADS / 64;
constexpr int PL_TILE_W = FRCNN_PLATE_TILE_W, PL_TILE_H = FRCNN_PLATE_TILE_H, PL_RUN = 4;                     // a thread's pixels
static_assert((PL_TILE_W / PL_RUN) * PL_TILE_H == PL_THREADS, "a thread is a run of a tile's row");

__device__ inline bool plate_real(int f, const int32_t* n_frames, const int32_t* gate) {
    return f < max(*n_frames, 0) && !(gate && *gate == 0);
}

// One round: the rows base .. base + 255 of the buffer whose clipped boxes meet the tile (tx0..tx1, ty0..ty1) compacted into s_box, in
// row order -> how many.  `table` NULL: every class (the BLOCK set); else the FILL set.  Every thread of the workgroup calls it, and the
// caller puts a barrier behind its reads of s_box.
__device__ inline int plate_round(int4* s_box, int* s_cnt, int base, int nd, const int32_t* bbox, const int32_t* cls, const uint8_t* table,
                                  int num_classes, int M, int h, int w, int tx0, int tx1, int ty0, int ty1) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = base + tid;
    bool hit = false;
    int4 q = make_int4(0, 0, 0, 0);
    if (r < nd) {
        bool chosen = true;
        if (table) {
            const int c = cls[r];
            chosen = c >= 0 && c < num_classes && table[c];
        }
        if (chosen) {
            const long long x1 = bbox[4 * r], y1 = bbox[4 * r + 1], x2 = bbox[4 * r + 2], y2 = bbox[4 * r + 3];
            const long long xa = max(min(x1, x2) - M, 0LL), xb = min(max(x1, x2) + M, (long long)w - 1);
            const long long ya = max(min(y1, y2) - M, 0LL), yb = min(max(y1, y2) + M, (long long)h - 1);
            hit = xa <= xb && ya <= yb && xb >= tx0 && xa <= tx1 && yb >= ty0 && ya <= ty1;
            q = make_int4((int)xa, (int)xb, (int)ya, (int)yb);              // (a hit lies inside the frame: it fits)
        }
    }
    const unsigned long long mask = __ballot(hit);
    if (lane == 0) s_cnt[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
    for (int k = 0; k < PL_WAVES; ++k) {
        const int c = s_cnt[k];
        before += k < wave ? c : 0;
        total += c;
    }
    if (hit) s_box[before + __popcll(mask & ((1ull << lane) - 1ull))] = q;
    __syncthreads();
    return total;
}

// The aligned word at q, of which only the bytes inside [lo, hi) exist.
__device__ inline uint32_t plate_word(const uint8_t* q, const uint8_t* lo, const uint8_t* hi) {
    if (q >= lo && q + 4 <= hi) return *reinterpret_cast<const uint32_t*>(q);
    uint32_t v = 0;
    for (int i = 0; i < 4; ++i)
        if (q + i >= lo && q + i < hi) v |= (uint32_t)q[i] << (8 * i);
    return v;
}

}  // namespace frcnn
