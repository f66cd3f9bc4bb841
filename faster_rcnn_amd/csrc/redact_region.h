// What csrc/redact_moving.hip shares with csrc/redact_region.hip: the ONE definition of a plane of weights (its header words and where
// its pieces lie), so that a plane either file builds is a plane frcnn_redact_region_prepare / frcnn_redact_region_apply_u8 take.
#pragma once
#include "redact.h"
#include "../../include/ext/frcnn_hip_redact_region.h"

namespace frcnn {

constexpr int RR_FMAX = FRCNN_REDACT_REGION_FEATHER_MAX;
constexpr int RR_HEAD = FRCNN_REDACT_REGION_HEAD_WORDS;
enum { RR_H, RR_W, RR_F, RR_COVERED, RR_FULL, RR_ONE };                     // words of the header
static_assert(RR_HEAD == 8 && RR_FMAX + 1 <= 255, "d1 is a byte");

// where the pieces of a plane lie, in bytes from its start
struct RegionLayout { size_t w_at, flags_at, hard_at, d1_at, total; };

__host__ __device__ inline RegionLayout region_layout(int h, int w) {
    RegionLayout L;
    const size_t cols = ((size_t)3 * w + RD_THREADS - 1) / RD_THREADS, rows = ((size_t)h + RD_TILE_ROWS - 1) / RD_TILE_ROWS;
    L.w_at = 4 * RR_HEAD;
    L.flags_at = align16(L.w_at + 2 * (size_t)h * w);
    L.hard_at = align16(L.flags_at + cols * rows);
    L.d1_at = align16(L.hard_at + ((size_t)h + 2 * RR_FMAX) * ((size_t)w + 2 * RR_FMAX));    // (sized for the largest feather)
    L.total = align16(L.d1_at + ((size_t)h + 2 * RR_FMAX) * (size_t)w);
    return L;
}

}  // namespace frcnn
