// Launch policy of the f32 convolution (conv_policy.hip, host code only): which tile, main loop and split-K / stream-K form a
// forward launch of a descriptor takes on each of the three f32 engines -- native (conv_igemm.hip), bf16x6 (conv_x6.hip) and f16x3
// (conv_h3.hip) -- and the workspace that needs.  conv_fwd_impl (conv_igemm.hip) launches what these functions choose, and the
// frcnn_conv2d_*config / *_workspace_bytes / _engine queries of the C ABI report it from the same functions.
#pragma once
#include "common.h"

namespace frcnn {

// Dev knobs of the policy, read from the environment once, on first use.  The conv lab (scripts/micro/conv_lab.hip) sets them in place.
struct ConvKnobs {
    int force_tile;             // FRCNN_FORCE_TILE: the native tile code that auto takes (0: the measured policy)
    int group_m;                // FRCNN_GROUP_M: tile-order group size, ConvArgs.group_m (-1: the policy's)
    bool scalar_epilogue;       // FRCNN_SCALAR_EPILOGUE: the 4-byte epilogue everywhere
    bool sk_shared;             // FRCNN_SK_SHARED: the balanced form beside other images' launches too (tile 50)
    long long x6_sk128_min;     // FRCNN_X6_SK128_MIN: bf16x6 split-K on 128x128 tiles from this many such tiles on (64)
    int h3_big_min_shared;      // FRCNN_H3_BIG_MIN_TILES_SHARED: f16x3 beside other passes: the 256x128 form from this many 128x128 tiles on (128)
    int h3_shared_small;        // FRCNN_H3_SHARED_SMALL: f16x3 beside other passes: the tile code of launches too small for 256x128 (81; 0: off)
    int h3_shared_small_rows;   // FRCNN_H3_SHARED_SMALL_ROWS: ... from this many output rows on (4096)
};
ConvKnobs& conv_knobs();

constexpr size_t SPLITK_TICKET_BYTES = 16384;      // head of a split-K / balanced workspace: one u32 per output tile (<= 4096 tiles)
constexpr int SK_SLOTS = 4;                        // balanced form: partial-tile slots per output tile (the policy keeps ranges long enough)

long long conv_tiles(const frcnn_conv_desc* d, int edge);                 // output tiles of edge x edge
size_t splitk_workspace_bytes(long long tiles, int slices, int edge);    // tickets + one f32 partial tile per (tile, slice)

// ---- native engine
int choose_config(const frcnn_conv_desc* d);               // tile code of a single-layer launch with a workspace at hand
int choose_splits(const frcnn_conv_desc* d, int cfg);      // split-K slices of the 64x64 kernels (1: none)
int choose_streamk(const frcnn_conv_desc* d, int cfg);     // balanced launch: workgroups, 0 = not this form
int streamk_edge(int cfg);                                 // tile edge of the balanced launch for cfg (128 / 64)
int native_tile_width(int cfg);                            // output columns per tile
int dual_config(int cfg);                                  // what the two-layer launch makes of a tile choice
int workspace_config(const frcnn_conv_desc* d, int cfg, bool has_workspace);   // ... and a launch without a workspace
int plain_config(int cfg);                                 // the tile a balanced code (61 / 62) runs when the form does not apply
int native_group_m(const frcnn_conv_desc* d, int cfg);     // ConvArgs.group_m

// ---- split engines (bf16x6, f16x3): one set of rules, these constants apart
struct SplitRule {
    const char* name;           // "x6" / "h3": messages say conv2d_fwd_<name>
    int planes;                 // 16-bit filter planes (the 2 GiB limit)
    int code0;                  // the engine's tile codes are code0 + 1 .. code0 + 7 (+4: 64x64, +7: 128x64 for 64-column layers)
    int force64, force128;      // tile codes that force the split-K tile edge: 74 / 84, 78 / 88
    int sk64, sk128;            // the split-K kernels' codes: 174 / 184, 171 / 181
    int min_chunks;             // split-K needs this many k-chunks (64 / 32; 32..63 only on grids under 256 tiles of 64x64)
    bool big_sk_tile;           // the 128x128 split-K tile from conv_knobs().x6_sk128_min such tiles on (else 64x64 unless forced)
    int (*wide_config)(const frcnn_conv_desc* d);     // tile code of a launch with more than 64 columns
    int (*tile_width)(int cfg);                       // output columns per tile (conv_x6.hip / conv_h3.hip)
};
const SplitRule& split_rule(int engine);                                    // FRCNN_ENGINE_X6 / FRCNN_ENGINE_H3
int split_config(const SplitRule& r, const frcnn_conv_desc* d, int n1);     // n1 > 0: a two-layer launch whose first layer has n1 columns
int split_slices(const SplitRule& r, const frcnn_conv_desc* d);
int split_sk_code(const SplitRule& r, const frcnn_conv_desc* d);            // the split-K kernel's tile code
size_t split_workspace_bytes(const SplitRule& r, const frcnn_conv_desc* d);
int split_group_m(const frcnn_conv_desc* d, int bn);

}  // namespace frcnn
