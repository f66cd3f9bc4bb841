// Launch policy of the f32 convolution engines (see conv_policy.h): tile choice, split-K and stream-K, workspace bytes, and the
// C ABI queries that report them.  Host code only.
#include "conv_policy.h"
#include "conv_f32_common.h"

namespace frcnn {

static long long env_ll(const char* name, long long dflt) {
    const char* v = getenv(name);
    return v ? atoll(v) : dflt;
}

ConvKnobs& conv_knobs() {
    static ConvKnobs k = {(int)env_ll("FRCNN_FORCE_TILE", 0), (int)env_ll("FRCNN_GROUP_M", -1), getenv("FRCNN_SCALAR_EPILOGUE") != nullptr,
                          getenv("FRCNN_SK_SHARED") != nullptr, env_ll("FRCNN_X6_SK128_MIN", 64), (int)env_ll("FRCNN_H3_BIG_MIN_TILES_SHARED", 128),
                          (int)env_ll("FRCNN_H3_SHARED_SMALL", 81), (int)env_ll("FRCNN_H3_SHARED_SMALL_ROWS", 4096)};
    return k;
}

static long long conv_rows(const frcnn_conv_desc* d) { return (long long)d->n * d->ho * d->wo; }

long long conv_tiles(const frcnn_conv_desc* d, int edge) {
    return ((conv_rows(d) + edge - 1) / edge) * ((d->cout + edge - 1) / edge);
}

size_t splitk_workspace_bytes(long long tiles, int slices, int edge) {
    return SPLITK_TICKET_BYTES + (size_t)tiles * slices * edge * edge * sizeof(float);
}

// ---- native engine

// what the two-layer launch (frcnn_conv2d_fwd_dual) makes of a single-layer tile choice
int dual_config(int cfg) {
    if (cfg >= 61) cfg -= 40;                               // no balanced form for the two-layer launch
    if (cfg < 11 || (cfg >= 41 && cfg <= 43)) cfg = 23;     // v2 main loops with the 2x2-wave tiles only
    return cfg;
}

// the 128x128 choice of a position-major multi-tap layer counted on the balanced form: without a workspace, 64x64 tiles
int workspace_config(const frcnn_conv_desc* d, int cfg, bool has_workspace) {
    return (cfg == 21 && !has_workspace && d->tile % 100 == 0 && d->layout && d->kh * d->kw > 1) ? 23 : cfg;
}

int plain_config(int cfg) { return (cfg == 61 || cfg == 62) ? cfg - 40 : cfg; }

int streamk_edge(int cfg) { return (cfg == 21 || cfg == 26 || cfg == 61) ? 128 : 64; }

int native_tile_width(int cfg) { return (cfg == 21 || cfg == 26 || cfg == 11 || cfg == 24 || cfg == 14) ? 128 : 64; }

int choose_config(const frcnn_conv_desc* d) {
    const int Kpad = (d->kh * d->kw * d->cin + BK - 1) / BK * BK;
    const bool generic = (d->cin % BK) != 0;
    const long long t128 = conv_tiles(d, 128);
    int cfg = d->tile % 100;    // 0 = auto; the hundreds digit(s) force the split-K factor (choose_splits)
    const int forced = conv_knobs().force_tile;
    if (cfg == 0 && forced && !generic) cfg = forced;
    const bool shared_chip = cfg == 50;                     // "auto, other launches run beside this one" (several images in flight)
    if (cfg == 50) cfg = 0;
    if (cfg == 0) {
        // measured on MI355X over every conv shape of the C2 pipeline (scripts/conv_shapes.py):
        // the 64x64 v2 kernel wins wherever the grid is small or k is short; 128x128 v2 only
        // pays once there are >= 1.5 tiles per CU slot AND a long k loop to amortise its prologue
        // position-major multi-tap layers skip padding-only taps per tile: tiles then differ in length, and only
        // a grid with several tiles per CU slot (64x64: 1840 tiles for the head 3x3) turns that into a shorter
        // launch (500 vs 570 us); the 460 128x128 tiles all start at once and the full-length ones set the time
        // (with several images in flight the neighbours fill the freed slots: pipelines then ask for tile 21)
        // round 2 (scripts/micro/conv_lab.hip): the mid-chunk-barrier main loop (23 / 26) beats the late-store loop on
        // every 64x64 launch (trunk + RPN head 1 355 -> 1 269 us per image, bit-identical) and on the 1x1 big-tile
        // launches (2048->512: 253 -> 246 us); the 3x3 big-tile launches keep the late-store loop (528 vs 539 us)
        if (generic) cfg = 2;
        else if (d->layout && d->kh * d->kw > 1 && !shared_chip) cfg = choose_streamk(d, 21) ? 21 : 23;   // balanced 128x128 beats both
        else if (t128 >= 384 && Kpad >= 1024) cfg = d->kh * d->kw == 1 ? 26 : 21;
        else cfg = 23;
    }
    if (d->layout && cfg >= 1 && cfg <= 4) cfg += 10;       // only the v2 main loop knows the position-major layout
    const bool fits_srd = (size_t)d->n * d->h * d->w * d->cin * 4 < 0x7fffffffull && (size_t)d->cout * Kpad * 4 < 0x7fffffffull;
    // the v2 main loops walk the filter taps through a 32-bit mask: larger filters (6x6 and up) stay on the v1 kernels
    const bool v1_only = !fits_srd || generic || d->kh * d->kw > 32;
    if (cfg >= 61 && v1_only) cfg -= 60;
    if (cfg >= 41 && v1_only) cfg = (cfg == 43) ? 3 : 1;
    if (cfg >= 23 && cfg <= 26 && v1_only) cfg = cfg >= 25 ? 1 : 2;
    if (cfg >= 21 && v1_only) cfg -= 20;
    if (cfg >= 11 && v1_only) cfg -= 10;
    if (generic) cfg = (cfg == 2) ? 2 : 3;
    return cfg;
}

// K-slices per output tile for the 64x64 kernel (1 = plain launch).  desc.tile / 100 forces a value (dev knob).
int choose_splits(const frcnn_conv_desc* d, int cfg) {
    if (cfg != 22 && cfg != 23) return 1;
    const long long tiles = conv_tiles(d, 64);
    const int nk = (d->kh * d->kw * d->cin + BK - 1) / BK;
    if (tiles * sizeof(unsigned) > SPLITK_TICKET_BYTES) return 1;
    int s = d->tile / 100;
    if (s <= 0) {
        // measured on MI355X (scripts/conv_shapes.py, C2 shapes): grids under 1.5 tiles per CU with >= 16 chunks
        // gain from 3 slices (stage 3/4 3x3 and 1x1-reduce, rpn_conv1: -10..-37 %); tiny grids (RPN heads, dense)
        // take enough slices for ~2 workgroups per CU, at least 4 chunks each; shorter k loops lose to the combine
        // 384..639 tiles with a long k loop (the detector head at 64 training RoIs: 392 tiles, 144 / 64 chunks) fill
        // 38-60 % of the 1024 slots: four slices take 174 -> 143 us (3x3) and 85 -> 76 us (2048 -> 512)
        if (tiles >= 384 && tiles < 640 && nk >= 64) return 4;
        if (tiles >= 384 || nk < 16) return 1;
        // (round 2, mid-chunk-barrier loop: 100..383 tiles with a LONG k loop take five slices -- stage-4 3x3 31.9 -> 30.9 us,
        // rpn_conv1 190.5 -> 178.8 us: 5 x 304 workgroups sit 6-deep on the 256 CUs where 3 x 304 sit 4-deep on some and 3 on others)
        s = tiles >= 100 ? (nk >= 64 ? 5 : 3) : (int)((456 + tiles - 1) / tiles);
        if (s > nk / 4) s = nk / 4;
        if (s > 16) s = 16;
    }
    if (s > nk) s = nk;
    if (s > 32) s = 32;
    return s < 1 ? 1 : s;
}

// Balanced (stream-K) launch: G workgroups for this descriptor, or 0 when the plain / split-K forms are better.
// Auto picks it for the two late-store tiles when the grid wastes >= 6 % of its last round of CU slots, the k loop is
// long enough for the partial-tile traffic not to matter (>= 32 chunks) and no tile can meet more than SK_SLOTS
// ranges.  desc.tile 61 / 62 force it (tests), a hundreds digit (forced split-K factor / "never split") disables it.
static int streamk_tile_taps(const frcnn_conv_desc* d, int tile_m, int BM) {
    const int RS = d->kh * d->kw;
    if (!d->layout) return RS;
    const long long M = conv_rows(d);
    const long long m0 = (long long)tile_m * BM;
    const long long m1 = (m0 + BM < M ? m0 + BM : M) - 1;
    const int pos_lo = (int)(m0 / d->n), pos_hi = (int)(m1 / d->n);
    if (pos_hi - pos_lo >= 8 || RS > 32) return RS;
    unsigned mk = 0;
    for (int pos = pos_lo; pos <= pos_hi; ++pos) {
        const int ho = pos / d->wo, wo = pos - ho * d->wo;
        const int h0 = ho * d->stride - d->pad_top, w0 = wo * d->stride - d->pad_left;
        for (int r = 0; r < d->kh; ++r)
            for (int sx = 0; sx < d->kw; ++sx)
                if ((unsigned)(h0 + r) < (unsigned)d->h && (unsigned)(w0 + sx) < (unsigned)d->w) mk |= 1u << (r * d->kw + sx);
    }
    return mk ? __builtin_popcount(mk) : RS;
}

int choose_streamk(const frcnn_conv_desc* d, int cfg) {
    const bool forced = (cfg == 61 || cfg == 62);
    if (!forced && (cfg != 21 && cfg != 22 && cfg != 26)) return 0;
    if (d->tile / 100 != 0 || (d->cin % BK) != 0) return 0;
    const int BM = streamk_edge(cfg);
    const bool big = BM == 128;
    const long long tiles_m = (conv_rows(d) + BM - 1) / BM, tiles_n = (d->cout + BM - 1) / BM;
    const long long tiles = tiles_m * tiles_n;
    const int slots = 256 * (big ? 2 : 4);                   // workgroups the chip holds at once (LDS: 2 x 74 KB / 4 x 37 KB per CU)
    const int RS = d->kh * d->kw;
    const int groups = d->cin / BK, nk_max = groups * RS;
    if (tiles_m > 1024 || tiles * sizeof(unsigned) > SPLITK_TICKET_BYTES) return 0;
    if ((size_t)tiles * SK_SLOTS * BM * BM * 4 >= 0x7fffffffull) return 0;
    const long long rounds = (tiles + slots - 1) / slots;
    const long long G = rounds * slots;
    if (!forced) {
        // measured (scripts/layout_compare.py, 300 RoIs): on the 128x128 tile the balanced form wins wherever it is
        // eligible (3x3 575 -> 483 us, 2048->512 276 -> 263, 1024->512 154 -> 149); on the 64x64 tile the partial-tile
        // traffic eats the gain (506 -> 520, 280 -> 294), and beside other images' launches (tile 50) the idle slots
        // are already taken: four images in flight run 3 % slower with it
        if (!big || (d->tile % 100 == 50 && !conv_knobs().sk_shared)) return 0;
        if (nk_max < 32 || tiles * 100 > G * 94 || tiles * 2 < G) return 0;
    }
    long long U = 0;
    for (int m = 0; m < tiles_m; ++m) U += (long long)groups * streamk_tile_taps(d, m, BM);
    U *= tiles_n;
    if (U < G || U / G < nk_max / 2 + 1) return 0;           // a tile would meet more than SK_SLOTS ranges
    return (int)G;
}

// tile order (ConvArgs.group_m): multi-round 64x64 launches with many column tiles walk groups of four row tiles
// (1x1 512->2048 on 14 700 rows: 276 -> 261 us, scripts/micro/conv_lab.hip under FRCNN_GROUP_M); single-round
// grids and the big tiles measured no difference and keep the plain order
// round 3 (scripts/group_m_sweep.sh, rocprofv3 --pmc FETCH_SIZE): the plain 128x128 launches gave the column tiles
// of one row tile to DIFFERENT XCDs (an XCD's run of ids was ~57 row tiles of one column tile), so every A row
// tile crossed the fabric once per column tile.  With groups of ONE row tile the column tiles that share A rows are
// neighbours on one XCD: 2048->512 on 14 700 rows fetches 105 instead of 259 MB (raw counter) at 287 vs 291 us, the
// 3x3 181 instead of 203 MB (its nine taps reach the neighbouring positions' rows, which live on other XCDs).
int native_group_m(const frcnn_conv_desc* d, int cfg) {
    if (conv_knobs().group_m >= 0) return conv_knobs().group_m;
    if ((cfg == 21 || cfg == 26) && d->cout > 128) return 1;
    return (cfg == 22 || cfg == 23) && conv_tiles(d, 64) > 1024 && d->cout >= 512 ? 4 : 0;
}

// ---- split engines

// The bf16x6 tile of a launch with more than 64 columns: 128x128 tiles on eight waves (two workgroups per CU); long k on a grid of
// >= 200 256x128 tiles: the 16-wave double-buffered form (head 3x3 337 vs 350 us, 2048 -> 512 157 vs 169; 512 -> 2048 ties and
// stays); under one 128x128 tile per CU, 64x64.
static int x6_wide_config(const frcnn_conv_desc* d) {
    const int K = d->kh * d->kw * d->cin;
    const long long t256 = ((conv_rows(d) + 255) / 256) * ((d->cout + 127) / 128);
    return conv_tiles(d, 128) >= 256 ? ((K >= 1024 && t256 >= 200) ? 76 : 71) : 74;
}

// The f16x3 tile of a launch with more than 64 columns: the double-buffered 256x128 forms wherever a launch has >= 256 tiles of
// 128x128 (lab: the head's 3x3 / 512 -> 2048 / 2048 -> 512 GEMMs 246 / 127 / 104 us on sixteen waves against 359 / 154 / 138 on the
// two-workgroup 128x128 tile and 331 / 147 / 148 on 64x64 tiles); everything smaller on 64x64 tiles.
static int h3_wide_config(const frcnn_conv_desc* d) {
    const ConvKnobs& k = conv_knobs();
    const bool shared = d->tile % 100 == 50;
    // beside other passes' launches the big tile pays from half as many tiles on (scripts/dev/r6_shared_big_min.sh: from 128 / 256 /
    // 512 / 1024 tiles 555.9 / 554.5 / 544.5 / 540.5 img/s): what it leaves idle, other passes fill
    const int cfg = conv_tiles(d, 128) >= (shared ? k.h3_big_min_shared : 256) ? 86 : 84;
    // Beside other passes' launches (tile code 50: the chip is saturated -- sixteen images per 29 ms against 1.9 ms of isolated conv time
    // per image -- and idle CUs are the other passes' to fill) a launch too small for the 256x128 form does its FLOPs cheaper on 128x128
    // tiles (eight waves, code 81) than on 64x64: stage 4's 256-column layers of a four-image pass, 544.2 -> 549.7 img/s, backbone in
    // flight 0.469 -> 0.458 ms per image (scripts/dev/r6_shared_small.sh; four waves of 64x64, code 83: 544.2).  Alone on the chip the
    // 64x64 tiles stay (150 workgroups of 128x128 leave 106 CUs idle).  Same chunk order: the same bits.  FRCNN_H3_SHARED_SMALL=0: off.
    if (shared && cfg == 84 && k.h3_shared_small && d->cout >= 128 && conv_rows(d) >= k.h3_shared_small_rows) return k.h3_shared_small;
    return cfg;
}

// Split-K on the split engines: 64x64 tiles (four waves) fill the chip from the smallest grids.  On bf16x6, from ~64 tiles of 128x128
// on, the eight-wave 128x128 tile (nine fragment reads per twelve MFMAs instead of six per six) is the better workgroup -- the detector
// head's 3x3 over 64 RoIs (3 136 rows, k 4 608), rpn_conv1.  On f16x3 that tile needs 154 registers with its two accumulator sets: one
// workgroup per CU, so the rule -- ONE round of two workgroups per CU -- does not carry over.  f16x3 also splits shorter reductions,
// on grids that leave most CUs idle (stage 4's 1x1 1024 -> 256 at 152 tiles: 21.9 us native split-K, 19.0 here).
const SplitRule& split_rule(int engine) {
    static const SplitRule x6 = {"x6", 3, 70, 74, 78, 174, 171, 64, true, x6_wide_config, x6_tile_width};
    static const SplitRule h3 = {"h3", 2, 80, 84, 88, 184, 181, 32, false, h3_wide_config, h3_tile_width};
    return engine == FRCNN_ENGINE_H3 ? h3 : x6;
}

// 64-column layers (a 128-wide tile would be half empty: stage 2's 3x3 48.8 us against 30.9 on 64x64 tiles, 36.3 native): 64x64,
// or 128x64 on four waves once there are >= 1024 of them (VGG16 conv1_2, 600 000 rows: 361 us against 389 / 458 native).
int split_config(const SplitRule& r, const frcnn_conv_desc* d, int n1) {
    const int t = d->tile % 100;
    if (t >= r.code0 + 1 && t <= r.code0 + 7) return t;
    int cfg;
    if (d->cout <= 64) cfg = ((conv_rows(d) + 127) / 128) >= 1024 ? r.code0 + 7 : r.code0 + 4;
    else cfg = r.wide_config(d);
    // the layer boundary of a paired launch must be a tile boundary (16-byte epilogue)
    if (n1 > 0 && (n1 % 128) != 0 && cfg != r.code0 + 7) cfg = r.code0 + 4;
    return cfg;
}

static int split_sk_edge(const SplitRule& r, const frcnn_conv_desc* d) {
    const int t = d->tile % 100;
    if (t == r.force128) return 128;
    if (t == r.force64 || !r.big_sk_tile) return 64;
    return conv_tiles(d, 128) >= conv_knobs().x6_sk128_min ? 128 : 64;
}

int split_sk_code(const SplitRule& r, const frcnn_conv_desc* d) { return split_sk_edge(r, d) == 128 ? r.sk128 : r.sk64; }

// slices: tile % 100 74 / 78 (84 / 88) force the 64 / 128 form, tile / 100 the slice count (dev)
int split_slices(const SplitRule& r, const frcnn_conv_desc* d) {
    if (d->cin % BK) return 1;
    const int t = d->tile % 100;
    if (t != 0 && t != 50 && t != r.force64 && t != r.force128) return 1;
    const int edge = split_sk_edge(r, d);
    const long long tiles = conv_tiles(d, edge), tiles64 = conv_tiles(d, 64);
    const int nk = (d->kh * d->kw * d->cin) / BK;
    if (tiles * sizeof(unsigned) > SPLITK_TICKET_BYTES) return 1;
    int s = d->tile / 100;
    if (s <= 0) {
        if (tiles64 >= 640 || nk < r.min_chunks || (nk < 64 && tiles64 >= 256)) return 1;
        if (edge == 128) s = (int)(512 / tiles);                     // ONE round of two workgroups per CU: 3 136 x 512 (100 tiles) 94 us at 5 slices, 110 at 4 or 6; rpn_conv1 (76 tiles) 161 at 6, 169 / 175 at 5 / 3
        else s = tiles >= 100 ? 3 : (int)((768 + tiles - 1) / tiles);      // sweep (MI355X): rpn_conv1 (304 tiles) 209 / 192 / 204 / 189 us at 2 / 3 / 4 / 5 slices, stage 4 3x3 (152) 32.6 / 34.2 / 33.4 at 3 / 4 / 6
        if (s > nk / 8) s = nk / 8;
        if (s > 16) s = 16;
    }
    if (s > nk) s = nk;
    return s < 1 ? 1 : s;
}

size_t split_workspace_bytes(const SplitRule& r, const frcnn_conv_desc* d) {
    if (!d || d->cin <= 0) return 0;
    const int splits = split_slices(r, d);
    if (splits <= 1) return 0;
    const int edge = split_sk_edge(r, d);
    return splitk_workspace_bytes(conv_tiles(d, edge), splits, edge);
}

// column tiles of a row tile adjacent on one XCD
int split_group_m(const frcnn_conv_desc* d, int bn) {
    return conv_knobs().group_m >= 0 ? conv_knobs().group_m : (d->cout > bn ? 1 : 0);
}

}  // namespace frcnn

using namespace frcnn;

extern "C" {

size_t frcnn_conv2d_workspace_bytes(const frcnn_conv_desc* d) {
    if (!d || d->cin <= 0 || (d->cin % BK) != 0) return 0;
    const int cfg = choose_config(d);
    if (choose_streamk(d, cfg)) return splitk_workspace_bytes(conv_tiles(d, streamk_edge(cfg)), SK_SLOTS, streamk_edge(cfg));
    const int splits = choose_splits(d, cfg);
    return splits > 1 ? splitk_workspace_bytes(conv_tiles(d, 64), splits, 64) : 0;
}

// Split-K workspace of the two-layer launch: the balanced (stream-K) form is not used there.
size_t frcnn_conv2d_dual_workspace_bytes(const frcnn_conv_desc* d) {
    if (!d || d->cin <= 0 || (d->cin % BK) != 0) return 0;
    const int splits = choose_splits(d, choose_config(d));
    return splits > 1 ? splitk_workspace_bytes(conv_tiles(d, 64), splits, 64) : 0;
}

size_t frcnn_conv2d_x6_workspace_bytes(const frcnn_conv_desc* d) { return split_workspace_bytes(split_rule(FRCNN_ENGINE_X6), d); }

size_t frcnn_conv2d_h3_workspace_bytes(const frcnn_conv_desc* d) { return split_workspace_bytes(split_rule(FRCNN_ENGINE_H3), d); }

// ---- which matrix path a forward launch of this descriptor should take: the measured policy, for hosts in any language.
// prefer: FRCNN_ENGINE_X6 / FRCNN_ENGINE_H3 = the split engine the caller has filter planes for (FRCNN_ENGINE_NATIVE: always native).
// An explicit tile code picks its engine (71..78: bf16x6, 81..88: f16x3).  Otherwise a split engine takes launches with cin % 32 == 0,
// at most 32 taps, >= 64 output columns and >= 256 output tiles of 64x64 (MI355X, configs[1] shapes, each launch alone on the chip:
// scripts/conv_shapes.py -- the head's 14 700-row GEMMs 236 / 148 / 115 us on f16x3, 352 / 208 / 166 on bf16x6, 531 / 282 / 267 native;
// almost every trunk layer wins by 5-15 %); smaller grids stay on the native split-K launches unless the engine's own split-K form
// applies (>= 128 columns, a workspace at hand: rpn_conv1, stage 4's 3x3).
enum { ENGINE_MIN_TILES = 256, ENGINE_MIN_COUT = 64 };

int frcnn_conv2d_engine(const frcnn_conv_desc* d, int prefer, int workspace_present) {
    if (!d) return fail(FRCNN_E_ARG, "conv2d_engine: null descriptor");
    if (prefer != FRCNN_ENGINE_NATIVE && prefer != FRCNN_ENGINE_X6 && prefer != FRCNN_ENGINE_H3)
        return fail(FRCNN_E_ARG, "conv2d_engine: unknown engine %d", prefer);
    const int t = d->tile % 100;
    const bool splittable = d->cin > 0 && (d->cin % BK) == 0;
    if (t >= 71 && t <= 78) return splittable ? FRCNN_ENGINE_X6 : FRCNN_ENGINE_NATIVE;
    if (t >= 81 && t <= 88) return splittable ? FRCNN_ENGINE_H3 : FRCNN_ENGINE_NATIVE;
    if (prefer == FRCNN_ENGINE_NATIVE || (t != 0 && t != 50)) return FRCNN_ENGINE_NATIVE;
    if (!splittable || d->cout < ENGINE_MIN_COUT || d->kh * d->kw > 32) return FRCNN_ENGINE_NATIVE;
    if (conv_tiles(d, 64) >= ENGINE_MIN_TILES) return prefer;
    const size_t need = split_workspace_bytes(split_rule(prefer), d);
    return (d->cout >= 128 && workspace_present && need > 0) ? prefer : FRCNN_ENGINE_NATIVE;
}

int frcnn_conv2d_config(const frcnn_conv_desc* d) {
    if (!d) return fail(FRCNN_E_ARG, "conv2d_config: null descriptor");
    if (d->cin == 3) return 30;                                 // the 3-channel stem kernel, whatever tile was asked for
    const int cfg = choose_config(d);
    if (choose_streamk(d, cfg)) return streamk_edge(cfg) == 128 ? 61 : 62;     // what a launch WITH a workspace runs
    return plain_config(cfg);                                   // (61 / 62 asked for, but the shape is not eligible)
}

int frcnn_conv2d_dual_config(const frcnn_conv_desc* d, int has_workspace) {
    if (!d) return fail(FRCNN_E_ARG, "conv2d_dual_config: null descriptor");
    return workspace_config(d, dual_config(choose_config(d)), has_workspace != 0);
}

int frcnn_conv2d_x6_config(const frcnn_conv_desc* d, int n1) {
    if (!d) return fail(FRCNN_E_ARG, "conv2d_x6_config: null descriptor");
    return split_config(split_rule(FRCNN_ENGINE_X6), d, n1);
}

int frcnn_conv2d_h3_config(const frcnn_conv_desc* d, int n1) {
    if (!d) return fail(FRCNN_E_ARG, "conv2d_h3_config: null descriptor");
    return split_config(split_rule(FRCNN_ENGINE_H3), d, n1);
}

}  // extern "C"
