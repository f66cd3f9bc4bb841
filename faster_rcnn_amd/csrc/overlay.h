// What the kernels that draw over a frame share (k_trails_draw, k_count_draw, k_zone_draw; DESIGN §8 "The id-table walk"): the palette, the
// tile a workgroup owns, the capsule around a segment, and the labels -- their glyphs, the decimal formatter, where a label goes and how
// it lands in a thread's column.  gfx950 only.
#pragma once
#include "common.h"
#include "../../include/ext/frcnn_hip_redact.h"

namespace frcnn {

// A workgroup owns a tile of 256 byte columns x 16 rows, as csrc/redact.hip's phase two does and for its reason (threads are bytes: 64
// lanes on 64 consecutive bytes are one coalesced access wherever a row of 3-byte pixels starts).
constexpr int OV_THREADS = 256, OV_TILE_ROWS = 16;

struct OvTile {
    int rowbytes, ty0, ty1, tx0, tx1;                                       // the frame's row; the tile's rows and the pixels its columns touch
    int j, x, c;                                                            // this thread's byte column, its pixel and channel
};

__device__ inline OvTile ov_tile(int h, int w) {
    OvTile t;
    const int j0 = blockIdx.x * OV_THREADS;
    t.rowbytes = 3 * w;
    t.ty0 = blockIdx.y * OV_TILE_ROWS;
    t.ty1 = min(t.ty0 + OV_TILE_ROWS, h) - 1;
    t.tx0 = j0 / 3;
    t.tx1 = min(j0 + OV_THREADS - 1, t.rowbytes - 1) / 3;
    t.j = j0 + threadIdx.x;
    t.x = t.j / 3;
    t.c = t.j - 3 * t.x;
    return t;
}

inline dim3 ov_grid(int h, int w) { return dim3((3 * w + OV_THREADS - 1) / OV_THREADS, (h + OV_TILE_ROWS - 1) / OV_TILE_ROWS); }

static __constant__ uint8_t OV_PALETTE[8][3] = {{255, 64, 64}, {64, 160, 255}, {255, 208, 0}, {255, 0, 255},
                                                {0, 224, 224}, {255, 128, 0}, {160, 96, 255}, {255, 255, 255}};

// channel ``c`` of a frame's pixel in colour ``i`` of 0..7; ``rgb``: the bytes are R, G, B (else B, G, R)
__device__ inline uint8_t ov_colour(int i, int c, int rgb) { return OV_PALETTE[i][rgb ? c : 2 - c]; }

// ---- capsules: the pixels within W / 2 of the segment A B

__device__ inline int ov_grow(int W) { return (W + 1) >> 1; }               // no pixel further than this from A B's bounding box is covered

// the box [x_lo, x_hi] x [y_lo, y_hi] grown by g meets the tile; the segment from ax to bx grown by g meets the thread's column
__device__ inline bool ov_meets(int x_lo, int x_hi, int y_lo, int y_hi, int g, const OvTile& t) {
    return x_hi + g >= t.tx0 && x_lo - g <= t.tx1 && y_hi + g >= t.ty0 && y_lo - g <= t.ty1;
}
__device__ inline bool ov_column_near(int ax, int bx, int g, int x) { return x >= min(ax, bx) - g && x <= max(ax, bx) + g; }

struct OvCapsule {                                                         // segment A B as the pixels of column x see it
    long long dx, dy, dd, px, qx, ay, by, r2, bound;
};

__device__ inline OvCapsule ov_capsule(int ax, int ay, int bx, int by, int x, int W) {
    OvCapsule s;
    s.dx = (long long)bx - ax;
    s.dy = (long long)by - ay;
    s.dd = s.dx * s.dx + s.dy * s.dy;
    s.px = (long long)x - ax;
    s.qx = (long long)x - bx;
    s.ay = ay;
    s.by = by;
    s.r2 = (long long)(W * W) >> 2;
    s.bound = ((long long)(W * W) * s.dd) >> 2;
    return s;
}

// Where the capsule covers pixel (x, y), ``dst`` becomes ``v``.  Beside the segment the test is cr^2 <= W^2 dd / 4 for the size cr of the
// cross product.  GUARD: cr is squared only under 2^31.  Lines and zones have 16-bit coordinates (-32768..65535) and W <= 9, so dd <=
// 2 (2^17)^2 = 2^35 and the bound is under 81 * 2^33 < 2^40: a cr of 2^31 or more, whose square is 2^62 or more, is never covered, and
// under 2^31 the square fits.  k_trails_draw goes without the guard, as it always has: the points of the lists that k_trails_update
// writes lie inside the frame, as the pixels do, in 0..32767, so every factor of cr is under 2^15 in size, |cr| < 2^31 and the square
// fits; the guard could not change a result there, and it costs that kernel a fifth of its time (289 us against 238 us on a full list
// over a 600x1000 frame).  A list handed over at the raw ABI holds whatever the caller's memory does; its pixels are the caller's too.
// (The function assigns where one that returned the answer would read better: compiled as a value, the answer is computed without
// branches and in seventeen more scalar registers, and k_count_draw and k_zone_draw would run seven waves a SIMD where they run eight.)
template <bool GUARD>
__device__ inline void capsule_paint(const OvCapsule& s, int y, int& dst, int v) {
    const long long py = (long long)y - s.ay, u = s.px * s.dx + py * s.dy;
    bool cov;
    if (s.dd == 0 || u <= 0) {
        cov = s.px * s.px + py * py <= s.r2;
    } else if (u >= s.dd) {
        const long long qy = (long long)y - s.by;
        cov = s.qx * s.qx + qy * qy <= s.r2;
    } else {
        long long cr = s.px * s.dy - py * s.dx;
        if (GUARD) cr = cr < 0 ? -cr : cr;
        cov = (!GUARD || cr < (1LL << 31)) && cr * cr <= s.bound;
    }
    if (cov) dst = v;
}

// ---- labels: 5 x 7 glyphs drawn at twice their size in cells of 12 x 16 pixels, a black box behind them

// the glyphs a label needs, rows as frcnn_annotate_u8's table has them (bit 4 = the leftmost column): ' ', '+', '-', '/', '0'..'9', 'L', 'Z'
enum { OV_G_SPACE = 0, OV_G_PLUS = 1, OV_G_MINUS = 2, OV_G_SLASH = 3, OV_G_0 = 4, OV_G_L = 14, OV_G_Z = 15 };
static __constant__ uint8_t OV_GLYPHS[16][7] = {
    {0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00}, {0x00, 0x04, 0x04, 0x1F, 0x04, 0x04, 0x00}, {0x00, 0x00, 0x00, 0x1F, 0x00, 0x00, 0x00},
    {0x00, 0x01, 0x02, 0x04, 0x08, 0x10, 0x00},
    {0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E}, {0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E}, {0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F},
    {0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E}, {0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02}, {0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E},
    {0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E}, {0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08}, {0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E},
    {0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C}, {0x10, 0x10, 0x10, 0x10, 0x10, 0x10, 0x1F}, {0x1F, 0x01, 0x02, 0x04, 0x08, 0x10, 0x1F}};
constexpr int OV_COL_BLACK = 8;                                             // a column's colours: -1 untouched, 0..7 the palette, 8 black

// max(value, 0) in decimal behind the ``n`` glyphs of ``t`` -> the glyphs there are then (at most ten more)
__device__ inline int ov_decimal(uint8_t* t, int n, int value) {
    unsigned v = (unsigned)max(value, 0);
    int nd = 1;
    for (unsigned p = v; p >= 10u; p /= 10u) nd += 1;
    for (int i = nd - 1; i >= 0; --i) {
        t[n + i] = (uint8_t)(OV_G_0 + v % 10u);
        v /= 10u;
    }
    return n + nd;
}

// The box of a label of ``n`` glyphs: its top left corner at (mx, my), moved into the frame where the box fits -> it meets the tile.
__device__ inline bool ov_label_place(int n, int mx, int my, int h, int w, const OvTile& t, int& x0, int& y0) {
    const int bw = 12 * n, bh = 16;
    x0 = bw <= w ? min(max(mx, 0), w - bw) : mx;
    y0 = bh <= h ? min(max(my, 0), h - bh) : my;
    return x0 <= t.tx1 && x0 + bw - 1 >= t.tx0 && y0 <= t.ty1 && y0 + bh - 1 >= t.ty0;
}

// The label ``txt`` of ``len`` glyphs at (x0, y0) into this thread's column: ink in ``colour``, the rest of the box black.
__device__ inline void ov_label_blit(const uint8_t* txt, int len, int x0, int y0, int colour, const OvTile& t, int (&col)[OV_TILE_ROWS]) {
    const int rel = t.x - x0;
    if (rel < 0 || rel >= 12 * len) return;
    const int k = (rel - 1) / 12, gx = (rel - 1) - 12 * k;
    const uint8_t* gl = OV_GLYPHS[txt[rel >= 1 ? k : 0]];
#pragma unroll
    for (int r = 0; r < OV_TILE_ROWS; ++r) {
        const int ry = t.ty0 + r - y0;
        if (ry < 0 || ry >= 16) continue;
        const bool ink = rel >= 1 && gx < 10 && ry >= 1 && ry <= 14 && ((gl[(ry - 1) >> 1] >> (4 - (gx >> 1))) & 1);
        col[r] = ink ? colour : OV_COL_BLACK;
    }
}

// ---- the refusals the draw entries share, and the update entries' of the frame

inline int ov_frame_ok(const char* who, int h, int w) {
    if (h < 1 || h > FRCNN_REDACT_MAX_SIDE || w < 1 || w > FRCNN_REDACT_MAX_SIDE)
        return fail(FRCNN_E_ARG, "%s: frame %dx%d out of range (sides 1..%d)", who, h, w, FRCNN_REDACT_MAX_SIDE);
    return FRCNN_OK;
}

inline int ov_width_ok(const char* who, int width, int most) {
    if (width < 1 || width > most) return fail(FRCNN_E_ARG, "%s: width=%d not in [1, %d]", who, width, most);
    return FRCNN_OK;
}

}  // namespace frcnn
