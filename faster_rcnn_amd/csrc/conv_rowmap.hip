// Class-sorted row tiles (include/ext/frcnn_hip_rowmap.h), host code only: the map that assigns the output rows of a layout-0
// convolution to row tiles so that a tile as a whole needs fewer filter taps, and the taps each tile walks.  conv_h3.hip's mapped ring
// instantiation (h3_ring_tile<.., ROWMAP>) reads both; conv_igemm.hip holds the launch's entry point beside the other launches'.
#include <vector>
#include "common.h"
#include "../../include/ext/frcnn_hip_rowmap.h"

namespace frcnn {

// the taps of filter (kh, kw) that meet the image at output position (ho, wo): bit r * kw + s; none -> all (h3_tap_mask's convention)
static uint32_t rowmap_class(const frcnn_conv_desc* d, int ho, int wo) {
    const int RS = d->kh * d->kw;
    const uint32_t all_taps = RS >= 32 ? 0xffffffffu : (1u << RS) - 1u;
    const int h0 = ho * d->stride - d->pad_top, w0 = wo * d->stride - d->pad_left;
    uint32_t mk = 0;
    for (int r = 0; r < d->kh; ++r)
        for (int s = 0; s < d->kw; ++s)
            if ((unsigned)(h0 + r) < (unsigned)d->h && (unsigned)(w0 + s) < (unsigned)d->w) mk |= 1u << (r * d->kw + s);
    return mk ? mk : all_taps;
}

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_rowmap_version(void) { return FRCNN_ROWMAP_VERSION; }

extern "C" int frcnn_conv_rowmap_build(const frcnn_conv_desc* d, int tile_rows, int order, int32_t* row_map, size_t map_capacity,
                                       uint32_t* tile_taps, size_t taps_capacity, int64_t* rows_out, int64_t* tap_tiles_out) {
    if (!d) return fail(FRCNN_E_ARG, "conv_rowmap_build: null descriptor");
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->kh <= 0 || d->kw <= 0 || d->stride <= 0 || d->ho <= 0 || d->wo <= 0 || d->pad_top < 0 || d->pad_left < 0)
        return fail(FRCNN_E_ARG, "conv_rowmap_build: bad shape");
    if (tile_rows <= 0 || tile_rows > 65536) return fail(FRCNN_E_ARG, "conv_rowmap_build: tile_rows out of range");
    if (order != FRCNN_ROWMAP_ORDER_RASTER && order != FRCNN_ROWMAP_ORDER_LONG_FIRST) return fail(FRCNN_E_ARG, "conv_rowmap_build: unknown order %d", order);
    if (d->layout) return fail(FRCNN_E_UNSUPPORTED, "conv_rowmap_build: layout 0 only (position-major rows skip taps per tile already)");
    if (d->kh * d->kw > 32) return fail(FRCNN_E_UNSUPPORTED, "conv_rowmap_build: at most 32 taps");
    if ((row_map == nullptr) != (tile_taps == nullptr)) return fail(FRCNN_E_ARG, "conv_rowmap_build: both buffers or neither");
    const long long npos = (long long)d->ho * d->wo, M = npos * d->n;
    if (npos > 0x7fffffffLL || M > 0x7fffffffLL) return fail(FRCNN_E_UNSUPPORTED, "conv_rowmap_build: 2^31 output rows or more");

    // the classes, in raster order of first appearance, and the positions of each in raster order
    struct Class { uint32_t taps; std::vector<int> pos; };
    std::vector<Class> classes;
    for (int pos = 0; pos < (int)npos; ++pos) {
        const uint32_t mk = rowmap_class(d, pos / d->wo, pos % d->wo);
        size_t c = 0;
        while (c < classes.size() && classes[c].taps != mk) ++c;
        if (c == classes.size()) classes.push_back({mk, {}});
        classes[c].pos.push_back(pos);
    }
    if (order == FRCNN_ROWMAP_ORDER_LONG_FIRST) {           // most taps first; stable: ties stay in order of first appearance
        for (size_t i = 1; i < classes.size(); ++i)
            for (size_t j = i; j > 0 && __builtin_popcount(classes[j].taps) > __builtin_popcount(classes[j - 1].taps); --j) std::swap(classes[j], classes[j - 1]);
    }

    // sizes first: a super-group holds tile_rows images, so every class of a full one fills whole tiles
    const long long G = tile_rows;
    long long rows = 0, tap_tiles = 0;
    for (long long g0 = 0; g0 < d->n; g0 += G) {
        const long long g = d->n - g0 < G ? d->n - g0 : G;
        for (const Class& c : classes) {
            const long long t = ((long long)c.pos.size() * g + tile_rows - 1) / tile_rows;
            rows += t * tile_rows;
            tap_tiles += t * __builtin_popcount(c.taps);
        }
    }
    if (rows > 0x7fffffffLL) return fail(FRCNN_E_UNSUPPORTED, "conv_rowmap_build: 2^31 mapped rows or more");
    if (rows_out) *rows_out = rows;
    if (tap_tiles_out) *tap_tiles_out = tap_tiles;
    const long long plain = (M + tile_rows - 1) / tile_rows * (d->kh * d->kw);       // layout 0 unmapped: every tile walks every tap
    const int pays = tap_tiles < plain ? 1 : 0;
    if (!row_map) return pays;
    if ((long long)map_capacity < rows || (long long)taps_capacity < rows / tile_rows)
        return fail(FRCNN_E_ARG, "conv_rowmap_build: buffers too small (%lld rows, %lld tiles)", rows, rows / tile_rows);

    long long j = 0;
    for (long long g0 = 0; g0 < d->n; g0 += G) {
        const long long g = d->n - g0 < G ? d->n - g0 : G;
        for (const Class& c : classes) {
            const long long first = j;
            for (long long img = g0; img < g0 + g; ++img)
                for (int pos : c.pos) row_map[j++] = (int32_t)(img * npos + pos);
            while (j % tile_rows) row_map[j++] = -1;
            for (long long t = first / tile_rows; t < j / tile_rows; ++t) tile_taps[t] = c.taps;    // (a tile never holds two classes: each is padded to a boundary)
        }
    }
    return pays;
}
