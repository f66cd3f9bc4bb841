/* Class-sorted row tiles for a convolution with zero padding: an EXTENSION of the C ABI of libfrcnn_hip.so (include/frcnn_hip.h, whose
 * revision and symbol table stay as they are: FRCNN_ABI_VERSION 110; the other extension headers likewise).  The entry points below
 * live in the same library, follow the same conventions (int status, message via frcnn_last_error, `stream` = hipStream_t or NULL) and
 * carry a revision of their own: a host that uses them checks frcnn_rowmap_version() == FRCNN_ROWMAP_VERSION besides frcnn_version().
 *   1 = frcnn_conv_rowmap_build, frcnn_conv2d_rowmap_available, frcnn_conv2d_fwd_h3_rowmap. */
#ifndef FRCNN_HIP_ROWMAP_H
#define FRCNN_HIP_ROWMAP_H
#include <stdint.h>
#include "../frcnn_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_ROWMAP_VERSION 1
int frcnn_rowmap_version(void);

/* Class order inside a super-group of images: as the classes first appear in raster order of the output positions, or the classes
 * with the most taps first (ties: first appearance). */
#define FRCNN_ROWMAP_ORDER_RASTER 0
#define FRCNN_ROWMAP_ORDER_LONG_FIRST 1

/* A layout-0 launch computes output row m = (img, ho, wo) in row tile m / tile_rows, so with small images ([roi][7][7][c] crops) every
 * tile holds every position and needs every filter tap, although for most rows some taps meet zero padding only.  A ROW MAP re-assigns
 * rows to tiles: tile row j computes output row row_map[j] (-1: none), and the rows are ordered
 *     [super-group of `tile_rows` images][class][image][position within class]
 * where the CLASS of an output position is the set of filter taps that meet the image there (bit r * kw + s; a position that meets
 * none counts as meeting all).  Every class of a full super-group fills whole tiles; the last, partial super-group pads each class
 * to a tile boundary with -1.  tile_taps[t] is the union of the classes of tile t's rows: the taps the tile has to walk.  The tensors
 * keep their layout; per output row the launch sums the same products in the same order, minus terms that were exactly zero.
 *
 * Host code, no device needed; depends on the shape only (n, ho, wo, h, w, kh, kw, stride, pads, tile_rows, order), so a caller
 * builds it once per shape.  row_map (int32, `map_capacity` words) and tile_taps (uint32, `taps_capacity` words) are HOST buffers and
 * may both be NULL to ask for the sizes only.  *rows_out (a multiple of tile_rows) and *tap_tiles_out (the sum over the tiles of their
 * tap counts) are always written when given.
 * Returns 1: the map saves tap-tiles against the unmapped launch (ceil(n * ho * wo / tile_rows) tiles of kh * kw taps);
 *         0: NOT AVAILABLE, it saves none (1x1 filters, no padding, too few images) -- the buffers, when given, still hold a valid map;
 *         negative: error (bad shape, layout 1, more than 32 taps, 2^31 rows or more, a buffer too small). */
int frcnn_conv_rowmap_build(const frcnn_conv_desc* d, int tile_rows, int order, int32_t* row_map, size_t map_capacity,
                            uint32_t* tile_taps, size_t taps_capacity, int64_t* rows_out, int64_t* tap_tiles_out);

/* Does frcnn_conv2d_fwd_h3_rowmap take this descriptor?  1 / 0 (negative: error).  Only the f16x3 engine's 256x128 form on sixteen
 * waves reading fp16 planes has the mode (frcnn_conv2d_h3_config 86, x_is_planes != 0; the mapped launch walks the three-stage ring
 * whatever the reduction's length), for layout 0, un-split, dense rows (ldy = ldres = 0), cin % 32 == 0, cout % 4 == 0, at most 32 taps.  Says
 * nothing about whether a map PAYS: that is frcnn_conv_rowmap_build's answer, with tile_rows = 256.  The launch policy never picks
 * the mode: a caller asks for it through the entry point below. */
int frcnn_conv2d_rowmap_available(const frcnn_conv_desc* d, int engine, int x_is_planes);

/* The map of a launch, in DEVICE memory: what frcnn_conv_rowmap_build(d, 256, ...) wrote. */
typedef struct frcnn_rowmap {
    const int32_t* row_map;      /* [rows] */
    const uint32_t* tile_taps;   /* [rows / 256] */
    int32_t rows;                /* a positive multiple of 256 */
    int32_t reserved;            /* 0 */
} frcnn_rowmap;

/* frcnn_conv2d_fwd_h3_planes (plane input, no residual) with its rows assigned to tiles by `map`.  Inputs and outputs are those of the
 * unmapped launch, in the same layout, and so are the results, bit for bit, and the magnitude record (a maximum over the same values).
 * The map is trusted: every value of row_map must be -1 or a row index below n * ho * wo, each row once, and tile_taps[t] must cover
 * the taps of tile t's rows (a missing tap bit drops products).  FRCNN_E_UNSUPPORTED wherever frcnn_conv2d_rowmap_available answers
 * 0; nothing is launched on a refusal. */
int frcnn_conv2d_fwd_h3_rowmap(const frcnn_conv_desc* d, const frcnn_h3_planes* x_planes, const float* x_amax, const void* w_planes_f16,
                               const float* scale, const float* shift, float* y, float* y_amax, const frcnn_h3_planes* y_planes,
                               float bound_c, float bound_d, const frcnn_rowmap* map, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_ROWMAP_H */
