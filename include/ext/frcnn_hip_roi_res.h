/* The RoI-resampled shortcut gathered inside a convolution's epilogue: an EXTENSION of the C ABI of libfrcnn_hip.so (include/frcnn_hip.h,
 * whose revision and symbol table stay as they are: FRCNN_ABI_VERSION 110).  The entry points below live in the same library, follow
 * the same conventions (int status, message via frcnn_last_error, `stream` = hipStream_t or NULL) and carry a revision of their own: a
 * host that uses them checks frcnn_roi_res_version() == FRCNN_ROI_RES_VERSION besides frcnn_version().
 *   1 = frcnn_roi_tap_table, frcnn_conv2d_roi_res_available, frcnn_conv2d_fwd_h3_roi_res. */
#ifndef FRCNN_HIP_ROI_RES_H
#define FRCNN_HIP_ROI_RES_H
#include <stdint.h>
#include "../frcnn_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_ROI_RES_VERSION 1
int frcnn_roi_res_version(void);

/* The residual of a launch whose output rows are RoI samples (row m = sample (roi, py, px)): instead of the resampled tensor
 * frcnn_roi_crop_resize_fwd_ex / _fwd_batch would write -- [rows][cout] f32, read back once -- the launch reads the MAP itself and a
 * table of taps, and forms each 16-byte piece of the residual in its epilogue:
 *     top = tl + (tr - tl) * tx;  bot = bl + (br - bl) * tx;  v = top + (bot - top) * ty          (no contraction: k_roi_fwd's roundings)
 * or the piece of `fill` for a rejected RoI.  Bit for bit the tensor the resampling launch writes (relu = 0), so the launch's result
 * is bit for bit that of the same launch with `residual` = that tensor.
 * map      [map_rows][cout] f32, 16-byte aligned, dense: the maps of all images one after the other (map_rows = images * rows * cols)
 * taps     frcnn_roi_tap_table's records, one per output row, in the launch's row order
 * fill     [cout] f32, 16-byte aligned, or NULL (zeros) */
typedef struct frcnn_roi_res {
    const float* map;
    const void* taps;
    const float* fill;
    int32_t map_rows;
    int32_t reserved;      /* 0 */
} frcnn_roi_res;

#define FRCNN_ROI_TAP_BYTES 32
/* One 32-byte record per sample into taps [n * pool * pool] (16-byte aligned): int32 tl, tr, bl, br -- ELEMENT offsets of the four
 * source rows in a map of `c` channels, image offset ((r / n_per_img) * rows * cols rows) included when n_per_img > 0 --, f32 tx, ty,
 * int32 ok (0: the RoI is rejected, offsets 0) and a zero word.  Row order: layout 0 = [roi][py][px], layout 1 = [py][px][roi]
 * (frcnn_conv_desc.layout).  The predicate and the arithmetic are those of frcnn_roi_crop_resize_fwd_ex.  n_per_img > 0 needs
 * n <= n_maps * n_per_img; n_per_img == 0: one map (n_maps is ignored).  One kernel, nothing zero-filled: safe to capture. */
int frcnn_roi_tap_table(int rows, int cols, int c, const float* rois, int n, int n_per_img, int n_maps, int pool, int layout,
                        void* taps, void* stream);

/* Would frcnn_conv2d_fwd_h3_roi_res take this descriptor?  1 / 0 (negative: error).  Only the f16x3 engine's 256x128 form on sixteen
 * waves has the mode (frcnn_conv2d_h3_config 86 / 85), un-split, inference, dense rows (ldy = ldres = 0), cout % 4 == 0, and not the
 * three-stage ring that plane input takes on a long reduction: every other engine (`engine`: FRCNN_ENGINE_*), tile and form answers 0. */
int frcnn_conv2d_roi_res_available(const frcnn_conv_desc* d, int engine, int x_is_planes);

/* frcnn_conv2d_fwd_h3_planes_res with the residual gathered from `res` (above).  With y_planes, residual_amax must bound the
 * resampled tensor: max(|map|, |fill|), frcnn_amax_merge of the map's record with max|fill|.  FRCNN_E_UNSUPPORTED where
 * frcnn_conv2d_roi_res_available answers 0. */
int frcnn_conv2d_fwd_h3_roi_res(const frcnn_conv_desc* d, const float* x, const frcnn_h3_planes* x_planes, const float* x_amax,
                                const void* w_planes_f16, const float* scale, const float* shift, const frcnn_roi_res* res,
                                const float* residual_amax, float* y, float* y_amax, const frcnn_h3_planes* y_planes,
                                float bound_c, float bound_d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_ROI_RES_H */
