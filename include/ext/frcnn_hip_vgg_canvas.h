/* VGG16 canvas passes: an EXTENSION of the C ABI of libfrcnn_hip.so (include/frcnn_hip.h, whose revision and symbol table stay as they
 * are: FRCNN_ABI_VERSION 110).  The entry points below live in the same library, follow the same conventions (int status, message via
 * frcnn_last_error, `stream` = hipStream_t or NULL) and carry a revision of their own: a host that uses them checks
 * frcnn_vgg_canvas_version() == FRCNN_VGG_CANVAS_VERSION besides frcnn_version().
 *   1 = frcnn_pool2d_fwd_extents, frcnn_pool2d_fwd_bf16_extents, frcnn_vgg_conv1_bf16_fwd_extents. */
#ifndef FRCNN_HIP_VGG_CANVAS_H
#define FRCNN_HIP_VGG_CANVAS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_VGG_CANVAS_VERSION 1
int frcnn_vgg_canvas_version(void);

/* VGG16 on padded canvases (images of different true sizes in one pass of fixed shape; each image sits at offset (0, 0) of its canvas:
 * no VGG16 layer's padding depends on the size, vgg.py:91-141).  true_hw [n][2] int32 DEVICE words = image i's true {rows, cols} at the
 * level of the INPUT tensor, read by the kernel (a captured launch serves every size of its canvas class); values beyond the canvas are
 * clamped.
 * frcnn_pool2d_fwd_extents / frcnn_pool2d_fwd_bf16_extents: the 2x2 / stride-2 max-pool (vgg.py:100, 108, 118, 128) of x [n][hc][wc][c]
 * (c % 4 == 0 f32, c % 8 == 0 bf16, 16-byte aligned) into y [n][hc/2][wc/2][c].  A cell inside floor(rows/2) x floor(cols/2) is
 * bit-identical to frcnn_pool2d_fwd / frcnn_pool2d_fwd_bf16 on the true-size tensor; EVERY other cell is written as zero and x is not
 * read for it (so x need not be masked: whatever lies beyond the true extent never gets through), including the row / column
 * floor(rows/2) / floor(cols/2) of an odd side, which VALID pooling drops.
 * frcnn_vgg_conv1_bf16_fwd_extents: frcnn_vgg_conv1_bf16_fwd (vgg.py:96-97) on canvases x [n][hc][wc][3]: inside image i's true extent
 * bit-identical to that launch on the true-size image (SAME padding is read as zeros at the TRUE border, whatever the canvas holds
 * beyond it), every other cell of out [n][hc][wc][64] is stored as zero. */
int frcnn_pool2d_fwd_extents(const float* x, int n, int hc, int wc, int c, const int32_t* true_hw, float* y, void* stream);
int frcnn_pool2d_fwd_bf16_extents(const void* x_bf16, int n, int hc, int wc, int c, const int32_t* true_hw, void* y_bf16, void* stream);
int frcnn_vgg_conv1_bf16_fwd_extents(const float* x, int n, int hc, int wc, const void* w_packed_bf16, const float* bias, const int32_t* true_hw,
                                     void* out_bf16, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_VGG_CANVAS_H */
