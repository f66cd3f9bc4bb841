/* The average pool behind a convolution taken inside that convolution's epilogue: an EXTENSION of the C ABI of libfrcnn_hip.so
 * (include/frcnn_hip.h, whose revision and symbol table stay as they are: FRCNN_ABI_VERSION 110; include/ext/frcnn_hip_roi_res.h and the
 * other extension headers likewise).  The entry points below live in the same library, follow the same conventions (int status, message
 * via frcnn_last_error, `stream` = hipStream_t or NULL) and carry a revision of their own: a host that uses them checks
 * frcnn_pool_epilogue_version() == FRCNN_POOL_EPILOGUE_VERSION besides frcnn_version().
 *   1 = frcnn_conv2d_pool_available, frcnn_conv2d_fwd_h3_pool. */
#ifndef FRCNN_HIP_POOL_EPILOGUE_H
#define FRCNN_HIP_POOL_EPILOGUE_H
#include <stdint.h>
#include "../frcnn_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_POOL_EPILOGUE_VERSION 1
int frcnn_pool_epilogue_version(void);

/* A 1x1 convolution whose output rows come in groups of `window` consecutive rows (the samples of one RoI in the
 * [roi][py][px][c] layout: window = pool * pool) and whose ONLY reader is the average over each group: instead of the
 * [rows][cout] f32 tensor the launch would write and frcnn_pool2d_fwd (is_max = 0) would read back once, the launch keeps each group
 * inside one workgroup and writes y [rows / window][cout]:
 *     acc = 0.0f;  acc += v[g * window + r] for r = 0 .. window - 1, in that order;  y[g] = acc / (float)window
 * with v what the plain launch stores (scale, shift, residual, activation) -- the additions and the division of frcnn_pool2d_fwd, so
 * the result is bit for bit that of the two launches.  y_amax, when given, receives max |y| of the POOLED values.
 *
 * Would frcnn_conv2d_fwd_h3_pool take this descriptor?  1 / 0 (negative: error).  Only the f16x3 engine's 256x128 form on sixteen
 * waves reading fp16 planes has the mode (frcnn_conv2d_h3_config 86 / 85, x_is_planes != 0), and only for: kh = kw = 1, stride 1, no
 * padding, layout 0, un-split, dense rows (ldy = ldres = 0), cin % 32 == 0, cout % 4 == 0, 1 <= window <= 256 dividing the row count,
 * and not the three-stage ring that plane input takes on a long reduction.  Every other engine (`engine`: FRCNN_ENGINE_*), tile and
 * form answers 0. */
int frcnn_conv2d_pool_available(const frcnn_conv_desc* d, int engine, int x_is_planes, int window);

/* frcnn_conv2d_fwd_h3_planes_res with the average over groups of `window` rows taken in the epilogue: y is [rows / window][cout] f32,
 * 16-byte aligned.  `residual`: NULL or the plain f32 tensor [rows][cout], 16-byte aligned.  The arguments the mode does not have are
 * part of the signature so that a host cannot pass them by mistake: x (f32 activations), residual_planes, mask and y_planes must be
 * NULL -- FRCNN_E_UNSUPPORTED otherwise, and wherever frcnn_conv2d_pool_available answers 0.  Nothing is launched on a refusal. */
int frcnn_conv2d_fwd_h3_pool(const frcnn_conv_desc* d, const float* x, const frcnn_h3_planes* x_planes, const float* x_amax,
                             const void* w_planes_f16, const float* scale, const float* shift, const float* residual,
                             const frcnn_h3_planes* residual_planes, const float* mask, int window, float* y, float* y_amax,
                             const frcnn_h3_planes* y_planes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_POOL_EPILOGUE_H */
