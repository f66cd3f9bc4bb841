// What csrc/redact_shape.hip shares with csrc/redact.hip: frcnn_redact_u8's argument checks, the tiling of phase two and the launch of
// phase one (a kernel is launched from the translation unit that defines it).
#pragma once
#include "common.h"
#include "../../include/ext/frcnn_hip_redact.h"

namespace frcnn {

constexpr int RD_THREADS = 256;                                             // a tile of phase two: 256 byte columns ...
constexpr int RD_TILE_ROWS = 16;                                            // ... x 16 rows, threads as bytes

// FRCNN_OK, or FRCNN_E_ARG with the message set under the name ``who``: everything frcnn_redact_u8 refuses
int redact_check(const char* who, const uint8_t* frame, int h, int w, const int32_t* det_bbox, const int32_t* det_cls, const int32_t* n_dets,
                 int max_rows, const uint8_t* redact, int num_classes, int mode, int size, int margin, const void* workspace,
                 size_t ws_bytes);

// Phase one on ``stream``: the cell means (PIXELATE) or the horizontal blur stage H (BLUR) of the whole frame into ``workspace``; no
// launch for FILL.  With *n_dets <= 0 nothing is written.  FRCNN_OK, or the launch's error under the name ``who``.
int redact_phase_one(const char* who, const uint8_t* frame, int h, int w, const int32_t* n_dets, int mode, int size, void* workspace,
                     hipStream_t stream);

}  // namespace frcnn
