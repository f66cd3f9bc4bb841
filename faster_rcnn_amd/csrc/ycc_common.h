// The Y'CbCr arithmetic every codec of the library shares, stated ONCE: the JFIF colour matrices in 16-bit fixed point (jpeg.hip,
// jpeg_opt.hip: RGB -> YCbCr; jpeg_dec_common.h: YCbCr -> RGB), libjpeg's "fancy" chroma upsampling (the triangle filter 3/4, 1/4 per
// axis: jpeg_dec_common.h) and its 2x2 box average with the alternating bias (jpeg_opt.hip).  y4m.hip runs the same functions on the
// planes of a YUV4MPEG2 frame.  Integers only; an arithmetic right shift of a negative int rounds towards minus infinity, as numpy's.
#pragma once
#include <stdint.h>

namespace frcnn {
namespace {

__device__ __forceinline__ int ycc_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// ------------------------------------------------------------------------------------------------------------- JFIF, full range
// R, G, B in 0..255 -> Y, Cb, Cr in 0..255 (libjpeg's jccolor.c: 16 fractional bits, Cb / Cr rounded with ONE_HALF - 1)
__device__ __forceinline__ void jfif_rgb_to_ycc(int r, int g, int b, int* Y, int* Cb, int* Cr) {
    const int chroma_round = (128 << 16) + 32767;
    *Y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    *Cb = (-11059 * r - 21709 * g + 32768 * b + chroma_round) >> 16;
    *Cr = (32768 * r - 27439 * g - 5329 * b + chroma_round) >> 16;
}

// Y in 0..255, Cb - 128, Cr - 128 -> R, G, B clamped to 0..255 (libjpeg's jdcolor.c)
__device__ __forceinline__ void jfif_ycc_to_rgb(int lum, int cb, int cr, int* r, int* g, int* b) {
    *r = ycc_clamp8(lum + ((91881 * cr + 32768) >> 16));
    *b = ycc_clamp8(lum + ((116130 * cb + 32768) >> 16));
    *g = ycc_clamp8(lum + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
}

// --------------------------------------------------------------------------------------------------- fancy (centred) upsampling
// one axis: the sample next to ``a`` on the side of ``b`` (bias 1 towards the lower index, 2 towards the higher; a == b at an edge)
__device__ __forceinline__ int fancy_tri(int a, int b, int odd) { return (3 * a + b + 1 + odd) >> 2; }

// the row of the plane that lies on the far side of full-size row ``y`` (``rows`` plane rows; the edge rows repeat)
__device__ __forceinline__ int fancy_far_row(int y, int rows) {
    const int yr = y >> 1;
    return (y & 1) ? (yr + 1 < rows ? yr + 1 : rows - 1) : (yr > 0 ? yr - 1 : 0);
}

// full-size column ``x`` of a row ``s`` of ``n`` samples, halved horizontally (h2v1)
__device__ __forceinline__ int fancy_h2v1(const uint8_t* s, int n, int x) {
    const int i = x >> 1;
    if (x == 0 || x == 2 * n - 1) return s[i];
    return fancy_tri(s[i], (x & 1) ? s[i + 1] : s[i - 1], x & 1);
}

// ... halved both ways (h2v2): ``near`` / ``far`` the two plane rows of the full-size row (fancy_far_row); 9-3-3-1 over 16
__device__ __forceinline__ int fancy_h2v2(const uint8_t* near, const uint8_t* far, int n, int x) {
    const int i = x >> 1;
    const int cs = 3 * near[i] + far[i];
    if (x == 0) return (4 * cs + 8) >> 4;
    if (x == 2 * n - 1) return (4 * cs + 7) >> 4;
    return (x & 1) ? (3 * cs + 3 * near[i + 1] + far[i + 1] + 7) >> 4 : (3 * cs + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
}

// ------------------------------------------------------------------------------------------------------------- 2x2 box average
// the sum of a 2x2 group's four samples -> their average; libjpeg's h2v2_downsample: bias 1 at even, 2 at odd output columns
__device__ __forceinline__ int box2x2(int sum, int out_col) { return (sum + 1 + (out_col & 1)) >> 2; }

}  // namespace
}  // namespace frcnn
