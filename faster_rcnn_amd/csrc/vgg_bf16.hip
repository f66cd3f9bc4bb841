// The two launches the bf16 conv path lacked for VGG16 (gfx950): block1_conv1 on the bf16 matrix cores and a bf16 max-pool.
//
// k_vgg_conv1_bf16 -- Conv2D(64, (3,3), activation='relu', padding='same', name='block1_conv1') (vgg.py:96-97): f32 NHWC image in (after
// vgg.preprocess), bf16 NHWC map out.  The arithmetic model is the bf16 ResNet stem's (stem_bf16.hip): pixels and filter taps rounded to
// bf16 once (nearest even), products accumulated in f32, bias and ReLU in f32, one rounding at the store.
//
// Bound: the STORE.  A 600 x 1000 image writes 600 * 1000 * 64 * 2 B = 76.8 MB and reads 7.2 MB; the 27-long reduction padded to 32 is
// ONE v_mfma_f32_16x16x32_bf16 per 16 pixels x 16 channels, four per 16 pixels (0.44 GFLOP-equivalent per image: nothing).  So the
// kernel is laid out for its store and everything else is kept simple:
//   * the filter is the A operand (rows = channels), the pixels the B operand (columns = pixels), so a lane's four accumulator
//     registers are four CHANNELS of ONE pixel (C/D map: col = lane & 15, row = 4 (lane >> 4) + reg).  The filter rows of the four MFMAs
//     are permuted (MFMA (h, t), row 4 g + r = channel 32 h + 8 g + 4 t + r) so that lane group g = lane >> 4 ends up with the eight
//     CONTIGUOUS channels 32 h + 8 g .. + 7 of its pixel in the two accumulators (h, 0), (h, 1): one 16-byte store per lane and h, and
//     the two stores of a wave cover 16 whole 128-byte pixels.
//   * a workgroup (4 waves) owns a run of 256 pixels of ONE image row; a wave owns 64 of them (four MFMA groups of 16).  The three input
//     rows under the run (258 pixels x 3 channels each) go through LDS rather than through per-lane global loads: every input value is
//     needed by nine output pixels and by a different k slot in each, so staging converts each value to bf16 once, applies the SAME
//     padding (zeros outside the image) once, and leaves the gather as eight unconditional 2-byte LDS reads per lane and group --
//     per-lane global gathers would be 8 bounds-checked 4-byte loads through the texture path the stores need.
//   * k order: k = (r * 3 + s) * 3 + c for filter row r, column s, channel c (HWIO order), k = 27..31 zero on BOTH operands (the pixel
//     fragment selects 0 there: nothing finite or not from a neighbouring pixel is multiplied by the zero taps).
//   * all offsets into the image and the map are 64-bit (block 1's map is 614 MB at eight images per pass).
//
// k_pool2_bf16 -- MaxPooling2D((2,2), strides=(2,2)) (vgg.py:100, 108, 118, 128), VALID: odd trailing rows / columns are dropped.  Eight
// channels per thread, 16-byte loads and stores.  The maximum of bf16 values is exact: no tolerance.  A later value replaces the running
// maximum only when it is strictly greater or a NaN, so a window that holds both -0.0 and +0.0 (and nothing positive) yields whichever
// of the two comes FIRST in (row, column) order, and a NaN in the window propagates.
#include "common.h"
#include "../../include/ext/frcnn_hip_vgg_canvas.h"

namespace frcnn {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

constexpr int VC_RUN = 256;                       // pixels of one image row per workgroup (64 per wave)
constexpr int VC_ROW = (VC_RUN + 2) * 3 + 2;      // staged bf16 per input row: 258 pixels x 3 channels (+ pad: 776)
constexpr int VC_STAGE = 3 * VC_ROW;              // 2328 values
constexpr int VC_NP = (VC_STAGE + 255) / 256;     // staging loads per thread
constexpr int VC_PACKED = 4 * 64 * 8;             // packed filter: [MFMA f = 2 h + t][lane][8] bf16

//
// EXT (frcnn_vgg_conv1_bf16_fwd_extents, a canvas pass): x and out are canvases [H][W]; image img occupies the top-left hw[2 img] x
// hw[2 img + 1] cells (device words, clamped to the canvas).  Staging reads zeros at and beyond the TRUE extent -- the padding a pass of
// the image's own size reads there, whatever the canvas holds -- so a cell inside the extent sees the operands of that pass in the same
// k slots: bit-identical.  Every other cell of the canvas is stored as zero (block1_conv2 is a 3x3 too); a run wholly outside the
// extent stores its zeros and leaves before the staging.  EXT = false compiles to the kernel as it was.
template <bool EXT>
__global__ void __launch_bounds__(256) k_vgg_conv1_bf16(const float* __restrict__ x, const bf16x8* __restrict__ wp, const float* __restrict__ bias,
                                                        int H, int W, const int* __restrict__ hw, __bf16* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) unsigned short rows[VC_STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = lane & 15, g = lane >> 4;
    const int x0 = blockIdx.x * VC_RUN, y = blockIdx.y, img = blockIdx.z;
    const float* xi = x + (size_t)img * H * W * 3;
    const int Ht = EXT ? max(0, min(hw[2 * img], H)) : H, Wt = EXT ? max(0, min(hw[2 * img + 1], W)) : W;      // the image's true extent
    if (EXT && (y >= Ht || x0 >= Wt)) {                        // (workgroup-uniform) nothing of the image under this run: zeros only
        u16x8* o = reinterpret_cast<u16x8*>(out + (((size_t)img * H + y) * (size_t)W + x0) * 64);
        const int n = min(VC_RUN, W - x0) * 8;
        const u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = tid; k < n; k += 256) o[k] = z;
        return;
    }

    // ---- stage rows y - 1 .. y + 1, pixels x0 - 1 .. x0 + 256 (f32 -> bf16 once, zeros outside the image: SAME padding).  All of a
    // thread's loads are issued before the first is used (as in the stem: a load -> convert -> store loop is a chain of round trips).
    float pv[VC_NP];
#pragma unroll
    for (int q = 0; q < VC_NP; ++q) {
        const int idx = tid + q * 256;
        const int r = idx / VC_ROW, col = idx - r * VC_ROW;
        const int gy = y - 1 + r, gx = x0 - 1 + col / 3;
        const bool ok = idx < VC_STAGE && col < (VC_RUN + 2) * 3 && (unsigned)gy < (unsigned)Ht && (unsigned)gx < (unsigned)Wt;
        pv[q] = ok ? xi[((size_t)gy * W + gx) * 3 + (col - (col / 3) * 3)] : 0.0f;
    }
#pragma unroll
    for (int q = 0; q < VC_NP; ++q) {
        const int idx = tid + q * 256;
        if (idx < VC_STAGE) rows[idx] = __builtin_bit_cast(unsigned short, (__bf16)pv[q]);
    }

    // ---- the whole filter and the bias live in registers: 4 fragments of 8 bf16, 16 floats
    bf16x8 fa[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) fa[f] = wp[f * 64 + lane];
    float bs[2][8];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 8; ++e) bs[h][e] = bias[32 * h + 8 * g + e];
    // this lane's eight k slots: k = 8 g + j -> filter row k / 9, offset k % 9 inside the nine contiguous values of that row
    int koff[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = 8 * g + j, r = k / 9;
        koff[j] = k < 27 ? r * VC_ROW + (k - 9 * r) : -1;
    }
    __syncthreads();

    __bf16* orow = out + ((size_t)img * H + y) * (size_t)W * 64;
#pragma unroll
    for (int grp = 0; grp < 4; ++grp) {
        const int px = wave * 64 + grp * 16 + p;                 // pixel of the run; staged pixel 0 is image column x0 - 1
        if (x0 + wave * 64 + grp * 16 >= W) break;               // (wave-uniform: the whole group lies beyond the row)
        u16x8 bv;
#pragma unroll
        for (int j = 0; j < 8; ++j) bv[j] = koff[j] >= 0 ? rows[koff[j] + px * 3] : (unsigned short)0;
        const bf16x8 fb = __builtin_bit_cast(bf16x8, bv);
        f32x4 acc[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
            acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[f], fb, z, 0, 0, 0);
        }
        if (x0 + px < W) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                u16x8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    o[e] = __builtin_bit_cast(unsigned short, (__bf16)fmaxf(acc[2 * h + (e >> 2)][e & 3] + bs[h][e], 0.0f));
                if (EXT && x0 + px >= Wt) o = u16x8{0, 0, 0, 0, 0, 0, 0, 0};      // on the canvas, beyond the image's last column
                *reinterpret_cast<u16x8*>(orow + (size_t)(x0 + px) * 64 + 32 * h + 8 * g) = o;
            }
        }
    }
}

// HWIO f32 [3][3][3][64] -> the four A fragments: element j of lane l of MFMA f = 2 h + t is tap k = 8 (l >> 4) + j of channel
// 32 h + 8 ((l & 15) >> 2) + 4 t + (l & 3); zero for k >= 27
__global__ void k_pack_vgg_conv1_bf16(const float* w, __bf16* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= VC_PACKED) return;
    const int j = i & 7, l = (i >> 3) & 63, f = i >> 9, h = f >> 1, t = f & 1;
    const int m = l & 15, k = 8 * (l >> 4) + j, ch = 32 * h + 8 * (m >> 2) + 4 * t + (m & 3);
    out[i] = k < 27 ? (__bf16)w[k * 64 + ch] : (__bf16)0.0f;
}

__global__ void __launch_bounds__(256) k_pool2_bf16(const u16x8* __restrict__ x, int n_img, int H, int W, int C8, int Ho, int Wo, u16x8* __restrict__ y) {
    const size_t total = (size_t)n_img * Ho * Wo * C8;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C8);
        size_t t = i / C8;
        const int wo = (int)(t % Wo); t /= Wo;
        const int ho = (int)(t % Ho);
        const int img = (int)(t / Ho);
        const u16x8* base = x + (((size_t)img * H + 2 * ho) * W + 2 * wo) * C8 + c;
        const u16x8 v[4] = {base[0], base[C8], base[(size_t)W * C8], base[(size_t)W * C8 + C8]};
        u16x8 best = v[0];
#pragma unroll
        for (int q = 1; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float a = __uint_as_float((unsigned)v[q][e] << 16), b = __uint_as_float((unsigned)best[e] << 16);
                best[e] = (a > b || a != a) ? v[q][e] : best[e];
            }
        y[i] = best;
    }
}

}  // namespace frcnn

using namespace frcnn;

extern "C" {

int frcnn_vgg_conv1_bf16_packed_elems(void) { return VC_PACKED; }

int frcnn_pack_vgg_conv1_weights_bf16(const float* w_hwio, void* packed_bf16, void* stream) {
    if (!w_hwio || !packed_bf16) return fail(FRCNN_E_ARG, "pack_vgg_conv1_weights_bf16: null pointer");
    k_pack_vgg_conv1_bf16<<<VC_PACKED / 256, 256, 0, as_stream(stream)>>>(w_hwio, (__bf16*)packed_bf16);
    return check_launch("pack_vgg_conv1_weights_bf16");
}

int frcnn_vgg_conv1_bf16_fwd(const float* x, int n, int h, int w, const void* w_packed_bf16, const float* bias, void* out_bf16, void* stream) {
    if (!x || !w_packed_bf16 || !bias || !out_bf16) return fail(FRCNN_E_ARG, "vgg_conv1_bf16_fwd: null pointer");
    if (n <= 0 || h <= 0 || w <= 0) return fail(FRCNN_E_ARG, "vgg_conv1_bf16_fwd: bad shape");
    if ((reinterpret_cast<uintptr_t>(w_packed_bf16) | reinterpret_cast<uintptr_t>(out_bf16)) & 15) return fail(FRCNN_E_ARG, "vgg_conv1_bf16_fwd: 16-byte aligned tensors");
    if (h > 65535 || n > 65535) return fail(FRCNN_E_UNSUPPORTED, "vgg_conv1_bf16_fwd: at most 65535 rows and 65535 images per launch");
    const dim3 grid((w + VC_RUN - 1) / VC_RUN, h, n);
    k_vgg_conv1_bf16<false><<<grid, 256, 0, as_stream(stream)>>>(x, (const bf16x8*)w_packed_bf16, bias, h, w, nullptr, (__bf16*)out_bf16);
    return check_launch("vgg_conv1_bf16_fwd");
}

int frcnn_vgg_conv1_bf16_fwd_extents(const float* x, int n, int hc, int wc, const void* w_packed_bf16, const float* bias, const int32_t* true_hw,
                                     void* out_bf16, void* stream) {
    if (!x || !w_packed_bf16 || !bias || !true_hw || !out_bf16) return fail(FRCNN_E_ARG, "vgg_conv1_bf16_fwd_extents: null pointer");
    if (n <= 0 || hc <= 0 || wc <= 0) return fail(FRCNN_E_ARG, "vgg_conv1_bf16_fwd_extents: bad shape");
    if ((reinterpret_cast<uintptr_t>(w_packed_bf16) | reinterpret_cast<uintptr_t>(out_bf16)) & 15) return fail(FRCNN_E_ARG, "vgg_conv1_bf16_fwd_extents: 16-byte aligned tensors");
    if (hc > 65535 || n > 65535) return fail(FRCNN_E_UNSUPPORTED, "vgg_conv1_bf16_fwd_extents: at most 65535 rows and 65535 images per launch");
    const dim3 grid((wc + VC_RUN - 1) / VC_RUN, hc, n);
    k_vgg_conv1_bf16<true><<<grid, 256, 0, as_stream(stream)>>>(x, (const bf16x8*)w_packed_bf16, bias, hc, wc, true_hw, (__bf16*)out_bf16);
    return check_launch("vgg_conv1_bf16_fwd_extents");
}

int frcnn_pool2d_fwd_bf16(const void* x_bf16, int n, int h, int w, int c, int k, int stride, void* y_bf16, void* stream) {
    if (!x_bf16 || !y_bf16 || n <= 0 || h <= 0 || w <= 0 || c <= 0 || k <= 0 || stride <= 0) return fail(FRCNN_E_ARG, "pool2d_fwd_bf16: bad argument");
    if (k != 2 || stride != 2) return fail(FRCNN_E_UNSUPPORTED, "pool2d_fwd_bf16: only the 2x2 / stride-2 max-pool (got k=%d stride=%d)", k, stride);
    if (c & 7) return fail(FRCNN_E_UNSUPPORTED, "pool2d_fwd_bf16: C must be a multiple of 8 (got %d)", c);
    if (h < 2 || w < 2) return fail(FRCNN_E_ARG, "pool2d_fwd_bf16: map smaller than the window");
    if ((reinterpret_cast<uintptr_t>(x_bf16) | reinterpret_cast<uintptr_t>(y_bf16)) & 15) return fail(FRCNN_E_ARG, "pool2d_fwd_bf16: 16-byte aligned tensors");
    const int Ho = (h - 2) / 2 + 1, Wo = (w - 2) / 2 + 1;
    const size_t total = (size_t)n * Ho * Wo * (c / 8);
    size_t grid = (total + 255) / 256;
    if (grid > 16384) grid = 16384;
    k_pool2_bf16<<<(int)grid, 256, 0, as_stream(stream)>>>((const u16x8*)x_bf16, n, h, w, c / 8, Ho, Wo, (u16x8*)y_bf16);
    return check_launch("pool2d_fwd_bf16");
}

}  // extern "C"
