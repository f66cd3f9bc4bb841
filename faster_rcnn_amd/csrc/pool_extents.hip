// MaxPooling2D((2,2), strides=(2,2)) (vgg.py:100, 108, 118, 128) on the tensors of a CANVAS pass (gfx950), f32 and bf16.
//
// x [n][hc][wc][c] is a conv output on canvases: image i's true map is the top-left hw[i] = {rows, cols} cells (device words), the
// rest is whatever bias and ReLU made of the zeros around it.  y [n][hc/2][wc/2][c]:
//   * a cell inside floor(rows / 2) x floor(cols / 2) is the maximum of its four inputs, all of which lie inside the true map: the
//     same comparisons in the same order as k_pool<true> (f32) / k_pool2_bf16 make on the true-size tensor, so bit-identical to them;
//   * every other cell is written as ZERO and nothing is read for it.  That includes row floor(rows / 2) / column floor(cols / 2) of
//     an odd side, whose window holds the image's last row / column and the outside: VALID pooling drops it on the true-size tensor.
// So the pooled map leaves already masked for the 3x3 convolution behind it, and the convolution in FRONT of a pool needs no
// k_zero_outside launch (boxes.hip): this kernel never looks at the cells that launch would have cleared.
//
// Memory-bound: 16-byte pieces (4 f32 / 8 bf16 channels), four loads and one store per inside piece, one store per outside piece.  A
// workgroup owns PE_RUN consecutive pieces of ONE output row (four per thread, the sixteen loads issued before the first comparison);
// whether it lies below the true rows or behind the true columns is uniform across it, and then it only stores zeros (as
// k_zero_outside does per row).  The extent is read from memory: one captured launch serves every image size of its canvas class.
#include "common.h"
#include "../../include/ext/frcnn_hip_vgg_canvas.h"

namespace frcnn {

typedef unsigned short pe_u16x8 __attribute__((ext_vector_type(8)));

constexpr int PE_PER_THREAD = 4;
constexpr int PE_RUN = 256 * PE_PER_THREAD;         // 16-byte pieces of one output row per workgroup

__device__ __forceinline__ float4 pe_max4(const float4 (&v)[4]) {
    float4 acc = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);          // k_pool<true>, window order (0,0) (0,1) (1,0) (1,1)
#pragma unroll
    for (int q = 0; q < 4; ++q) { acc.x = fmaxf(acc.x, v[q].x); acc.y = fmaxf(acc.y, v[q].y); acc.z = fmaxf(acc.z, v[q].z); acc.w = fmaxf(acc.w, v[q].w); }
    return acc;
}

__device__ __forceinline__ pe_u16x8 pe_max4(const pe_u16x8 (&v)[4]) {
    pe_u16x8 best = v[0];                                                          // k_pool2_bf16: strictly greater or a NaN replaces
#pragma unroll
    for (int q = 1; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float a = __uint_as_float((unsigned)v[q][e] << 16), b = __uint_as_float((unsigned)best[e] << 16);
            best[e] = (a > b || a != a) ? v[q][e] : best[e];
        }
    return best;
}

// V = float4 (f32) or pe_u16x8 (bf16): one 16-byte piece of a cell's channels; CP = pieces per cell
template <typename V>
__global__ void __launch_bounds__(256) k_pool2_extents(const V* __restrict__ x, int H, int W, int CP, int Ho, int Wo, const int* __restrict__ hw, V* __restrict__ y) {
    const int ho = blockIdx.y, img = blockIdx.z, row_pieces = Wo * CP;
    const int p0 = blockIdx.x * PE_RUN;
    const int ht = max(0, min(hw[2 * img], H)) >> 1, wt = max(0, min(hw[2 * img + 1], W)) >> 1;      // the pooled true map
    V* yr = y + ((size_t)img * Ho + ho) * (size_t)row_pieces;
    const int in_pieces = ho < ht ? wt * CP : 0;               // pieces of this output row inside the pooled true map
    V zero;
    __builtin_memset(&zero, 0, sizeof(V));
    if (p0 >= in_pieces) {                                     // (workgroup-uniform) below the true rows or behind the true columns
#pragma unroll
        for (int q = 0; q < PE_PER_THREAD; ++q) {
            const int p = p0 + q * 256 + threadIdx.x;
            if (p < row_pieces) yr[p] = zero;
        }
        return;
    }
    const V* xr = x + ((size_t)img * H + 2 * ho) * (size_t)W * CP;
    const size_t down = (size_t)W * CP;
    V v[PE_PER_THREAD][4];
#pragma unroll
    for (int q = 0; q < PE_PER_THREAD; ++q) {
        const int p = p0 + q * 256 + threadIdx.x;
        if (p < in_pieces) {
            const int wo = p / CP, c = p - wo * CP;
            const V* base = xr + (size_t)(2 * wo) * CP + c;
            v[q][0] = base[0]; v[q][1] = base[CP]; v[q][2] = base[down]; v[q][3] = base[down + CP];
        }
    }
#pragma unroll
    for (int q = 0; q < PE_PER_THREAD; ++q) {
        const int p = p0 + q * 256 + threadIdx.x;
        if (p < in_pieces) yr[p] = pe_max4(v[q]);
        else if (p < row_pieces) yr[p] = zero;
    }
}

template <typename V>
static int launch_pool2_extents(const char* what, const void* x, int n, int hc, int wc, int c, int per_piece, const int32_t* true_hw, void* y, void* stream) {
    if (!x || !y || !true_hw || n <= 0 || hc < 2 || wc < 2 || c <= 0) return fail(FRCNN_E_ARG, "%s: bad argument (a canvas of at least 2 x 2 cells)", what);
    if (c % per_piece) return fail(FRCNN_E_UNSUPPORTED, "%s: C must be a multiple of %d (got %d)", what, per_piece, c);
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) return fail(FRCNN_E_ARG, "%s: 16-byte aligned tensors", what);
    const int Ho = hc / 2, Wo = wc / 2, CP = c / per_piece;
    if (Ho > 65535 || n > 65535 || (long long)Wo * CP > 0x7fffffffLL - PE_RUN) return fail(FRCNN_E_UNSUPPORTED, "%s: at most 65535 output rows and 65535 images per launch", what);
    const dim3 grid((Wo * CP + PE_RUN - 1) / PE_RUN, Ho, n);
    k_pool2_extents<V><<<grid, 256, 0, as_stream(stream)>>>((const V*)x, hc, wc, CP, Ho, Wo, true_hw, (V*)y);
    return check_launch(what);
}

}  // namespace frcnn

using namespace frcnn;

extern "C" {

int frcnn_vgg_canvas_version(void) { return FRCNN_VGG_CANVAS_VERSION; }

int frcnn_pool2d_fwd_extents(const float* x, int n, int hc, int wc, int c, const int32_t* true_hw, float* y, void* stream) {
    return launch_pool2_extents<float4>("pool2d_fwd_extents", x, n, hc, wc, c, 4, true_hw, y, stream);
}

int frcnn_pool2d_fwd_bf16_extents(const void* x_bf16, int n, int hc, int wc, int c, const int32_t* true_hw, void* y_bf16, void* stream) {
    return launch_pool2_extents<pe_u16x8>("pool2d_fwd_bf16_extents", x_bf16, n, hc, wc, c, 8, true_hw, y_bf16, stream);
}

}  // extern "C"
