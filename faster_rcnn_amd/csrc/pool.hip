// Pooling, the detector's row softmax and the split of its fused dense heads (f32, NHWC or position-major).
#include "common.h"

namespace frcnn {

// ------------------------------------------------------------------------------------
// pooling (NHWC, VALID): MaxPooling2D (resnet.py:412, vgg.py:100-128) / AveragePooling2D (resnet.py:515)
template <bool IS_MAX>
__global__ void k_pool(const float4* x, int n_img, int H, int W, int C4, int k, int stride, int Ho, int Wo, float4* y) {
    const size_t total = (size_t)n_img * Ho * Wo * C4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        size_t t = i / C4;
        const int wo = (int)(t % Wo); t /= Wo;
        const int ho = (int)(t % Ho);
        const int img = (int)(t / Ho);
        const float4* base = x + (((size_t)img * H + ho * stride) * W + wo * stride) * C4 + c;
        float4 acc = IS_MAX ? make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY) : make_float4(0, 0, 0, 0);
        for (int r = 0; r < k; ++r)
            for (int s = 0; s < k; ++s) {
                const float4 v = base[((size_t)r * W + s) * C4];
                if (IS_MAX) { acc.x = fmaxf(acc.x, v.x); acc.y = fmaxf(acc.y, v.y); acc.z = fmaxf(acc.z, v.z); acc.w = fmaxf(acc.w, v.w); }
                else { acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; }
            }
        if (!IS_MAX) { const float inv = (float)(k * k); acc.x /= inv; acc.y /= inv; acc.z /= inv; acc.w /= inv; }
        y[i] = acc;
    }
}

// k_pool writing its result as the f16x3 engine's two fp16 planes (hi, lo under the scale 2^*pexp) for the convolution behind it: a window's
// maximum / mean cannot exceed the largest |input|, so the scale comes from the INPUT's magnitude record before the launch
// (frcnn_amax_merge), as for the RoI resampling (roi.hip k_roi_fwd_planes).  VGG's block<n>_conv1 layers then stage their input unchanged.
template <bool IS_MAX>
__global__ void __launch_bounds__(256) k_pool_planes(const float4* x, int n_img, int H, int W, int C4, int k, int stride, int Ho, int Wo,
                                                     const int* pexp, unsigned* status, _Float16* planes, size_t plane_elems) {
    __builtin_amdgcn_s_setreg(1 | (23 << 6), 1u);         // MODE.FP16_OVFL (conv_f32_common.h, the engine's fences)
    typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
    const size_t total = (size_t)n_img * Ho * Wo * C4;
    const unsigned sb = (unsigned)(*pexp + 127) << 23;
    float sc;
    __builtin_memcpy(&sc, &sb, 4);
    unsigned seen = 0u;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        size_t t = i / C4;
        const int wo = (int)(t % Wo); t /= Wo;
        const int ho = (int)(t % Ho);
        const int img = (int)(t / Ho);
        const float4* base = x + (((size_t)img * H + ho * stride) * W + wo * stride) * C4 + c;
        float4 acc = IS_MAX ? make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY) : make_float4(0, 0, 0, 0);
        for (int r = 0; r < k; ++r)
            for (int s = 0; s < k; ++s) {
                const float4 v = base[((size_t)r * W + s) * C4];
                if (IS_MAX) { acc.x = fmaxf(acc.x, v.x); acc.y = fmaxf(acc.y, v.y); acc.z = fmaxf(acc.z, v.z); acc.w = fmaxf(acc.w, v.w); }
                else { acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; }
            }
        if (!IS_MAX) { const float inv = (float)(k * k); acc.x /= inv; acc.y /= inv; acc.z /= inv; acc.w /= inv; }
        const float xs[4] = {acc.x * sc, acc.y * sc, acc.z * sc, acc.w * sc};
        f16x4 h, l;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const _Float16 a1 = (_Float16)xs[q];
            h[q] = a1; l[q] = (_Float16)((xs[q] - (float)a1) * 2048.0f);
            unsigned short hb;
            __builtin_memcpy(&hb, &a1, 2);
            seen = seen > (unsigned)(hb & 0x7fffu) ? seen : (unsigned)(hb & 0x7fffu);
        }
        reinterpret_cast<f16x4*>(planes)[i] = h;
        reinterpret_cast<f16x4*>(planes + plane_elems)[i] = l;
    }
    if (status) {
#pragma unroll
        for (int o = 32; o; o >>= 1) { const unsigned t = __shfl_xor(seen, o); seen = seen > t ? seen : t; }
        const unsigned bits = seen > 0x7bffu ? 7u : seen == 0x7bffu ? 3u : seen >= 0x7800u ? 1u : 0u;
        if ((threadIdx.x & 63) == 0 && bits) atomicOr(status, bits);
    }
}

// AveragePooling2D over ALL positions of position-major tensors x[pos][img][c] (frcnn_conv_desc.layout == 1):
// y[img][c] = (sum over pos, in raster order) / npos -- the same additions and the same division as k_pool<false>
// performs on the NHWC tensor, so the result is bit-identical.
__global__ void k_avgpool_pos_major(const float4* x, int npos, int n_img, int C4, float4* y) {
    const size_t total = (size_t)n_img * C4, plane = total;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        float4 acc = make_float4(0, 0, 0, 0);
        for (int q = 0; q < npos; ++q) { const float4 v = x[(size_t)q * plane + i]; acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; }
        const float inv = (float)npos;
        acc.x /= inv; acc.y /= inv; acc.z /= inv; acc.w /= inv;
        y[i] = acc;
    }
}

// row softmax over the first `cols` entries of each row (Dense(..., activation='softmax'), resnet.py:522)
__global__ void k_softmax_rows(const float* x, int rows, int cols, int ldx, float* y, int ldy) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const float* xr = x + (size_t)r * ldx;
    float mx = -INFINITY;
    for (int c = 0; c < cols; ++c) mx = fmaxf(mx, xr[c]);
    float sum = 0.0f;
    for (int c = 0; c < cols; ++c) sum += expf(xr[c] - mx);
    for (int c = 0; c < cols; ++c) y[(size_t)r * ldy + c] = expf(xr[c] - mx) / sum;
}

// The two dense heads of the detector run as ONE GEMM (kernels concatenated along the output axis): this splits its
// rows back into dense_class_C (softmax over the first `cols` entries, exactly k_softmax_rows) and dense_reg_C (the
// remaining `tail` entries, copied) -- resnet.py:522-533, vgg.py:241-247.
// Round 6: 32 lanes per row (one thread per row walked its 21 + 80 columns alone: 32 us for the 64 rows of a training step, on the
// step's critical path).  The arithmetic is the one-thread loop's, bit for bit: the maximum is order-independent, every lane adds
// e_0, e_1, ... in column order (the other lanes' values arrive by shuffle), the quotients and the copy are per column.
__global__ void __launch_bounds__(256) k_dense_heads_split(const float* x, int rows, int cols, int tail, int ldx, float* cls, float* reg) {
    const int lane = threadIdx.x & 31, r = blockIdx.x * 8 + (threadIdx.x >> 5);
    if (r >= rows) return;                                   // (a whole 32-lane group leaves together)
    const float* xr = x + (size_t)r * ldx;
    float mx = -INFINITY;
    for (int c = lane; c < cols; c += 32) mx = fmaxf(mx, xr[c]);
#pragma unroll
    for (int o = 16; o; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 32));
    float sum = 0.0f;
    for (int c0 = 0; c0 < cols; c0 += 32) {
        const float e = c0 + lane < cols ? expf(xr[c0 + lane] - mx) : 0.0f;
        const int cnt = cols - c0 < 32 ? cols - c0 : 32;
        for (int k = 0; k < cnt; ++k) sum += __shfl(e, k, 32);
    }
    for (int c = lane; c < cols; c += 32) cls[(size_t)r * cols + c] = expf(xr[c] - mx) / sum;
    for (int c = lane; c < tail; c += 32) reg[(size_t)r * tail + c] = xr[cols + c];
}

}  // namespace frcnn

using namespace frcnn;

extern "C" {

int frcnn_pool2d_fwd(const float* x, int n, int h, int w, int c, int k, int stride, int is_max, float* y, void* stream) {
    if (!x || !y || n <= 0 || h < k || w < k || c <= 0 || (c & 3) || k <= 0 || stride <= 0) return fail(FRCNN_E_ARG, "pool2d_fwd: bad argument (C must be a multiple of 4)");
    const int Ho = (h - k) / stride + 1, Wo = (w - k) / stride + 1;
    const size_t total = (size_t)n * Ho * Wo * (c / 4);
    int grid = (int)((total + 255) / 256);
    if (grid > 8192) grid = 8192;
    if (is_max) k_pool<true><<<grid, 256, 0, as_stream(stream)>>>((const float4*)x, n, h, w, c / 4, k, stride, Ho, Wo, (float4*)y);
    else k_pool<false><<<grid, 256, 0, as_stream(stream)>>>((const float4*)x, n, h, w, c / 4, k, stride, Ho, Wo, (float4*)y);
    return check_launch("pool2d_fwd");
}

int frcnn_pool2d_fwd_planes(const float* x, int n, int h, int w, int c, int k, int stride, int is_max, const frcnn_h3_planes* out, void* stream) {
    if (!x || !out || !out->planes || !out->exponent || n <= 0 || h < k || w < k || c <= 0 || (c & 3) || k <= 0 || stride <= 0 || (reinterpret_cast<uintptr_t>(out->planes) & 15))
        return fail(FRCNN_E_ARG, "pool2d_fwd_planes: bad argument (C must be a multiple of 4, planes 16-byte aligned, exponent set before the launch)");
    const int Ho = (h - k) / stride + 1, Wo = (w - k) / stride + 1;
    const size_t total = (size_t)n * Ho * Wo * (c / 4);
    int grid = (int)((total + 255) / 256);
    if (grid > 8192) grid = 8192;
    if (is_max) k_pool_planes<true><<<grid, 256, 0, as_stream(stream)>>>((const float4*)x, n, h, w, c / 4, k, stride, Ho, Wo, out->exponent, (unsigned*)out->status, (_Float16*)out->planes, total * 4);
    else k_pool_planes<false><<<grid, 256, 0, as_stream(stream)>>>((const float4*)x, n, h, w, c / 4, k, stride, Ho, Wo, out->exponent, (unsigned*)out->status, (_Float16*)out->planes, total * 4);
    return check_launch("pool2d_fwd_planes");
}

int frcnn_avgpool_pos_major(const float* x, int npos, int n, int c, float* y, void* stream) {
    if (!x || !y || npos <= 0 || n <= 0 || c <= 0 || (c & 3)) return fail(FRCNN_E_ARG, "avgpool_pos_major: bad argument (C must be a multiple of 4)");
    const size_t total = (size_t)n * (c / 4);
    int grid = (int)((total + 255) / 256);
    if (grid > 8192) grid = 8192;
    k_avgpool_pos_major<<<grid, 256, 0, as_stream(stream)>>>((const float4*)x, npos, n, c / 4, (float4*)y);
    return check_launch("avgpool_pos_major");
}

int frcnn_softmax_rows(const float* x, int rows, int cols, int ldx, float* y, int ldy, void* stream) {
    if (rows < 0 || cols <= 0 || ldx < cols || ldy < cols) return fail(FRCNN_E_ARG, "softmax_rows: bad argument");
    if (rows == 0) return FRCNN_OK;
    if (!x || !y) return fail(FRCNN_E_ARG, "softmax_rows: null pointer");
    k_softmax_rows<<<(rows + 63) / 64, 64, 0, as_stream(stream)>>>(x, rows, cols, ldx, y, ldy);
    return check_launch("softmax_rows");
}

int frcnn_dense_heads_split(const float* x, int rows, int cols, int tail, int ldx, float* cls, float* reg, void* stream) {
    if (rows < 0 || cols <= 0 || tail < 0 || ldx < cols + tail) return fail(FRCNN_E_ARG, "dense_heads_split: bad argument");
    if (rows == 0) return FRCNN_OK;
    if (!x || !cls || (tail && !reg)) return fail(FRCNN_E_ARG, "dense_heads_split: null pointer");
    k_dense_heads_split<<<(rows + 7) / 8, 256, 0, as_stream(stream)>>>(x, rows, cols, tail, ldx, cls, reg);
    return check_launch("dense_heads_split");
}

}  // extern "C"
