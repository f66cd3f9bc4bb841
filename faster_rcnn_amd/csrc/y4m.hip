// YUV4MPEG2 frames on the device (include/ext/frcnn_hip_y4m.h): planar Y'CbCr -> interleaved RGB for the frames a pass reads
// (k_y4m_decode: up to 64 frames of mixed sizes and chroma modes in one launch, blocks indexed by (item, tile) from the device-side item
// table) and interleaved RGB -> planar Y'CbCr for the frames it has drawn into (k_y4m_encode: the B frames of a pass in one launch).
//
// Pure streaming: a lane owns a group of 2x2 pixels (the 4:2:0 modes: one chroma sample's footprint) or of 1x4 (the others), reads its
// group's samples once, writes its pixels once.  No LDS, no atomics, nothing data-dependent: every byte value is a sample, a frame cannot
// be damaged, so there is no status to report; what can be wrong (sizes, offsets) is known from the header and refused on the host.  A
// y4m row has no padding and a frame may start at any byte, so a group's bytes move as words of 2 or 4 bytes where their address is a
// multiple of the word (decided per group from the address itself) and byte by byte elsewhere -- ragged right edges included.
//
// The arithmetic is ycc_common.h's (the JFIF matrices, fancy upsampling, the 2x2 box average: what the JPEG codecs run) plus the two
// things y4m adds: a co-sited chroma axis and the limited-range BT.601 matrices.  tests/y4m_ref.py restates all of it in numpy.
#include <type_traits>

#include "common.h"
#include "ycc_common.h"
#include "../../include/ext/frcnn_hip_y4m.h"

namespace frcnn {
namespace {

using Plan = frcnn_y4m_plan_t;
using Item = frcnn_y4m_batch_item_t;
constexpr int Y4M_THREADS = 256;                                // groups per tile

// ------------------------------------------------------------------------------------------------------------------ host sizes
__host__ __device__ inline bool y4m_v2(int chroma) { return chroma == FRCNN_Y4M_C420JPEG || chroma == FRCNN_Y4M_C420MPEG2; }
__host__ __device__ inline int y4m_cw(int w, int chroma) { return chroma >= FRCNN_Y4M_C444 ? w : (w + 1) >> 1; }
__host__ __device__ inline int y4m_ch(int h, int chroma) { return y4m_v2(chroma) ? (h + 1) >> 1 : h; }

inline size_t y4m_frame_bytes(int h, int w, int chroma) {
    if (h < 1 || w < 1 || h > FRCNN_Y4M_MAX_SIDE || w > FRCNN_Y4M_MAX_SIDE || chroma < 0 || chroma > FRCNN_Y4M_CMONO) return 0;
    const size_t luma = (size_t)h * (size_t)w;
    return chroma == FRCNN_Y4M_CMONO ? luma : luma + 2 * (size_t)y4m_cw(w, chroma) * (size_t)y4m_ch(h, chroma);
}

// groups of a frame (2x2 or 1x4 pixels): at most 2^28 for sides <= 32768
inline uint32_t y4m_groups(int h, int w, int chroma) {
    return y4m_v2(chroma) ? (uint32_t)((w + 1) / 2) * (uint32_t)((h + 1) / 2) : (uint32_t)((w + 3) / 4) * (uint32_t)h;
}

inline uint32_t y4m_tiles(int h, int w, int chroma) { return (y4m_groups(h, w, chroma) + Y4M_THREADS - 1) / Y4M_THREADS; }

int y4m_check_plan(const char* who, const Plan& p, int item) {
    const size_t bytes = y4m_frame_bytes(p.h, p.w, p.chroma);
    if (!bytes) return fail(FRCNN_E_ARG, "%s: item %d: h=%d w=%d (1..%d), chroma=%d (0..%d)", who, item, p.h, p.w, FRCNN_Y4M_MAX_SIDE, p.chroma, FRCNN_Y4M_CMONO);
    if (p.range != FRCNN_Y4M_LIMITED && p.range != FRCNN_Y4M_FULL) return fail(FRCNN_E_ARG, "%s: item %d: range=%d (0 limited, 1 full)", who, item, p.range);
    if ((size_t)p.frame_bytes != bytes) return fail(FRCNN_E_ARG, "%s: item %d: frame_bytes=%u, a %dx%d frame of chroma mode %d has %zu", who, item, p.frame_bytes, p.w, p.h, p.chroma, bytes);
    return FRCNN_OK;
}

// ------------------------------------------------------------------------------------------------------------ a group's bytes
// N bytes at p: as N / sizeof(Word) words when all ``n`` == N are wanted and p is a multiple of the word, else ``n`` single bytes
template <int N, class Word>
__device__ __forceinline__ void ld_group(const uint8_t* p, int n, int (&b)[N]) {
    constexpr int WB = sizeof(Word);
    static_assert(N % WB == 0, "whole words");
    if (n == N && (reinterpret_cast<uintptr_t>(p) & (WB - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < N / WB; ++k) {
            const uint32_t v = reinterpret_cast<const Word*>(p)[k];
#pragma unroll
            for (int j = 0; j < WB; ++j) b[k * WB + j] = (int)((v >> (8 * j)) & 255u);
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) b[k] = k < n ? (int)p[k] : 0;
    }
}

template <int N, class Word>
__device__ __forceinline__ void st_group(uint8_t* p, int n, const int (&b)[N]) {
    constexpr int WB = sizeof(Word);
    static_assert(N % WB == 0, "whole words");
    if (n == N && (reinterpret_cast<uintptr_t>(p) & (WB - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < N / WB; ++k) {
            uint32_t v = 0;
#pragma unroll
            for (int j = 0; j < WB; ++j) v |= (uint32_t)b[k * WB + j] << (8 * j);
            reinterpret_cast<Word*>(p)[k] = (Word)v;
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < n) p[k] = (uint8_t)b[k];
    }
}

// --------------------------------------------------------------------------------------------------------------------- colour
// BT.601, limited range (the header states the table): Y, Cb - 128, Cr - 128 -> R, G, B
__device__ __forceinline__ void bt601_ycc_to_rgb(int lum, int cb, int cr, int* r, int* g, int* b) {
    const int l = 76309 * (lum - 16) + 32768;
    *r = ycc_clamp8((l + 104597 * cr) >> 16);
    *g = ycc_clamp8((l - 25675 * cb - 53279 * cr) >> 16);
    *b = ycc_clamp8((l + 132201 * cb) >> 16);
}

__device__ __forceinline__ void bt601_rgb_to_ycc(int r, int g, int b, int* Y, int* Cb, int* Cr) {
    *Y = ycc_clamp8(16 + ((16829 * r + 33039 * g + 6416 * b + 32768) >> 16));
    *Cb = ycc_clamp8(128 + ((-9714 * r - 19071 * g + 28784 * b + 32768) >> 16));
    *Cr = ycc_clamp8(128 + ((28784 * r - 24103 * g - 4681 * b + 32768) >> 16));
}

// ------------------------------------------------------------------------------------------------------------------ upsampling
// a co-sited axis: the sample itself at even positions, the rounded mean of it and the next (the last one repeated) at odd ones
__device__ __forceinline__ int cosited(int a, int b, int odd) { return odd ? (a + b + 1) >> 1 : a; }

// the chroma sample of full-size pixel (x, y) from a plane of cw x ch samples
__device__ __forceinline__ int y4m_chroma(const uint8_t* c, int chroma, int cw, int ch, int x, int y) {
    if (chroma == FRCNN_Y4M_C444) return c[(size_t)y * cw + x];
    const int i = x >> 1, i1 = i + 1 < cw ? i + 1 : cw - 1;
    if (chroma == FRCNN_Y4M_C422) {
        const uint8_t* row = c + (size_t)y * cw;
        return cosited(row[i], row[i1], x & 1);
    }
    const uint8_t* near = c + (size_t)(y >> 1) * cw;
    const uint8_t* far = c + (size_t)fancy_far_row(y, ch) * cw;
    if (chroma == FRCNN_Y4M_C420JPEG) return fancy_h2v2(near, far, cw, x);
    const int a = fancy_tri(near[i], far[i], y & 1);            // C420MPEG2: the centred axis first, then the co-sited one
    return (x & 1) ? cosited(a, fancy_tri(near[i1], far[i1], y & 1), 1) : a;
}

// ----------------------------------------------------------------------------------------------------------------------- decode
// group ``gid`` of one frame: GW x GH pixels (2 x 2 or 4 x 1)
template <int GW, int GH>
__device__ __forceinline__ void y4m_decode_group(const Plan& p, const uint8_t* src, uint8_t* dst, int bgr, uint32_t gid) {
    using Word = typename std::conditional<GW == 4, uint32_t, uint16_t>::type;
    const int h = p.h, w = p.w, chroma = p.chroma;
    const uint32_t gxn = (uint32_t)((w + GW - 1) / GW), gyn = (uint32_t)((h + GH - 1) / GH);
    if (gid >= gxn * gyn) return;
    const int gy = (int)(gid / gxn), gx = (int)(gid - (uint32_t)gy * gxn);
    const int x0 = gx * GW, y0 = gy * GH;
    const int nx = w - x0 < GW ? w - x0 : GW;
    const int cw = y4m_cw(w, chroma), ch = y4m_ch(h, chroma);
    const uint8_t* cbp = src + (size_t)h * (size_t)w;
    const uint8_t* crp = cbp + (size_t)cw * (size_t)ch;
#pragma unroll
    for (int r = 0; r < GH; ++r) {
        const int y = y0 + r;
        if (y >= h) break;
        int lum[GW], px[3 * GW];
        ld_group<GW, Word>(src + (size_t)y * (size_t)w + x0, nx, lum);
#pragma unroll
        for (int k = 0; k < GW; ++k) {
            int R = 0, G = 0, B = 0;
            if (k < nx) {
                int cb = 0, cr = 0;
                if (chroma != FRCNN_Y4M_CMONO) {
                    cb = y4m_chroma(cbp, chroma, cw, ch, x0 + k, y) - 128;
                    cr = y4m_chroma(crp, chroma, cw, ch, x0 + k, y) - 128;
                }
                if (p.range == FRCNN_Y4M_FULL) jfif_ycc_to_rgb(lum[k], cb, cr, &R, &G, &B);
                else bt601_ycc_to_rgb(lum[k], cb, cr, &R, &G, &B);
            }
            px[3 * k] = bgr ? B : R; px[3 * k + 1] = G; px[3 * k + 2] = bgr ? R : B;
        }
        st_group<3 * GW, Word>(dst + ((size_t)y * (size_t)w + x0) * 3, 3 * nx, px);
    }
}

__device__ __forceinline__ void y4m_decode_body(const Item& it, const uint8_t* files, uint8_t* out, int bgr, uint32_t tile) {
    const uint32_t gid = tile * Y4M_THREADS + threadIdx.x;
    if (y4m_v2(it.plan.chroma)) y4m_decode_group<2, 2>(it.plan, files + it.file_off, out + it.out_off, bgr, gid);
    else y4m_decode_group<4, 1>(it.plan, files + it.file_off, out + it.out_off, bgr, gid);
}

// grid (tiles of the batch's largest item, items): the blocks past a smaller item's extent return at once
__global__ void __launch_bounds__(Y4M_THREADS) k_y4m_decode(const Item* items, const uint8_t* files, uint8_t* out, int bgr) {
    const Item it = items[blockIdx.y];
    y4m_decode_body(it, files, out, bgr, blockIdx.x);
}

// the batch of one, its item a kernel argument
__global__ void __launch_bounds__(Y4M_THREADS) k_y4m_decode_one(const Item it, const uint8_t* files, uint8_t* out, int bgr) {
    y4m_decode_body(it, files, out, bgr, blockIdx.x);
}

// ----------------------------------------------------------------------------------------------------------------------- encode
__device__ __forceinline__ void y4m_rgb_to_ycc(int range, int r, int g, int b, int* Y, int* Cb, int* Cr) {
    if (range == FRCNN_Y4M_FULL) jfif_rgb_to_ycc(r, g, b, Y, Cb, Cr);
    else bt601_rgb_to_ycc(r, g, b, Y, Cb, Cr);
}

// grid (tiles, frames); S420: a lane owns a 2x2 group (one chroma sample), else 1x4 pixels
template <bool S420>
__global__ void __launch_bounds__(Y4M_THREADS) k_y4m_encode(const uint8_t* frames, size_t frame_stride, int h, int w, int bgr, int range,
                                                            uint8_t* out, size_t out_stride) {
    constexpr int GW = S420 ? 2 : 4, GH = S420 ? 2 : 1;
    using Word = typename std::conditional<S420, uint16_t, uint32_t>::type;
    const uint32_t gxn = (uint32_t)((w + GW - 1) / GW), gyn = (uint32_t)((h + GH - 1) / GH);
    const uint32_t gid = blockIdx.x * Y4M_THREADS + threadIdx.x;
    if (gid >= gxn * gyn) return;
    const int gy = (int)(gid / gxn), gx = (int)(gid - (uint32_t)gy * gxn);
    const int x0 = gx * GW, y0 = gy * GH;
    const int nx = w - x0 < GW ? w - x0 : GW;
    const uint8_t* frame = frames + (size_t)blockIdx.y * frame_stride;
    uint8_t* yp = out + (size_t)blockIdx.y * out_stride;
    const int cw = S420 ? (w + 1) >> 1 : w, ch = S420 ? (h + 1) >> 1 : h;
    uint8_t* cbp = yp + (size_t)h * (size_t)w;
    uint8_t* crp = cbp + (size_t)cw * (size_t)ch;
    int sb = 0, sr = 0;
#pragma unroll
    for (int r = 0; r < GH; ++r) {
        const int y = y0 + r < h ? y0 + r : h - 1;              // (the last row repeats into a group that reaches past the frame)
        int px[3 * GW], Y[GW], Cb[GW], Cr[GW];
        ld_group<3 * GW, Word>(frame + ((size_t)y * (size_t)w + x0) * 3, 3 * nx, px);
#pragma unroll
        for (int k = 0; k < GW; ++k) {
            const int q = k < nx ? k : nx - 1;                  // (... and the last column)
            y4m_rgb_to_ycc(range, px[3 * q + (bgr ? 2 : 0)], px[3 * q + 1], px[3 * q + (bgr ? 0 : 2)], &Y[k], &Cb[k], &Cr[k]);
            sb += Cb[k]; sr += Cr[k];
        }
        if (y0 + r < h) {
            st_group<GW, Word>(yp + (size_t)y * (size_t)w + x0, nx, Y);
            if constexpr (!S420) {
                st_group<GW, Word>(cbp + (size_t)y * (size_t)w + x0, nx, Cb);
                st_group<GW, Word>(crp + (size_t)y * (size_t)w + x0, nx, Cr);
            }
        }
    }
    if constexpr (S420) {
        cbp[(size_t)gy * cw + gx] = (uint8_t)box2x2(sb, gx);
        crp[(size_t)gy * cw + gx] = (uint8_t)box2x2(sr, gx);
    }
}

}  // namespace
}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_y4m_version(void) { return FRCNN_Y4M_VERSION; }

extern "C" size_t frcnn_y4m_frame_bytes(int h, int w, int chroma) { return y4m_frame_bytes(h, w, chroma); }

extern "C" int frcnn_y4m_decode_batch_u8(const frcnn_y4m_batch_item_t* items_host, const frcnn_y4m_batch_item_t* items_dev, int n,
                                         const uint8_t* files_dev, size_t files_capacity, int bgr, uint8_t* out_dev, size_t out_capacity,
                                         int32_t* status_dev, void* workspace, size_t workspace_capacity, void* stream) {
    const char* who = "y4m_decode_batch_u8";
    (void)status_dev; (void)workspace; (void)workspace_capacity;
    if (!items_host || !items_dev || !files_dev || !out_dev) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (n < 1 || n > FRCNN_Y4M_BATCH_MAX) return fail(FRCNN_E_ARG, "%s: n=%d, 1..%d frames go into one batch", who, n, FRCNN_Y4M_BATCH_MAX);
    if (reinterpret_cast<uintptr_t>(items_dev) & 7u) return fail(FRCNN_E_ARG, "%s: items_dev must be 8-byte aligned", who);
    Range outs[FRCNN_Y4M_BATCH_MAX];
    uint32_t tiles = 0;
    for (int i = 0; i < n; ++i) {
        const Item& it = items_host[i];
        if (const int code = y4m_check_plan(who, it.plan, i)) return code;
        const unsigned long long frame = (unsigned long long)it.plan.h * (unsigned long long)it.plan.w * 3ull;
        if (it.file_off > files_capacity || it.plan.frame_bytes > files_capacity - it.file_off)
            return fail(FRCNN_E_ARG, "%s: item %d: file_off %llu + %u bytes > files_capacity %zu", who, i, (unsigned long long)it.file_off, it.plan.frame_bytes, files_capacity);
        if (it.out_off > out_capacity || frame > out_capacity - it.out_off)
            return fail(FRCNN_E_ARG, "%s: item %d: out_off %llu + %llu bytes > out_capacity %zu", who, i, (unsigned long long)it.out_off, frame, out_capacity);
        outs[i] = {it.out_off, it.out_off + frame, i};
        const uint32_t t = y4m_tiles(it.plan.h, it.plan.w, it.plan.chroma);
        tiles = t > tiles ? t : tiles;
    }
    const int clash = range_overlap(outs, n);
    if (clash >= 0) return fail(FRCNN_E_ARG, "%s: the output ranges of items %d and %d overlap", who, outs[clash].item, outs[clash + 1].item);
    k_y4m_decode<<<dim3(tiles, (unsigned)n), Y4M_THREADS, 0, as_stream(stream)>>>(items_dev, files_dev, out_dev, bgr ? 1 : 0);
    return check_launch(who);
}

extern "C" int frcnn_y4m_decode_u8(const uint8_t* frame_dev, size_t frame_capacity, const frcnn_y4m_plan_t* plan, int bgr, uint8_t* out_dev,
                                   size_t out_capacity, void* stream) {
    const char* who = "y4m_decode_u8";
    if (!frame_dev || !plan || !out_dev) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (const int code = y4m_check_plan(who, *plan, 0)) return code;
    if (plan->frame_bytes > frame_capacity) return fail(FRCNN_E_ARG, "%s: a frame of %u bytes, %zu given", who, plan->frame_bytes, frame_capacity);
    if ((unsigned long long)plan->h * (unsigned long long)plan->w * 3ull > out_capacity)
        return fail(FRCNN_E_ARG, "%s: out of %zu bytes for a %dx%d frame", who, out_capacity, plan->w, plan->h);
    Item it = {};
    it.plan = *plan;
    k_y4m_decode_one<<<y4m_tiles(plan->h, plan->w, plan->chroma), Y4M_THREADS, 0, as_stream(stream)>>>(it, frame_dev, out_dev, bgr ? 1 : 0);
    return check_launch(who);
}

extern "C" int frcnn_y4m_encode_u8(const uint8_t* frames_dev, size_t frame_stride, int n, int h, int w, int bgr, int chroma, int range,
                                   uint8_t* out_dev, size_t out_stride, size_t out_capacity, void* stream) {
    const char* who = "y4m_encode_u8";
    if (!frames_dev || !out_dev) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (n < 1 || n > FRCNN_Y4M_BATCH_MAX) return fail(FRCNN_E_ARG, "%s: n=%d, 1..%d frames go into one launch", who, n, FRCNN_Y4M_BATCH_MAX);
    if (chroma != FRCNN_Y4M_C420JPEG && chroma != FRCNN_Y4M_C444) return fail(FRCNN_E_ARG, "%s: chroma=%d: 420jpeg (0) or 444 (3) on output", who, chroma);
    if (range != FRCNN_Y4M_LIMITED && range != FRCNN_Y4M_FULL) return fail(FRCNN_E_ARG, "%s: range=%d (0 limited, 1 full)", who, range);
    const size_t record = y4m_frame_bytes(h, w, chroma);
    if (!record) return fail(FRCNN_E_ARG, "%s: h=%d w=%d (1..%d)", who, h, w, FRCNN_Y4M_MAX_SIDE);
    const size_t frame = (size_t)h * (size_t)w * 3;
    if (frame_stride < frame || out_stride < record) return fail(FRCNN_E_ARG, "%s: frame_stride %zu / out_stride %zu for frames of %zu and records of %zu bytes", who, frame_stride, out_stride, frame, record);
    if ((size_t)(n - 1) * out_stride + record > out_capacity) return fail(FRCNN_E_ARG, "%s: %d records of stride %zu > out_capacity %zu", who, n, out_stride, out_capacity);
    const dim3 grid(y4m_tiles(h, w, chroma), (unsigned)n);
    if (chroma == FRCNN_Y4M_C420JPEG) k_y4m_encode<true><<<grid, Y4M_THREADS, 0, as_stream(stream)>>>(frames_dev, frame_stride, h, w, bgr ? 1 : 0, range, out_dev, out_stride);
    else k_y4m_encode<false><<<grid, Y4M_THREADS, 0, as_stream(stream)>>>(frames_dev, frame_stride, h, w, bgr ? 1 : 0, range, out_dev, out_stride);
    return check_launch(who);
}
