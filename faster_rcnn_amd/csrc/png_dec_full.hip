// The rest of PNG's still images decoded on the device (include/ext/frcnn_hip_png_dec_full.h): palette files, 1/2/4-bit and 16-bit
// samples, grey + alpha and Adam7 interlace, beside everything png_dec.hip takes.  THREE launches per batch, whatever the number of
// files, that allocate nothing, synchronise nothing and read nothing on the host.  gfx950 (CDNA4) only, wave64 throughout, plain HIP:
// vector stores and vector atomics, no inline assembly.  PNG is lossless: Pillow is the oracle, byte for byte.
//
//   k_png_dec_inflate<FItem> png_dec_common.h's kernel around pd_inflate_body, the one revision 1 runs on ITS items: ONE workgroup of 512
//                            lanes per file.
//   k_png_dec_full_unfilter  grid (7, files), ONE wave per (pass, file).  A file without interlace is its pass 0 alone; an Adam7 file
//                            has up to seven sub-images one behind the other in the inflated bytes, each with its own rows, its own row
//                            length and a zero row above its first: independent, so they run side by side.  A workgroup whose pass is
//                            absent (pw == 0 or ph == 0, or passes 1..6 of a file without interlace) returns as a whole.  Within a
//                            pass, revision 1's diagonal wavefront: strips of 64 rows, lane l takes row base + l at filter unit t - l in
//                            step t; the unit above comes from lane l - 1's previous step through wave shuffles, the unit above left is
//                            the one that came the step before, the left one the lane's own.  The filter unit is bpp = max(1,
//                            bits_per_pixel / 8) bytes, one of 1, 2, 3, 4, 6, 8, carried in 64 bits; a row is ceil(pw * bits_per_pixel /
//                            8) bytes, a whole number of units.  EVERY lane writes its reconstructed unit back over the filtered bytes
//                            (a byte is read raw by its own lane alone, and before that lane writes it); lane 0 of the next strip reads
//                            the row above from there, behind a barrier.
//   k_png_dec_full_expand    grid (ceil(max h * w / 256), files), ONE lane per output pixel.  The lane finds the pass that holds its
//                            pixel (y0 + r * dy, x0 + i * dx) -> (pass, r, i), reads sample i of row r of that pass (sub-byte samples
//                            MSB first), then the palette lookup, the grey scaling (x 255, 85, 17) or the high byte of a 16-bit sample,
//                            and writes R,G,B or B,G,R.  Reconstruction needs whole bytes, expansion needs samples: two passes over the
//                            inflated bytes keep both simple, and the second is a coalesced write of the frame.
//
// Bounds (the argument of png_dec.hip, extended).  The host checks on items_host (png_dec_host.h: pd_check_batch, stated there once for
// both decoders) that every item's stream, palette (colour type 3), region and frame lie inside the buffers, that regions and frames are
// disjoint, and that inflated_len is the sum over the existing passes of ph * (1 + ceil(pw * bits / 8)) for the plan's h, w, colour
// type, depth and interlace; the kernels compute every address from those fields through the SAME functions (pdf_pass, pdf_pass_offset,
// which live beside that check), never from anything read from the stream.  The inflate is
// pd_inflate_body with stream_len and inflated_len.  The unfilter wave of pass k reads and writes rows
// offset_k + row * (1 + rowbytes_k) + [0, 1 + rowbytes_k) for row < ph_k only: inside [0, inflated_len) since the passes' sizes sum to
// it.  The expand lane exists for row < h, x < w only (its index is below h * w) and writes that pixel alone; the sample it reads lies
// at byte 1 + floor(i * bits / 8) + (at most 7) of a row of its pass with i < pw_k: inside that row.  A palette index is compared with
// plte_entries (1..256, checked on the host) before the lookup at 3 * index + [0, 3) of the item's 768 staged bytes.  A filter byte above
// 4 in any pass sets FRCNN_PNG_DEC_FILTER (an atomic OR: the passes' waves share the word) and is treated as 0.  Loops run over h, w
// and the pass table.  The one barrier of the unfilter kernel closes a strip: the strip count depends on ph_k alone, uniform over the
// workgroup, and the early return is decided by blockIdx and the plan.
#include "png_dec_host.h"

namespace frcnn {
namespace {

constexpr int PDF_EXPAND_THREADS = 256;

// ------------------------------------------------------------------------------------------------------------------- the kernels
__device__ __forceinline__ unsigned long long pdf_shfl_up1(unsigned long long v) {
    const uint32_t lo = __shfl_up((uint32_t)v, 1, 64), hi = __shfl_up((uint32_t)(v >> 32), 1, 64);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long pdf_load_unit(const uint8_t* p, int bpp) {
    unsigned long long v = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (k < bpp) v |= (unsigned long long)p[k] << (8 * k);
    return v;
}

// grid = (pass, item), one wave: the pass's rows reconstructed in place
__global__ void __launch_bounds__(PD_UNF_THREADS) k_png_dec_full_unfilter(const FItem* __restrict__ items, uint8_t* workspace, int32_t* status) {
    const FItem& it = items[blockIdx.y];
    const int k = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int interlace = it.plan.interlace, h = it.plan.h, w = it.plan.w;
    const int bits = pdf_channels(it.plan.colour_type) * it.plan.bit_depth;
    const PdfPass pass = pdf_pass(k, interlace, h, w);
    if (pass.pw <= 0 || pass.ph <= 0) return;                   // (uniform: blockIdx and the plan)
    const int bpp = bits >= 8 ? bits / 8 : 1;
    const uint32_t rowbytes = (uint32_t)pdf_rowbytes(pass.pw, bits);
    const int units = (int)(rowbytes / (uint32_t)bpp), ph = pass.ph;     // (bits >= 8: rowbytes = pw * bpp; below: bpp = 1)
    const size_t stride = 1 + (size_t)rowbytes;
    uint8_t* rows = workspace + it.ws_off + pdf_pass_offset(k, interlace, h, w, bits);
    uint32_t flagged = 0;
    for (int base = 0; base < ph; base += 64) {
        const int row = base + lane;
        const bool live = row < ph;
        uint8_t* src = rows + (size_t)(live ? row : 0) * stride;
        uint32_t ft = live ? (uint32_t)src[0] : 0u;
        if (ft > 4u) { flagged |= ST_FILTER; ft = 0u; }
        const uint8_t* up = base > 0 ? rows + (size_t)(base - 1) * stride + 1 : nullptr;    // the previous strip's last row, reconstructed
        unsigned long long a = 0, c = 0, cur = 0;
        for (int t = 0; t < units + 63; ++t) {
            unsigned long long b = pdf_shfl_up1(cur);           // lane - 1 stood at this unit of the row above a step ago
            const int x = t - lane;
            const bool on = live && x >= 0 && x < units;
            if (lane == 0) b = (on && up) ? pdf_load_unit(up + (size_t)x * bpp, bpp) : 0ull;
            if (on) {
                uint8_t* px = src + 1 + (size_t)x * bpp;
                const unsigned long long raw = pdf_load_unit(px, bpp);
                unsigned long long v = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if (j < bpp) {
                        const int sh = 8 * j;
                        const uint32_t pr = pd_predict(ft, (int)((a >> sh) & 255u), (int)((b >> sh) & 255u), (int)((c >> sh) & 255u));
                        const uint32_t byte = ((uint32_t)(raw >> sh) + pr) & 255u;
                        v |= (unsigned long long)byte << sh;
                        px[j] = (uint8_t)byte;
                    }
                }
                cur = v;
                c = b;
                a = v;
            }
        }
        __threadfence_block();
        __syncthreads();                                        // (lane 0 of the next strip reads what lane 63 wrote)
    }
    const int bad = __any((int)flagged);
    if (bad && lane == 0) atomicOr(reinterpret_cast<unsigned int*>(status + blockIdx.y), (unsigned int)ST_FILTER);
}

// grid = (pixel blocks, item), one lane per output pixel
__global__ void __launch_bounds__(PDF_EXPAND_THREADS) k_png_dec_full_expand(const uint8_t* __restrict__ files, const FItem* __restrict__ items,
                                                                             const uint8_t* __restrict__ workspace, int bgr, uint8_t* __restrict__ out) {
    const FItem& it = items[blockIdx.y];
    const int h = it.plan.h, w = it.plan.w, colour = it.plan.colour_type, depth = it.plan.bit_depth, interlace = it.plan.interlace;
    const unsigned long long idx = (unsigned long long)blockIdx.x * PDF_EXPAND_THREADS + threadIdx.x;
    if (idx >= (unsigned long long)h * (unsigned long long)w) return;
    const int y = (int)(idx / (unsigned)w), x = (int)(idx % (unsigned)w);
    int k = 0;
    if (interlace) {
        if (y & 1) k = 6;
        else if (x & 1) k = 5;
        else if (y & 2) k = 4;
        else if (x & 2) k = 3;
        else if (y & 4) k = 2;
        else if (x & 4) k = 1;
        else k = 0;
    }
    const int channels = pdf_channels(colour), bits = channels * depth;
    const PdfPass pass = pdf_pass(k, interlace, h, w);
    const int r = (y - pass.y0) / pass.dy, i = (x - pass.x0) / pass.dx;     // (exact: the pass was chosen by the low bits of y and x)
    const uint8_t* row = workspace + it.ws_off + pdf_pass_offset(k, interlace, h, w, bits) + (size_t)r * (1 + (size_t)pdf_rowbytes(pass.pw, bits)) + 1;
    uint32_t s0, s1, s2;
    if (depth < 8) {                                            // one sample per pixel (grey or palette), MSB first
        const uint32_t bit = (uint32_t)i * (uint32_t)depth;
        s0 = ((uint32_t)row[bit >> 3] >> (8u - (uint32_t)depth - (bit & 7u))) & ((1u << depth) - 1u);
        s1 = s2 = s0;
    } else {
        const size_t step = depth == 16 ? 2 : 1;                // (16-bit: the high byte comes first)
        const uint8_t* px = row + (size_t)i * (size_t)channels * step;
        s0 = px[0];
        s1 = s2 = s0;
        if (channels >= 3) { s1 = px[step]; s2 = px[2 * step]; }
    }
    if (colour == 3) {
        const uint8_t* pal = files + it.plte_off;
        const bool in = s0 < it.plan.plte_entries;              // (entries <= 256: 3 * s0 + 2 < 768)
        const uint32_t e = in ? s0 : 0u;
        s0 = in ? pal[3u * e] : 0u;
        s1 = in ? pal[3u * e + 1u] : 0u;
        s2 = in ? pal[3u * e + 2u] : 0u;
    } else if (depth < 8) {
        s0 *= depth == 1 ? 255u : (depth == 2 ? 85u : 17u);
        s1 = s2 = s0;
    }
    uint8_t* dst = out + it.out_off + idx * 3ull;
    dst[0] = (uint8_t)(bgr ? s2 : s0);
    dst[1] = (uint8_t)s1;
    dst[2] = (uint8_t)(bgr ? s0 : s2);
}

}  // namespace
}  // namespace frcnn

using namespace frcnn;

// ------------------------------------------------------------------------------- the entry points: the host half is png_dec_host.h
extern "C" int frcnn_png_dec_full_version(void) { return FRCNN_PNG_DEC_FULL_VERSION; }

extern "C" int frcnn_png_dec_full_plan(const uint8_t* file_host, size_t len, frcnn_png_dec_full_plan_t* plan) {
    if (!plan || (!file_host && len)) return fail(FRCNN_E_ARG, "png_dec_full_plan: null pointer");
    return pd_walk("png_dec_full_plan", pd_ihdr_full, file_host, len, plan);
}

extern "C" int frcnn_png_dec_full_spans(const uint8_t* file_host, size_t len, const frcnn_png_dec_full_plan_t* plan, uint32_t* spans, size_t capacity) {
    return pd_spans("png_dec_full_spans", file_host, len, plan, spans, capacity);
}

extern "C" size_t frcnn_png_dec_full_workspace_bytes(const frcnn_png_dec_full_plan_t* plan) { return pd_workspace_bytes(plan); }

extern "C" size_t frcnn_png_dec_full_batch_layout(const frcnn_png_dec_full_plan_t* plans, int n, uint64_t* ws_off) { return pd_batch_layout(plans, n, ws_off); }

extern "C" int frcnn_png_decode_full_batch_u8(const frcnn_png_dec_full_batch_item_t* items_host, const frcnn_png_dec_full_batch_item_t* items_dev, int n,
                                              const uint8_t* files_dev, size_t files_capacity, int bgr, uint8_t* out_dev, size_t out_capacity,
                                              int32_t* status_dev, void* workspace, size_t workspace_capacity, void* stream) {
    if (const int code = pd_check_batch("png_decode_full_batch_u8", items_host, items_dev, n, files_dev, files_capacity, out_dev, out_capacity,
                                        status_dev, workspace, workspace_capacity))
        return code;
    unsigned long long pixels = 0;                              // the largest frame: the expand kernel's grid
    for (int i = 0; i < n; ++i) {
        const unsigned long long area = (unsigned long long)items_host[i].plan.h * items_host[i].plan.w;
        if (area > pixels) pixels = area;
    }
    hipStream_t s = as_stream(stream);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    const unsigned blocks = (unsigned)((pixels + PDF_EXPAND_THREADS - 1) / PDF_EXPAND_THREADS);    // (pixels < 2^32: at most 2^24 blocks)
    k_png_dec_inflate<FItem><<<n, PD_THREADS, 0, s>>>(files_dev, items_dev, ws, status_dev);
    k_png_dec_full_unfilter<<<dim3(7, n), PD_UNF_THREADS, 0, s>>>(items_dev, ws, status_dev);
    k_png_dec_full_expand<<<dim3(blocks, n), PDF_EXPAND_THREADS, 0, s>>>(files_dev, items_dev, ws, bgr ? 1 : 0, out_dev);
    return check_launch("png_decode_full_batch_u8");
}
