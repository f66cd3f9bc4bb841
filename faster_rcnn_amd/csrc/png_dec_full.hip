// The rest of PNG's still images decoded on the device (include/ext/frcnn_hip_png_dec_full.h): palette files, 1/2/4-bit and 16-bit
// samples, grey + alpha and Adam7 interlace, beside everything png_dec.hip takes.  THREE launches per batch, whatever the number of
// files, that allocate nothing, synchronise nothing and read nothing on the host.  gfx950 (CDNA4) only, wave64 throughout, plain HIP:
// vector stores and vector atomics, no inline assembly.  PNG is lossless: Pillow is the oracle, byte for byte.
//
//   k_png_dec_full_inflate   pd_inflate_body of png_dec_common.h, the code k_png_dec_inflate runs: ONE workgroup of 512 lanes per file.
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
// Bounds (the argument of png_dec.hip, extended).  The host checks on items_host that every item's stream, palette (colour type 3),
// region and frame lie inside the buffers, that regions and frames are disjoint, and that inflated_len is the sum over the existing
// passes of ph * (1 + ceil(pw * bits / 8)) for the plan's h, w, colour type, depth and interlace; the kernels compute every address from
// those fields through the SAME function (pdf_pass, pdf_pass_offset), never from anything read from the stream.  The inflate is
// pd_inflate_body with stream_len and inflated_len.  The unfilter wave of pass k reads and writes rows
// offset_k + row * (1 + rowbytes_k) + [0, 1 + rowbytes_k) for row < ph_k only: inside [0, inflated_len) since the passes' sizes sum to
// it.  The expand lane exists for row < h, x < w only (its index is below h * w) and writes that pixel alone; the sample it reads lies
// at byte 1 + floor(i * bits / 8) + (at most 7) of a row of its pass with i < pw_k: inside that row.  A palette index is compared with
// plte_entries (1..256, checked on the host) before the lookup at 3 * index + [0, 3) of the item's 768 staged bytes.  A filter byte above
// 4 in any pass sets FRCNN_PNG_DEC_FILTER (an atomic OR: the passes' waves share the word) and is treated as 0.  Loops run over h, w
// and the pass table.  The one barrier of the unfilter kernel closes a strip: the strip count depends on ph_k alone, uniform over the
// workgroup, and the early return is decided by blockIdx and the plan.
#include "png_dec_common.h"
#include "../../include/ext/frcnn_hip_png_dec_full.h"

namespace frcnn {
namespace {

constexpr int PDF_EXPAND_THREADS = 256;
static_assert(FRCNN_PNG_DEC_FULL_PLTE_BYTES == 768, "256 entries of R,G,B");

using FPlan = frcnn_png_dec_full_plan_t;
using FItem = frcnn_png_dec_full_batch_item_t;

// samples per pixel of a colour type, 0 for one PNG does not have
__host__ __device__ inline int pdf_channels(int colour) { return colour == 0 || colour == 3 ? 1 : (colour == 2 ? 3 : (colour == 4 ? 2 : (colour == 6 ? 4 : 0))); }

// nullptr for a (colour type, depth) pair of the supported set, else what it is
inline const char* pdf_pair_fault(int colour, int depth) {
    if (pdf_channels(colour) == 0) return "colour type";
    const bool listed = colour == 0 ? (depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16)
                      : colour == 3 ? (depth == 1 || depth == 2 || depth == 4 || depth == 8) : (depth == 8 || depth == 16);
    if (!listed) return "depth / colour type pair";
    if (colour == 0 && depth == 16) return "16-bit grey";
    return nullptr;
}

struct PdfPass { int x0, y0, dx, dy, pw, ph; };

// Pass k (0..6) of an h x w frame: the seven Adam7 sub-images, or the frame itself as pass 0 (the others absent: pw = ph = 0).
__host__ __device__ inline PdfPass pdf_pass(int k, int interlace, int h, int w) {
    PdfPass p;
    if (!interlace) {
        p.x0 = 0; p.y0 = 0; p.dx = 1; p.dy = 1;
        p.pw = k == 0 ? w : 0;
        p.ph = k == 0 ? h : 0;
        return p;
    }
    const int s = 4 * k;                                        // a nibble per pass: x0 = 0 4 0 2 0 1 0, y0 = 0 0 4 0 2 0 1, dx = 8 8 4 4 2 2 1, dy = 8 8 8 4 4 2 2
    p.x0 = (int)((0x0102040u >> s) & 15u);
    p.y0 = (int)((0x1020400u >> s) & 15u);
    p.dx = (int)((0x1224488u >> s) & 15u);
    p.dy = (int)((0x2244888u >> s) & 15u);
    p.pw = w > p.x0 ? (w - p.x0 + p.dx - 1) / p.dx : 0;
    p.ph = h > p.y0 ? (h - p.y0 + p.dy - 1) / p.dy : 0;
    return p;
}

__host__ __device__ inline unsigned long long pdf_rowbytes(int pw, int bits) { return ((unsigned long long)pw * (unsigned)bits + 7ull) / 8ull; }

// bytes of the passes in front of pass k (k = 7: of all passes, the inflated length)
__host__ __device__ inline unsigned long long pdf_pass_offset(int k, int interlace, int h, int w, int bits) {
    unsigned long long at = 0;
    for (int j = 0; j < k; ++j) {
        const PdfPass p = pdf_pass(j, interlace, h, w);
        if (p.pw > 0 && p.ph > 0) at += (unsigned long long)p.ph * (1ull + pdf_rowbytes(p.pw, bits));
    }
    return at;
}

// nullptr when the plan's fields agree with each other (what the kernels' bounds rest on), else what is wrong
inline const char* pdf_plan_fault(const FPlan& p) {
    if (p.h < 1 || p.w < 1 || p.h > 65535 || p.w > 65535) return "sides outside 1..65535";
    if (const char* what = pdf_pair_fault(p.colour_type, p.bit_depth)) return what;
    if (p.interlace != 0 && p.interlace != 1) return "interlace";
    const unsigned long long inflated = pdf_pass_offset(7, p.interlace, p.h, p.w, pdf_channels(p.colour_type) * p.bit_depth);
    if (inflated >= FRCNN_PNG_DEC_MAX_INFLATED || inflated != p.inflated_len) return "inflated length";
    if (p.stream_len < 6 || p.stream_len >= PD_MAX_STREAM) return "stream length";
    if (p.colour_type == 3 && (p.plte_entries < 1 || p.plte_entries > 256)) return "palette entries outside 1..256";
    return nullptr;
}

// ------------------------------------------------------------------------------------------------------------------- the kernels
// grid.x = item: the inflate of revision 1
__global__ void __launch_bounds__(PD_THREADS) k_png_dec_full_inflate(const uint8_t* files, const FItem* __restrict__ items, uint8_t* workspace, int32_t* status) {
    const FItem& it = items[blockIdx.x];
    pd_inflate_body(files + it.file_off, it.plan.stream_len, it.plan.inflated_len, workspace + it.ws_off, status + blockIdx.x);
}

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

// ------------------------------------------------------------------------------------------------------------------ the planner
#define PDF_UNSUPPORTED(...) return fail(FRCNN_E_UNSUPPORTED, "png_dec_full_plan: " __VA_ARGS__)

int pdf_plan(const uint8_t* d, size_t n, FPlan* out) {
    static const uint8_t SIG[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    FPlan p = {};
    if (n == 0) PDF_UNSUPPORTED("empty file");
    if (n < 8) PDF_UNSUPPORTED("not a PNG file (no signature)");
    for (int i = 0; i < 8; ++i)
        if (d[i] != SIG[i]) PDF_UNSUPPORTED("not a PNG file (no signature)");
    if (n > 0xFFFFFFFFull) PDF_UNSUPPORTED("a file of %zu bytes", n);
    p.file_len = (uint32_t)n;
    size_t pos = 8;
    bool ihdr = false, iend = false, closed = false, late_plte = false;
    unsigned long long stream = 0;
    uint8_t zh[2] = {0, 0};
    while (!iend) {
        if (pos + 12 > n) PDF_UNSUPPORTED("truncated: the chunk at byte %zu is cut short%s", pos, pos == n ? " (no IEND)" : "");
        const size_t clen = pd_be32(d + pos);
        const uint8_t* type = d + pos + 4;
        if (clen > n - pos - 12) PDF_UNSUPPORTED("truncated: chunk %.4s at byte %zu is cut short", (const char*)type, pos);
        const uint8_t* data = type + 4;
        auto named = [&](const char* s) { return type[0] == (uint8_t)s[0] && type[1] == (uint8_t)s[1] && type[2] == (uint8_t)s[2] && type[3] == (uint8_t)s[3]; };
        if (!ihdr) {
            if (!named("IHDR") || clen != 13) PDF_UNSUPPORTED("the first chunk is not IHDR");
            if (pd_crc(type, 4 + clen) != pd_be32(data + clen)) PDF_UNSUPPORTED("CRC mismatch in IHDR");
            ihdr = true;
            const uint32_t w = pd_be32(data), h = pd_be32(data + 4);
            const int depth = data[8], colour = data[9];
            if (pdf_channels(colour) == 0) PDF_UNSUPPORTED("colour type %d", colour);
            if (colour == 0 && depth == 16)
                PDF_UNSUPPORTED("16-bit grey (colour type 0 at depth 16: Pillow reads it as I;16 and saturates, so the host decodes it)");
            if (pdf_pair_fault(colour, depth)) PDF_UNSUPPORTED("%d-bit samples with colour type %d: not a pair the PNG specification lists", depth, colour);
            if (data[10] != 0) PDF_UNSUPPORTED("compression method %d", data[10]);
            if (data[11] != 0) PDF_UNSUPPORTED("filter method %d", data[11]);
            if (data[12] > 1) PDF_UNSUPPORTED("interlace method %d", data[12]);
            if (w < 1 || h < 1 || w > 65535 || h > 65535) PDF_UNSUPPORTED("frame %ux%u: both sides in 1..65535", h, w);
            p.h = (int32_t)h;
            p.w = (int32_t)w;
            p.colour_type = colour;
            p.bit_depth = depth;
            p.interlace = data[12];
        } else if (named("IDAT")) {
            if (closed) PDF_UNSUPPORTED("IDAT chunks that do not follow each other");
            if (pd_crc(type, 4 + clen) != pd_be32(data + clen)) PDF_UNSUPPORTED("CRC mismatch in the IDAT at byte %zu", pos);
            if (!p.idat_count) p.idat_off = (uint32_t)pos;
            p.idat_count += 1;
            for (size_t i = 0; i < clen && stream + i < 2; ++i) zh[stream + i] = data[i];
            stream += clen;
        } else {
            if (p.idat_count) closed = true;
            if (named("IEND")) iend = true;
            else if (named("acTL") || named("fcTL") || named("fdAT")) PDF_UNSUPPORTED("APNG (chunk %.4s)", (const char*)type);
            else if (named("IHDR")) PDF_UNSUPPORTED("two IHDR chunks");
            else if (named("PLTE")) {
                if (p.colour_type == 3) {                       // (in every other colour type a PLTE is a suggestion: skipped)
                    if (p.idat_count) late_plte = true;
                    else {
                        if (p.plte_entries) PDF_UNSUPPORTED("two PLTE chunks");
                        if (clen < 3 || clen > 768 || clen % 3) PDF_UNSUPPORTED("a PLTE of %zu bytes: 1 to 256 entries of 3", clen);
                        if (pd_crc(type, 4 + clen) != pd_be32(data + clen)) PDF_UNSUPPORTED("CRC mismatch in PLTE");
                        p.plte_off = (uint32_t)(pos + 8);
                        p.plte_entries = (uint32_t)(clen / 3);
                    }
                }
            } else if (!(type[0] & 0x20)) PDF_UNSUPPORTED("unknown critical chunk %.4s", (const char*)type);
        }
        pos += 12 + clen;
    }
    if (!p.idat_count) PDF_UNSUPPORTED("no IDAT");
    if (p.colour_type == 3 && !p.plte_entries) {
        if (late_plte) PDF_UNSUPPORTED("palette file with its PLTE behind an IDAT");
        PDF_UNSUPPORTED("palette file without PLTE");
    }
    if (stream >= PD_MAX_STREAM) PDF_UNSUPPORTED("IDAT payload of %llu bytes (the device takes fewer than %u)", stream, PD_MAX_STREAM);
    if (stream < 6) PDF_UNSUPPORTED("truncated: a zlib stream of %llu bytes", stream);
    if ((zh[0] & 15) != 8) PDF_UNSUPPORTED("zlib compression method %d", zh[0] & 15);
    if ((zh[0] >> 4) > 7) PDF_UNSUPPORTED("zlib window above 32 KiB");
    if ((((unsigned)zh[0] << 8) | zh[1]) % 31u) PDF_UNSUPPORTED("bad zlib header check");
    if (zh[1] & 0x20) PDF_UNSUPPORTED("zlib preset dictionary");
    const unsigned long long inflated = pdf_pass_offset(7, p.interlace, p.h, p.w, pdf_channels(p.colour_type) * p.bit_depth);
    if (inflated >= FRCNN_PNG_DEC_MAX_INFLATED) PDF_UNSUPPORTED("frame %dx%d inflates to %llu bytes (the device takes fewer than 2^31)", p.h, p.w, inflated);
    p.stream_len = (uint32_t)stream;
    p.inflated_len = (uint32_t)inflated;
    *out = p;
    return FRCNN_OK;
}

}  // namespace
}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_png_dec_full_version(void) { return FRCNN_PNG_DEC_FULL_VERSION; }

extern "C" int frcnn_png_dec_full_plan(const uint8_t* file_host, size_t len, frcnn_png_dec_full_plan_t* plan) {
    if (!plan || (!file_host && len)) return fail(FRCNN_E_ARG, "png_dec_full_plan: null pointer");
    return pdf_plan(file_host, len, plan);
}

extern "C" int frcnn_png_dec_full_spans(const uint8_t* file_host, size_t len, const frcnn_png_dec_full_plan_t* plan, uint32_t* spans, size_t capacity) {
    if (!file_host || !plan || !spans) return fail(FRCNN_E_ARG, "png_dec_full_spans: null pointer");
    if (capacity < plan->idat_count) return fail(FRCNN_E_ARG, "png_dec_full_spans: room for %zu spans, the plan has %u", capacity, plan->idat_count);
    if (len != plan->file_len) return fail(FRCNN_E_ARG, "png_dec_full_spans: a file of %zu bytes, the plan was made of %u", len, plan->file_len);
    size_t pos = plan->idat_off;
    unsigned long long sum = 0;
    for (uint32_t k = 0; k < plan->idat_count; ++k) {
        if (pos > len || len - pos < 12) return fail(FRCNN_E_ARG, "png_dec_full_spans: not the file the plan was made of");
        const size_t clen = pd_be32(file_host + pos);
        if (clen > len - pos - 12 || file_host[pos + 4] != 'I' || file_host[pos + 5] != 'D' || file_host[pos + 6] != 'A' || file_host[pos + 7] != 'T')
            return fail(FRCNN_E_ARG, "png_dec_full_spans: not the file the plan was made of");
        spans[2 * k] = (uint32_t)(pos + 8);
        spans[2 * k + 1] = (uint32_t)clen;
        sum += clen;
        pos += 12 + clen;
    }
    if (sum != plan->stream_len) return fail(FRCNN_E_ARG, "png_dec_full_spans: not the file the plan was made of");
    return FRCNN_OK;
}

extern "C" size_t frcnn_png_dec_full_workspace_bytes(const frcnn_png_dec_full_plan_t* plan) {
    if (!plan || pdf_plan_fault(*plan)) return 0;
    return pd_align16(plan->inflated_len);
}

extern "C" size_t frcnn_png_dec_full_batch_layout(const frcnn_png_dec_full_plan_t* plans, int n, uint64_t* ws_off) {
    if (!plans || !ws_off || n < 1 || n > FRCNN_PNG_DEC_BATCH_MAX) return 0;
    for (int i = 0; i < n; ++i)
        if (pdf_plan_fault(plans[i])) return 0;
    size_t at = 0;
    for (int i = 0; i < n; ++i) { ws_off[i] = at; at += pd_align16(plans[i].inflated_len); }
    return at;
}

extern "C" int frcnn_png_decode_full_batch_u8(const frcnn_png_dec_full_batch_item_t* items_host, const frcnn_png_dec_full_batch_item_t* items_dev, int n,
                                              const uint8_t* files_dev, size_t files_capacity, int bgr, uint8_t* out_dev, size_t out_capacity,
                                              int32_t* status_dev, void* workspace, size_t workspace_capacity, void* stream) {
    if (!items_host || !items_dev || !files_dev || !out_dev || !status_dev || !workspace) return fail(FRCNN_E_ARG, "png_decode_full_batch_u8: null pointer");
    if (n < 1 || n > FRCNN_PNG_DEC_BATCH_MAX) return fail(FRCNN_E_ARG, "png_decode_full_batch_u8: n=%d outside 1..%d", n, FRCNN_PNG_DEC_BATCH_MAX);
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return fail(FRCNN_E_ARG, "png_decode_full_batch_u8: workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(status_dev) & 3u) return fail(FRCNN_E_ARG, "png_decode_full_batch_u8: status_dev must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(items_dev) & 7u) return fail(FRCNN_E_ARG, "png_decode_full_batch_u8: items_dev must be 8-byte aligned");
    PdRange outs[FRCNN_PNG_DEC_BATCH_MAX], regions[FRCNN_PNG_DEC_BATCH_MAX];
    unsigned long long pixels = 0;
    for (int i = 0; i < n; ++i) {
        const FItem& it = items_host[i];
        const FPlan& p = it.plan;
        if (const char* what = pdf_plan_fault(p)) return fail(FRCNN_E_ARG, "png_decode_full_batch_u8: item %d: the plan contradicts itself (%s)", i, what);
        const unsigned long long area = (unsigned long long)p.h * p.w, frame = area * 3, need = pd_align16(p.inflated_len);
        if (it.file_off > files_capacity || p.stream_len > files_capacity - it.file_off)
            return fail(FRCNN_E_ARG, "png_decode_full_batch_u8: item %d: file_off=%llu + stream_len=%u beyond files_capacity=%zu", i, (unsigned long long)it.file_off, p.stream_len, files_capacity);
        if (p.colour_type == 3 && (it.plte_off > files_capacity || FRCNN_PNG_DEC_FULL_PLTE_BYTES > files_capacity - it.plte_off))
            return fail(FRCNN_E_ARG, "png_decode_full_batch_u8: item %d: plte_off=%llu + %d beyond files_capacity=%zu", i, (unsigned long long)it.plte_off, FRCNN_PNG_DEC_FULL_PLTE_BYTES, files_capacity);
        if (it.out_off > out_capacity || frame > out_capacity - it.out_off)
            return fail(FRCNN_E_ARG, "png_decode_full_batch_u8: item %d: out_off=%llu + %d * %d * 3 beyond out_capacity=%zu", i, (unsigned long long)it.out_off, p.h, p.w, out_capacity);
        if (it.ws_off & 15u) return fail(FRCNN_E_ARG, "png_decode_full_batch_u8: item %d: ws_off=%llu must be 16-byte aligned", i, (unsigned long long)it.ws_off);
        if (it.ws_off > workspace_capacity || need > workspace_capacity - it.ws_off)
            return fail(FRCNN_E_ARG, "png_decode_full_batch_u8: item %d: ws_off=%llu + %llu beyond workspace_capacity=%zu", i, (unsigned long long)it.ws_off, need, workspace_capacity);
        outs[i] = {it.out_off, it.out_off + frame, i};
        regions[i] = {it.ws_off, it.ws_off + need, i};
        if (area > pixels) pixels = area;
    }
    int k = pd_overlap(outs, n);
    if (k >= 0) return fail(FRCNN_E_ARG, "png_decode_full_batch_u8: the output ranges of items %d and %d overlap", outs[k].item, outs[k + 1].item);
    k = pd_overlap(regions, n);
    if (k >= 0) return fail(FRCNN_E_ARG, "png_decode_full_batch_u8: the workspace regions of items %d and %d overlap", regions[k].item, regions[k + 1].item);
    hipStream_t s = as_stream(stream);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    const unsigned blocks = (unsigned)((pixels + PDF_EXPAND_THREADS - 1) / PDF_EXPAND_THREADS);    // (pixels < 2^32: at most 2^24 blocks)
    k_png_dec_full_inflate<<<n, PD_THREADS, 0, s>>>(files_dev, items_dev, ws, status_dev);
    k_png_dec_full_unfilter<<<dim3(7, n), PD_UNF_THREADS, 0, s>>>(items_dev, ws, status_dev);
    k_png_dec_full_expand<<<dim3(blocks, n), PDF_EXPAND_THREADS, 0, s>>>(files_dev, items_dev, ws, bgr ? 1 : 0, out_dev);
    return check_launch("png_decode_full_batch_u8");
}
