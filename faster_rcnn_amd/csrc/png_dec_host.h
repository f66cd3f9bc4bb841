// The host half of the two device PNG decoders, in ONE place: png_dec.hip (revision 1 of include/ext/frcnn_hip_png_dec.h) and
// png_dec_full.hip (include/ext/frcnn_hip_png_dec_full.h) keep their own reconstruction kernels and their own extern "C" entry points;
// everything those entry points do before a launch is here.  The chunk walker (pd_walk: one walk, the IHDR acceptance check handed in),
// the IDAT span walk, the workspace size and the batch layout, the plan-consistency check (pd_plan_fault) with the pass geometry it rests
// on, and the argument check of a batch (pd_check_batch).  A revision-1 plan is checked as the full-format plan that says the same
// (pd_widen).  Everything sits in an unnamed namespace, as in png_dec_common.h.
//
// Bounds, the host's share (the kernels' share is at the top of png_dec.hip and png_dec_full.hip, which refer to this text).  The
// planner never reads past d + n: a chunk's 12 bytes of frame and its clen bytes of data are compared with the rest of the file before
// either is looked at, and the span walk repeats that against the plan's offsets.  pd_check_batch runs on items_host, the table the
// caller keeps, and refuses with FRCNN_E_ARG before any launch or device call unless for every item: the plan agrees with itself
// (pd_plan_fault: inflated_len IS the sum over the existing passes of ph * (1 + ceil(pw * bits / 8)) for the plan's h, w, colour type,
// depth and interlace, computed by pdf_pass / pdf_pass_offset, the SAME functions the full-format kernels compute their addresses with;
// for revision 1 that is h * (1 + w * channels)); [file_off, file_off + stream_len) lies inside files_capacity, for a colour-type-3 item
// also [plte_off, plte_off + 768); [out_off, out_off + h * w * 3) inside out_capacity; [ws_off, ws_off + align16(inflated_len)) inside
// workspace_capacity, ws_off 16-byte aligned; and no two items' output ranges or workspace regions overlap.  The kernels rest on
// plan.stream_len, plan.inflated_len, h, w and the format fields alone, never on anything read from the stream.
#pragma once
#include <type_traits>

#include "png_dec_common.h"
#include "../../include/ext/frcnn_hip_png_dec_full.h"

namespace frcnn {
namespace {

using Plan = frcnn_png_dec_plan_t;
using Item = frcnn_png_dec_batch_item_t;
using FPlan = frcnn_png_dec_full_plan_t;
using FItem = frcnn_png_dec_full_batch_item_t;
static_assert(FRCNN_PNG_DEC_FULL_PLTE_BYTES == 768, "256 entries of R,G,B");

// ------------------------------------------------------------------------------------------------------------ the pass geometry
// samples per pixel of a colour type, 0 for one PNG does not have
__host__ __device__ inline int pdf_channels(int colour) { return colour == 0 || colour == 3 ? 1 : (colour == 2 ? 3 : (colour == 4 ? 2 : (colour == 6 ? 4 : 0))); }

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

// ------------------------------------------------------------------------------------------------------- is a plan what it says
const char PD_NO_COLOUR[] = "colour type";

// nullptr for a (colour type, depth) pair of the supported set, else what it is
inline const char* pdf_pair_fault(int colour, int depth) {
    if (pdf_channels(colour) == 0) return PD_NO_COLOUR;
    const bool listed = colour == 0 ? (depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16)
                      : colour == 3 ? (depth == 1 || depth == 2 || depth == 4 || depth == 8) : (depth == 8 || depth == 16);
    if (!listed) return "depth / colour type pair";
    if (colour == 0 && depth == 16) return "16-bit grey";
    return nullptr;
}

// nullptr when the plan's fields agree with each other (what the kernels' bounds rest on), else what is wrong
inline const char* pd_plan_fault(const FPlan& p) {
    if (p.h < 1 || p.w < 1 || p.h > 65535 || p.w > 65535) return "sides outside 1..65535";
    if (const char* what = pdf_pair_fault(p.colour_type, p.bit_depth)) return what;
    if (p.interlace != 0 && p.interlace != 1) return "interlace";
    const unsigned long long inflated = pdf_pass_offset(7, p.interlace, p.h, p.w, pdf_channels(p.colour_type) * p.bit_depth);
    if (inflated >= FRCNN_PNG_DEC_MAX_INFLATED || inflated != p.inflated_len) return "inflated length";
    if (p.stream_len < 6 || p.stream_len >= PD_MAX_STREAM) return "stream length";
    if (p.colour_type == 3 && (p.plte_entries < 1 || p.plte_entries > 256)) return "palette entries outside 1..256";
    return nullptr;
}

// The full-format plan that says what a revision-1 plan says: depth 8, no interlace, no palette; a channel count revision 1 does not
// have becomes a colour type PNG does not have.
inline FPlan pd_widen(const Plan& p) {
    FPlan f = {};
    f.h = p.h; f.w = p.w; f.bit_depth = 8;
    f.colour_type = p.channels == 1 ? 0 : (p.channels == 3 ? 2 : (p.channels == 4 ? 6 : -1));
    f.file_len = p.file_len; f.idat_off = p.idat_off; f.idat_count = p.idat_count;
    f.stream_len = p.stream_len; f.inflated_len = p.inflated_len;
    return f;
}

inline const char* pd_plan_fault(const Plan& p) {
    const char* what = pd_plan_fault(pd_widen(p));
    return what == PD_NO_COLOUR ? "channels" : what;           // (a revision-1 plan says its colour type in ``channels``)
}

// ------------------------------------------------------------------------------------------------------------------ the planner
#define PD_UNSUPPORTED(fmt, ...) return fail(FRCNN_E_UNSUPPORTED, "%s: " fmt, who, ##__VA_ARGS__)

// What the walker asks of its caller: FRCNN_OK for an IHDR (``ihdr``: its 13 bytes, sides ``h`` x ``w``) of the caller's supported set,
// else the refusal made with PD_UNSUPPORTED.
using PdIhdrCheck = int (*)(const char* who, const uint8_t* ihdr, uint32_t h, uint32_t w);

// Revision 1: 8-bit grey, RGB and RGBA without interlace.
inline int pd_ihdr_rev1(const char* who, const uint8_t* ihdr, uint32_t h, uint32_t w) {
    const int depth = ihdr[8], colour = ihdr[9];
    if (colour == 3) PD_UNSUPPORTED("palette (colour type 3)");
    if (colour == 4) PD_UNSUPPORTED("grey + alpha (colour type 4)");
    if (colour != 0 && colour != 2 && colour != 6) PD_UNSUPPORTED("colour type %d", colour);
    if (depth != 8) PD_UNSUPPORTED("%d-bit samples", depth);
    if (ihdr[10] != 0) PD_UNSUPPORTED("compression method %d", ihdr[10]);
    if (ihdr[11] != 0) PD_UNSUPPORTED("filter method %d", ihdr[11]);
    if (ihdr[12] != 0) PD_UNSUPPORTED("interlaced (Adam7)");
    if (w < 1 || h < 1 || w > 65535 || h > 65535) PD_UNSUPPORTED("frame %ux%u: both sides in 1..65535", h, w);
    return FRCNN_OK;
}

// The full format: every pair the PNG specification lists but 16-bit grey, with or without Adam7.
inline int pd_ihdr_full(const char* who, const uint8_t* ihdr, uint32_t h, uint32_t w) {
    const int depth = ihdr[8], colour = ihdr[9];
    if (pdf_channels(colour) == 0) PD_UNSUPPORTED("colour type %d", colour);
    if (colour == 0 && depth == 16)
        PD_UNSUPPORTED("16-bit grey (colour type 0 at depth 16: Pillow reads it as I;16 and saturates, so the host decodes it)");
    if (pdf_pair_fault(colour, depth)) PD_UNSUPPORTED("%d-bit samples with colour type %d: not a pair the PNG specification lists", depth, colour);
    if (ihdr[10] != 0) PD_UNSUPPORTED("compression method %d", ihdr[10]);
    if (ihdr[11] != 0) PD_UNSUPPORTED("filter method %d", ihdr[11]);
    if (ihdr[12] > 1) PD_UNSUPPORTED("interlace method %d", ihdr[12]);
    if (w < 1 || h < 1 || w > 65535 || h > 65535) PD_UNSUPPORTED("frame %ux%u: both sides in 1..65535", h, w);
    return FRCNN_OK;
}

// The chunk walk of both planners: ``who`` names the entry point in the refusals, ``accepts`` is its IHDR check.  A PLTE counts for
// colour type 3 alone (which pd_ihdr_rev1 never lets this far); in every other colour type it is a suggestion and skipped.
inline int pd_walk(const char* who, PdIhdrCheck accepts, const uint8_t* d, size_t n, FPlan* out) {
    static const uint8_t SIG[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    FPlan p = {};
    if (n == 0) PD_UNSUPPORTED("empty file");
    if (n < 8) PD_UNSUPPORTED("not a PNG file (no signature)");
    for (int i = 0; i < 8; ++i)
        if (d[i] != SIG[i]) PD_UNSUPPORTED("not a PNG file (no signature)");
    if (n > 0xFFFFFFFFull) PD_UNSUPPORTED("a file of %zu bytes", n);
    p.file_len = (uint32_t)n;
    size_t pos = 8;
    bool ihdr = false, iend = false, closed = false, late_plte = false;
    unsigned long long stream = 0;
    uint8_t zh[2] = {0, 0};
    while (!iend) {
        if (pos + 12 > n) PD_UNSUPPORTED("truncated: the chunk at byte %zu is cut short%s", pos, pos == n ? " (no IEND)" : "");
        const size_t clen = pd_be32(d + pos);
        const uint8_t* type = d + pos + 4;
        if (clen > n - pos - 12) PD_UNSUPPORTED("truncated: chunk %.4s at byte %zu is cut short", (const char*)type, pos);
        const uint8_t* data = type + 4;
        auto named = [&](const char* s) { return type[0] == (uint8_t)s[0] && type[1] == (uint8_t)s[1] && type[2] == (uint8_t)s[2] && type[3] == (uint8_t)s[3]; };
        if (!ihdr) {
            if (!named("IHDR") || clen != 13) PD_UNSUPPORTED("the first chunk is not IHDR");
            if (pd_crc(type, 4 + clen) != pd_be32(data + clen)) PD_UNSUPPORTED("CRC mismatch in IHDR");
            ihdr = true;
            const uint32_t w = pd_be32(data), h = pd_be32(data + 4);
            if (const int code = accepts(who, data, h, w)) return code;
            p.h = (int32_t)h;
            p.w = (int32_t)w;
            p.bit_depth = data[8];
            p.colour_type = data[9];
            p.interlace = data[12];
        } else if (named("IDAT")) {
            if (closed) PD_UNSUPPORTED("IDAT chunks that do not follow each other");
            if (pd_crc(type, 4 + clen) != pd_be32(data + clen)) PD_UNSUPPORTED("CRC mismatch in the IDAT at byte %zu", pos);
            if (!p.idat_count) p.idat_off = (uint32_t)pos;
            p.idat_count += 1;
            for (size_t i = 0; i < clen && stream + i < 2; ++i) zh[stream + i] = data[i];
            stream += clen;
        } else {
            if (p.idat_count) closed = true;
            if (named("IEND")) iend = true;
            else if (named("acTL") || named("fcTL") || named("fdAT")) PD_UNSUPPORTED("APNG (chunk %.4s)", (const char*)type);
            else if (named("IHDR")) PD_UNSUPPORTED("two IHDR chunks");
            else if (named("PLTE")) {
                if (p.colour_type == 3) {
                    if (p.idat_count) late_plte = true;
                    else {
                        if (p.plte_entries) PD_UNSUPPORTED("two PLTE chunks");
                        if (clen < 3 || clen > 768 || clen % 3) PD_UNSUPPORTED("a PLTE of %zu bytes: 1 to 256 entries of 3", clen);
                        if (pd_crc(type, 4 + clen) != pd_be32(data + clen)) PD_UNSUPPORTED("CRC mismatch in PLTE");
                        p.plte_off = (uint32_t)(pos + 8);
                        p.plte_entries = (uint32_t)(clen / 3);
                    }
                }
            } else if (!(type[0] & 0x20)) PD_UNSUPPORTED("unknown critical chunk %.4s", (const char*)type);
        }
        pos += 12 + clen;
    }
    if (!p.idat_count) PD_UNSUPPORTED("no IDAT");
    if (p.colour_type == 3 && !p.plte_entries) {
        if (late_plte) PD_UNSUPPORTED("palette file with its PLTE behind an IDAT");
        PD_UNSUPPORTED("palette file without PLTE");
    }
    if (stream >= PD_MAX_STREAM) PD_UNSUPPORTED("IDAT payload of %llu bytes (the device takes fewer than %u)", stream, PD_MAX_STREAM);
    if (stream < 6) PD_UNSUPPORTED("truncated: a zlib stream of %llu bytes", stream);
    if ((zh[0] & 15) != 8) PD_UNSUPPORTED("zlib compression method %d", zh[0] & 15);
    if ((zh[0] >> 4) > 7) PD_UNSUPPORTED("zlib window above 32 KiB");
    if ((((unsigned)zh[0] << 8) | zh[1]) % 31u) PD_UNSUPPORTED("bad zlib header check");
    if (zh[1] & 0x20) PD_UNSUPPORTED("zlib preset dictionary");
    const unsigned long long inflated = pdf_pass_offset(7, p.interlace, p.h, p.w, pdf_channels(p.colour_type) * p.bit_depth);
    if (inflated >= FRCNN_PNG_DEC_MAX_INFLATED) PD_UNSUPPORTED("frame %dx%d inflates to %llu bytes (the device takes fewer than 2^31)", p.h, p.w, inflated);
    p.stream_len = (uint32_t)stream;
    p.inflated_len = (uint32_t)inflated;
    *out = p;
    return FRCNN_OK;
}

#undef PD_UNSUPPORTED

// ------------------------------------------------------------------------------- spans, sizes: the same for either kind of plan
template <class P>
int pd_spans(const char* who, const uint8_t* file_host, size_t len, const P* plan, uint32_t* spans, size_t capacity) {
    if (!file_host || !plan || !spans) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (capacity < plan->idat_count) return fail(FRCNN_E_ARG, "%s: room for %zu spans, the plan has %u", who, capacity, plan->idat_count);
    if (len != plan->file_len) return fail(FRCNN_E_ARG, "%s: a file of %zu bytes, the plan was made of %u", who, len, plan->file_len);
    size_t pos = plan->idat_off;
    unsigned long long sum = 0;
    for (uint32_t k = 0; k < plan->idat_count; ++k) {
        if (pos > len || len - pos < 12) return fail(FRCNN_E_ARG, "%s: not the file the plan was made of", who);
        const size_t clen = pd_be32(file_host + pos);
        if (clen > len - pos - 12 || file_host[pos + 4] != 'I' || file_host[pos + 5] != 'D' || file_host[pos + 6] != 'A' || file_host[pos + 7] != 'T')
            return fail(FRCNN_E_ARG, "%s: not the file the plan was made of", who);
        spans[2 * k] = (uint32_t)(pos + 8);
        spans[2 * k + 1] = (uint32_t)clen;
        sum += clen;
        pos += 12 + clen;
    }
    if (sum != plan->stream_len) return fail(FRCNN_E_ARG, "%s: not the file the plan was made of", who);
    return FRCNN_OK;
}

template <class P>
size_t pd_workspace_bytes(const P* plan) {
    if (!plan || pd_plan_fault(*plan)) return 0;
    return align16(plan->inflated_len);
}

template <class P>
size_t pd_batch_layout(const P* plans, int n, uint64_t* ws_off) {
    if (!plans || !ws_off || n < 1 || n > FRCNN_PNG_DEC_BATCH_MAX) return 0;
    for (int i = 0; i < n; ++i)
        if (pd_plan_fault(plans[i])) return 0;
    size_t at = 0;
    for (int i = 0; i < n; ++i) { ws_off[i] = at; at += align16(plans[i].inflated_len); }
    return at;
}

// ------------------------------------------------------------------------------------------------ the arguments of a batch call
// FRCNN_OK when the kernels may run on these arguments (the Bounds text above), else FRCNN_E_ARG with the reason, ``who`` in front.
template <class I>
int pd_check_batch(const char* who, const I* items_host, const I* items_dev, int n, const uint8_t* files_dev, size_t files_capacity,
                   const uint8_t* out_dev, size_t out_capacity, const int32_t* status_dev, const void* workspace, size_t workspace_capacity) {
    if (!items_host || !items_dev || !files_dev || !out_dev || !status_dev || !workspace) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (n < 1 || n > FRCNN_PNG_DEC_BATCH_MAX) return fail(FRCNN_E_ARG, "%s: n=%d outside 1..%d", who, n, FRCNN_PNG_DEC_BATCH_MAX);
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return fail(FRCNN_E_ARG, "%s: workspace must be 16-byte aligned", who);
    if (reinterpret_cast<uintptr_t>(status_dev) & 3u) return fail(FRCNN_E_ARG, "%s: status_dev must be 4-byte aligned", who);
    if (reinterpret_cast<uintptr_t>(items_dev) & 7u) return fail(FRCNN_E_ARG, "%s: items_dev must be 8-byte aligned", who);
    Range outs[FRCNN_PNG_DEC_BATCH_MAX], regions[FRCNN_PNG_DEC_BATCH_MAX];
    for (int i = 0; i < n; ++i) {
        const I& it = items_host[i];
        const auto& p = it.plan;
        if (const char* what = pd_plan_fault(p)) return fail(FRCNN_E_ARG, "%s: item %d: the plan contradicts itself (%s)", who, i, what);
        const unsigned long long frame = (unsigned long long)p.h * p.w * 3, need = align16(p.inflated_len);
        if (it.file_off > files_capacity || p.stream_len > files_capacity - it.file_off)
            return fail(FRCNN_E_ARG, "%s: item %d: file_off=%llu + stream_len=%u beyond files_capacity=%zu", who, i, (unsigned long long)it.file_off, p.stream_len, files_capacity);
        if constexpr (std::is_same<I, FItem>::value) {          // (the one item type with a palette)
            if (p.colour_type == 3 && (it.plte_off > files_capacity || FRCNN_PNG_DEC_FULL_PLTE_BYTES > files_capacity - it.plte_off))
                return fail(FRCNN_E_ARG, "%s: item %d: plte_off=%llu + %d beyond files_capacity=%zu", who, i, (unsigned long long)it.plte_off, FRCNN_PNG_DEC_FULL_PLTE_BYTES, files_capacity);
        }
        if (it.out_off > out_capacity || frame > out_capacity - it.out_off)
            return fail(FRCNN_E_ARG, "%s: item %d: out_off=%llu + %d * %d * 3 beyond out_capacity=%zu", who, i, (unsigned long long)it.out_off, p.h, p.w, out_capacity);
        if (it.ws_off & 15u) return fail(FRCNN_E_ARG, "%s: item %d: ws_off=%llu must be 16-byte aligned", who, i, (unsigned long long)it.ws_off);
        if (it.ws_off > workspace_capacity || need > workspace_capacity - it.ws_off)
            return fail(FRCNN_E_ARG, "%s: item %d: ws_off=%llu + %llu beyond workspace_capacity=%zu", who, i, (unsigned long long)it.ws_off, need, workspace_capacity);
        outs[i] = {it.out_off, it.out_off + frame, i};
        regions[i] = {it.ws_off, it.ws_off + need, i};
    }
    int k = range_overlap(outs, n);
    if (k >= 0) return fail(FRCNN_E_ARG, "%s: the output ranges of items %d and %d overlap", who, outs[k].item, outs[k + 1].item);
    k = range_overlap(regions, n);
    if (k >= 0) return fail(FRCNN_E_ARG, "%s: the workspace regions of items %d and %d overlap", who, regions[k].item, regions[k + 1].item);
    return FRCNN_OK;
}

}  // namespace
}  // namespace frcnn
