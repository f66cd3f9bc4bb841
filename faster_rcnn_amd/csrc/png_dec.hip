// PNG files decoded on the device (include/ext/frcnn_hip_png_dec.h): the zlib stream of a .png file (its IDAT payloads back to back, staged
// by the caller) in device memory -> an (h, w, 3) uint8 frame, the counterpart of the encoder (png.hip).  TWO launches per batch, whatever
// the number of files, that allocate nothing, synchronise nothing and read nothing on the host.  gfx950 (CDNA4) only, wave64 throughout,
// plain HIP: vector stores and LDS atomics, no inline assembly.  PNG is lossless: Pillow is the oracle, byte for byte.
//
//   k_png_dec_inflate   ONE workgroup of 512 lanes per file.  The deflate blocks are walked in order, uniformly by the workgroup.  A stored
//                       block is a cooperative copy.  For a fixed or dynamic block the code-length code, the literal/length code and the
//                       distance code are built in LDS as canonical codes: a lookahead table over 10 bits (length << 9 | symbol, indexed
//                       by the bits as they come, i.e. by the reversed code) and first / maxcode / delta per length for the longer codes.
//                       Then the block's data is taken in WINDOWS of 8 KiB of compressed stream on a fixed grid, staged in LDS, a stretch
//                       of S = 128 bits per lane.  A lane's state is its entry bit alone: a literal, or length + extra + distance +
//                       extra, is ONE token (at most 48 bits).  Every lane guesses that a token starts at its first bit, decodes to the
//                       end of its stretch (or to an end-of-block or an invalid code, which it hands on as its exit) and gives its exit to
//                       the next lane; every lane whose entry changed decodes again; the loop ends when no entry changed (a workgroup
//                       flag) and after 512 rounds at the latest, since round r fixes entry r for good.  The first validated end-of-block
//                       ends the block: the lanes behind it receive ENDED as their entry and count nothing.  A window without one hands
//                       its last exit to the next window, the tables stay.  A scan of the lanes' output-byte counts gives every token its
//                       position; the literals are written in parallel; the matches are resolved in rounds: each lane offers its next
//                       match, an LDS atomicMin finds the earliest unresolved one, and a match copies once its source lies wholly below
//                       that position (or when it IS the earliest: its source then starts below it and it copies in order, which is also
//                       right for distance < length).  A round always frees the earliest, so the rounds end.  At the end: the inflated
//                       length against h * (1 + w * channels) and the Adler-32 of the inflated bytes against the stream's.
//   k_png_dec_unfilter  ONE wave per file.  Strips of 64 rows follow one another; lane l takes row base + l at pixel t - l in step t, a
//                       diagonal wavefront: the pixel above comes from lane l - 1's previous step through a wave shuffle, the pixel above
//                       left is the one that came the step before, the left one the lane's own.  The last lane writes its reconstructed
//                       row back over the filtered bytes; lane 0 of the next strip reads the row above from there.  The frame is written
//                       directly as R,G,B or B,G,R, grey replicated, alpha dropped: there is no third pass.
//
// Bounds: why no input makes a kernel read or write outside its stream, its workspace region and its frame.  The host checks, on the
// table it is given, that every item's stream, region and frame lie inside the buffers and that regions and frames are disjoint; the
// kernels rest on plan.stream_len, plan.inflated_len, h, w, channels alone, never on anything read from the stream.  (a) The stream is
// read through pd_gbyte (zero at and past stream_len) and, staged through it, from the LDS window; the window is read through pd_peek,
// which returns zero for a word index outside the array.  (b) Every store into the workspace is `if (position < inflated_len)`; a match
// source is position - distance with distance <= position checked first, hence below a position that was itself checked.  A stored
// block's length is checked against the rest of the stream and the rest of the output before the copy.  (c) Table indices: a code length
// is masked to 0..15; a sorted-symbol index is checked against the table's count; the lookahead index is masked to 10 bits; literal/length
// symbols above 285 and distance symbols above 29 are invalid codes; the length list is filled only while it stays inside its 320 entries.
// (d) The unfilter kernel reads rows row * (1 + w * channels) + [0, 1 + w * channels) for row < h only: inside inflated_len; it writes
// pixel (row, x) for row < h, x < w.  Loops: a token is at least one bit long and a lane stops at the end of its stretch; the round loops
// are bounded as said above; a window starts at or past the previous window's end and the walk stops at the end of the stream (a token
// that would start at or past it is an invalid code); a block consumes at least three bits.  Whatever decides a barrier is read from LDS
// words that are written before a barrier and not again until every lane has read them: the workgroup never diverges around one.
//
// pd_inflate_body, the codes and the predictor live in png_dec_common.h: png_dec_full.hip (palette, sub-byte and 16-bit samples, grey +
// alpha, Adam7; include/ext/frcnn_hip_png_dec_full.h) runs the same inflate, and (a) - (c) hold for it with ITS plan's stream_len and
// inflated_len.  (d) extended to its two other kernels: k_png_dec_full_unfilter's wave of pass k touches rows offset_k + row * (1 +
// rowbytes_k) + [0, 1 + rowbytes_k) for row < ph_k only, where pw_k, ph_k, rowbytes_k and offset_k come from h, w, colour type, depth and
// interlace through the function with which the host checked that the passes sum to inflated_len; k_png_dec_full_expand has one lane per
// pixel (row < h, x < w), reads one sample inside such a row and, for a palette file, entry index < plte_entries <= 256 of the item's 768
// staged palette bytes, which the host checked to lie inside files_capacity; a filter byte above 4 in any pass sets FRCNN_PNG_DEC_FILTER;
// the unfilter kernel's one barrier and its early return are decided by blockIdx and the plan alone.  The full text is at the top of
// png_dec_full.hip.
#include "png_dec_common.h"

namespace frcnn {
namespace {

using Plan = frcnn_png_dec_plan_t;
using Item = frcnn_png_dec_batch_item_t;

// nullptr when the plan's fields agree with each other (what the kernels' bounds rest on), else what is wrong
inline const char* pd_plan_fault(const Plan& p) {
    if (p.h < 1 || p.w < 1 || p.h > 65535 || p.w > 65535) return "sides outside 1..65535";
    if (p.channels != 1 && p.channels != 3 && p.channels != 4) return "channels";
    const unsigned long long inflated = (unsigned long long)p.h * (1ull + (unsigned long long)p.w * p.channels);
    if (inflated >= FRCNN_PNG_DEC_MAX_INFLATED || inflated != p.inflated_len) return "inflated length";
    if (p.stream_len < 6 || p.stream_len >= PD_MAX_STREAM) return "stream length";
    return nullptr;
}

// grid.x = item.  The item lies in device memory at an address that is uniform over the workgroup and that nothing written here aliases.
__global__ void __launch_bounds__(PD_THREADS) k_png_dec_inflate(const uint8_t* files, const Item* __restrict__ items, uint8_t* workspace, int32_t* status) {
    const Item& it = items[blockIdx.x];
    pd_inflate_body(files + it.file_off, it.plan.stream_len, it.plan.inflated_len, workspace + it.ws_off, status + blockIdx.x);
}

// ------------------------------------------------------------------------------------------------------------- unfilter and pack
__device__ __forceinline__ uint32_t pd_load_pixel(const uint8_t* p, int bpp) {
    uint32_t v = p[0];
    if (bpp > 1) v |= (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    if (bpp > 3) v |= (uint32_t)p[3] << 24;
    return v;
}

// One wave: ``rows`` the inflated bytes (a filter byte and w * channels bytes per row), overwritten where a strip's last row is kept.
__device__ __forceinline__ void pd_unfilter_body(uint8_t* rows, const Plan& plan, int bgr, uint8_t* frame, int32_t* status) {
    const int lane = (int)threadIdx.x, h = plan.h, w = plan.w, bpp = plan.channels;
    const size_t stride = 1 + (size_t)w * (size_t)bpp;
    uint32_t flagged = 0;
    for (int base = 0; base < h; base += 64) {
        const int row = base + lane;
        const bool live = row < h;
        uint8_t* src = rows + (size_t)(live ? row : 0) * stride;
        uint32_t ft = live ? (uint32_t)src[0] : 0u;
        if (ft > 4u) { flagged |= ST_FILTER; ft = 0u; }
        const uint8_t* up = base > 0 ? rows + (size_t)(base - 1) * stride + 1 : nullptr;    // the previous strip's last row, reconstructed
        const bool keep = lane == 63 && base + 64 < h;
        uint32_t a = 0, c = 0, cur = 0;
        for (int t = 0; t < w + 63; ++t) {
            uint32_t b = __shfl_up(cur, 1, 64);                 // lane - 1 stood at this pixel of the row above a step ago
            const int x = t - lane;
            const bool on = live && x >= 0 && x < w;
            if (lane == 0) b = (on && up) ? pd_load_pixel(up + (size_t)x * bpp, bpp) : 0u;
            if (on) {
                uint8_t* px = src + 1 + (size_t)x * bpp;
                const uint32_t raw = pd_load_pixel(px, bpp);
                uint32_t v = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int sh = 8 * k;
                    const uint32_t pr = pd_predict(ft, (int)((a >> sh) & 255u), (int)((b >> sh) & 255u), (int)((c >> sh) & 255u));
                    v |= (((raw >> sh) + pr) & 255u) << sh;
                }
                if (bpp == 1) v &= 255u; else if (bpp == 3) v &= 0xFFFFFFu;
                cur = v;
                const uint32_t c0 = v & 255u, c1 = bpp == 1 ? c0 : (v >> 8) & 255u, c2 = bpp == 1 ? c0 : (v >> 16) & 255u;
                uint8_t* dst = frame + ((size_t)row * (size_t)w + (size_t)x) * 3;
                dst[0] = (uint8_t)(bgr ? c2 : c0);
                dst[1] = (uint8_t)c1;
                dst[2] = (uint8_t)(bgr ? c0 : c2);
                if (keep) {
                    px[0] = (uint8_t)c0;
                    if (bpp > 1) { px[1] = (uint8_t)(v >> 8); px[2] = (uint8_t)(v >> 16); }
                    if (bpp > 3) px[3] = (uint8_t)(v >> 24);
                }
                c = b;
                a = v;
            }
        }
        __threadfence_block();
        __syncthreads();                                        // (lane 0 of the next strip reads what lane 63 kept)
    }
    const int bad = __any((int)flagged);                        // (the inflate kernel, the word's other writer, ran in the launch before)
    if (bad && lane == 0) *status = (int32_t)((uint32_t)*status | ST_FILTER);
}

// grid.x = item, one wave
__global__ void __launch_bounds__(PD_UNF_THREADS) k_png_dec_unfilter(const Item* __restrict__ items, uint8_t* workspace, int bgr, uint8_t* out, int32_t* status) {
    const Item& it = items[blockIdx.x];
    pd_unfilter_body(workspace + it.ws_off, it.plan, bgr, out + it.out_off, status + blockIdx.x);
}

// ------------------------------------------------------------------------------------------------------------------ the planner
#define PD_UNSUPPORTED(...) return fail(FRCNN_E_UNSUPPORTED, "png_dec_plan: " __VA_ARGS__)

int pd_plan(const uint8_t* d, size_t n, Plan* out) {
    static const uint8_t SIG[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    Plan p = {};
    if (n == 0) PD_UNSUPPORTED("empty file");
    if (n < 8) PD_UNSUPPORTED("not a PNG file (no signature)");
    for (int i = 0; i < 8; ++i)
        if (d[i] != SIG[i]) PD_UNSUPPORTED("not a PNG file (no signature)");
    if (n > 0xFFFFFFFFull) PD_UNSUPPORTED("a file of %zu bytes", n);
    p.file_len = (uint32_t)n;
    size_t pos = 8;
    bool ihdr = false, iend = false, closed = false;
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
            const int depth = data[8], colour = data[9];
            if (colour == 3) PD_UNSUPPORTED("palette (colour type 3)");
            if (colour == 4) PD_UNSUPPORTED("grey + alpha (colour type 4)");
            if (colour != 0 && colour != 2 && colour != 6) PD_UNSUPPORTED("colour type %d", colour);
            if (depth != 8) PD_UNSUPPORTED("%d-bit samples", depth);
            if (data[10] != 0) PD_UNSUPPORTED("compression method %d", data[10]);
            if (data[11] != 0) PD_UNSUPPORTED("filter method %d", data[11]);
            if (data[12] != 0) PD_UNSUPPORTED("interlaced (Adam7)");
            if (w < 1 || h < 1 || w > 65535 || h > 65535) PD_UNSUPPORTED("frame %ux%u: both sides in 1..65535", h, w);
            p.h = (int32_t)h;
            p.w = (int32_t)w;
            p.channels = colour == 0 ? 1 : (colour == 2 ? 3 : 4);
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
            else if (!(type[0] & 0x20) && !named("PLTE")) PD_UNSUPPORTED("unknown critical chunk %.4s", (const char*)type);
        }
        pos += 12 + clen;
    }
    if (!p.idat_count) PD_UNSUPPORTED("no IDAT");
    if (stream >= PD_MAX_STREAM) PD_UNSUPPORTED("IDAT payload of %llu bytes (the device takes fewer than %u)", stream, PD_MAX_STREAM);
    if (stream < 6) PD_UNSUPPORTED("truncated: a zlib stream of %llu bytes", stream);
    if ((zh[0] & 15) != 8) PD_UNSUPPORTED("zlib compression method %d", zh[0] & 15);
    if ((zh[0] >> 4) > 7) PD_UNSUPPORTED("zlib window above 32 KiB");
    if ((((unsigned)zh[0] << 8) | zh[1]) % 31u) PD_UNSUPPORTED("bad zlib header check");
    if (zh[1] & 0x20) PD_UNSUPPORTED("zlib preset dictionary");
    const unsigned long long inflated = (unsigned long long)p.h * (1ull + (unsigned long long)p.w * p.channels);
    if (inflated >= FRCNN_PNG_DEC_MAX_INFLATED) PD_UNSUPPORTED("frame %dx%d inflates to %llu bytes (the device takes fewer than 2^31)", p.h, p.w, inflated);
    p.stream_len = (uint32_t)stream;
    p.inflated_len = (uint32_t)inflated;
    *out = p;
    return FRCNN_OK;
}

}  // namespace
}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_png_dec_version(void) { return FRCNN_PNG_DEC_VERSION; }

extern "C" int frcnn_png_dec_plan(const uint8_t* file_host, size_t len, frcnn_png_dec_plan_t* plan) {
    if (!plan || (!file_host && len)) return fail(FRCNN_E_ARG, "png_dec_plan: null pointer");
    return pd_plan(file_host, len, plan);
}

extern "C" int frcnn_png_dec_spans(const uint8_t* file_host, size_t len, const frcnn_png_dec_plan_t* plan, uint32_t* spans, size_t capacity) {
    if (!file_host || !plan || !spans) return fail(FRCNN_E_ARG, "png_dec_spans: null pointer");
    if (capacity < plan->idat_count) return fail(FRCNN_E_ARG, "png_dec_spans: room for %zu spans, the plan has %u", capacity, plan->idat_count);
    if (len != plan->file_len) return fail(FRCNN_E_ARG, "png_dec_spans: a file of %zu bytes, the plan was made of %u", len, plan->file_len);
    size_t pos = plan->idat_off;
    unsigned long long sum = 0;
    for (uint32_t k = 0; k < plan->idat_count; ++k) {
        if (pos > len || len - pos < 12) return fail(FRCNN_E_ARG, "png_dec_spans: not the file the plan was made of");
        const size_t clen = pd_be32(file_host + pos);
        if (clen > len - pos - 12 || file_host[pos + 4] != 'I' || file_host[pos + 5] != 'D' || file_host[pos + 6] != 'A' || file_host[pos + 7] != 'T')
            return fail(FRCNN_E_ARG, "png_dec_spans: not the file the plan was made of");
        spans[2 * k] = (uint32_t)(pos + 8);
        spans[2 * k + 1] = (uint32_t)clen;
        sum += clen;
        pos += 12 + clen;
    }
    if (sum != plan->stream_len) return fail(FRCNN_E_ARG, "png_dec_spans: not the file the plan was made of");
    return FRCNN_OK;
}

extern "C" size_t frcnn_png_dec_workspace_bytes(const frcnn_png_dec_plan_t* plan) {
    if (!plan || pd_plan_fault(*plan)) return 0;
    return pd_align16(plan->inflated_len);
}

extern "C" size_t frcnn_png_dec_batch_layout(const frcnn_png_dec_plan_t* plans, int n, uint64_t* ws_off) {
    if (!plans || !ws_off || n < 1 || n > FRCNN_PNG_DEC_BATCH_MAX) return 0;
    for (int i = 0; i < n; ++i)
        if (pd_plan_fault(plans[i])) return 0;
    size_t at = 0;
    for (int i = 0; i < n; ++i) { ws_off[i] = at; at += pd_align16(plans[i].inflated_len); }
    return at;
}

extern "C" int frcnn_png_decode_batch_u8(const frcnn_png_dec_batch_item_t* items_host, const frcnn_png_dec_batch_item_t* items_dev, int n,
                                         const uint8_t* files_dev, size_t files_capacity, int bgr, uint8_t* out_dev, size_t out_capacity,
                                         int32_t* status_dev, void* workspace, size_t workspace_capacity, void* stream) {
    if (!items_host || !items_dev || !files_dev || !out_dev || !status_dev || !workspace) return fail(FRCNN_E_ARG, "png_decode_batch_u8: null pointer");
    if (n < 1 || n > FRCNN_PNG_DEC_BATCH_MAX) return fail(FRCNN_E_ARG, "png_decode_batch_u8: n=%d outside 1..%d", n, FRCNN_PNG_DEC_BATCH_MAX);
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return fail(FRCNN_E_ARG, "png_decode_batch_u8: workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(status_dev) & 3u) return fail(FRCNN_E_ARG, "png_decode_batch_u8: status_dev must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(items_dev) & 7u) return fail(FRCNN_E_ARG, "png_decode_batch_u8: items_dev must be 8-byte aligned");
    PdRange outs[FRCNN_PNG_DEC_BATCH_MAX], regions[FRCNN_PNG_DEC_BATCH_MAX];
    for (int i = 0; i < n; ++i) {
        const Item& it = items_host[i];
        const Plan& p = it.plan;
        if (const char* what = pd_plan_fault(p)) return fail(FRCNN_E_ARG, "png_decode_batch_u8: item %d: the plan contradicts itself (%s)", i, what);
        const unsigned long long frame = (unsigned long long)p.h * p.w * 3, need = pd_align16(p.inflated_len);
        if (it.file_off > files_capacity || p.stream_len > files_capacity - it.file_off)
            return fail(FRCNN_E_ARG, "png_decode_batch_u8: item %d: file_off=%llu + stream_len=%u beyond files_capacity=%zu", i, (unsigned long long)it.file_off, p.stream_len, files_capacity);
        if (it.out_off > out_capacity || frame > out_capacity - it.out_off)
            return fail(FRCNN_E_ARG, "png_decode_batch_u8: item %d: out_off=%llu + %d * %d * 3 beyond out_capacity=%zu", i, (unsigned long long)it.out_off, p.h, p.w, out_capacity);
        if (it.ws_off & 15u) return fail(FRCNN_E_ARG, "png_decode_batch_u8: item %d: ws_off=%llu must be 16-byte aligned", i, (unsigned long long)it.ws_off);
        if (it.ws_off > workspace_capacity || need > workspace_capacity - it.ws_off)
            return fail(FRCNN_E_ARG, "png_decode_batch_u8: item %d: ws_off=%llu + %llu beyond workspace_capacity=%zu", i, (unsigned long long)it.ws_off, need, workspace_capacity);
        outs[i] = {it.out_off, it.out_off + frame, i};
        regions[i] = {it.ws_off, it.ws_off + need, i};
    }
    int k = pd_overlap(outs, n);
    if (k >= 0) return fail(FRCNN_E_ARG, "png_decode_batch_u8: the output ranges of items %d and %d overlap", outs[k].item, outs[k + 1].item);
    k = pd_overlap(regions, n);
    if (k >= 0) return fail(FRCNN_E_ARG, "png_decode_batch_u8: the workspace regions of items %d and %d overlap", regions[k].item, regions[k + 1].item);
    hipStream_t s = as_stream(stream);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    k_png_dec_inflate<<<n, PD_THREADS, 0, s>>>(files_dev, items_dev, ws, status_dev);
    k_png_dec_unfilter<<<n, PD_UNF_THREADS, 0, s>>>(items_dev, ws, bgr ? 1 : 0, out_dev, status_dev);
    return check_launch("png_decode_batch_u8");
}
