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
// table it is given, that every item's stream, region and frame lie inside the buffers and that regions and frames are disjoint (the
// checks and what they establish: png_dec_host.h, one text for both decoders); the kernels rest on plan.stream_len, plan.inflated_len,
// h, w, channels alone, never on anything read from the stream.  (a) The stream is
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
// pd_inflate_body, the kernel around it (k_png_dec_inflate<Item>), the codes and the predictor live in png_dec_common.h: png_dec_full.hip (palette, sub-byte and 16-bit samples, grey +
// alpha, Adam7; include/ext/frcnn_hip_png_dec_full.h) runs the same inflate, and (a) - (c) hold for it with ITS plan's stream_len and
// inflated_len.  (d) extended to its two other kernels: k_png_dec_full_unfilter's wave of pass k touches rows offset_k + row * (1 +
// rowbytes_k) + [0, 1 + rowbytes_k) for row < ph_k only, where pw_k, ph_k, rowbytes_k and offset_k come from h, w, colour type, depth and
// interlace through the function with which the host checked that the passes sum to inflated_len; k_png_dec_full_expand has one lane per
// pixel (row < h, x < w), reads one sample inside such a row and, for a palette file, entry index < plte_entries <= 256 of the item's 768
// staged palette bytes, which the host checked to lie inside files_capacity; a filter byte above 4 in any pass sets FRCNN_PNG_DEC_FILTER;
// the unfilter kernel's one barrier and its early return are decided by blockIdx and the plan alone.  The full text is at the top of
// png_dec_full.hip.
#include "png_dec_host.h"

namespace frcnn {
namespace {

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

}  // namespace
}  // namespace frcnn

using namespace frcnn;

// ------------------------------------------------------------------------------- the entry points: the host half is png_dec_host.h
extern "C" int frcnn_png_dec_version(void) { return FRCNN_PNG_DEC_VERSION; }

extern "C" int frcnn_png_dec_plan(const uint8_t* file_host, size_t len, frcnn_png_dec_plan_t* plan) {
    if (!plan || (!file_host && len)) return fail(FRCNN_E_ARG, "png_dec_plan: null pointer");
    FPlan full;
    if (const int code = pd_walk("png_dec_plan", pd_ihdr_rev1, file_host, len, &full)) return code;
    *plan = {full.h, full.w, pdf_channels(full.colour_type), full.file_len, full.idat_off, full.idat_count, full.stream_len, full.inflated_len};
    return FRCNN_OK;
}

extern "C" int frcnn_png_dec_spans(const uint8_t* file_host, size_t len, const frcnn_png_dec_plan_t* plan, uint32_t* spans, size_t capacity) {
    return pd_spans("png_dec_spans", file_host, len, plan, spans, capacity);
}

extern "C" size_t frcnn_png_dec_workspace_bytes(const frcnn_png_dec_plan_t* plan) { return pd_workspace_bytes(plan); }

extern "C" size_t frcnn_png_dec_batch_layout(const frcnn_png_dec_plan_t* plans, int n, uint64_t* ws_off) { return pd_batch_layout(plans, n, ws_off); }

extern "C" int frcnn_png_decode_batch_u8(const frcnn_png_dec_batch_item_t* items_host, const frcnn_png_dec_batch_item_t* items_dev, int n,
                                         const uint8_t* files_dev, size_t files_capacity, int bgr, uint8_t* out_dev, size_t out_capacity,
                                         int32_t* status_dev, void* workspace, size_t workspace_capacity, void* stream) {
    if (const int code = pd_check_batch("png_decode_batch_u8", items_host, items_dev, n, files_dev, files_capacity, out_dev, out_capacity, status_dev,
                                        workspace, workspace_capacity))
        return code;
    hipStream_t s = as_stream(stream);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    k_png_dec_inflate<Item><<<n, PD_THREADS, 0, s>>>(files_dev, items_dev, ws, status_dev);
    k_png_dec_unfilter<<<n, PD_UNF_THREADS, 0, s>>>(items_dev, ws, bgr ? 1 : 0, out_dev, status_dev);
    return check_launch("png_decode_batch_u8");
}
