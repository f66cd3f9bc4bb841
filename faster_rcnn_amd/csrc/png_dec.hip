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
#include "common.h"
#include "../../include/ext/frcnn_hip_png_dec.h"

namespace frcnn {
namespace {

constexpr int PD_THREADS = 512;
constexpr uint32_t PD_S = 128;                                  // bits of a lane's stretch (a token is at most 48)
constexpr uint32_t PD_WIN_BITS = PD_THREADS * PD_S;
constexpr uint32_t PD_WIN_WORDS = PD_WIN_BITS / 32 + 4;         // (a token that starts in the window ends within 64 bits behind it)
constexpr int PD_LOOK = 10;
constexpr uint32_t PD_ENDED = 0xFFFFFFFFu, PD_ERR = 0xFFFFFFFEu;    // exits that are no bit position: end-of-block seen, invalid code
constexpr uint32_t PD_NONE = 0xFFFFFFFFu;
constexpr uint32_t PD_MAX_STREAM = FRCNN_PNG_DEC_MAX_STREAM;    // (see the header: what bounds the inflate kernel's worst case)
constexpr int PD_UNF_THREADS = 64;
static_assert(PD_WIN_BITS / 8 == FRCNN_PNG_DEC_WINDOW_BYTES, "the header states the window");

using Plan = frcnn_png_dec_plan_t;
using Item = frcnn_png_dec_batch_item_t;

constexpr uint32_t ST_CODE = FRCNN_PNG_DEC_CODE, ST_BLOCK = FRCNN_PNG_DEC_BLOCK, ST_OVERSUB = FRCNN_PNG_DEC_OVERSUBSCRIBED,
                   ST_DISTANCE = FRCNN_PNG_DEC_DISTANCE, ST_OVERRUN = FRCNN_PNG_DEC_OVERRUN, ST_UNDERRUN = FRCNN_PNG_DEC_UNDERRUN,
                   ST_ADLER = FRCNN_PNG_DEC_ADLER, ST_FILTER = FRCNN_PNG_DEC_FILTER;

__host__ __device__ inline size_t pd_align16(size_t v) { return (v + 15) / 16 * 16; }

// nullptr when the plan's fields agree with each other (what the kernels' bounds rest on), else what is wrong
inline const char* pd_plan_fault(const Plan& p) {
    if (p.h < 1 || p.w < 1 || p.h > 65535 || p.w > 65535) return "sides outside 1..65535";
    if (p.channels != 1 && p.channels != 3 && p.channels != 4) return "channels";
    const unsigned long long inflated = (unsigned long long)p.h * (1ull + (unsigned long long)p.w * p.channels);
    if (inflated >= FRCNN_PNG_DEC_MAX_INFLATED || inflated != p.inflated_len) return "inflated length";
    if (p.stream_len < 6 || p.stream_len >= PD_MAX_STREAM) return "stream length";
    return nullptr;
}

// --------------------------------------------------------------------------------------------------------------------- the codes
struct PdHuff {
    uint16_t look[1 << PD_LOOK];        // by the next 10 bits of the stream: length << 9 | symbol, 0: a longer code or none
    uint16_t sorted[320];               // the symbols by (length, symbol)
    int first[16], maxcode[16], delta[16], offs[16];    // per length: the first and the largest code (-1: none), symbol index = code + delta
    int count, over;
};

// The canonical code of n <= 320 lengths, by the whole workgroup (uniform: barriers inside).
__device__ __forceinline__ void pd_build(PdHuff& h, const uint8_t* lens, uint32_t n) {
    const uint32_t tid = threadIdx.x, threads = blockDim.x;
    for (uint32_t x = tid; x < (1u << PD_LOOK); x += threads) h.look[x] = 0;
    if (tid == 0) {
        for (int l = 0; l < 16; ++l) h.offs[l] = 0;
        for (uint32_t i = 0; i < n; ++i) h.offs[lens[i] & 15u] += 1;
        int code = 0, k = 0, left = 1, over = 0;
        h.first[0] = 0; h.maxcode[0] = -1; h.delta[0] = 0;
        for (int l = 1; l < 16; ++l) {
            const int c = h.offs[l];
            left = left * 2 - c;
            if (left < 0) { over = 1; left = 0; }
            h.first[l] = code;
            h.maxcode[l] = c ? code + c - 1 : -1;
            h.delta[l] = k - code;
            h.offs[l] = k;
            code = (code + c) << 1;
            k += c;
        }
        h.count = k;
        h.over = over;
    }
    __syncthreads();
    for (uint32_t x = tid; x < n; x += threads) {
        const uint32_t l = lens[x] & 15u;
        if (!l) continue;
        int rank = 0;
        for (uint32_t y = 0; y < x; ++y) rank += (lens[y] & 15u) == l;
        const int k = h.offs[l] + rank, code = h.first[l] + rank;
        if (k < 320) h.sorted[k] = (uint16_t)x;
        if (l <= (uint32_t)PD_LOOK && code < (1 << l)) {
            const uint32_t rev = __brev((uint32_t)code) >> (32u - l);
            const uint16_t e = (uint16_t)((l << 9) | x);
            for (uint32_t j = 0; j < (1u << (PD_LOOK - l)); ++j) h.look[rev | (j << l)] = e;
        }
    }
    __syncthreads();
}

constexpr uint32_t PD_INVALID = 0xFFFFu;

// the symbol whose code starts the 15 bits ``b`` (as they come in the stream), its length in *len
__device__ __forceinline__ uint32_t pd_sym(const PdHuff& h, uint32_t b, uint32_t* len) {
    const uint32_t e = h.look[b & ((1u << PD_LOOK) - 1u)];
    if (e) { *len = e >> 9; return e & 511u; }
    const uint32_t r = __brev(b & 0x7FFFu) >> 17;               // the 15 bits, first bit on top
    for (int l = PD_LOOK + 1; l < 16; ++l) {
        const int code = (int)(r >> (15 - l));
        if (code <= h.maxcode[l]) {
            const int k = code + h.delta[l];
            *len = (uint32_t)l;
            return (code >= h.first[l] && k >= 0 && k < h.count && k < 320) ? (uint32_t)h.sorted[k] : PD_INVALID;
        }
    }
    *len = 15;
    return PD_INVALID;
}

__device__ __forceinline__ uint32_t pd_gbyte(const uint8_t* s, uint32_t len, uint32_t i) { return i < len ? (uint32_t)s[i] : 0u; }

// n <= 16 bits at bit ``pos`` of the stream in global memory (the block headers: one lane)
__device__ __forceinline__ uint32_t pd_gbits(const uint8_t* s, uint32_t len, uint32_t pos, uint32_t n) {
    const uint32_t i = pos >> 3;
    const uint32_t v = pd_gbyte(s, len, i) | pd_gbyte(s, len, i + 1u) << 8 | pd_gbyte(s, len, i + 2u) << 16 | pd_gbyte(s, len, i + 3u) << 24;
    return (v >> (pos & 7u)) & ((1u << n) - 1u);
}

struct PdCtx {
    const uint32_t* win;                // the window's bytes in LDS, little-endian words
    uint32_t wbase, lenbits;            // the window's first bit; the stream's bits
    const PdHuff* ll;
    const PdHuff* dd;
};

// 32 bits from bit ``pos`` on
__device__ __forceinline__ uint32_t pd_peek(const PdCtx& c, uint32_t pos) {
    const uint32_t rel = pos - c.wbase, i = rel >> 5;
    if (i + 1u >= PD_WIN_WORDS) return 0u;                      // (also pos < wbase: rel wraps)
    const unsigned long long v = ((unsigned long long)c.win[i + 1u] << 32) | c.win[i];
    return (uint32_t)(v >> (rel & 31u));
}

// kind 0: a literal (dist = the byte), 1: a match, 2: end of block, 3: no token of this code starts here
struct PdTok { uint32_t next, len, dist, kind; };

__device__ __forceinline__ PdTok pd_token(const PdCtx& c, uint32_t pos) {
    PdTok t = {pos, 0u, 0u, 3u};
    if (pos >= c.lenbits) return t;
    uint32_t v = pd_peek(c, pos), l = 0;
    const uint32_t sym = pd_sym(*c.ll, v & 0x7FFFu, &l);
    if (sym > 285u) return t;
    pos += l;
    t.next = pos;
    if (sym < 256u) { t.len = 1u; t.dist = sym; t.kind = 0u; return t; }
    if (sym == 256u) { t.kind = 2u; return t; }
    const uint32_t s = sym - 257u;                              // 0..28
    uint32_t eb = (s < 8u || s == 28u) ? 0u : (s >> 2) - 1u;
    uint32_t base = s < 8u ? s + 3u : (s == 28u ? 258u : ((4u + (s & 3u)) << eb) + 3u);
    v = pd_peek(c, pos);
    const uint32_t length = base + (v & ((1u << eb) - 1u));
    pos += eb;
    v >>= eb;                                                   // (eb <= 5: 27 bits left, a code has at most 15)
    const uint32_t ds = pd_sym(*c.dd, v & 0x7FFFu, &l);
    if (ds > 29u) return t;
    pos += l;
    eb = ds < 4u ? 0u : (ds >> 1) - 1u;
    base = ds < 4u ? ds + 1u : ((2u + (ds & 1u)) << eb) + 1u;
    v = pd_peek(c, pos);
    t.dist = base + (v & ((1u << eb) - 1u));
    t.len = length;
    t.next = pos + eb;
    t.kind = 1u;
    return t;
}

// F_i: whole tokens from ``entry`` until the next would start at or past ``end``; -> the exit: that bit position, ENDED behind an
// end-of-block (*eob: the bit behind it) or ERR at an invalid code; *count: the bytes the tokens make.
__device__ __forceinline__ uint32_t pd_run(const PdCtx& c, uint32_t entry, uint32_t end, uint32_t* count, uint32_t* eob) {
    *count = 0;
    if (entry >= PD_ERR) return entry;
    uint32_t pos = entry, n = 0;
    while (pos < end) {
        const PdTok t = pd_token(c, pos);
        if (t.kind == 2u) { *eob = t.next; *count = n; return PD_ENDED; }
        if (t.kind == 3u) { *count = n; return PD_ERR; }
        n += t.len;
        pos = t.next;
    }
    *count = n;
    return pos;
}

// inclusive sum over the wave
__device__ __forceinline__ uint32_t pd_wave_scan(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

struct PdClOrder { uint8_t at[19]; };
__constant__ PdClOrder PD_CL_ORDER = {{16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15}};

// The zlib stream of ONE file inflated by the whole workgroup (blockDim.x == PD_THREADS) into out[0, plan.inflated_len).
__device__ __forceinline__ void pd_inflate_body(const uint8_t* stream, const Plan& plan, uint8_t* out, int32_t* status) {
    __shared__ PdHuff s_ll, s_dd, s_cl;
    __shared__ uint32_t s_win[PD_WIN_WORDS];
    __shared__ uint8_t s_lens[320], s_cllens[32];
    __shared__ uint32_t s_exit[PD_THREADS];
    __shared__ uint32_t s_part[PD_THREADS / 64];
    __shared__ uint32_t s_hdr[4], s_min[2], s_adler[2];
    __shared__ uint32_t s_changed, s_status, s_eob;
    const uint32_t tid = threadIdx.x;
    const uint32_t len = plan.stream_len, lenbits = len * 8u, cap = plan.inflated_len;
    if (tid == 0) { s_status = 0; s_changed = 0; s_eob = 0; s_min[0] = s_min[1] = PD_NONE; s_adler[0] = s_adler[1] = 0; }
    __syncthreads();

    uint32_t pos = 16u, o = 0u, fatal = 0u, flagged = 0u;       // pos, o, fatal: uniform over the workgroup (o <= cap throughout)
    for (;;) {
        // ---- the block's header
        if (tid == 0) {
            uint32_t f = 0, bf = 0, bt = 0;
            if (pos + 3u > lenbits) f = ST_UNDERRUN;
            else { bf = pd_gbits(stream, len, pos, 1); bt = pd_gbits(stream, len, pos + 1u, 2); if (bt == 3u) f = ST_BLOCK; }
            s_hdr[0] = bf; s_hdr[1] = bt; s_hdr[2] = f;
        }
        __syncthreads();
        const uint32_t bfinal = s_hdr[0], btype = s_hdr[1];
        fatal = s_hdr[2];
        __syncthreads();                                        // (s_hdr is written again below)
        if (fatal) break;
        pos += 3u;
        if (btype == 0u) {
            // ---- stored: LEN, NLEN at the next byte, the bytes copied
            const uint32_t p = (pos + 7u) >> 3;
            if (tid == 0) {
                uint32_t f = 0, n = 0;
                if (p + 4u > len) f = ST_UNDERRUN;
                else {
                    n = pd_gbyte(stream, len, p) | pd_gbyte(stream, len, p + 1u) << 8;
                    const uint32_t nn = pd_gbyte(stream, len, p + 2u) | pd_gbyte(stream, len, p + 3u) << 8;
                    if ((n ^ nn) != 0xFFFFu) f = ST_BLOCK;
                    else if (n > len - (p + 4u)) f = ST_UNDERRUN;
                    else if (n > cap - o) f = ST_OVERRUN;
                }
                s_hdr[0] = n; s_hdr[2] = f;
            }
            __syncthreads();
            const uint32_t n = s_hdr[0];
            fatal = s_hdr[2];
            __syncthreads();
            if (fatal) break;
            for (uint32_t i = tid; i < n; i += PD_THREADS) out[o + i] = stream[p + 4u + i];     // (o + n <= cap, p + 4 + n <= len)
            o += n;
            pos = (p + 4u + n) * 8u;
            __threadfence_block();
            __syncthreads();                                    // (later matches read these bytes)
        } else {
            // ---- the code lengths: the fixed ones, or the dynamic block's list decoded by one lane with the code-length code
            uint32_t hlit = 288u, hdist = 32u;
            if (btype == 1u) {
                for (uint32_t x = tid; x < 320u; x += PD_THREADS) s_lens[x] = (uint8_t)(x < 144u ? 8 : (x < 256u ? 9 : (x < 280u ? 7 : (x < 288u ? 8 : 5))));
                __syncthreads();
            } else {
                if (tid == 0) {
                    uint32_t f = 0, q = pos;
                    const uint32_t nl = pd_gbits(stream, len, q, 5) + 257u, nd = pd_gbits(stream, len, q + 5u, 5) + 1u, nc = pd_gbits(stream, len, q + 10u, 4) + 4u;
                    q += 14u;
                    for (int i = 0; i < 32; ++i) s_cllens[i] = 0;
                    if (q + 3u * nc > lenbits) f = ST_UNDERRUN;
                    else if (nl > 286u || nd > 30u) f = ST_CODE;
                    else for (uint32_t i = 0; i < nc; ++i) { s_cllens[PD_CL_ORDER.at[i]] = (uint8_t)pd_gbits(stream, len, q, 3); q += 3u; }
                    s_hdr[0] = nl; s_hdr[1] = nd; s_hdr[2] = f; s_hdr[3] = q;
                }
                __syncthreads();
                hlit = s_hdr[0]; hdist = s_hdr[1]; fatal = s_hdr[2];
                const uint32_t q0 = s_hdr[3];
                __syncthreads();
                if (fatal) break;
                pd_build(s_cl, s_cllens, 19u);
                if (s_cl.over) { fatal = ST_OVERSUB; break; }   // (written before pd_build's barriers, not again before the next block's)
                if (tid == 0) {
                    uint32_t f = 0, q = q0, i = 0;
                    const uint32_t total = hlit + hdist;        // <= 316
                    while (i < total) {
                        if (q >= lenbits) { f = ST_UNDERRUN; break; }
                        uint32_t l = 0;
                        const uint32_t sym = pd_sym(s_cl, pd_gbits(stream, len, q, 15), &l);
                        if (sym > 18u) { f = ST_CODE; break; }
                        q += l;
                        if (sym < 16u) { s_lens[i++] = (uint8_t)sym; continue; }
                        uint32_t rep, val = 0;
                        if (sym == 16u) {
                            if (i == 0u) { f = ST_CODE; break; }
                            val = s_lens[i - 1u];
                            rep = 3u + pd_gbits(stream, len, q, 2); q += 2u;
                        } else if (sym == 17u) { rep = 3u + pd_gbits(stream, len, q, 3); q += 3u; }
                        else { rep = 11u + pd_gbits(stream, len, q, 7); q += 7u; }
                        if (rep > total - i) { f = ST_CODE; break; }
                        for (uint32_t k = 0; k < rep; ++k) s_lens[i++] = (uint8_t)val;
                    }
                    s_hdr[2] = f; s_hdr[3] = q;
                }
                __syncthreads();
                fatal = s_hdr[2];
                pos = s_hdr[3];
                __syncthreads();
                if (fatal) break;
            }
            pd_build(s_ll, s_lens, hlit);
            pd_build(s_dd, s_lens + hlit, hdist);
            if (s_ll.over || s_dd.over) { fatal = ST_OVERSUB; break; }

            // ---- the block's data, a window of the stream at a time
            PdCtx c;
            c.win = s_win;
            c.lenbits = lenbits;
            c.ll = &s_ll;
            c.dd = &s_dd;
            uint32_t entry0 = pos;
            for (;;) {
                if (entry0 >= lenbits) { fatal = ST_UNDERRUN; break; }
                const uint32_t wbase = entry0 / PD_WIN_BITS * PD_WIN_BITS;
                c.wbase = wbase;
                for (uint32_t x = tid; x < PD_WIN_WORDS; x += PD_THREADS) {
                    const uint32_t b = wbase / 8u + 4u * x;
                    s_win[x] = pd_gbyte(stream, len, b) | pd_gbyte(stream, len, b + 1u) << 8 | pd_gbyte(stream, len, b + 2u) << 16 | pd_gbyte(stream, len, b + 3u) << 24;
                }
                __syncthreads();
                // rounds: exit[i] = F_i(entry[i]) for every lane whose entry changed, entry[i + 1] = exit[i], until nothing changes
                const uint32_t start = wbase + tid * PD_S, end = start + PD_S;
                uint32_t entry = start > entry0 ? start : entry0, count = 0, eob = 0, exitv = 0;
                bool changed = true;
                for (uint32_t round = 0; round < (uint32_t)PD_THREADS; ++round) {
                    if (changed) {
                        exitv = pd_run(c, entry, end, &count, &eob);
                        s_exit[tid] = exitv;
                    }
                    __syncthreads();
                    changed = false;
                    if (tid > 0u) {
                        const uint32_t e = s_exit[tid - 1u];
                        if (e != entry) { entry = e; changed = true; }
                    }
                    if (changed) atomicOr(&s_changed, 1u);
                    __syncthreads();
                    const uint32_t any = s_changed;
                    __syncthreads();
                    if (!any) break;
                    if (tid == 0) s_changed = 0;                // (read again only behind the next round's barriers)
                }
                // every lane's first output byte, the window's total, where the block ends if it does
                const uint32_t incl = pd_wave_scan(count);
                if ((tid & 63u) == 63u) s_part[tid >> 6] = incl;
                if (exitv == PD_ENDED && entry < PD_ERR) s_eob = eob;   // (the one lane that saw the end-of-block on the validated chain)
                __syncthreads();
                uint32_t before = incl - count, total = 0;
                for (uint32_t k = 0; k < (uint32_t)PD_THREADS / 64u; ++k) {
                    const uint32_t part = s_part[k];
                    total += part;
                    if (k < (tid >> 6)) before += part;
                }
                const uint32_t xlast = s_exit[PD_THREADS - 1], eob_at = s_eob;
                // the literals
                const bool walk = entry < PD_ERR;
                uint32_t q = entry, op = o + before;
                while (walk && q < end) {
                    const PdTok t = pd_token(c, q);
                    if (t.kind >= 2u) break;
                    if (t.kind == 0u) { if (op < cap) out[op] = (uint8_t)t.dist; else flagged |= ST_OVERRUN; }
                    op += t.len;
                    q = t.next;
                }
                __threadfence_block();
                __syncthreads();
                // the matches, in rounds
                q = entry; op = o + before;
                bool live = walk, have = false;
                uint32_t mdst = 0, mlen = 0, mdist = 0, par = 0;
                for (;;) {
                    if (live && !have) {
                        live = false;
                        while (q < end) {
                            const PdTok t = pd_token(c, q);
                            if (t.kind >= 2u) break;
                            q = t.next;
                            if (t.kind == 1u) { have = true; live = true; mdst = op; mlen = t.len; mdist = t.dist; op += t.len; break; }
                            op += 1u;
                        }
                    }
                    if (have) atomicMin(&s_min[par], mdst);
                    __syncthreads();
                    const uint32_t m = s_min[par];
                    if (tid == 0) s_min[par ^ 1u] = PD_NONE;    // (last read before the previous round's closing barrier)
                    if (m == PD_NONE) break;
                    if (have) {
                        if (mdist > mdst) { flagged |= ST_DISTANCE; have = false; }
                        else if (mdst == m || mdst - mdist + mlen <= m) {
                            const uint8_t* src = out + (mdst - mdist);
                            for (uint32_t k = 0; k < mlen; ++k) {
                                if (mdst + k < cap) out[mdst + k] = src[k]; else flagged |= ST_OVERRUN;
                            }
                            have = false;
                        }
                    }
                    __threadfence_block();
                    __syncthreads();
                    par ^= 1u;
                }
                if (total > cap - o) { fatal = ST_OVERRUN; break; }
                o += total;
                if (xlast == PD_ERR) { fatal = ST_CODE; break; }
                if (xlast == PD_ENDED) { pos = eob_at; break; }
                entry0 = xlast;
                __syncthreads();                                // (the window, s_part and s_exit are written again)
            }
            if (fatal) break;
            __syncthreads();
        }
        if (bfinal) break;
    }

    // ---- the length, the Adler-32
    __syncthreads();
    if (!fatal && o != cap) fatal = ST_UNDERRUN;
    const uint32_t tail = (pos + 7u) >> 3;
    if (!fatal && tail + 4u > len) fatal = ST_UNDERRUN;
    if (!fatal) {
        unsigned long long a = 0, b = 0;
        for (uint32_t i = tid; i < cap; i += PD_THREADS) {
            const uint32_t d = out[i];
            a += d;
            b += (unsigned long long)(cap - i) * d;
        }
        atomicAdd(&s_adler[0], (uint32_t)(a % 65521ull));
        atomicAdd(&s_adler[1], (uint32_t)(b % 65521ull));
    }
    if (flagged) atomicOr(&s_status, flagged);
    __syncthreads();
    if (tid == 0) {
        uint32_t s = s_status | fatal;
        if (!fatal) {
            const uint32_t lo = (1u + s_adler[0]) % 65521u, hi = (cap % 65521u + s_adler[1]) % 65521u;
            const uint32_t want = pd_gbyte(stream, len, tail) << 24 | pd_gbyte(stream, len, tail + 1u) << 16 | pd_gbyte(stream, len, tail + 2u) << 8 | pd_gbyte(stream, len, tail + 3u);
            if (((hi << 16) | lo) != want) s |= ST_ADLER;
        }
        if (s) *status = (int32_t)((uint32_t)*status | s);
    }
}

// grid.x = item.  The item lies in device memory at an address that is uniform over the workgroup and that nothing written here aliases.
__global__ void __launch_bounds__(PD_THREADS) k_png_dec_inflate(const uint8_t* files, const Item* __restrict__ items, uint8_t* workspace, int32_t* status) {
    const Item& it = items[blockIdx.x];
    pd_inflate_body(files + it.file_off, it.plan, workspace + it.ws_off, status + blockIdx.x);
}

// ------------------------------------------------------------------------------------------------------------- unfilter and pack
__device__ __forceinline__ uint32_t pd_load_pixel(const uint8_t* p, int bpp) {
    uint32_t v = p[0];
    if (bpp > 1) v |= (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    if (bpp > 3) v |= (uint32_t)p[3] << 24;
    return v;
}

__device__ __forceinline__ uint32_t pd_predict(uint32_t ft, int a, int b, int c) {
    if (ft == 1u) return (uint32_t)a;
    if (ft == 2u) return (uint32_t)b;
    if (ft == 3u) return (uint32_t)((a + b) >> 1);
    if (ft == 4u) {
        const int p = a + b - c;
        const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
        return (uint32_t)((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c));
    }
    return 0u;
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

struct PdCrcTable {
    uint32_t t[256];
    PdCrcTable() {
        for (uint32_t n = 0; n < 256; ++n) {
            uint32_t c = n;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[n] = c;
        }
    }
};

inline uint32_t pd_crc(const uint8_t* d, size_t n) {
    static const PdCrcTable table;
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = table.t[(c ^ d[i]) & 255u] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

inline uint32_t pd_be32(const uint8_t* d) { return (uint32_t)d[0] << 24 | (uint32_t)d[1] << 16 | (uint32_t)d[2] << 8 | d[3]; }

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

struct PdRange { unsigned long long lo, hi; int item; };

// -1, or the index of an item of (sorted by lo) ``r`` that reaches into its successor
inline int pd_overlap(PdRange* r, int n) {
    for (int i = 1; i < n; ++i)                                // (insertion sort: n <= 64)
        for (int j = i; j > 0 && r[j].lo < r[j - 1].lo; --j) { const PdRange t = r[j]; r[j] = r[j - 1]; r[j - 1] = t; }
    for (int i = 0; i + 1 < n; ++i)
        if (r[i].hi > r[i + 1].lo) return i;
    return -1;
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
