// What the device PNG decoder's translation units share (png_dec.hip: revision 1 of include/ext/frcnn_hip_png_dec.h; png_dec_full.hip:
// palette, sub-byte and 16-bit samples, grey + alpha and Adam7, include/ext/frcnn_hip_png_dec_full.h): the parallel inflate of one zlib
// stream by one workgroup (its description and its bounds argument are at the top of png_dec.hip) with the kernel that runs it for either
// kind of item, the filter predictor and the CRC-32.  The host half of both decoders (planner, spans, sizes, argument checks) is
// png_dec_host.h, which includes this file.  Everything sits in an unnamed namespace: each translation unit has its own copy,
// __constant__ data included.
#pragma once
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

constexpr uint32_t ST_CODE = FRCNN_PNG_DEC_CODE, ST_BLOCK = FRCNN_PNG_DEC_BLOCK, ST_OVERSUB = FRCNN_PNG_DEC_OVERSUBSCRIBED,
                   ST_DISTANCE = FRCNN_PNG_DEC_DISTANCE, ST_OVERRUN = FRCNN_PNG_DEC_OVERRUN, ST_UNDERRUN = FRCNN_PNG_DEC_UNDERRUN,
                   ST_ADLER = FRCNN_PNG_DEC_ADLER, ST_FILTER = FRCNN_PNG_DEC_FILTER;

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

// The zlib stream of ONE file (``len`` bytes) inflated by the whole workgroup (blockDim.x == PD_THREADS) into out[0, cap).
__device__ __forceinline__ void pd_inflate_body(const uint8_t* stream, uint32_t len, uint32_t cap, uint8_t* out, int32_t* status) {
    __shared__ PdHuff s_ll, s_dd, s_cl;
    __shared__ uint32_t s_win[PD_WIN_WORDS];
    __shared__ uint8_t s_lens[320], s_cllens[32];
    __shared__ uint32_t s_exit[PD_THREADS];
    __shared__ uint32_t s_part[PD_THREADS / 64];
    __shared__ uint32_t s_hdr[4], s_min[2], s_adler[2];
    __shared__ uint32_t s_changed, s_status, s_eob;
    const uint32_t tid = threadIdx.x;
    const uint32_t lenbits = len * 8u;
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

// grid.x = item, for either kind of item.  The item lies in device memory at an address that is uniform over the workgroup and that
// nothing written here aliases.
template <class I>
__global__ void __launch_bounds__(PD_THREADS) k_png_dec_inflate(const uint8_t* files, const I* __restrict__ items, uint8_t* workspace, int32_t* status) {
    const I& it = items[blockIdx.x];
    pd_inflate_body(files + it.file_off, it.plan.stream_len, it.plan.inflated_len, workspace + it.ws_off, status + blockIdx.x);
}

// ---------------------------------------------------------------------------------------------------------------- the predictor
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

// ------------------------------------------------------------------------------------------------------------ host-side helpers
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

}  // namespace
}  // namespace frcnn
