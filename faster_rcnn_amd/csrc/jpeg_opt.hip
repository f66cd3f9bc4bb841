// The device JPEG encoder's two size options (include/ext/frcnn_hip_jpeg_opt.h): 4:2:0 chroma and per-frame optimised Huffman tables,
// in the launch layout of jpeg.hip, whose kernels and files stay as they are.  gfx950 (CDNA4) only, wave64 throughout.  Integer
// arithmetic, plain vector stores, LDS atomics and integer global atomics only: the file is a function of (frame, quality, subsampling,
// huffman) alone, and tests/jpeg_opt_ref.py states the same rules in Python; the two agree byte for byte.
//
// The stream is jpeg.hip's with two knobs.  4:2:0: Y at 2x2, Cb Cr at 1x1, an MCU of 16x16 pixels coded as Y00 Y01 Y10 Y11 Cb Cr, chroma
// averaged per 2x2 group with libjpeg's alternating bias, 8 MCUs per restart interval.  An interval is 48 blocks in both samplings, so
// the interval kernel's LDS carries over (a block's bound grows by 3 bits: an optimised DC code is at most 12 bits, Annex K's 9).
// Optimised tables: the four DHT segments carry tables built from the frame's own symbol counts.
//
//   k_opt_clear      the four 256-entry histograms in the workspace to zero: the call clears them itself, a captured graph replays it.
//   k_opt_interval   <4:2:0?, statistics?>: one workgroup per interval, one wave per MCU walking its 3 or 6 blocks, lane = pixel, then
//                    coefficient (at 4:2:0 a lane reads four luma pixels and the 2x2 groups of its chroma sample from the 16x16 tile);
//                    jpeg.hip's permute DCT, quantisation and ballot zero runs.  The statistics form counts the symbols in LDS and adds
//                    the workgroup's counts to the device histograms; the coding form takes the four codes from the workspace (or the
//                    compile-time Annex K codes) into LDS and scans / ORs / stuffs as k_jpeg_interval does.  The quantised coefficients
//                    are RECOMPUTED in the coding form, not kept: int16 coefficients would be 6 bytes written and 6 read per pixel
//                    (3 + 3 at 4:2:0) against 3 bytes of frame read again, the DCT is 16 permutes and multiply-adds per lane and
//                    block, and one kernel body serves both forms.
//   k_opt_tables     one workgroup, one wave per table: libjpeg's jpeg_gen_optimal_table.  Counts, tree and depth of a lane's five
//                    symbols (257 over 64 lanes) live in registers; a merge step finds the two smallest counts (the largest index on
//                    a tie) by two shuffle minima over (count << 9 | 256 - index) and deepens every symbol of the two trees -- at most
//                    256 steps, the serial stretch; length limiting and the canonical codes are lane 0's, HUFFVAL's order a rank count.
//   k_opt_finish     one workgroup: exclusive scan of the sizes from the header's length on; the header: jpeg.hip's constant image up to
//                    SOF0 (tables, size, sampling factors patched in), the four DHT segments from the table records, DRI and SOS.
//   k_opt_gather     as k_jpeg_gather.
#include "jpeg_common.h"
#include "../../include/ext/frcnn_hip_jpeg_opt.h"

namespace frcnn {
namespace {

constexpr int OPT_BLOCKS = 48;                                  // per interval: 16 MCUs of 3 blocks, 8 MCUs of 6
constexpr int OPT_BLOCK_BITS = 23 + 63 * 26;                    // DC: a 12-bit code + 11 bits; AC: a 16-bit code + 10 bits each
constexpr int OPT_MAX_BITS = OPT_BLOCKS * OPT_BLOCK_BITS;       // 79728 per interval
constexpr int OPT_BITWORDS = (OPT_MAX_BITS + 31) / 32 + 3;      // (a lane's 48 bits touch three words)
constexpr int OPT_MAX_BYTES = (OPT_MAX_BITS + 7) / 8;           // 9966 before stuffing
constexpr int OPT_SLOT = (2 * OPT_MAX_BYTES + 2 + 8 + 15) / 16 * 16;       // stuffed + RSTm, and 8 more: the gather reads whole dwords
constexpr int OPT_PREFIX = JPEG_DIM_AT + 14;                    // SOI .. SOF0: the DHT segments start here
constexpr int OPT_TAIL = 20;                                    // DRI and SOS
constexpr int OPT_SAMPLING_AT = JPEG_DIM_AT + 6;                // Y's sampling factors in SOF0
constexpr int OPT_DRI_AT = OPT_TAIL - 16;                       // the interval's two bytes within the tail
constexpr int OPT_MAX_DEPTH = 257;                              // a tree over 257 leaves is at most this deep
constexpr int OPT_TABLE_THREADS = 256;
constexpr uint32_t OPT_HIST_BYTES = 4 * 256 * 4, OPT_CODE_BYTES = 4 * 256 * 4, OPT_RECORD_BYTES = 4 * sizeof(frcnn_jpeg_opt_table_t);
static_assert(JPEG_BLOCK_BYTES == (OPT_BLOCK_BITS + 7) / 8, "a block's bound in bytes is revision 1's");
static_assert(sizeof(frcnn_jpeg_opt_table_t) == 276 && OPT_RECORD_BYTES % 16 == 0, "the table record");
static_assert(OPT_PREFIX + 4 * 21 + 2 * (12 + 162) + OPT_TAIL == JPEG_HEADER_BYTES, "the header's layout");

// ---------------------------------------------------------------------------------------------------------------- host sizes
inline bool opt_sampling_ok(int subsampling) { return subsampling == FRCNN_JPEG_OPT_444 || subsampling == FRCNN_JPEG_OPT_420; }

inline bool opt_huffman_ok(int huffman) { return huffman == FRCNN_JPEG_OPT_STANDARD || huffman == FRCNN_JPEG_OPT_OPTIMIZED; }

inline unsigned long long opt_mcus(int h, int w, int subsampling) {
    const unsigned long long side = subsampling == FRCNN_JPEG_OPT_420 ? 16 : 8;
    return (((unsigned long long)h + side - 1) / side) * (((unsigned long long)w + side - 1) / side);
}

inline unsigned long long opt_intervals(int h, int w, int subsampling) {
    const unsigned long long per = subsampling == FRCNN_JPEG_OPT_420 ? 8 : 16;
    return (opt_mcus(h, w, subsampling) + per - 1) / per;
}

inline unsigned long long opt_bound(int h, int w, int subsampling) {
    if (!opt_sampling_ok(subsampling) || h < 1 || w < 1 || h > 65535 || w > 65535) return 0;
    const unsigned long long blocks = (subsampling == FRCNN_JPEG_OPT_420 ? 6ull : 3ull) * opt_mcus(h, w, subsampling);
    const unsigned long long b = JPEG_HEADER_BYTES + 2ull + 2ull * JPEG_BLOCK_BYTES * blocks + 4ull * opt_intervals(h, w, subsampling);
    return b <= JPEG_MAX_FILE ? b : 0;
}

inline unsigned long long opt_meta_bytes(unsigned long long nint) { return (2ull * 4ull * nint + 15ull) / 16ull * 16ull; }

// ---------------------------------------------------------------------------------------------------------- device helpers
__device__ __forceinline__ unsigned long long wave_min64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, d, 64), hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

// one pixel (clamped to the frame: the last column / row repeated) -> Y, Cb, Cr in 0..255, 16 fractional bits
__device__ __forceinline__ void load_ycc(const uint8_t* frame, int h, int w, int bgr, int y, int x, int* Y, int* Cb, int* Cr) {
    const int py = y < h ? y : h - 1, px = x < w ? x : w - 1;
    const uint8_t* p = frame + ((size_t)py * (size_t)w + (size_t)px) * 3;
    const int r = p[bgr ? 2 : 0], g = p[1], b = p[bgr ? 0 : 2];
    jfif_rgb_to_ycc(r, g, b, Y, Cb, Cr);
}

// ------------------------------------------------------------------------------------------------------------------ kernels
__global__ void __launch_bounds__(256) k_opt_clear(uint32_t* hist) { hist[blockIdx.x * 256 + threadIdx.x] = 0u; }

// codes: [4][256] symbol -> code | length << 16 in DHT order (DC luma, AC luma, DC chroma, AC chroma), or null for Annex K's;
// hist (STATS): [4][256] in the same order; meta: [2][nint] uint32 = interval size in bytes (stuffed, with its RSTm), its offset
template <bool S420, bool STATS>
__global__ void __launch_bounds__(S420 ? 512 : 1024) k_opt_interval(const uint8_t* frame, int h, int w, int bgr, JpegQuant quant,
                                                                    const uint32_t* codes, uint32_t* hist, uint8_t* slots, uint32_t* meta,
                                                                    uint32_t nint) {
    constexpr int WAVES = S420 ? 8 : 16, NB = S420 ? 6 : 3, LUMA = S420 ? 4 : 1, THREADS = 64 * WAVES;
    static_assert(WAVES * NB == OPT_BLOCKS && OPT_BLOCKS <= 64, "one wave scans the interval's blocks");
    __shared__ uint32_t s_bits[STATS ? 1 : OPT_BITWORDS];
    __shared__ __align__(16) uint8_t s_out[STATS ? 16 : OPT_SLOT];
    __shared__ uint32_t s_tab[4][256];                          // the four codes; the four histograms in the statistics form
    __shared__ uint8_t s_q[2][64];
    __shared__ int s_dcv[WAVES][NB];
    __shared__ uint32_t s_tot[64];
    __shared__ uint32_t s_part[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t interval = blockIdx.x;
    const int side = S420 ? 16 : 8;
    const int mw = (w + side - 1) / side, mh = (h + side - 1) / side;
    const uint32_t mcus = (uint32_t)mw * (uint32_t)mh;
    const uint32_t first = interval * WAVES;
    const uint32_t count = mcus - first < (uint32_t)WAVES ? mcus - first : (uint32_t)WAVES;
    const bool live = (uint32_t)wave < count;                   // (a wave past a short last interval works on its last MCU and emits nothing)

    if constexpr (!STATS)
        for (int i = tid; i < OPT_BITWORDS; i += THREADS) s_bits[i] = 0u;
    for (int i = tid; i < 1024; i += THREADS) {
        const int t = i >> 8, s = i & 255;
        uint32_t v = 0u;
        if constexpr (!STATS) v = codes ? codes[i] : ((t & 1) ? JPEG_TABLES.ac[t >> 1][s] : (s < 16 ? JPEG_TABLES.dc[t >> 1][s] : 0u));
        s_tab[t][s] = v;
    }
    if (tid < 128) s_q[tid >> 6][tid & 63] = quant.q[tid >> 6][tid & 63];
    if (tid < 64) s_tot[tid] = 0u;

    // ---- the MCU's samples, 128 subtracted for the DCT
    const uint32_t m = live ? first + (uint32_t)wave : first + count - 1u;
    const int my = (int)(m / (uint32_t)mw), mx = (int)(m - (uint32_t)my * (uint32_t)mw);
    int comp[NB];
    if constexpr (!S420) {
        int Y, Cb, Cr;
        load_ycc(frame, h, w, bgr, my * 8 + (lane >> 3), mx * 8 + (lane & 7), &Y, &Cb, &Cr);
        comp[0] = Y - 128; comp[1] = Cb - 128; comp[NB - 1] = Cr - 128;
    } else {
        int Cb, Cr, sb = 0, sr = 0;
#pragma unroll
        for (int b = 0; b < LUMA; ++b) {                        // block b: the tile's quadrant (b >> 1, b & 1)
            int Y;
            load_ycc(frame, h, w, bgr, my * 16 + 8 * (b >> 1) + (lane >> 3), mx * 16 + 8 * (b & 1) + (lane & 7), &Y, &Cb, &Cr);
            comp[b] = Y - 128;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {                           // chroma sample (lane >> 3, lane & 7): its 2x2 group of the tile
            int Y;
            load_ycc(frame, h, w, bgr, my * 16 + 2 * (lane >> 3) + (k >> 1), mx * 16 + 2 * (lane & 7) + (k & 1), &Y, &Cb, &Cr);
            sb += Cb; sr += Cr;
        }
        comp[NB - 2] = box2x2(sb, lane) - 128;                  // (libjpeg's h2v2_downsample: ycc_common.h)
        comp[NB - 1] = box2x2(sr, lane) - 128;
    }

    int crow[8], ccol[8];                                       // COS[lane & 7][.] for the row pass, COS[lane >> 3][.] for the column pass
#pragma unroll
    for (int k = 0; k < 8; ++k) { crow[k] = JPEG_TABLES.cos[8 * (lane & 7) + k]; ccol[k] = JPEG_TABLES.cos[8 * (lane >> 3) + k]; }
    const int zz = JPEG_TABLES.zigzag[lane];
    __syncthreads();

    // ---- DCT, quantisation, zigzag: coef[c] = coefficient ``lane`` (zigzag) of the MCU's block c
    int coef[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) {
        int acc = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x) acc += crow[x] * __shfl(comp[c], (lane & 56) | x, 64);         // t[y][u], lane = 8y + u
        const int t = (acc + 512) >> 10;
        acc = 0;
#pragma unroll
        for (int y = 0; y < 8; ++y) acc += ccol[y] * __shfl(t, 8 * y + (lane & 7), 64);             // F[v][u], lane = 8v + u
        const int f = __shfl(acc, zz, 64);
        const uint32_t q = s_q[c >= LUMA ? 1 : 0][lane];
        const int mag = (int)(((uint32_t)(f < 0 ? -f : f) + (q << 15)) / (q << 16));
        coef[c] = f < 0 ? -mag : mag;
        if (lane == 0) s_dcv[wave][c] = coef[c];
    }
    __syncthreads();

    // ---- every lane's symbol: the DC difference (lane 0), a non-zero AC coefficient behind its zero run (one ZRL per 16 zeros in
    // front of its code), EOB (lane 63 when it is zero).  zrl[c]: the ZRL codes' bits, bits[c]: the code and its value bits.
    unsigned long long zrl[NB];
    uint32_t bits[NB], nzrl[NB], nbits[NB], before[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) {
        uint32_t* dc = s_tab[c >= LUMA ? 2 : 0];
        uint32_t* ac = s_tab[c >= LUMA ? 3 : 1];
        const int v = coef[c];
        const unsigned long long nonzero = __ballot(v != 0) | 1ull;           // (position 0 bounds the first run whatever the DC is)
        unsigned long long zv = 0;
        uint32_t bv = 0, nz = 0, n = 0, low;
        if (lane == 0) {
            int pred = 0;                                       // the previous block of the same component in this interval
            if (S420 && c > 0 && c < LUMA) pred = s_dcv[wave][c - 1];
            else if (wave > 0) pred = s_dcv[wave - 1][c < LUMA ? LUMA - 1 : c];
            const uint32_t size = category(v - pred, &low);
            if constexpr (STATS) {
                if (live) atomicAdd(&dc[size], 1u);
            } else {
                const uint32_t e = dc[size];
                bv = ((e & 0xFFFFu) << size) | low;
                n = (e >> 16) + size;
            }
        } else if (v != 0) {
            const uint32_t run = (uint32_t)lane - (63u - (uint32_t)__clzll((long long)(nonzero & ((1ull << lane) - 1ull)))) - 1u;
            const uint32_t size = category(v, &low), sym = ((run & 15u) << 4) | size;
            if constexpr (STATS) {
                if (live) {
                    atomicAdd(&ac[sym], 1u);
                    if (run >> 4) atomicAdd(&ac[0xF0], run >> 4);
                }
            } else {
                const uint32_t e = ac[sym], z = ac[0xF0];
                for (uint32_t k = 0; k < (run >> 4); ++k) { zv = (zv << (z >> 16)) | (z & 0xFFFFu); nz += z >> 16; }
                bv = ((e & 0xFFFFu) << size) | low;
                n = (e >> 16) + size;
            }
        } else if (lane == 63) {
            if constexpr (STATS) {
                if (live) atomicAdd(&ac[0], 1u);
            } else {
                bv = ac[0] & 0xFFFFu;
                n = ac[0] >> 16;
            }
        }
        if constexpr (!STATS) {
            n = live ? n : 0u;
            nz = live ? nz : 0u;
            const uint32_t incl = wave_scan(n + nz);
            zrl[c] = zv; bits[c] = bv; nzrl[c] = nz; nbits[c] = n; before[c] = incl - n - nz;
            if (lane == 63) s_tot[NB * wave + c] = incl;
        }
    }
    __syncthreads();
    if constexpr (STATS) {                                                // the workgroup's counts into the device histograms
        for (int i = tid; i < 1024; i += THREADS) {
            const uint32_t v = s_tab[i >> 8][i & 255];
            if (v) atomicAdd(&hist[i], v);
        }
        return;
    }
    const uint32_t blocks_incl = wave_scan(s_tot[lane]);         // (entries past the interval's blocks are zero)
    const uint32_t total_bits = __shfl(blocks_incl, 63, 64);
#pragma unroll
    for (int c = 0; c < NB; ++c) {
        const uint32_t base = __shfl(blocks_incl - s_tot[lane], NB * wave + c, 64) + before[c];
        if (nzrl[c]) or_bits(s_bits, base, zrl[c], nzrl[c]);                           // (at most 3 x 16 bits)
        if (nbits[c]) or_bits(s_bits, base + nzrl[c], (unsigned long long)bits[c], nbits[c]);       // (at most 16 + 11)
    }
    if (tid == 0 && (total_bits & 7u)) {                         // pad to a byte with 1-bits
        const uint32_t pad = 8u - (total_bits & 7u);
        atomicOr(&s_bits[total_bits >> 5], ((1u << pad) - 1u) << (32u - (total_bits & 31u) - pad));
    }
    __syncthreads();

    // ---- bytes: each lane a stretch, 0x00 behind every 0xFF, RSTm behind all intervals but the last
    const uint32_t nbytes = (total_bits + 7u) >> 3, per = (nbytes + THREADS - 1) / THREADS;
    const uint32_t b0 = (uint32_t)tid * per < nbytes ? (uint32_t)tid * per : nbytes, b1 = b0 + per < nbytes ? b0 + per : nbytes;
    uint32_t ff = 0;
    for (uint32_t i = b0; i < b1; ++i) ff += ((s_bits[i >> 2] >> (24u - 8u * (i & 3u))) & 255u) == 255u ? 1u : 0u;
    uint32_t ff_total = 0;
    uint32_t at = b0 + block_scan<WAVES>(ff, s_part, &ff_total);
    for (uint32_t i = b0; i < b1; ++i) {
        const uint32_t v = (s_bits[i >> 2] >> (24u - 8u * (i & 3u))) & 255u;
        s_out[at++] = (uint8_t)v;
        if (v == 255u) s_out[at++] = 0;
    }
    uint32_t size = nbytes + ff_total;
    if (interval + 1u < nint) {
        if (tid == 0) { s_out[size] = 0xFF; s_out[size + 1u] = (uint8_t)(0xD0u + (interval & 7u)); }
        size += 2u;
    }
    __syncthreads();
    uint32_t* slot = reinterpret_cast<uint32_t*>(slots + (size_t)interval * OPT_SLOT);       // (slots and OPT_SLOT are 16-byte aligned)
    const uint32_t* out_words = reinterpret_cast<const uint32_t*>(s_out);
    for (uint32_t i = tid; i < (size + 3u) / 4u; i += THREADS) slot[i] = out_words[i];
    if (tid == 0) meta[interval] = size;
}

// hist [4][256] -> records [4] (BITS, HUFFVAL, count) and, when ``codes`` is not null, [4][256] symbol -> code | length << 16
__global__ void __launch_bounds__(OPT_TABLE_THREADS) k_opt_tables(const uint32_t* hist, frcnn_jpeg_opt_table_t* records, uint32_t* codes) {
    __shared__ uint32_t s_bits[4][OPT_MAX_DEPTH + 3];           // codes per length, the pseudo-symbol's included
    __shared__ uint32_t s_cnt[4][OPT_MAX_DEPTH + 3];            // symbols 0..255 per tree depth, then the first HUFFVAL position of a depth
    __shared__ uint16_t s_depth[4][256];
    __shared__ uint32_t s_first[4][17], s_cum[4][18];           // per length: its first code, the HUFFVAL positions in front of it
    const int tid = threadIdx.x, lane = tid & 63, t = tid >> 6;
    for (int i = lane; i < OPT_MAX_DEPTH + 3; i += 64) { s_bits[t][i] = 0u; s_cnt[t][i] = 0u; }

    // ---- the tree: lane owns symbols lane + 64 k; symbol 256 (lane 0, k = 4) is the pseudo-symbol of count 1
    unsigned long long f[5];
    int grp[5];
    uint32_t depth[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int s = lane + 64 * k;
        f[k] = k < 4 ? hist[256 * t + s] : (lane == 0 ? 1ull : 0ull);
        grp[k] = f[k] ? s : -1;
        depth[k] = 0u;
    }
    const unsigned long long none = ~0ull;
    for (int step = 0; step < 256; ++step) {
        unsigned long long best = none;
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (f[k]) { const unsigned long long key = (f[k] << 9) | (unsigned long long)(256 - (lane + 64 * k)); best = key < best ? key : best; }
        const unsigned long long k1 = wave_min64(best);
        if (k1 == none) break;
        const int c1 = 256 - (int)(k1 & 511ull);
        best = none;
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (f[k] && lane + 64 * k != c1) {
                const unsigned long long key = (f[k] << 9) | (unsigned long long)(256 - (lane + 64 * k));
                best = key < best ? key : best;
            }
        const unsigned long long k2 = wave_min64(best);
        if (k2 == none) break;
        const int c2 = 256 - (int)(k2 & 511ull);
        const unsigned long long sum = (k1 >> 9) + (k2 >> 9);
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int s = lane + 64 * k;
            if (s == c1) f[k] = sum;
            if (s == c2) f[k] = 0ull;
            if (grp[k] == c1 || grp[k] == c2) { depth[k] += 1u; grp[k] = c1; }
        }
    }
    __syncthreads();                                            // (the cleared counters)
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int s = lane + 64 * k;
        if (depth[k]) {                                         // (depth <= 256 < OPT_MAX_DEPTH + 3)
            atomicAdd(&s_bits[t][depth[k]], 1u);
            if (s < 256) atomicAdd(&s_cnt[t][depth[k]], 1u);
        }
        if (s < 256) s_depth[t][s] = (uint16_t)depth[k];
    }
    __syncthreads();

    // ---- lane 0: lengths past 16 pulled in from the longest down, the pseudo-symbol removed, the canonical codes' starts
    if (lane == 0) {
        uint32_t* b = s_bits[t];
        for (int i = OPT_MAX_DEPTH; i > 16; --i) {
            while (b[i] > 0u) {
                int j = i - 2;
                while (j > 0 && b[j] == 0u) --j;
                if (j == 0) break;
                b[i] -= 2u; b[i - 1] += 1u; b[j + 1] += 2u; b[j] -= 1u;
            }
        }
        int i = 16;
        while (i > 0 && b[i] == 0u) --i;
        if (i > 0) b[i] -= 1u;
        uint32_t at = 0;                                        // first HUFFVAL position of every depth
        for (int d = 1; d <= OPT_MAX_DEPTH; ++d) { const uint32_t n = s_cnt[t][d]; s_cnt[t][d] = at; at += n; }
        uint32_t code = 0, cum = 0;
        for (int len = 1; len <= 16; ++len) {
            s_first[t][len] = code; s_cum[t][len] = cum;
            code = (code + b[len]) << 1; cum += b[len];
        }
        s_cum[t][17] = cum;
        records[t].count = cum;
    }
    __syncthreads();

    // ---- HUFFVAL by (depth, symbol): a symbol's position = its depth's first + the smaller symbols of the same depth; its code
    const uint32_t total = s_cum[t][17];
    if (lane < 16) records[t].bits[lane] = (uint8_t)s_bits[t][lane + 1];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int s = lane + 64 * k;
        const uint32_t d = s_depth[t][s];
        uint32_t entry = 0u;
        if (d) {
            uint32_t pos = s_cnt[t][d];
            for (int i = 0; i < s; ++i) pos += s_depth[t][i] == d ? 1u : 0u;
            if (pos < 256u) records[t].huffval[pos] = (uint8_t)s;
            for (int len = 1; len <= 16; ++len)
                if (pos >= s_cum[t][len] && pos < s_cum[t][len + 1]) entry = (s_first[t][len] + pos - s_cum[t][len]) | ((uint32_t)len << 16);
        }
        if (codes) codes[256 * t + s] = entry;
        if ((uint32_t)s >= total) records[t].huffval[s] = 0;    // (positions past the table)
    }
}

// records: the four tables, or null for Annex K's (the constant header image holds them)
__global__ void __launch_bounds__(JPEG_COPY_THREADS) k_opt_finish(int h, int w, JpegQuant quant, int s420, const frcnn_jpeg_opt_table_t* records,
                                                                   uint32_t* meta, uint32_t nint, uint8_t* out, int32_t* out_len) {
    __shared__ uint32_t s_part[JPEG_COPY_THREADS / 64];
    const int tid = threadIdx.x;
    int seg[5] = {OPT_PREFIX, 0, 0, 0, 0};                      // where the DHT segments and the tail start
    const int std_n[4] = {12, 162, 12, 162}, ids[4] = {0x00, 0x10, 0x01, 0x11};
    for (int t = 0; t < 4; ++t) {
        int n = records ? (int)records[t].count : std_n[t];
        n = n < std_n[t] ? n : std_n[t];                        // (no table of a frame is longer than Annex K's; a bound whatever the counts)
        seg[t + 1] = seg[t] + 21 + n;
    }
    const int header = seg[4] + OPT_TAIL;
    uint32_t offset = (uint32_t)header;
    for (uint32_t i0 = 0; i0 < nint; i0 += JPEG_COPY_THREADS) {
        const uint32_t i = i0 + tid;
        uint32_t sum = 0;
        const uint32_t before = block_scan<JPEG_COPY_THREADS / 64>(i < nint ? meta[i] : 0u, s_part, &sum);
        if (i < nint) meta[(size_t)nint + i] = offset + before;
        offset += sum;
    }
    const int restart = s420 ? 8 : 16;
    for (int i = tid; i < header; i += JPEG_COPY_THREADS) {
        uint32_t v;
        if (i < OPT_PREFIX) {
            v = JPEG_HEADER.b[i];
            if (i >= JPEG_Q0_AT && i < JPEG_Q0_AT + 64) v = quant.q[0][i - JPEG_Q0_AT];
            if (i >= JPEG_Q1_AT && i < JPEG_Q1_AT + 64) v = quant.q[1][i - JPEG_Q1_AT];
            if (i >= JPEG_DIM_AT && i < JPEG_DIM_AT + 4) v = ((i < JPEG_DIM_AT + 2 ? h : w) >> (8 * ((JPEG_DIM_AT + 1 - i) & 1))) & 255;
            if (i == OPT_SAMPLING_AT) v = s420 ? 0x22 : 0x11;
        } else if (i >= seg[4]) {
            const int k = i - seg[4];
            v = JPEG_HEADER.b[JPEG_HEADER_BYTES - OPT_TAIL + k];
            if (k == OPT_DRI_AT) v = restart >> 8;
            if (k == OPT_DRI_AT + 1) v = restart & 255;
        } else if (!records) {
            v = JPEG_HEADER.b[i];
        } else {
            int t = 0;
            while (t < 3 && i >= seg[t + 1]) ++t;
            const int k = i - seg[t], n = seg[t + 1] - seg[t] - 21;
            v = k == 0 ? 0xFF : k == 1 ? 0xC4 : k == 2 ? (19 + n) >> 8 : k == 3 ? (19 + n) & 255 : k == 4 ? ids[t]
                : k < 21 ? records[t].bits[k - 5] : records[t].huffval[k - 21];
        }
        out[i] = (uint8_t)v;
    }
    if (tid == 0) {
        out[offset] = 0xFF; out[offset + 1u] = 0xD9;             // EOI
        *out_len = (int32_t)(offset + 2u);
    }
}

__global__ void __launch_bounds__(JPEG_COPY_THREADS) k_opt_gather(const uint8_t* slots, const uint32_t* meta, uint32_t nint, uint8_t* out) {
    const uint32_t interval = blockIdx.x;
    gather_interval(slots + (size_t)interval * OPT_SLOT, meta[interval], out + meta[(size_t)nint + interval], threadIdx.x);
}

template <bool S420>
void opt_launch(const uint8_t* frame, int h, int w, int bgr, const JpegQuant& quant, bool optimized, uint8_t* out, int32_t* out_len,
                uint8_t* ws, uint32_t nint, hipStream_t s) {
    constexpr int threads = S420 ? 512 : 1024;
    uint32_t* meta = reinterpret_cast<uint32_t*>(ws);
    uint8_t* at = ws + opt_meta_bytes(nint);
    uint32_t* codes = nullptr;
    frcnn_jpeg_opt_table_t* records = nullptr;
    if (optimized) {
        uint32_t* hist = reinterpret_cast<uint32_t*>(at);
        codes = reinterpret_cast<uint32_t*>(at + OPT_HIST_BYTES);
        records = reinterpret_cast<frcnn_jpeg_opt_table_t*>(at + OPT_HIST_BYTES + OPT_CODE_BYTES);
        at += OPT_HIST_BYTES + OPT_CODE_BYTES + OPT_RECORD_BYTES;
        k_opt_clear<<<4, 256, 0, s>>>(hist);
        k_opt_interval<S420, true><<<nint, threads, 0, s>>>(frame, h, w, bgr, quant, nullptr, hist, nullptr, nullptr, nint);
        k_opt_tables<<<1, OPT_TABLE_THREADS, 0, s>>>(hist, records, codes);
    }
    k_opt_interval<S420, false><<<nint, threads, 0, s>>>(frame, h, w, bgr, quant, codes, nullptr, at, meta, nint);
    k_opt_finish<<<1, JPEG_COPY_THREADS, 0, s>>>(h, w, quant, S420 ? 1 : 0, records, meta, nint, out, out_len);
    k_opt_gather<<<nint, JPEG_COPY_THREADS, 0, s>>>(at, meta, nint, out);
}

}  // namespace
}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_jpeg_opt_version(void) { return FRCNN_JPEG_OPT_VERSION; }

extern "C" int frcnn_jpeg_opt_restart_mcus(int subsampling) {
    return subsampling == FRCNN_JPEG_OPT_420 ? 8 : (subsampling == FRCNN_JPEG_OPT_444 ? 16 : 0);
}

extern "C" size_t frcnn_jpeg_opt_bound(int h, int w, int subsampling) { return (size_t)opt_bound(h, w, subsampling); }

extern "C" size_t frcnn_jpeg_opt_workspace_bytes(int h, int w, int subsampling, int huffman) {
    if (!opt_bound(h, w, subsampling) || !opt_huffman_ok(huffman)) return 0;
    const unsigned long long nint = opt_intervals(h, w, subsampling);
    const unsigned long long tables = huffman == FRCNN_JPEG_OPT_OPTIMIZED ? OPT_HIST_BYTES + OPT_CODE_BYTES + OPT_RECORD_BYTES : 0;
    return (size_t)(opt_meta_bytes(nint) + tables + nint * OPT_SLOT);
}

extern "C" int frcnn_jpeg_opt_encode_u8(const uint8_t* frame, int h, int w, int bgr, int quality, int subsampling, int huffman, uint8_t* out,
                                        size_t out_capacity, int32_t* out_len, void* workspace, void* stream) {
    if (!opt_sampling_ok(subsampling)) return fail(FRCNN_E_ARG, "jpeg_opt_encode_u8: subsampling=%d (444 or 420)", subsampling);
    if (!opt_huffman_ok(huffman)) return fail(FRCNN_E_ARG, "jpeg_opt_encode_u8: huffman=%d (0 standard, 1 optimized)", huffman);
    if (h < 1 || w < 1) return fail(FRCNN_E_UNSUPPORTED, "jpeg_opt_encode_u8: frame %dx%d: both sides must be at least 1", h, w);
    if (h > 65535 || w > 65535) return fail(FRCNN_E_UNSUPPORTED, "jpeg_opt_encode_u8: frame %dx%d: a JPEG side is at most 65535", h, w);
    const size_t bound = frcnn_jpeg_opt_bound(h, w, subsampling);
    if (!bound) return fail(FRCNN_E_UNSUPPORTED, "jpeg_opt_encode_u8: frame %dx%d: the largest file would pass 2 GiB", h, w);
    if (quality < 1 || quality > 100) return fail(FRCNN_E_ARG, "jpeg_opt_encode_u8: quality=%d outside 1..100", quality);
    if (!frame || !out || !out_len || !workspace) return fail(FRCNN_E_ARG, "jpeg_opt_encode_u8: null pointer");
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return fail(FRCNN_E_ARG, "jpeg_opt_encode_u8: workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(out_len) & 3u) return fail(FRCNN_E_ARG, "jpeg_opt_encode_u8: out_len must be 4-byte aligned");
    if (out_capacity < bound)
        return fail(FRCNN_E_ARG, "jpeg_opt_encode_u8: out_capacity=%zu below frcnn_jpeg_opt_bound(%d, %d, %d)=%zu", out_capacity, h, w,
                    subsampling, bound);
    const JpegQuant quant = jpeg_quant(quality);
    const uint32_t nint = (uint32_t)opt_intervals(h, w, subsampling);
    const bool optimized = huffman == FRCNN_JPEG_OPT_OPTIMIZED;
    if (subsampling == FRCNN_JPEG_OPT_420)
        opt_launch<true>(frame, h, w, bgr ? 1 : 0, quant, optimized, out, out_len, static_cast<uint8_t*>(workspace), nint, as_stream(stream));
    else
        opt_launch<false>(frame, h, w, bgr ? 1 : 0, quant, optimized, out, out_len, static_cast<uint8_t*>(workspace), nint, as_stream(stream));
    return check_launch("jpeg_opt_encode_u8");
}

extern "C" int frcnn_jpeg_opt_build_tables(const uint32_t* hist, void* tables_out, void* stream) {
    if (!hist || !tables_out) return fail(FRCNN_E_ARG, "jpeg_opt_build_tables: null pointer");
    if ((reinterpret_cast<uintptr_t>(hist) | reinterpret_cast<uintptr_t>(tables_out)) & 3u)
        return fail(FRCNN_E_ARG, "jpeg_opt_build_tables: hist and tables_out must be 4-byte aligned");
    k_opt_tables<<<1, OPT_TABLE_THREADS, 0, as_stream(stream)>>>(hist, static_cast<frcnn_jpeg_opt_table_t*>(tables_out), nullptr);
    return check_launch("jpeg_opt_build_tables");
}
