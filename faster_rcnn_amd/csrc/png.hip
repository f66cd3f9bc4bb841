// PNG files encoded on the device (include/ext/frcnn_hip_png.h): an (h, w, 3) uint8 frame -> the bytes of a .png file, in a
// fixed sequence of three launches that allocates nothing, synchronises nothing and reads no host value that varies per frame
// (capturable in a hipGraph, replayable at fixed addresses).  gfx950 (CDNA4) only.  Integer arithmetic throughout: the file is
// a function of the frame's bytes alone.
//
// The stream.  Every scanline is filtered with Sub (type 1): 1 + 3w bytes per row.  The filtered stream is cut into BANDS of
// PNG_BAND_ROWS rows; one workgroup turns one band into one IDAT chunk that holds either
//   (fixed)   one non-final deflate block with the fixed Huffman code -- literals, and a match at distance 1 of length 3..258
//             for every run of a byte equal to its predecessor (after Sub, flat regions are runs of zeros) -- then end-of-block
//             and an empty non-final stored block (000, pad to a byte, 00 00 FF FF: the sync flush), which leaves the band
//             byte-aligned, or
//   (stored)  stored blocks (00, LEN, ~LEN, at most 65535 bytes each) when the fixed form would be longer.  Stored blocks are
//             byte-aligned by themselves and carry no flush.
// Band 0's data starts with the zlib header 78 01.  A last IDAT holds the final empty stored block 01 00 00 FF FF and the
// Adler-32 of the whole filtered stream.  One chunk per band: each CRC-32 covers one workgroup's bytes only.
//
// frcnn_png_bound(h, w), the largest file the encoder can produce -- the stored form bounds every band, because the fixed form is
// kept only where it is not longer:
//     8 (signature) + 25 (IHDR) + 21 (closing IDAT: 12 + 5 + 4) + 12 (IEND)                               = 66
//   + per band of n filtered bytes: 12 (length, type, CRC) + n + 5 * ceil(n / 65535)
//   + 2 (the zlib header, in band 0).
// With one row per band that is 17 bytes on 3w + 1 (0.46 % of a 375x1242 frame).
//
// Launches: k_png_band (one workgroup per band: the whole chunk into the band's fixed-stride slot of the workspace, its size and
// its Adler-32 parts beside it), k_png_finish (one workgroup: exclusive scan of the chunk sizes, the Adler-32 combined, signature,
// IHDR, closing IDAT, IEND and the length word), k_png_gather (one workgroup per band: the chunk copied behind its predecessors,
// in dwords where the destination is aligned).
//
// A second mode, ``huffman`` (include/ext/frcnn_hip_png_huff.h; k_png_huff_band further down), chooses a filter per scanline and
// builds a Huffman code per band of eight rows; it shares the finish and gather launches, the bound's formula and the helpers here.
#include "common.h"
#include "../../include/ext/frcnn_hip_png.h"
#include "../../include/ext/frcnn_hip_png_huff.h"

namespace frcnn {

constexpr int PNG_BAND_ROWS = 1;        // 375 bands for a KITTI frame: more than one per CU (256)
constexpr int PNG_THREADS = 256;
constexpr int PNG_WAVES = PNG_THREADS / 64;
constexpr int PNG_PIECE = 16;           // consecutive filtered bytes one lane turns into tokens
constexpr int PNG_TILE = PNG_THREADS * PNG_PIECE;      // a band is worked through in tiles of 4096 bytes; a run ends at a tile's edge
// a tile's bits: at most 9 per byte (a literal >= 144; a match is at most 18 bits for at least 3 bytes) behind at most 31 carried
constexpr int PNG_BITWORDS = (31 + 9 * PNG_TILE) / 32 + 2;
constexpr uint32_t PNG_ADLER_MOD = 65521u;
constexpr uint32_t PNG_CRC_POLY = 0xEDB88320u;
constexpr int PNG_FIXED_BYTES = 66;     // signature, IHDR, closing IDAT, IEND
constexpr int PNG_HEAD_BYTES = 33;      // signature + IHDR
constexpr unsigned long long PNG_MAX_STREAM = 0x7FFFFFFFull;

// ---------------------------------------------------------------------------------------------------------------- host sizes
static inline unsigned long long stored_bytes(unsigned long long n) { return n + 5ull * ((n + 65534ull) / 65535ull); }

static inline bool png_shape_ok(int h, int w) {
    return h >= 1 && w >= 1 && (unsigned long long)h * (1ull + 3ull * (unsigned long long)w) <= PNG_MAX_STREAM;
}

static inline unsigned long long png_bands(int h, int band_rows = PNG_BAND_ROWS) {
    return ((unsigned long long)h + band_rows - 1) / band_rows;
}

// a slot holds the largest chunk of a band, and 8 bytes more: the gather reads whole dwords
static inline unsigned long long png_slot_stride(int h, int w, int band_rows = PNG_BAND_ROWS) {
    const unsigned long long rows = h < band_rows ? h : band_rows;
    return (12ull + 2ull + stored_bytes(rows * (1ull + 3ull * w)) + 8ull + 15ull) / 16ull * 16ull;
}

static inline unsigned long long png_meta_bytes(int h, int band_rows = PNG_BAND_ROWS) {
    return (4ull * 4ull * png_bands(h, band_rows) + 15ull) / 16ull * 16ull;
}

// the stored form of every band plus the framing (the header comment's formula), for bands of ``band_rows`` rows
static inline unsigned long long png_bound_rows(int h, int w, int band_rows) {
    const unsigned long long stride = 1ull + 3ull * w, full = (unsigned long long)h / band_rows, rest = (unsigned long long)h % band_rows;
    unsigned long long b = PNG_FIXED_BYTES + 2ull + full * (12ull + stored_bytes(band_rows * stride));
    if (rest) b += 12ull + stored_bytes(rest * stride);
    return b;
}

// ---------------------------------------------------------------------------------------------------------- device helpers
struct OpAdd { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; } };
struct OpMax { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; } };
struct OpMin { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a < b ? a : b; } };
struct OpXor { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a ^ b; } };

// Exclusive scan of one value per lane over the workgroup (REV: from the last lane down), wave64 shuffles inside a wave and
// PNG_WAVES partials through LDS.  Every lane of the workgroup calls it; ``total`` receives the reduction over all lanes.
template <class Op, bool REV>
__device__ uint32_t block_scan(uint32_t v, uint32_t ident, Op op, uint32_t* s_part, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = REV ? __shfl_down(x, d, 64) : __shfl_up(x, d, 64);
        if (REV ? lane + d < 64 : lane >= d) x = op(x, t);
    }
    if (lane == (REV ? 0 : 63)) s_part[wave] = x;
    uint32_t e = REV ? __shfl_down(x, 1, 64) : __shfl_up(x, 1, 64);
    if (lane == (REV ? 63 : 0)) e = ident;
    __syncthreads();
    uint32_t pre = ident, tot = ident;
#pragma unroll
    for (int k = 0; k < PNG_WAVES; ++k) {
        const uint32_t p = s_part[k];
        tot = op(tot, p);
        if (REV ? k > wave : k < wave) pre = op(pre, p);
    }
    __syncthreads();
    if (total) *total = tot;
    return op(pre, e);
}

// CRC-32 (reflected, polynomial 0xEDB88320) as arithmetic in GF(2)[x] mod P, bit 31 = x^0: a * b mod P
__device__ uint32_t gf2_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m != 0; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ PNG_CRC_POLY : b >> 1;
    }
    return p;
}

// x^(8 n) mod P: crc(A || B) = crc(A) * x^(8 len(B)) ^ crc(B) for finished CRCs (the conditioning cancels)
__device__ uint32_t gf2_x_pow_bytes(uint32_t n) {
    uint32_t sq = 0x40000000u;                                             // x^1
    sq = gf2_mul(sq, sq); sq = gf2_mul(sq, sq); sq = gf2_mul(sq, sq);      // x^8
    uint32_t r = 0x80000000u;                                              // x^0
    for (; n != 0; n >>= 1) {
        if (n & 1u) r = gf2_mul(sq, r);
        sq = gf2_mul(sq, sq);
    }
    return r;
}

__device__ __forceinline__ uint32_t crc_byte(uint32_t crc, uint32_t byte) {
    crc ^= byte;
#pragma unroll
    for (int k = 0; k < 8; ++k) crc = (crc & 1u) ? (crc >> 1) ^ PNG_CRC_POLY : crc >> 1;
    return crc;
}

__device__ uint32_t crc_bytes(const uint8_t* p, uint32_t n) {
    uint32_t crc = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; ++i) crc = crc_byte(crc, p[i]);
    return crc ^ 0xFFFFFFFFu;
}

__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}

// byte ``col`` of filtered scanline ``row``: the filter type, then Sub over pixels in RGB order (bgr: the frame holds B, G, R)
__device__ __forceinline__ uint32_t png_filtered(const uint8_t* frame, int w, int bgr, int row, int col) {
    if (col == 0) return 1u;
    const int x = col - 1, px = x / 3, ch = x - 3 * px;
    const uint8_t* p = frame + ((size_t)row * (size_t)w + (size_t)px) * 3 + (bgr ? 2 - ch : ch);
    const uint32_t left = px > 0 ? p[-3] : 0u;
    return (p[0] - left) & 255u;
}

// fixed-code tokens, as (bits, LSB first) | count << 24.  Huffman codes enter the stream most significant bit first.
__device__ __forceinline__ uint32_t png_literal(uint32_t v) {
    return v < 144u ? (__brev(0x30u + v) >> 24) | (8u << 24) : (__brev(0x190u + v - 144u) >> 23) | (9u << 24);
}

// a match of ``len`` in [3, 258] at distance 1: length symbol 257 + k, its extra bits, distance code 0 (5 zero bits)
__device__ __forceinline__ uint32_t png_match(uint32_t len) {
    const uint32_t m = len - 3u;
    uint32_t k, eb, ev;
    if (len == 258u) { k = 28u; eb = 0u; ev = 0u; }
    else if (m < 8u) { k = m; eb = 0u; ev = 0u; }
    else { eb = 29u - __clz(m); k = 4u * eb + 4u + ((m >> eb) & 3u); ev = m & ((1u << eb) - 1u); }
    uint32_t code, cb;
    if (k < 23u) { code = __brev(k + 1u) >> 25; cb = 7u; }                  // symbols 257..279: 7 bits, 0000001..
    else { code = __brev(0xC0u + k - 23u) >> 24; cb = 8u; }                 // symbols 280..285: 8 bits, 11000000..
    return (code | (ev << cb)) | ((cb + eb + 5u) << 24);
}

// ------------------------------------------------------------------------------------------------------------------ kernels
// meta: [4][nbands] uint32 = chunk size, chunk offset in the file (k_png_finish), Adler parts A = sum of bytes and
// B = sum of (n - i) * byte_i, both mod 65521.
__global__ void __launch_bounds__(PNG_THREADS) k_png_band(const uint8_t* frame, int h, int w, int bgr, uint8_t* slots,
                                                           unsigned long long slot_stride, uint32_t* meta, uint32_t nbands) {
    __shared__ __align__(16) uint8_t s_b[PNG_TILE];
    __shared__ uint32_t s_bits[PNG_BITWORDS];
    __shared__ uint32_t s_part[PNG_WAVES];
    const int tid = threadIdx.x;
    const uint32_t band = blockIdx.x;
    const int stride = 1 + 3 * w;
    const int row0 = (int)band * PNG_BAND_ROWS;
    const int rows = h - row0 < PNG_BAND_ROWS ? h - row0 : PNG_BAND_ROWS;
    const int n = rows * stride;
    uint8_t* slot = slots + (size_t)band * (size_t)slot_stride;
    uint8_t* data = slot + 8;
    uint32_t* pay = reinterpret_cast<uint32_t*>(data);                      // (slots and slot_stride are 16-byte aligned)
    const uint32_t cap_words = (uint32_t)((slot_stride - 8) / 4);
    const uint32_t pre = band == 0 ? 2u : 0u;
    const uint32_t stored = pre + (uint32_t)n + 5u * (uint32_t)((n + 65534) / 65535);

    // the bit stream so far: ``wbase`` whole words stored, ``cb`` bits waiting in ``carry`` (uniform over the workgroup)
    uint32_t carry = band == 0 ? (0x0178u | (2u << 16)) : 2u;              // [78 01] BFINAL = 0, BTYPE = 01
    uint32_t cb = band == 0 ? 19u : 3u, wbase = 0;
    uint32_t acc_a = 0, acc_b = 0;

    for (int t0 = 0; t0 < n; t0 += PNG_TILE) {
        const int tn = n - t0 < PNG_TILE ? n - t0 : PNG_TILE;
        // ---- filter into LDS, lanes side by side; the Adler sums on the way (per tile and lane below 2^29)
        uint32_t a = 0, b = 0;
#pragma unroll 4
        for (int k = 0; k < PNG_PIECE; ++k) {
            const int j = k * PNG_THREADS + tid;
            if (j < tn) {
                const int q = t0 + j, r = q / stride;
                const uint32_t v = png_filtered(frame, w, bgr, row0 + r, q - r * stride);
                s_b[j] = (uint8_t)v;
                a += v;
                b += v * ((uint32_t)(n - q) % PNG_ADLER_MOD);
            }
        }
        acc_a = (acc_a + a) % PNG_ADLER_MOD;
        acc_b = (acc_b + b % PNG_ADLER_MOD) % PNG_ADLER_MOD;
        for (int i = tid; i < PNG_BITWORDS; i += PNG_THREADS) s_bits[i] = i == 0 ? carry : 0u;
        __syncthreads();

        // ---- classify: bit k of ``cont`` = byte base + k repeats its predecessor (never the tile's first byte)
        const int base = tid * PNG_PIECE;
        uint32_t cont = 0;
        uint32_t bytes[PNG_PIECE / 4];
#pragma unroll
        for (int k = 0; k < PNG_PIECE / 4; ++k) bytes[k] = reinterpret_cast<const uint32_t*>(s_b)[tid * (PNG_PIECE / 4) + k];
        uint32_t prev = base > 0 ? s_b[base - 1] : 0x100u;
#pragma unroll
        for (int k = 0; k < PNG_PIECE; ++k) {
            const uint32_t v = (bytes[k >> 2] >> (8 * (k & 3))) & 255u;
            if (base + k < tn && v == prev) cont |= 1u << k;
            prev = v;
        }
        const uint32_t in_tile = base >= tn ? 0u : (tn - base >= PNG_PIECE ? 0xFFFFu : (1u << (tn - base)) - 1u);
        const uint32_t starts = in_tile & ~cont;                            // bytes that are no continuation
        const uint32_t stops = 0xFFFFu & ~cont;                             // ... and those past the tile's end: a run stops there
        // the last start at or before each byte (as index + 1) and the first stop after it
        const uint32_t my_start = starts ? (uint32_t)(base + 32 - __clz(starts)) : 0u;
        const uint32_t my_stop = stops ? (uint32_t)(base + __ffs(stops) - 1) : 0x7FFFFFFFu;
        const uint32_t start_before = block_scan<OpMax, false>(my_start, 0u, OpMax(), s_part, nullptr);
        const uint32_t stop_after = block_scan<OpMin, true>(my_stop, 0x7FFFFFFFu, OpMin(), s_part, nullptr);

        // ---- tokens: a run [rs, e) is cut into matches of 258 from its start; a last piece shorter than 3 becomes literals
        uint32_t tok[PNG_PIECE];
        uint32_t nbits = 0;
#pragma unroll
        for (int k = 0; k < PNG_PIECE; ++k) {
            const uint32_t v = (bytes[k >> 2] >> (8 * (k & 3))) & 255u;
            uint32_t t = 0;
            if ((in_tile >> k) & 1u) {
                if (!((cont >> k) & 1u)) t = png_literal(v);
                else {
                    const uint32_t below = starts & ((2u << k) - 1u), above = stops & ~((2u << k) - 1u);
                    const uint32_t rs = below ? (uint32_t)(base + 32 - __clz(below)) : start_before;   // (start index + 1)
                    uint32_t e = above ? (uint32_t)(base + __ffs(above) - 1) : stop_after;
                    e = e < (uint32_t)tn ? e : (uint32_t)tn;
                    const uint32_t o = (uint32_t)(base + k) - rs, piece = o / 258u, left = (e - rs) - piece * 258u;
                    const uint32_t len = left < 258u ? left : 258u;
                    if (len < 3u) t = png_literal(v);
                    else if (o - piece * 258u == 0u) t = png_match(len);
                }
            }
            tok[k] = t;
            nbits += t >> 24;
        }
        uint32_t tile_bits = 0;
        uint32_t pos = cb + block_scan<OpAdd, false>(nbits, 0u, OpAdd(), s_part, &tile_bits);
#pragma unroll
        for (int k = 0; k < PNG_PIECE; ++k) {
            const uint32_t c = tok[k] >> 24;
            if (c) {
                const uint32_t val = tok[k] & 0xFFFFFFu, sh = pos & 31u;
                atomicOr(&s_bits[pos >> 5], val << sh);
                if (sh + c > 32u) atomicOr(&s_bits[(pos >> 5) + 1], val >> (32u - sh));
                pos += c;
            }
        }
        __syncthreads();
        // ---- whole words to the slot; what would pass the stored form's size is dropped (the band is then re-emitted stored)
        const uint32_t end_bits = cb + tile_bits, full = end_bits >> 5;
        for (uint32_t i = tid; i < full; i += PNG_THREADS)
            if (wbase + i < cap_words) pay[wbase + i] = s_bits[i];
        carry = s_bits[full];
        cb = end_bits & 31u;
        wbase += full;
        __syncthreads();
    }

    // ---- end-of-block (7 zero bits), the empty stored block: 000, pad, 00 00 FF FF
    const uint32_t tail = (cb + 10u + 7u) / 8u;                            // bytes still to come from ``carry`` (<= 6)
    const unsigned long long fixed_len = 4ull * wbase + tail + 4ull;
    const bool use_stored = fixed_len > stored;
    const uint32_t dlen = use_stored ? stored : (uint32_t)fixed_len;
    if (!use_stored) {
        if (tid == 0) {
            uint8_t* p = data + 4ull * wbase;
            for (uint32_t i = 0; i < tail; ++i) p[i] = i < 4u ? (uint8_t)(carry >> (8u * i)) : (uint8_t)0;
            p[tail] = 0; p[tail + 1] = 0; p[tail + 2] = 0xFF; p[tail + 3] = 0xFF;
        }
    } else {
        if (band == 0 && tid == 0) { data[0] = 0x78; data[1] = 0x01; }
        const int nblk = (n + 65534) / 65535;
        for (int k = tid; k < nblk; k += PNG_THREADS) {
            const uint32_t len = (uint32_t)(n - k * 65535 < 65535 ? n - k * 65535 : 65535);
            uint8_t* p = data + pre + (size_t)k * 65540u;
            p[0] = 0; p[1] = (uint8_t)len; p[2] = (uint8_t)(len >> 8); p[3] = (uint8_t)~len; p[4] = (uint8_t)(~len >> 8);
        }
        for (int q = tid; q < n; q += PNG_THREADS) {
            const int r = q / stride;
            data[pre + 5u * (uint32_t)(q / 65535 + 1) + (uint32_t)q] = (uint8_t)png_filtered(frame, w, bgr, row0 + r, q - r * stride);
        }
    }
    if (tid == 0) { put_be32(slot, dlen); slot[4] = 'I'; slot[5] = 'D'; slot[6] = 'A'; slot[7] = 'T'; }
    __syncthreads();

    // ---- CRC-32 over type + data: each lane its stretch, combined by x^(8 * bytes behind the stretch)
    const uint32_t clen = dlen + 4u, per = (clen + PNG_THREADS - 1) / PNG_THREADS;
    const uint32_t c0 = (uint32_t)tid * per < clen ? (uint32_t)tid * per : clen, c1 = c0 + per < clen ? c0 + per : clen;
    uint32_t part = c1 > c0 ? gf2_mul(gf2_x_pow_bytes(clen - c1), crc_bytes(slot + 4 + c0, c1 - c0)) : 0u;
    uint32_t crc = 0;
    block_scan<OpXor, false>(part, 0u, OpXor(), s_part, &crc);
    uint32_t sum_a = 0, sum_b = 0;
    block_scan<OpAdd, false>(acc_a, 0u, OpAdd(), s_part, &sum_a);
    block_scan<OpAdd, false>(acc_b, 0u, OpAdd(), s_part, &sum_b);
    if (tid == 0) {
        put_be32(data + dlen, crc);
        meta[band] = dlen + 12u;
        meta[2 * (size_t)nbands + band] = sum_a % PNG_ADLER_MOD;
        meta[3 * (size_t)nbands + band] = sum_b % PNG_ADLER_MOD;
    }
}

template <int BAND_ROWS>
__global__ void __launch_bounds__(PNG_THREADS) k_png_finish(int h, int w, uint32_t* meta, uint32_t nbands, uint8_t* out,
                                                             int32_t* out_len) {
    __shared__ uint32_t s_part[PNG_WAVES];
    const int tid = threadIdx.x;
    const unsigned long long stride = 1ull + 3ull * (unsigned long long)w, total = (unsigned long long)h * stride;
    uint32_t offset = PNG_HEAD_BYTES, a = 0, b = 0;
    for (uint32_t b0 = 0; b0 < nbands; b0 += PNG_THREADS) {
        const uint32_t band = b0 + tid;
        const bool live = band < nbands;
        uint32_t sum = 0;
        const uint32_t before = block_scan<OpAdd, false>(live ? meta[band] : 0u, 0u, OpAdd(), s_part, &sum);
        if (live) {
            meta[(size_t)nbands + band] = offset + before;
            // a band's bytes weigh (bytes behind the band) more in s2 than inside the band alone
            unsigned long long end = ((unsigned long long)band + 1ull) * BAND_ROWS * stride;
            end = end < total ? end : total;
            const unsigned long long ba = meta[2 * (size_t)nbands + band], bb = meta[3 * (size_t)nbands + band];
            a = (a + (uint32_t)ba) % PNG_ADLER_MOD;
            b = (uint32_t)((b + bb + ba * ((total - end) % PNG_ADLER_MOD)) % PNG_ADLER_MOD);
        }
        offset += sum;
    }
    uint32_t sum_a = 0, sum_b = 0;
    block_scan<OpAdd, false>(a, 0u, OpAdd(), s_part, &sum_a);
    block_scan<OpAdd, false>(b, 0u, OpAdd(), s_part, &sum_b);
    if (tid != 0) return;
    const uint32_t s1 = (1u + sum_a) % PNG_ADLER_MOD, s2 = (uint32_t)((total + sum_b) % PNG_ADLER_MOD);
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    for (int i = 0; i < 8; ++i) out[i] = sig[i];
    uint8_t* p = out + 8;
    put_be32(p, 13u); p[4] = 'I'; p[5] = 'H'; p[6] = 'D'; p[7] = 'R';
    put_be32(p + 8, (uint32_t)w); put_be32(p + 12, (uint32_t)h);
    p[16] = 8; p[17] = 2; p[18] = 0; p[19] = 0; p[20] = 0;                  // 8 bits, colour type 2 (RGB), no interlace
    put_be32(p + 21, crc_bytes(p + 4, 17u));
    p = out + offset;
    put_be32(p, 9u); p[4] = 'I'; p[5] = 'D'; p[6] = 'A'; p[7] = 'T';
    p[8] = 1; p[9] = 0; p[10] = 0; p[11] = 0xFF; p[12] = 0xFF;              // BFINAL = 1, stored, empty
    put_be32(p + 13, (s2 << 16) | s1);
    put_be32(p + 17, crc_bytes(p + 4, 13u));
    p += 21;
    put_be32(p, 0u); p[4] = 'I'; p[5] = 'E'; p[6] = 'N'; p[7] = 'D';
    put_be32(p + 8, 0xAE426082u);
    *out_len = (int32_t)(offset + 33u);
}

__global__ void __launch_bounds__(PNG_THREADS) k_png_gather(const uint8_t* slots, unsigned long long slot_stride, const uint32_t* meta,
                                                             uint32_t nbands, uint8_t* out) {
    const uint32_t band = blockIdx.x, tid = threadIdx.x;
    const uint8_t* src = slots + (size_t)band * (size_t)slot_stride;
    const uint32_t n = meta[band];
    uint8_t* dst = out + meta[(size_t)nbands + band];
    // bytes up to the destination's dword boundary, dwords funnelled from two aligned source dwords, bytes at the end
    uint32_t head = (uint32_t)((4u - (reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u);
    head = head < n ? head : n;
    if (tid < head) dst[tid] = src[tid];
    const uint32_t words = (n - head) / 4u, shift = 8u * head;
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(src);
    uint32_t* dw = reinterpret_cast<uint32_t*>(dst + head);
    for (uint32_t i = tid; i < words; i += PNG_THREADS)
        dw[i] = shift ? (sw[i] >> shift) | (sw[i + 1] << (32u - shift)) : sw[i];
    const uint32_t done = head + 4u * words;
    if (tid < n - done) dst[done + tid] = src[done + tid];
}

// ------------------------------------------------------------------------------------------------------------ huffman mode
// include/ext/frcnn_hip_png_huff.h.  A band is PNG_HUFF_BAND_ROWS rows; one workgroup makes its IDAT chunk in three walks over the band:
//   choose   per row the filter (None, Sub, Up, Average, Paeth) with the smallest sum of |filtered byte as int8|, lowest type on a tie;
//   count    filter a 4096-byte tile into LDS, tokenise it as the runs mode does, count literal/length symbols in LDS (Adler sums on the way);
//   emit     the same tokens again, now through the band's own code: bit counts scanned, bits ORed into LDS words, the bit position
//            carried from tile to tile (tiles inside a band are not byte-aligned).
// Between count and emit: code lengths limited to 15 bits, canonical codes, the block header (every length spelt out through a
// code-length code limited to 7 bits; the distance alphabet is code 0 alone, one bit), and the exact size of the dynamic block -- a
// band whose dynamic form is not strictly shorter than its stored form is written as stored blocks of the filtered bytes.
// tests/png_huff_ref.py states the same rules in Python; the two agree byte for byte.
#ifndef FRCNN_PNG_HUFF_BAND_ROWS
#define FRCNN_PNG_HUFF_BAND_ROWS 8     // (a build-time override exists for the 4-against-8 measurement of DESIGN section 8 only)
#endif
constexpr int PNG_HUFF_BAND_ROWS = FRCNN_PNG_HUFF_BAND_ROWS;
constexpr int HUFF_SYMS = 286;          // literal/length alphabet
constexpr int HUFF_PAD = 288;
constexpr int HUFF_CL_SYMS = 19;
// a tile's bits: at most 15 per byte (a literal; a match is at most 15 + 5 + 1 for at least 3 bytes) behind at most 31 carried
constexpr int PNG_HUFF_BITWORDS = (31 + 15 * PNG_TILE) / 32 + 2;
// the order in which the header lists the code-length code's own lengths (RFC 1951 3.2.7)
__constant__ uint8_t HUFF_CL_ORDER[HUFF_CL_SYMS] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// byte ``col`` of scanline ``row`` under filter ``ft``; the prior row is the RAW one (zero above row 0), so rows are independent
__device__ __forceinline__ uint32_t png_filtered_ft(const uint8_t* frame, int w, int bgr, int row, int col, uint32_t ft) {
    if (col == 0) return ft;
    const int x = col - 1, px = x / 3, ch = x - 3 * px;
    const uint8_t* p = frame + ((size_t)row * (size_t)w + (size_t)px) * 3 + (bgr ? 2 - ch : ch);
    const int v = p[0];
    if (ft == 0u) return (uint32_t)v;
    const int a = px > 0 ? p[-3] : 0;
    if (ft == 1u) return (uint32_t)(v - a) & 255u;
    const uint8_t* q = p - (size_t)w * 3;
    const int b = row > 0 ? q[0] : 0;
    if (ft == 2u) return (uint32_t)(v - b) & 255u;
    if (ft == 3u) return (uint32_t)(v - ((a + b) >> 1)) & 255u;
    const int c = (row > 0 && px > 0) ? q[-3] : 0;
    const int pp = a + b - c, pa = abs(pp - a), pb = abs(pp - b), pc = abs(pp - c);
    const int pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    return (uint32_t)(v - pred) & 255u;
}

__device__ __forceinline__ uint32_t abs_int8(uint32_t v) { return v < 128u ? v : 256u - v; }

// extra bits behind length symbol ``s`` (257..285)
__device__ __forceinline__ uint32_t huff_extra_bits(uint32_t s) {
    const uint32_t k = s - 257u;
    return (k < 8u || k == 28u) ? 0u : (k - 4u) / 4u;
}

// The tile in s_b[0 .. tn) -> this lane's tokens for its PNG_PIECE bytes, the runs mode's tokenisation: 0 = none, else
// (symbol + 1) | extra value << 16 | extra bits << 24.  Every lane of the workgroup calls it.
__device__ __forceinline__ void png_tile_tokens(const uint8_t* s_b, int tn, uint32_t* s_part, uint32_t (&tok)[PNG_PIECE]) {
    const int tid = threadIdx.x, base = tid * PNG_PIECE;
    uint32_t cont = 0;
    uint32_t bytes[PNG_PIECE / 4];
#pragma unroll
    for (int k = 0; k < PNG_PIECE / 4; ++k) bytes[k] = reinterpret_cast<const uint32_t*>(s_b)[tid * (PNG_PIECE / 4) + k];
    uint32_t prev = base > 0 ? s_b[base - 1] : 0x100u;
#pragma unroll
    for (int k = 0; k < PNG_PIECE; ++k) {
        const uint32_t v = (bytes[k >> 2] >> (8 * (k & 3))) & 255u;
        if (base + k < tn && v == prev) cont |= 1u << k;
        prev = v;
    }
    const uint32_t in_tile = base >= tn ? 0u : (tn - base >= PNG_PIECE ? 0xFFFFu : (1u << (tn - base)) - 1u);
    const uint32_t starts = in_tile & ~cont, stops = 0xFFFFu & ~cont;
    const uint32_t my_start = starts ? (uint32_t)(base + 32 - __clz(starts)) : 0u;
    const uint32_t my_stop = stops ? (uint32_t)(base + __ffs(stops) - 1) : 0x7FFFFFFFu;
    const uint32_t start_before = block_scan<OpMax, false>(my_start, 0u, OpMax(), s_part, nullptr);
    const uint32_t stop_after = block_scan<OpMin, true>(my_stop, 0x7FFFFFFFu, OpMin(), s_part, nullptr);
#pragma unroll
    for (int k = 0; k < PNG_PIECE; ++k) {
        const uint32_t v = (bytes[k >> 2] >> (8 * (k & 3))) & 255u;
        uint32_t t = 0;
        if ((in_tile >> k) & 1u) {
            if (!((cont >> k) & 1u)) t = v + 1u;
            else {
                const uint32_t below = starts & ((2u << k) - 1u), above = stops & ~((2u << k) - 1u);
                const uint32_t rs = below ? (uint32_t)(base + 32 - __clz(below)) : start_before;       // (start index + 1)
                uint32_t e = above ? (uint32_t)(base + __ffs(above) - 1) : stop_after;
                e = e < (uint32_t)tn ? e : (uint32_t)tn;
                const uint32_t o = (uint32_t)(base + k) - rs, piece = o / 258u, left = (e - rs) - piece * 258u;
                const uint32_t len = left < 258u ? left : 258u;
                if (len < 3u) t = v + 1u;
                else if (o - piece * 258u == 0u) {
                    const uint32_t m = len - 3u;
                    uint32_t sk, eb = 0u, ev = 0u;
                    if (len == 258u) sk = 28u;
                    else if (m < 8u) sk = m;
                    else { eb = 29u - __clz(m); sk = 4u * eb + 4u + ((m >> eb) & 3u); ev = m & ((1u << eb) - 1u); }
                    t = (257u + sk + 1u) | (ev << 16) | (eb << 24);
                }
            }
        }
        tok[k] = t;
    }
}

// LDS of the code builder (one set serves the literal/length code and then the code-length code)
struct HuffScratch {
    uint32_t w[HUFF_PAD];               // leaf weights, sorted by (count, symbol)
    uint32_t iw[HUFF_PAD];              // inner nodes' weights, in the order they were made
    uint16_t sym[HUFF_PAD];             // sorted position -> symbol
    uint16_t pl[HUFF_PAD], pi[HUFF_PAD];// parent (an inner node) of a leaf / an inner node
    uint16_t depth[HUFF_PAD];           // of the inner nodes
    uint32_t count[16];                 // symbols per length
    uint32_t start[17];                 // sorted positions [start[l], start[l] + count[l]) get length l: the longest first
    uint32_t next[16];                  // first canonical code of a length
    uint32_t m;
};

// freq[0 .. n) -> code[0 .. n) = (the canonical code, bit-reversed for an LSB-first stream) | length << 24, 0 for an unused symbol;
// no length above ``maxbits``.  The rules of tests/png_huff_ref.py code_lengths(): two-queue Huffman over the leaves sorted by
// (count, symbol), a leaf before an inner node of equal weight; depths clamped to maxbits; per unit of Kraft excess one leaf of the
// longest length below maxbits goes one level down and takes a maxbits leaf beside it; lengths dealt out over the sorted symbols,
// longest first.  At least two symbols have a count (symbol 256 and a filter byte; length 0 or 1 and another).  Every lane calls it.
__device__ void huff_build(const uint32_t* freq, int n, uint32_t maxbits, uint32_t* code, HuffScratch& h) {
    const int tid = threadIdx.x;
    if (tid < 16) h.count[tid] = 0;
    if (tid == 0) h.m = 0;
    __syncthreads();
    for (int s = tid; s < n; s += PNG_THREADS) {
        const uint32_t f = freq[s];
        code[s] = 0;
        if (f) {
            uint32_t rank = 0;
            for (int j = 0; j < n; ++j) {
                const uint32_t g = freq[j];
                rank += (g != 0u && (g < f || (g == f && j < s))) ? 1u : 0u;
            }
            h.w[rank] = f;
            h.sym[rank] = (uint16_t)s;
            atomicAdd(&h.m, 1u);
        }
    }
    __syncthreads();
    const uint32_t m = h.m;
    if (tid == 0) {
        uint32_t li = 0, ii = 0;
        for (uint32_t k = 0; k + 1 < m; ++k) {
            uint32_t total = 0;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                if (li < m && (ii >= k || h.w[li] <= h.iw[ii])) { h.pl[li] = (uint16_t)k; total += h.w[li]; ++li; }
                else { h.pi[ii] = (uint16_t)k; total += h.iw[ii]; ++ii; }
            }
            h.iw[k] = total;
        }
        h.depth[m - 2] = 0;
        for (int k = (int)m - 3; k >= 0; --k) h.depth[k] = (uint16_t)(h.depth[h.pi[k]] + 1u);
    }
    __syncthreads();
    for (uint32_t i = tid; i < m; i += PNG_THREADS) {
        const uint32_t d = h.depth[h.pl[i]] + 1u;
        atomicAdd(&h.count[d < maxbits ? d : maxbits], 1u);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t kraft = 0;
        for (uint32_t l = 1; l <= maxbits; ++l) kraft += h.count[l] << (maxbits - l);
        for (uint32_t over = kraft - (1u << maxbits); over != 0; --over) {
            uint32_t b = maxbits - 1u;
            while (h.count[b] == 0u) --b;
            h.count[b] -= 1u; h.count[b + 1u] += 2u; h.count[maxbits] -= 1u;
        }
        uint32_t at = 0, c = 0;
        h.count[0] = 0;
        for (uint32_t l = maxbits; l >= 1u; --l) { h.start[l] = at; at += h.count[l]; }
        for (uint32_t l = 1; l <= maxbits; ++l) { c = (c + h.count[l - 1u]) << 1; h.next[l] = c; }
    }
    __syncthreads();
    for (uint32_t i = tid; i < m; i += PNG_THREADS) {
        uint32_t l = maxbits;
        while (!(i >= h.start[l] && i < h.start[l] + h.count[l])) --l;
        code[h.sym[i]] = l << 24;
    }
    __syncthreads();
    uint32_t mine[(HUFF_PAD + PNG_THREADS - 1) / PNG_THREADS];
    for (int s = tid, r = 0; s < n; s += PNG_THREADS, ++r) {
        const uint32_t l = code[s] >> 24;
        uint32_t c = 0;
        if (l) {
            c = h.next[l];
            for (int j = 0; j < s; ++j) c += (code[j] >> 24) == l ? 1u : 0u;
            c = (__brev(c) >> (32u - l)) | (l << 24);
        }
        mine[r] = c;
    }
    __syncthreads();
    for (int s = tid, r = 0; s < n; s += PNG_THREADS, ++r) code[s] = mine[r];
    __syncthreads();
}

// a 64-bit sum over the workgroup through two 32-bit scans (a lane's value below 2^44)
__device__ unsigned long long block_sum64(unsigned long long v, uint32_t* s_part) {
    uint32_t lo = 0, hi = 0;
    block_scan<OpAdd, false>((uint32_t)(v & 0xFFFFull), 0u, OpAdd(), s_part, &lo);
    block_scan<OpAdd, false>((uint32_t)(v >> 16), 0u, OpAdd(), s_part, &hi);
    return ((unsigned long long)hi << 16) + lo;
}

// s_bits[0 .. full) to the slot behind the ``wbase`` words already there; the bit position moves on by ``bits``
__device__ __forceinline__ void huff_flush_words(const uint32_t* s_bits, uint32_t* pay, uint32_t cap_words, uint32_t bits, uint32_t& carry,
                                                 uint32_t& cb, uint32_t& wbase) {
    const uint32_t end_bits = cb + bits, full = end_bits >> 5;
    for (uint32_t i = threadIdx.x; i < full; i += PNG_THREADS)
        if (wbase + i < cap_words) pay[wbase + i] = s_bits[i];
    carry = s_bits[full];
    cb = end_bits & 31u;
    wbase += full;
    __syncthreads();
}

__global__ void __launch_bounds__(PNG_THREADS) k_png_huff_band(const uint8_t* frame, int h, int w, int bgr, uint8_t* slots,
                                                                unsigned long long slot_stride, uint32_t* meta, uint32_t nbands) {
    __shared__ __align__(16) uint8_t s_b[PNG_TILE];
    __shared__ uint32_t s_bits[PNG_HUFF_BITWORDS];
    __shared__ uint32_t s_part[PNG_WAVES];
    __shared__ unsigned long long s_cost[PNG_HUFF_BAND_ROWS][PNG_WAVES][5];
    __shared__ uint32_t s_ft[PNG_HUFF_BAND_ROWS];
    __shared__ uint32_t s_freq[HUFF_PAD], s_code[HUFF_PAD];                 // literal/length counts; codes as huff_build leaves them
    __shared__ uint32_t s_clfreq[HUFF_CL_SYMS], s_clcode[HUFF_CL_SYMS];
    __shared__ uint32_t s_hclen;
    __shared__ HuffScratch s_h;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t band = blockIdx.x;
    const int stride = 1 + 3 * w;
    const int row0 = (int)band * PNG_HUFF_BAND_ROWS;
    const int rows = h - row0 < PNG_HUFF_BAND_ROWS ? h - row0 : PNG_HUFF_BAND_ROWS;
    const int n = rows * stride;
    uint8_t* slot = slots + (size_t)band * (size_t)slot_stride;
    uint8_t* data = slot + 8;
    uint32_t* pay = reinterpret_cast<uint32_t*>(data);                      // (slots and slot_stride are 16-byte aligned)
    const uint32_t cap_words = (uint32_t)((slot_stride - 8) / 4);
    const uint32_t pre = band == 0 ? 2u : 0u;
    const uint32_t stored = pre + (uint32_t)n + 5u * (uint32_t)((n + 65534) / 65535);

    // ---- choose: five sums per row, lanes side by side along the row, reduced in 64 bits
    for (int r = 0; r < rows; ++r) {
        unsigned long long cost[5] = {0, 0, 0, 0, 0};
        for (int col = 1 + tid; col < stride; col += PNG_THREADS) {
#pragma unroll
            for (uint32_t ft = 0; ft < 5u; ++ft) cost[ft] += abs_int8(png_filtered_ft(frame, w, bgr, row0 + r, col, ft));
        }
#pragma unroll
        for (int ft = 0; ft < 5; ++ft) {
            unsigned long long c = cost[ft];
            for (int d = 32; d >= 1; d >>= 1) c += __shfl_down(c, d, 64);
            if (lane == 0) s_cost[r][wave][ft] = c;
        }
    }
    for (int i = tid; i < HUFF_PAD; i += PNG_THREADS) s_freq[i] = i == 256 ? 1u : 0u;
    __syncthreads();
    if (tid < rows) {
        unsigned long long best = ~0ull;
        uint32_t pick = 0;
        for (uint32_t ft = 0; ft < 5u; ++ft) {
            unsigned long long c = 0;
            for (int k = 0; k < PNG_WAVES; ++k) c += s_cost[tid][k][ft];
            if (c < best) { best = c; pick = ft; }
        }
        s_ft[tid] = pick;
    }
    __syncthreads();

    // ---- count: symbols of the band's tokens, the Adler sums on the way (per tile and lane below 2^29)
    uint32_t acc_a = 0, acc_b = 0;
    uint32_t tok[PNG_PIECE];
    for (int t0 = 0; t0 < n; t0 += PNG_TILE) {
        const int tn = n - t0 < PNG_TILE ? n - t0 : PNG_TILE;
        uint32_t a = 0, b = 0;
#pragma unroll 4
        for (int k = 0; k < PNG_PIECE; ++k) {
            const int j = k * PNG_THREADS + tid;
            if (j < tn) {
                const int q = t0 + j, r = q / stride;
                const uint32_t v = png_filtered_ft(frame, w, bgr, row0 + r, q - r * stride, s_ft[r]);
                s_b[j] = (uint8_t)v;
                a += v;
                b += v * ((uint32_t)(n - q) % PNG_ADLER_MOD);
            }
        }
        acc_a = (acc_a + a) % PNG_ADLER_MOD;
        acc_b = (acc_b + b % PNG_ADLER_MOD) % PNG_ADLER_MOD;
        __syncthreads();
        png_tile_tokens(s_b, tn, s_part, tok);
#pragma unroll
        for (int k = 0; k < PNG_PIECE; ++k)
            if (tok[k]) atomicAdd(&s_freq[(tok[k] & 0xFFFFu) - 1u], 1u);
        __syncthreads();
    }

    // ---- the band's code, the header's code, the size of the dynamic form
    huff_build(s_freq, HUFF_SYMS, 15u, s_code, s_h);
    uint32_t last = 0;
    for (int s = tid; s < HUFF_SYMS; s += PNG_THREADS)
        if (s_code[s]) last = (uint32_t)s;
    uint32_t nlit = 0;
    block_scan<OpMax, false>(last, 0u, OpMax(), s_part, &nlit);
    nlit += 1u;                                                             // >= 257: symbol 256 always has a code
    if (tid < HUFF_CL_SYMS) s_clfreq[tid] = tid == 1 ? 1u : 0u;             // (the distance alphabet: code 0 alone, length 1)
    __syncthreads();
    for (uint32_t s = tid; s < nlit; s += PNG_THREADS) atomicAdd(&s_clfreq[s_code[s] >> 24], 1u);
    __syncthreads();
    huff_build(s_clfreq, HUFF_CL_SYMS, 7u, s_clcode, s_h);
    if (tid == 0) {
        uint32_t hc = 4;
        for (uint32_t i = 4; i < (uint32_t)HUFF_CL_SYMS; ++i)
            if (s_clcode[HUFF_CL_ORDER[i]]) hc = i + 1u;
        s_hclen = hc;
    }
    unsigned long long bits = 0;
    for (int s = tid; s < HUFF_SYMS; s += PNG_THREADS)
        bits += (unsigned long long)s_freq[s] * ((s_code[s] >> 24) + (s > 256 ? huff_extra_bits((uint32_t)s) + 1u : 0u));
    if (tid < HUFF_CL_SYMS) bits += (unsigned long long)s_clfreq[tid] * (s_clcode[tid] >> 24);
    bits = block_sum64(bits, s_part);                                       // (its barriers publish s_hclen)
    const uint32_t hclen = s_hclen;
    bits += 8ull * pre + 3ull + 14ull + 3ull * hclen + 3ull;                // zlib header, block header, HLIT HDIST HCLEN, ..., 000
    const unsigned long long dynamic_len = (bits + 7ull) / 8ull + 4ull;
    const bool use_stored = dynamic_len >= stored;
    uint32_t dlen = stored;

    if (!use_stored) {
        // ---- emit.  The bit stream so far: ``wbase`` whole words in the slot, ``cb`` bits waiting in ``carry`` (uniform)
        uint32_t carry = band == 0 ? (0x0178u | (4u << 16)) : 4u;          // [78 01] BFINAL = 0, BTYPE = 10
        uint32_t cb = band == 0 ? 19u : 3u, wbase = 0;
        // the header: fixed fields by one lane, then the nlit + 1 lengths, two per lane
        for (int i = tid; i < PNG_HUFF_BITWORDS; i += PNG_THREADS) s_bits[i] = 0u;
        __syncthreads();
        const uint32_t fixed_bits = 14u + 3u * hclen;
        if (tid == 0) {
            uint32_t pos = cb;
            s_bits[0] = carry;
            auto put = [&](uint32_t val, uint32_t c) {
                const uint32_t sh = pos & 31u;
                s_bits[pos >> 5] |= val << sh;
                if (sh + c > 32u) s_bits[(pos >> 5) + 1] |= val >> (32u - sh);
                pos += c;
            };
            put(nlit - 257u, 5u); put(0u, 5u); put(hclen - 4u, 4u);
            for (uint32_t i = 0; i < hclen; ++i) put(s_clcode[HUFF_CL_ORDER[i]] >> 24, 3u);
        }
        __syncthreads();
        {
            uint32_t t2[2], nb = 0;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const uint32_t i = 2u * tid + k;
                t2[k] = i < nlit ? s_clcode[s_code[i] >> 24] : (i == nlit ? s_clcode[1] : 0u);
                nb += t2[k] >> 24;
            }
            uint32_t seq_bits = 0;
            uint32_t pos = cb + fixed_bits + block_scan<OpAdd, false>(nb, 0u, OpAdd(), s_part, &seq_bits);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const uint32_t c = t2[k] >> 24;
                if (c) {
                    const uint32_t val = t2[k] & 0xFFFFFFu, sh = pos & 31u;
                    atomicOr(&s_bits[pos >> 5], val << sh);
                    if (sh + c > 32u) atomicOr(&s_bits[(pos >> 5) + 1], val >> (32u - sh));
                    pos += c;
                }
            }
            __syncthreads();
            huff_flush_words(s_bits, pay, cap_words, fixed_bits + seq_bits, carry, cb, wbase);
        }
        for (int t0 = 0; t0 < n; t0 += PNG_TILE) {
            const int tn = n - t0 < PNG_TILE ? n - t0 : PNG_TILE;
#pragma unroll 4
            for (int k = 0; k < PNG_PIECE; ++k) {
                const int j = k * PNG_THREADS + tid;
                if (j < tn) {
                    const int q = t0 + j, r = q / stride;
                    s_b[j] = (uint8_t)png_filtered_ft(frame, w, bgr, row0 + r, q - r * stride, s_ft[r]);
                }
            }
            for (int i = tid; i < PNG_HUFF_BITWORDS; i += PNG_THREADS) s_bits[i] = i == 0 ? carry : 0u;
            __syncthreads();
            png_tile_tokens(s_b, tn, s_part, tok);
            uint32_t nbits = 0;
#pragma unroll
            for (int k = 0; k < PNG_PIECE; ++k) {
                uint32_t t = 0;
                if (tok[k]) {
                    const uint32_t c = s_code[(tok[k] & 0xFFFFu) - 1u], cl = c >> 24, eb = tok[k] >> 24;
                    t = (c & 0xFFFFFFu) | (((tok[k] >> 16) & 0xFFu) << cl);
                    // behind a length symbol: its extra bits and the one-bit distance code 0
                    t |= (cl + eb + ((tok[k] & 0xFFFFu) > 257u ? 1u : 0u)) << 24;
                }
                tok[k] = t;
                nbits += t >> 24;
            }
            uint32_t tile_bits = 0;
            uint32_t pos = cb + block_scan<OpAdd, false>(nbits, 0u, OpAdd(), s_part, &tile_bits);
#pragma unroll
            for (int k = 0; k < PNG_PIECE; ++k) {
                const uint32_t c = tok[k] >> 24;
                if (c) {
                    const uint32_t val = tok[k] & 0xFFFFFFu, sh = pos & 31u;
                    atomicOr(&s_bits[pos >> 5], val << sh);
                    if (sh + c > 32u) atomicOr(&s_bits[(pos >> 5) + 1], val >> (32u - sh));
                    pos += c;
                }
            }
            __syncthreads();
            huff_flush_words(s_bits, pay, cap_words, tile_bits, carry, cb, wbase);
        }
        // ---- end-of-block, the empty stored block: 000, pad, 00 00 FF FF
        const uint32_t eob = s_code[256], eob_bits = eob >> 24;
        const unsigned long long fin = (unsigned long long)carry | ((unsigned long long)(eob & 0xFFFFFFu) << cb);
        const uint32_t tail = (cb + eob_bits + 3u + 7u) / 8u;              // bytes still to come (<= 7)
        dlen = 4u * wbase + tail + 4u;                                      // (= dynamic_len)
        if (tid == 0) {
            uint8_t* p = data + 4ull * wbase;
            for (uint32_t i = 0; i < tail; ++i) p[i] = (uint8_t)(fin >> (8u * i));
            p[tail] = 0; p[tail + 1] = 0; p[tail + 2] = 0xFF; p[tail + 3] = 0xFF;
        }
    } else {
        if (band == 0 && tid == 0) { data[0] = 0x78; data[1] = 0x01; }
        const int nblk = (n + 65534) / 65535;
        for (int k = tid; k < nblk; k += PNG_THREADS) {
            const uint32_t len = (uint32_t)(n - k * 65535 < 65535 ? n - k * 65535 : 65535);
            uint8_t* p = data + pre + (size_t)k * 65540u;
            p[0] = 0; p[1] = (uint8_t)len; p[2] = (uint8_t)(len >> 8); p[3] = (uint8_t)~len; p[4] = (uint8_t)(~len >> 8);
        }
        for (int q = tid; q < n; q += PNG_THREADS) {
            const int r = q / stride;
            data[pre + 5u * (uint32_t)(q / 65535 + 1) + (uint32_t)q] = (uint8_t)png_filtered_ft(frame, w, bgr, row0 + r, q - r * stride, s_ft[r]);
        }
    }
    if (tid == 0) { put_be32(slot, dlen); slot[4] = 'I'; slot[5] = 'D'; slot[6] = 'A'; slot[7] = 'T'; }
    __syncthreads();

    // ---- CRC-32 over type + data: each lane its stretch, combined by x^(8 * bytes behind the stretch)
    const uint32_t clen = dlen + 4u, per = (clen + PNG_THREADS - 1) / PNG_THREADS;
    const uint32_t c0 = (uint32_t)tid * per < clen ? (uint32_t)tid * per : clen, c1 = c0 + per < clen ? c0 + per : clen;
    uint32_t part = c1 > c0 ? gf2_mul(gf2_x_pow_bytes(clen - c1), crc_bytes(slot + 4 + c0, c1 - c0)) : 0u;
    uint32_t crc = 0;
    block_scan<OpXor, false>(part, 0u, OpXor(), s_part, &crc);
    uint32_t sum_a = 0, sum_b = 0;
    block_scan<OpAdd, false>(acc_a, 0u, OpAdd(), s_part, &sum_a);
    block_scan<OpAdd, false>(acc_b, 0u, OpAdd(), s_part, &sum_b);
    if (tid == 0) {
        put_be32(data + dlen, crc);
        meta[band] = dlen + 12u;
        meta[2 * (size_t)nbands + band] = sum_a % PNG_ADLER_MOD;
        meta[3 * (size_t)nbands + band] = sum_b % PNG_ADLER_MOD;
    }
}

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_png_version(void) { return FRCNN_PNG_VERSION; }

extern "C" int frcnn_png_band_rows(void) { return PNG_BAND_ROWS; }

extern "C" size_t frcnn_png_bound(int h, int w) {
    if (!png_shape_ok(h, w)) return 0;
    return (size_t)png_bound_rows(h, w, PNG_BAND_ROWS);
}

extern "C" size_t frcnn_png_workspace_bytes(int h, int w) {
    if (!png_shape_ok(h, w)) return 0;
    return (size_t)(png_meta_bytes(h) + png_bands(h) * png_slot_stride(h, w));
}

extern "C" int frcnn_png_encode_u8(const uint8_t* frame, int h, int w, int bgr, uint8_t* out, size_t out_capacity, int32_t* out_len,
                                   void* workspace, void* stream) {
    if (h < 1 || w < 1) return fail(FRCNN_E_UNSUPPORTED, "png_encode_u8: frame %dx%d: both sides must be at least 1", h, w);
    if (!png_shape_ok(h, w))
        return fail(FRCNN_E_UNSUPPORTED, "png_encode_u8: frame %dx%d: the filtered stream (h * (1 + 3w) bytes) would pass 2 GiB", h, w);
    if (!frame || !out || !out_len || !workspace) return fail(FRCNN_E_ARG, "png_encode_u8: null pointer");
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return fail(FRCNN_E_ARG, "png_encode_u8: workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(out_len) & 3u) return fail(FRCNN_E_ARG, "png_encode_u8: out_len must be 4-byte aligned");
    const size_t bound = frcnn_png_bound(h, w);
    if (out_capacity < bound)
        return fail(FRCNN_E_ARG, "png_encode_u8: out_capacity=%zu below frcnn_png_bound(%d, %d)=%zu", out_capacity, h, w, bound);
    const uint32_t nbands = (uint32_t)png_bands(h);
    uint32_t* meta = static_cast<uint32_t*>(workspace);
    uint8_t* slots = static_cast<uint8_t*>(workspace) + png_meta_bytes(h);
    const unsigned long long slot_stride = png_slot_stride(h, w);
    hipStream_t s = as_stream(stream);
    k_png_band<<<nbands, PNG_THREADS, 0, s>>>(frame, h, w, bgr ? 1 : 0, slots, slot_stride, meta, nbands);
    k_png_finish<PNG_BAND_ROWS><<<1, PNG_THREADS, 0, s>>>(h, w, meta, nbands, out, out_len);
    k_png_gather<<<nbands, PNG_THREADS, 0, s>>>(slots, slot_stride, meta, nbands, out);
    return check_launch("png_encode_u8");
}

// ---------------------------------------------------------------------------------- include/ext/frcnn_hip_png_huff.h
extern "C" int frcnn_png_huff_version(void) { return FRCNN_PNG_HUFF_VERSION; }

extern "C" int frcnn_png_huff_band_rows(void) { return PNG_HUFF_BAND_ROWS; }

extern "C" size_t frcnn_png_huff_bound(int h, int w) {
    if (!png_shape_ok(h, w)) return 0;
    return (size_t)png_bound_rows(h, w, PNG_HUFF_BAND_ROWS);
}

extern "C" size_t frcnn_png_huff_workspace_bytes(int h, int w) {
    if (!png_shape_ok(h, w)) return 0;
    return (size_t)(png_meta_bytes(h, PNG_HUFF_BAND_ROWS) + png_bands(h, PNG_HUFF_BAND_ROWS) * png_slot_stride(h, w, PNG_HUFF_BAND_ROWS));
}

extern "C" int frcnn_png_huff_encode_u8(const uint8_t* frame, int h, int w, int bgr, uint8_t* out, size_t out_capacity, int32_t* out_len,
                                        void* workspace, void* stream) {
    if (h < 1 || w < 1) return fail(FRCNN_E_UNSUPPORTED, "png_huff_encode_u8: frame %dx%d: both sides must be at least 1", h, w);
    if (!png_shape_ok(h, w))
        return fail(FRCNN_E_UNSUPPORTED, "png_huff_encode_u8: frame %dx%d: the filtered stream (h * (1 + 3w) bytes) would pass 2 GiB", h, w);
    if (!frame || !out || !out_len || !workspace) return fail(FRCNN_E_ARG, "png_huff_encode_u8: null pointer");
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return fail(FRCNN_E_ARG, "png_huff_encode_u8: workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(out_len) & 3u) return fail(FRCNN_E_ARG, "png_huff_encode_u8: out_len must be 4-byte aligned");
    const size_t bound = frcnn_png_huff_bound(h, w);
    if (out_capacity < bound)
        return fail(FRCNN_E_ARG, "png_huff_encode_u8: out_capacity=%zu below frcnn_png_huff_bound(%d, %d)=%zu", out_capacity, h, w, bound);
    const uint32_t nbands = (uint32_t)png_bands(h, PNG_HUFF_BAND_ROWS);
    uint32_t* meta = static_cast<uint32_t*>(workspace);
    uint8_t* slots = static_cast<uint8_t*>(workspace) + png_meta_bytes(h, PNG_HUFF_BAND_ROWS);
    const unsigned long long slot_stride = png_slot_stride(h, w, PNG_HUFF_BAND_ROWS);
    hipStream_t s = as_stream(stream);
    k_png_huff_band<<<nbands, PNG_THREADS, 0, s>>>(frame, h, w, bgr ? 1 : 0, slots, slot_stride, meta, nbands);
    k_png_finish<PNG_HUFF_BAND_ROWS><<<1, PNG_THREADS, 0, s>>>(h, w, meta, nbands, out, out_len);
    k_png_gather<<<nbands, PNG_THREADS, 0, s>>>(slots, slot_stride, meta, nbands, out);
    return check_launch("png_huff_encode_u8");
}
