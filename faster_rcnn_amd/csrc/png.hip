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
#include "common.h"
#include "../../include/ext/frcnn_hip_png.h"

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

static inline unsigned long long png_bands(int h) { return ((unsigned long long)h + PNG_BAND_ROWS - 1) / PNG_BAND_ROWS; }

// a slot holds the largest chunk of a band, and 8 bytes more: the gather reads whole dwords
static inline unsigned long long png_slot_stride(int h, int w) {
    const unsigned long long rows = h < PNG_BAND_ROWS ? h : PNG_BAND_ROWS;
    return (12ull + 2ull + stored_bytes(rows * (1ull + 3ull * w)) + 8ull + 15ull) / 16ull * 16ull;
}

static inline unsigned long long png_meta_bytes(int h) { return (4ull * 4ull * png_bands(h) + 15ull) / 16ull * 16ull; }

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
            unsigned long long end = ((unsigned long long)band + 1ull) * PNG_BAND_ROWS * stride;
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

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_png_version(void) { return FRCNN_PNG_VERSION; }

extern "C" int frcnn_png_band_rows(void) { return PNG_BAND_ROWS; }

extern "C" size_t frcnn_png_bound(int h, int w) {
    if (!png_shape_ok(h, w)) return 0;
    const unsigned long long stride = 1ull + 3ull * w, full = (unsigned long long)h / PNG_BAND_ROWS, rest = (unsigned long long)h % PNG_BAND_ROWS;
    unsigned long long b = PNG_FIXED_BYTES + 2ull + full * (12ull + stored_bytes(PNG_BAND_ROWS * stride));
    if (rest) b += 12ull + stored_bytes(rest * stride);
    return (size_t)b;
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
    k_png_finish<<<1, PNG_THREADS, 0, s>>>(h, w, meta, nbands, out, out_len);
    k_png_gather<<<nbands, PNG_THREADS, 0, s>>>(slots, slot_stride, meta, nbands, out);
    return check_launch("png_encode_u8");
}
