// What the device JPEG encoder's translation units share (jpeg.hip: revision 1 of include/ext/frcnn_hip_jpeg.h; jpeg_opt.hip: 4:2:0 and
// optimised Huffman tables, include/ext/frcnn_hip_jpeg_opt.h): the Annex K tables, the integer cosines, the constant header image, the
// scans and the bit writer.  Everything sits in an unnamed namespace: each translation unit has its own copy, __constant__ data included.
#pragma once
#include "common.h"
#include "ycc_common.h"
#include "../../include/ext/frcnn_hip_jpeg.h"

namespace frcnn {
namespace {

constexpr int JPEG_RESTART_MCUS = FRCNN_JPEG_RESTART_MCUS;
constexpr int JPEG_THREADS = 64 * JPEG_RESTART_MCUS;            // k_jpeg_interval: one wave per MCU
constexpr int JPEG_BLOCKS = 3 * JPEG_RESTART_MCUS;              // blocks per interval
constexpr int JPEG_BLOCK_BITS = 20 + 63 * 26;
constexpr int JPEG_BLOCK_BYTES = (JPEG_BLOCK_BITS + 7) / 8;     // 208
constexpr int JPEG_MAX_BITS = JPEG_BLOCKS * JPEG_BLOCK_BITS;    // 79584 per interval
constexpr int JPEG_BITWORDS = (JPEG_MAX_BITS + 31) / 32 + 3;    // (a lane's 59 bits touch three words)
constexpr int JPEG_MAX_BYTES = (JPEG_MAX_BITS + 7) / 8;         // 9948 before stuffing
constexpr int JPEG_SLOT = (2 * JPEG_MAX_BYTES + 2 + 8 + 15) / 16 * 16;     // stuffed + RSTm, and 8 more: the gather reads whole dwords
constexpr int JPEG_COPY_THREADS = 256;                          // k_jpeg_finish, k_jpeg_gather
constexpr int JPEG_HEADER_BYTES = 629;
constexpr int JPEG_Q0_AT = 25, JPEG_Q1_AT = 94, JPEG_DIM_AT = 163;          // where the header takes the tables and h, w
constexpr unsigned long long JPEG_MAX_FILE = 0x7FFFFFFFull;
static_assert(JPEG_THREADS <= 1024 && JPEG_BLOCKS <= 64, "one wave scans the interval's blocks");

struct JpegQuant { uint8_t q[2][64]; };                          // luma, chroma; zigzag order (kernel argument, by value)

// ITU-T T.81 Annex K.1, K.2 (natural order)
constexpr uint8_t K1_LUMA[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                                 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                                 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t K2_CHROMA[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                                   47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                   99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// zigzag position -> natural index 8 * v + u
constexpr uint8_t ZIGZAG[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// round(2^13 * c(u) / 2 * cos(k pi / 16)): [0] is u = 0 (c = 1 / sqrt 2), [k] the cosine of k * pi / 16 for u > 0
constexpr int COS_MAG[8] = {2896, 4017, 3784, 3406, 2896, 2276, 1567, 799};

// COS[u][x] of the 8-point DCT-II: the angle (2x + 1) u * pi / 16 folded into the first quadrant
constexpr int dct_cos(int u, int x) {
    if (u == 0) return COS_MAG[0];
    int k = ((2 * x + 1) * u) % 32;                             // cos has period 32 (in units of pi / 16)
    if (k > 16) k = 32 - k;
    return k == 8 ? 0 : (k < 8 ? COS_MAG[k] : -COS_MAG[16 - k]);
}

// Annex K.3: BITS (codes per length 1..16) and HUFFVAL (symbols in code order) of tables K.3 - K.6
struct HuffSpec { uint8_t bits[16]; uint8_t vals[162]; int n; };
constexpr HuffSpec DC_LUMA = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr HuffSpec DC_CHROMA = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr HuffSpec AC_LUMA = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08,
     0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
     0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
     0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
     0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
     0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA}, 162};
constexpr HuffSpec AC_CHROMA = {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
     0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
     0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
     0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
     0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
     0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA}, 162};

// What the kernels read, made at compile time: cosines per lane, zigzag, and the four codes as symbol -> code | length << 16 (Annex C:
// codes of one length are consecutive, in HUFFVAL order), [0] DC luma, [1] DC chroma (16 entries used), [2] AC luma, [3] AC chroma.
struct JpegTables {
    int16_t cos[64];                    // [u][x]
    uint8_t zigzag[64];
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};

constexpr void fill_codes(const HuffSpec& s, uint32_t* out) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.bits[len - 1]; ++i) out[s.vals[k++]] = code++ | ((uint32_t)len << 16);
        code <<= 1;
    }
}

constexpr JpegTables make_tables() {
    JpegTables t = {};
    for (int u = 0; u < 8; ++u)
        for (int x = 0; x < 8; ++x) t.cos[8 * u + x] = (int16_t)dct_cos(u, x);
    for (int i = 0; i < 64; ++i) t.zigzag[i] = ZIGZAG[i];
    fill_codes(DC_LUMA, t.dc[0]);
    fill_codes(DC_CHROMA, t.dc[1]);
    fill_codes(AC_LUMA, t.ac[0]);
    fill_codes(AC_CHROMA, t.ac[1]);
    return t;
}

// SOI .. SOS with zeros where the quantisation tables (JPEG_Q0_AT, JPEG_Q1_AT) and height, width (JPEG_DIM_AT) go
struct JpegHeader { uint8_t b[JPEG_HEADER_BYTES]; int n, q0, q1, dim; };

constexpr JpegHeader make_header() {
    JpegHeader h = {};
    int n = 0;
    auto put = [&](int v) { h.b[n++] = (uint8_t)v; };
    auto seg = [&](int marker, int payload) { put(0xFF); put(marker); put((payload + 2) >> 8); put((payload + 2) & 255); };
    put(0xFF); put(0xD8);
    seg(0xE0, 14);                                              // APP0: "JFIF\0", 1.01, no units, 1:1, no thumbnail
    put('J'); put('F'); put('I'); put('F'); put(0); put(1); put(1); put(0); put(0); put(1); put(0); put(1); put(0); put(0);
    seg(0xDB, 65); put(0); h.q0 = n; n += 64;                   // DQT: 8-bit entries, table 0 (luma), table 1 (chroma)
    seg(0xDB, 65); put(1); h.q1 = n; n += 64;
    seg(0xC0, 15); put(8); h.dim = n; n += 4;                   // SOF0: 8 bits, h, w, three components of 1x1; Y table 0, Cb Cr table 1
    put(3); put(1); put(0x11); put(0); put(2); put(0x11); put(1); put(3); put(0x11); put(1);
    const HuffSpec* specs[4] = {&DC_LUMA, &AC_LUMA, &DC_CHROMA, &AC_CHROMA};
    const int ids[4] = {0x00, 0x10, 0x01, 0x11};                // (class << 4 | table)
    for (int t = 0; t < 4; ++t) {
        seg(0xC4, 17 + specs[t]->n); put(ids[t]);
        for (int i = 0; i < 16; ++i) put(specs[t]->bits[i]);
        for (int i = 0; i < specs[t]->n; ++i) put(specs[t]->vals[i]);
    }
    seg(0xDD, 2); put(JPEG_RESTART_MCUS >> 8); put(JPEG_RESTART_MCUS & 255);
    seg(0xDA, 10); put(3); put(1); put(0x00); put(2); put(0x11); put(3); put(0x11); put(0); put(63); put(0);
    h.n = n;
    return h;
}

constexpr JpegHeader HEADER_IMAGE = make_header();
static_assert(HEADER_IMAGE.n == JPEG_HEADER_BYTES && HEADER_IMAGE.q0 == JPEG_Q0_AT && HEADER_IMAGE.q1 == JPEG_Q1_AT &&
              HEADER_IMAGE.dim == JPEG_DIM_AT, "the header's layout");

__constant__ JpegTables JPEG_TABLES = make_tables();
__constant__ JpegHeader JPEG_HEADER = make_header();

// ---------------------------------------------------------------------------------------------------------------- host sizes
inline unsigned long long jpeg_mcus(int h, int w) { return (((unsigned long long)h + 7) / 8) * (((unsigned long long)w + 7) / 8); }

inline unsigned long long jpeg_intervals(int h, int w) { return (jpeg_mcus(h, w) + JPEG_RESTART_MCUS - 1) / JPEG_RESTART_MCUS; }

inline unsigned long long jpeg_bound(int h, int w) {
    if (h < 1 || w < 1 || h > 65535 || w > 65535) return 0;
    const unsigned long long b = JPEG_HEADER_BYTES + 2ull + 2ull * JPEG_BLOCK_BYTES * 3ull * jpeg_mcus(h, w) + 4ull * jpeg_intervals(h, w);
    return b <= JPEG_MAX_FILE ? b : 0;
}

inline unsigned long long jpeg_meta_bytes(int h, int w) { return (2ull * 4ull * jpeg_intervals(h, w) + 15ull) / 16ull * 16ull; }

// the IJG quality rule (quality 1..100) over Annex K.1 / K.2, in zigzag order as the DQT segments hold them
inline JpegQuant jpeg_quant(int quality) {
    JpegQuant quant;
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        const int l = (K1_LUMA[ZIGZAG[i]] * scale + 50) / 100, c = (K2_CHROMA[ZIGZAG[i]] * scale + 50) / 100;
        quant.q[0][i] = (uint8_t)(l < 1 ? 1 : (l > 255 ? 255 : l));
        quant.q[1][i] = (uint8_t)(c < 1 ? 1 : (c > 255 ? 255 : c));
    }
    return quant;
}

// ---------------------------------------------------------------------------------------------------------- device helpers
// inclusive sum over the wave
__device__ __forceinline__ uint32_t wave_scan(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// Exclusive sum of one value per lane over a workgroup of WAVES waves; ``total`` receives the sum.  Every lane calls it.
template <int WAVES>
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* s_part, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = wave_scan(v);
    if (lane == 63) s_part[wave] = incl;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < WAVES; ++k) {
        const uint32_t p = s_part[k];
        tot += p;
        if (k < wave) pre += p;
    }
    __syncthreads();
    *total = tot;
    return pre + incl - v;
}

// ``n`` bits (the low bits of ``v``, first bit = the highest) into the big-endian bit stream of ``s_bits`` at bit ``pos``
__device__ __forceinline__ void or_bits(uint32_t* s_bits, uint32_t pos, unsigned long long v, uint32_t n) {
    const unsigned long long top = v << (64u - n);              // (1 <= n <= 59)
    const uint32_t hi = (uint32_t)(top >> 32), lo = (uint32_t)top, sh = pos & 31u, at = pos >> 5;
    const uint32_t w0 = hi >> sh, w1 = sh ? (hi << (32u - sh)) | (lo >> sh) : lo, w2 = sh ? lo << (32u - sh) : 0u;
    atomicOr(&s_bits[at], w0);
    if (w1) atomicOr(&s_bits[at + 1], w1);
    if (w2) atomicOr(&s_bits[at + 2], w2);
}

// (category, its low bits) of a DC difference or an AC coefficient
__device__ __forceinline__ uint32_t category(int v, uint32_t* low) {
    const uint32_t size = 32u - (uint32_t)__clz(v < 0 ? -v : v);           // (__clz(0) = 32)
    *low = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
    return size;
}

// One interval's ``n`` bytes from its slot ``src`` (16-byte aligned) to ``dst`` (any alignment) by a workgroup of JPEG_COPY_THREADS:
// bytes up to the destination's dword boundary, dwords funnelled from two aligned source dwords, bytes at the end (as k_png_gather)
__device__ __forceinline__ void gather_interval(const uint8_t* src, uint32_t n, uint8_t* dst, uint32_t tid) {
    uint32_t head = (uint32_t)((4u - (reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u);
    head = head < n ? head : n;
    if (tid < head) dst[tid] = src[tid];
    const uint32_t words = (n - head) / 4u, shift = 8u * head;
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(src);
    uint32_t* dw = reinterpret_cast<uint32_t*>(dst + head);
    for (uint32_t i = tid; i < words; i += JPEG_COPY_THREADS)
        dw[i] = shift ? (sw[i] >> shift) | (sw[i + 1] << (32u - shift)) : sw[i];
    const uint32_t done = head + 4u * words;
    if (tid < n - done) dst[done + tid] = src[done + tid];
}

}  // namespace
}  // namespace frcnn
