// JPEG files encoded on the device (include/ext/frcnn_hip_jpeg.h): an (h, w, 3) uint8 frame -> the bytes of a baseline JFIF .jpg file,
// in the launch layout of the PNG encoder (png.hip): three launches that allocate nothing, synchronise nothing and read no host value
// that varies per frame (capturable in a hipGraph).  gfx950 (CDNA4) only, wave64 throughout.  Integer arithmetic throughout: the file is
// a function of (frame, quality) alone, and tests/jpeg_ref.py states the same rules in Python; the two agree byte for byte.
//
// The stream.  SOF0, 8 bits, Y Cb Cr at 1x1 each (4:4:4: the drawn boxes are 3 pixels wide), so an MCU is one 8x8 block of each
// component.  Quantisation tables: ITU-T T.81 Annex K.1 / K.2 scaled by the IJG quality rule, computed on the host per call and passed
// to the kernels BY VALUE (a captured pass bakes them in).  Huffman tables: Annex K.3, written as they stand.  The entropy-coded data is
// cut into restart intervals of JPEG_RESTART_MCUS MCUs in raster order: an interval starts with DC predictors of 0 and ends padded to a
// byte with 1-bits, so intervals are independent and one workgroup codes one of them.
//
//   k_jpeg_interval  one workgroup per interval, one wave per MCU, lane = pixel, then coefficient: colour transform (16 fractional bits),
//                    the 8x8 DCT as a row pass and a column pass of lane permutes over an integer cosine table, one division to
//                    quantise, a permute into zigzag order; the zero runs from a ballot; per lane at most 3 ZRL + a code + value bits
//                    (59 bits); bit counts scanned across the wave and the interval's 48 blocks, bits ORed into LDS words; then bytes:
//                    0xFF bytes counted by a scan, stuffed bytes and the RSTm marker staged in LDS and copied to the interval's slot
//                    of the workspace in dwords, its size to a table.
//   k_jpeg_finish    one workgroup: exclusive scan of the sizes, the header (a constant image with the quantisation tables and the
//                    frame's size patched in), EOI and the length word.
//   k_jpeg_gather    one workgroup per interval: its bytes copied behind the header, dwords funnelled to the destination's alignment.
//
// Sizes.  A block is at most 20 + 63 * 26 = 1658 bits (DC: a 9-bit code + 11 bits; AC: a 16-bit code + 10 bits each): 208 bytes, 416
// with every byte stuffed.  frcnn_jpeg_bound = header + 2 + per interval (416 * 3 * MCUs + 2 + 2).
#include "common.h"
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

// ------------------------------------------------------------------------------------------------------------------ kernels
// meta: [2][nint] uint32 = interval size in bytes (stuffed, with its RSTm), its offset in the file (k_jpeg_finish)
__global__ void __launch_bounds__(JPEG_THREADS) k_jpeg_interval(const uint8_t* frame, int h, int w, int bgr, JpegQuant quant, uint8_t* slots,
                                                                 uint32_t* meta, uint32_t nint) {
    __shared__ uint32_t s_bits[JPEG_BITWORDS];
    __shared__ __align__(16) uint8_t s_out[JPEG_SLOT];
    __shared__ uint32_t s_ac[2][256], s_dc[2][16];
    __shared__ uint8_t s_q[2][64];
    __shared__ int s_pred[3][JPEG_RESTART_MCUS];
    __shared__ uint32_t s_tot[64];
    __shared__ uint32_t s_part[JPEG_RESTART_MCUS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t interval = blockIdx.x;
    const int mw = (w + 7) / 8, mh = (h + 7) / 8;
    const uint32_t mcus = (uint32_t)mw * (uint32_t)mh;
    const uint32_t first = interval * JPEG_RESTART_MCUS;
    const uint32_t count = mcus - first < (uint32_t)JPEG_RESTART_MCUS ? mcus - first : (uint32_t)JPEG_RESTART_MCUS;
    const bool live = (uint32_t)wave < count;                   // (a wave past a short last interval works on its last MCU and emits nothing)

    for (int i = tid; i < JPEG_BITWORDS; i += JPEG_THREADS) s_bits[i] = 0u;
    if (tid < 512) s_ac[tid >> 8][tid & 255] = JPEG_TABLES.ac[tid >> 8][tid & 255];
    if (tid < 32) s_dc[tid >> 4][tid & 15] = JPEG_TABLES.dc[tid >> 4][tid & 15];
    if (tid < 128) s_q[tid >> 6][tid & 63] = quant.q[tid >> 6][tid & 63];
    if (tid < 64) s_tot[tid] = 0u;

    // ---- the MCU's pixels (the last column / row repeated past the frame), colour transform with 16 fractional bits
    const uint32_t m = live ? first + (uint32_t)wave : first + count - 1u;
    const int my = (int)(m / (uint32_t)mw), mx = (int)(m - (uint32_t)my * (uint32_t)mw);
    const int py = my * 8 + (lane >> 3) < h ? my * 8 + (lane >> 3) : h - 1, px = mx * 8 + (lane & 7) < w ? mx * 8 + (lane & 7) : w - 1;
    const uint8_t* p = frame + ((size_t)py * (size_t)w + (size_t)px) * 3;
    const int r = p[bgr ? 2 : 0], g = p[1], b = p[bgr ? 0 : 2];
    const int chroma_round = (128 << 16) + 32767;
    int comp[3];
    comp[0] = ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16) - 128;
    comp[1] = ((-11059 * r - 21709 * g + 32768 * b + chroma_round) >> 16) - 128;
    comp[2] = ((32768 * r - 27439 * g - 5329 * b + chroma_round) >> 16) - 128;

    int crow[8], ccol[8];                                       // COS[lane & 7][.] for the row pass, COS[lane >> 3][.] for the column pass
#pragma unroll
    for (int k = 0; k < 8; ++k) { crow[k] = JPEG_TABLES.cos[8 * (lane & 7) + k]; ccol[k] = JPEG_TABLES.cos[8 * (lane >> 3) + k]; }
    const int zz = JPEG_TABLES.zigzag[lane];
    __syncthreads();

    // ---- DCT, quantisation, zigzag: coef[c] = coefficient ``lane`` (zigzag) of the MCU's block of component c
    int coef[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int acc = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x) acc += crow[x] * __shfl(comp[c], (lane & 56) | x, 64);         // t[y][u], lane = 8y + u
        const int t = (acc + 512) >> 10;
        acc = 0;
#pragma unroll
        for (int y = 0; y < 8; ++y) acc += ccol[y] * __shfl(t, 8 * y + (lane & 7), 64);             // F[v][u], lane = 8v + u
        const int f = __shfl(acc, zz, 64);
        const uint32_t q = s_q[c ? 1 : 0][lane];
        const int mag = (int)(((uint32_t)(f < 0 ? -f : f) + (q << 15)) / (q << 16));
        coef[c] = f < 0 ? -mag : mag;
        if (lane == 0) s_pred[c][wave] = coef[c];
    }
    __syncthreads();

    // ---- every lane's bits: the DC difference (lane 0), a non-zero AC coefficient behind its zero run, EOB (lane 63 when it is zero)
    unsigned long long bits[3];
    uint32_t nbits[3], before[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t* ac = s_ac[c ? 1 : 0];
        const int v = coef[c];
        const unsigned long long nonzero = __ballot(v != 0) | 1ull;           // (position 0 bounds the first run whatever the DC is)
        unsigned long long bv = 0;
        uint32_t n = 0, low;
        if (lane == 0) {
            const uint32_t size = category(v - (wave > 0 ? s_pred[c][wave - 1] : 0), &low), e = s_dc[c ? 1 : 0][size];
            bv = ((unsigned long long)(e & 0xFFFFu) << size) | low;
            n = (e >> 16) + size;
        } else if (v != 0) {
            const uint32_t run = (uint32_t)lane - (63u - (uint32_t)__clzll((long long)(nonzero & ((1ull << lane) - 1ull)))) - 1u;
            const uint32_t size = category(v, &low), e = ac[((run & 15u) << 4) | size], zrl = ac[0xF0];
            for (uint32_t k = 0; k < (run >> 4); ++k) { bv = (bv << (zrl >> 16)) | (zrl & 0xFFFFu); n += zrl >> 16; }
            bv = (((bv << (e >> 16)) | (e & 0xFFFFu)) << size) | low;
            n += (e >> 16) + size;
        } else if (lane == 63) {
            bv = ac[0] & 0xFFFFu;
            n = ac[0] >> 16;
        }
        n = live ? n : 0u;
        const uint32_t incl = wave_scan(n);
        bits[c] = bv; nbits[c] = n; before[c] = incl - n;
        if (lane == 63) s_tot[3 * wave + c] = incl;
    }
    __syncthreads();
    const uint32_t blocks_incl = wave_scan(s_tot[lane]);         // (entries past the interval's blocks are zero)
    const uint32_t total_bits = __shfl(blocks_incl, 63, 64);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t base = __shfl(blocks_incl - s_tot[lane], 3 * wave + c, 64);
        if (nbits[c]) or_bits(s_bits, base + before[c], bits[c], nbits[c]);
    }
    if (tid == 0 && (total_bits & 7u)) {                         // pad to a byte with 1-bits
        const uint32_t pad = 8u - (total_bits & 7u);
        atomicOr(&s_bits[total_bits >> 5], ((1u << pad) - 1u) << (32u - (total_bits & 31u) - pad));
    }
    __syncthreads();

    // ---- bytes: each lane a stretch, 0x00 behind every 0xFF, RSTm behind all intervals but the last
    const uint32_t nbytes = (total_bits + 7u) >> 3, per = (nbytes + JPEG_THREADS - 1) / JPEG_THREADS;
    const uint32_t b0 = (uint32_t)tid * per < nbytes ? (uint32_t)tid * per : nbytes, b1 = b0 + per < nbytes ? b0 + per : nbytes;
    uint32_t ff = 0;
    for (uint32_t i = b0; i < b1; ++i) ff += ((s_bits[i >> 2] >> (24u - 8u * (i & 3u))) & 255u) == 255u ? 1u : 0u;
    uint32_t ff_total = 0;
    uint32_t at = b0 + block_scan<JPEG_RESTART_MCUS>(ff, s_part, &ff_total);
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
    uint32_t* slot = reinterpret_cast<uint32_t*>(slots + (size_t)interval * JPEG_SLOT);      // (slots and JPEG_SLOT are 16-byte aligned)
    const uint32_t* out_words = reinterpret_cast<const uint32_t*>(s_out);
    for (uint32_t i = tid; i < (size + 3u) / 4u; i += JPEG_THREADS) slot[i] = out_words[i];
    if (tid == 0) meta[interval] = size;
}

__global__ void __launch_bounds__(JPEG_COPY_THREADS) k_jpeg_finish(int h, int w, JpegQuant quant, uint32_t* meta, uint32_t nint, uint8_t* out,
                                                                    int32_t* out_len) {
    __shared__ uint32_t s_part[JPEG_COPY_THREADS / 64];
    const int tid = threadIdx.x;
    uint32_t offset = JPEG_HEADER_BYTES;
    for (uint32_t i0 = 0; i0 < nint; i0 += JPEG_COPY_THREADS) {
        const uint32_t i = i0 + tid;
        uint32_t sum = 0;
        const uint32_t before = block_scan<JPEG_COPY_THREADS / 64>(i < nint ? meta[i] : 0u, s_part, &sum);
        if (i < nint) meta[(size_t)nint + i] = offset + before;
        offset += sum;
    }
    for (int i = tid; i < JPEG_HEADER_BYTES; i += JPEG_COPY_THREADS) {
        uint32_t v = JPEG_HEADER.b[i];
        if (i >= JPEG_Q0_AT && i < JPEG_Q0_AT + 64) v = quant.q[0][i - JPEG_Q0_AT];
        if (i >= JPEG_Q1_AT && i < JPEG_Q1_AT + 64) v = quant.q[1][i - JPEG_Q1_AT];
        if (i >= JPEG_DIM_AT && i < JPEG_DIM_AT + 4) v = ((i < JPEG_DIM_AT + 2 ? h : w) >> (8 * ((JPEG_DIM_AT + 1 - i) & 1))) & 255;
        out[i] = (uint8_t)v;
    }
    if (tid == 0) {
        out[offset] = 0xFF; out[offset + 1u] = 0xD9;             // EOI
        *out_len = (int32_t)(offset + 2u);
    }
}

__global__ void __launch_bounds__(JPEG_COPY_THREADS) k_jpeg_gather(const uint8_t* slots, const uint32_t* meta, uint32_t nint, uint8_t* out) {
    const uint32_t interval = blockIdx.x, tid = threadIdx.x;
    const uint8_t* src = slots + (size_t)interval * JPEG_SLOT;
    const uint32_t n = meta[interval];
    uint8_t* dst = out + meta[(size_t)nint + interval];
    // bytes up to the destination's dword boundary, dwords funnelled from two aligned source dwords, bytes at the end (as k_png_gather)
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

using namespace frcnn;

extern "C" int frcnn_jpeg_version(void) { return FRCNN_JPEG_VERSION; }

extern "C" int frcnn_jpeg_restart_mcus(void) { return JPEG_RESTART_MCUS; }

extern "C" size_t frcnn_jpeg_header_bytes(void) { return JPEG_HEADER_BYTES; }

extern "C" size_t frcnn_jpeg_bound(int h, int w) { return (size_t)jpeg_bound(h, w); }

extern "C" size_t frcnn_jpeg_workspace_bytes(int h, int w) {
    if (!jpeg_bound(h, w)) return 0;
    return (size_t)(jpeg_meta_bytes(h, w) + jpeg_intervals(h, w) * JPEG_SLOT);
}

extern "C" int frcnn_jpeg_encode_u8(const uint8_t* frame, int h, int w, int bgr, int quality, uint8_t* out, size_t out_capacity,
                                    int32_t* out_len, void* workspace, void* stream) {
    if (h < 1 || w < 1) return fail(FRCNN_E_UNSUPPORTED, "jpeg_encode_u8: frame %dx%d: both sides must be at least 1", h, w);
    if (h > 65535 || w > 65535) return fail(FRCNN_E_UNSUPPORTED, "jpeg_encode_u8: frame %dx%d: a JPEG side is at most 65535", h, w);
    const size_t bound = frcnn_jpeg_bound(h, w);
    if (!bound) return fail(FRCNN_E_UNSUPPORTED, "jpeg_encode_u8: frame %dx%d: the largest file would pass 2 GiB", h, w);
    if (quality < 1 || quality > 100) return fail(FRCNN_E_ARG, "jpeg_encode_u8: quality=%d outside 1..100", quality);
    if (!frame || !out || !out_len || !workspace) return fail(FRCNN_E_ARG, "jpeg_encode_u8: null pointer");
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return fail(FRCNN_E_ARG, "jpeg_encode_u8: workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(out_len) & 3u) return fail(FRCNN_E_ARG, "jpeg_encode_u8: out_len must be 4-byte aligned");
    if (out_capacity < bound)
        return fail(FRCNN_E_ARG, "jpeg_encode_u8: out_capacity=%zu below frcnn_jpeg_bound(%d, %d)=%zu", out_capacity, h, w, bound);
    // the IJG quality rule over Annex K.1 / K.2, in zigzag order as the DQT segments hold them
    JpegQuant quant;
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        const int l = (K1_LUMA[ZIGZAG[i]] * scale + 50) / 100, c = (K2_CHROMA[ZIGZAG[i]] * scale + 50) / 100;
        quant.q[0][i] = (uint8_t)(l < 1 ? 1 : (l > 255 ? 255 : l));
        quant.q[1][i] = (uint8_t)(c < 1 ? 1 : (c > 255 ? 255 : c));
    }
    const uint32_t nint = (uint32_t)jpeg_intervals(h, w);
    uint32_t* meta = static_cast<uint32_t*>(workspace);
    uint8_t* slots = static_cast<uint8_t*>(workspace) + jpeg_meta_bytes(h, w);
    hipStream_t s = as_stream(stream);
    k_jpeg_interval<<<nint, JPEG_THREADS, 0, s>>>(frame, h, w, bgr ? 1 : 0, quant, slots, meta, nint);
    k_jpeg_finish<<<1, JPEG_COPY_THREADS, 0, s>>>(h, w, quant, meta, nint, out, out_len);
    k_jpeg_gather<<<nint, JPEG_COPY_THREADS, 0, s>>>(slots, meta, nint, out);
    return check_launch("jpeg_encode_u8");
}
