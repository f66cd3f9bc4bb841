// What the device JPEG decoder's translation units share (jpeg_dec.hip: baseline files, include/ext/frcnn_hip_jpeg_dec.h and its batch
// header; jpeg_dec_full.hip: progressive files, include/ext/frcnn_hip_jpeg_dec_full.h): the workspace layout, the subsequence cut, the
// Huffman tables in LDS, the byte-stuffing / RSTm window of the entropy walk, and the whole back half behind the coefficients: the DC
// sums, the ISLOW IDCT, the fancy chroma upsampling and the colour conversion.  The __global__ kernels stay with their translation
// unit (they differ in the item they read); the __device__ bodies here are what both run.  Everything sits in an unnamed namespace:
// each translation unit has its own copy, __constant__ data included.
#pragma once
#include "common.h"
#include "ycc_common.h"
#include "../../include/ext/frcnn_hip_jpeg_dec.h"

namespace frcnn {
namespace {

constexpr int DEC_MAX_LANES = 1024;
constexpr uint32_t DEC_MIN_S = 32;
constexpr uint32_t DEC_MAX_SCAN = FRCNN_JPEG_DEC_MAX_SCAN;    // (see the header: what bounds the entropy kernel's worst case)
constexpr int DEC_LOOK = 9;
constexpr int DEC_IDCT_THREADS = 256, DEC_IDCT_BLOCKS = DEC_IDCT_THREADS / 8;
constexpr int DEC_COLOUR_THREADS = 256;
constexpr int DEC_DC_THREADS = 1024;

using Plan = frcnn_jpeg_dec_plan_t;

struct DecZigzag { uint8_t at[64]; };
// zigzag position -> natural index 8 * v + u
__constant__ DecZigzag DEC_ZIGZAG = {{0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                      35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}};

// ------------------------------------------------------------------------------------------------------------------- host sizes
struct DecPlanes { uint8_t* p[3]; int pw[3]; };
struct DecLayout { size_t coef, flags, plane[3], total; int pw[3], ph[3]; };

// (also on the device: a batched kernel finds its item's arrays from the plan it reads)
__host__ __device__ inline DecLayout dec_layout(const Plan& p) {
    DecLayout l = {};
    size_t at = 0;
    l.coef = at; at += align16((size_t)p.expected_blocks * 128);
    l.flags = at; at += align16((size_t)p.expected_blocks);
#pragma unroll
    for (int c = 0; c < 3; ++c) {                               // (constant indices: the device keeps the struct in registers)
        if (c >= p.components) continue;
        l.pw[c] = p.mcus_x * 8 * (c ? 1 : p.hs);
        l.ph[c] = p.mcus_y * 8 * (c ? 1 : p.vs);
        l.plane[c] = at; at += align16((size_t)l.pw[c] * (size_t)l.ph[c]);
    }
    l.total = at;
    return l;
}

inline void dec_subsequences(uint32_t scan_len, uint32_t* S, uint32_t* N) {
    uint32_t s = ((scan_len + DEC_MAX_LANES - 1) / DEC_MAX_LANES + 3) / 4 * 4;
    s = s < DEC_MIN_S ? DEC_MIN_S : s;
    const uint32_t n = (scan_len + s - 1) / s;
    *S = s;
    *N = n < 1 ? 1 : n;
}

// ------------------------------------------------------------------------------------------------------- the Huffman tables in LDS
struct HuffLds {
    uint16_t look[4][1 << DEC_LOOK];    // [slot] (baseline: class * 2 + id)
    uint8_t vals[4][256];
    uint8_t bits[4][16];
    int maxcode[4][17], delta[4][17];   // per length 1..16: the largest code (-1: none), symbol index = code + delta
    int count[4];
};

// Four tables by the whole workgroup (uniform: barriers inside; the caller's writes in front of the call are behind the first of them).
// off[t]: BITS (16 bytes) with HUFFVAL behind them, bytes into ``file``, 0 = no table in slot t; n[t]: its symbols (<= 256).  BITS and
// HUFFVAL from the file, maxcode / delta per length (one lane per table), then the lookahead table: one lane per symbol finds its code
// and fills the 2^(9 - length) entries that start with it.
__device__ __forceinline__ void dec_huff_build(HuffLds& h, const uint8_t* file, const uint32_t (&off)[4], const uint32_t (&n)[4]) {
    const uint32_t tid = threadIdx.x, threads = blockDim.x;
    for (uint32_t x = tid; x < 4u << DEC_LOOK; x += threads) h.look[x >> DEC_LOOK][x & ((1u << DEC_LOOK) - 1u)] = 0;
    for (uint32_t x = tid; x < 4u * 256u; x += threads) {
        const uint32_t t = x >> 8, j = x & 255u;
        const uint32_t o = t == 0 ? off[0] : (t == 1 ? off[1] : (t == 2 ? off[2] : off[3]));
        const uint32_t cnt = o ? (t == 0 ? n[0] : (t == 1 ? n[1] : (t == 2 ? n[2] : n[3]))) : 0u;
        h.vals[t][j] = j < cnt ? file[o + 16u + j] : (uint8_t)0;
        if (j < 16u) h.bits[t][j] = o ? file[o + j] : (uint8_t)0;
    }
    __syncthreads();
    if (tid < 4u) {
        int code = 0, k = 0;
        const uint32_t o = tid == 0 ? off[0] : (tid == 1 ? off[1] : (tid == 2 ? off[2] : off[3]));
        const uint32_t cnt = tid == 0 ? n[0] : (tid == 1 ? n[1] : (tid == 2 ? n[2] : n[3]));
        h.count[tid] = o ? (int)cnt : 0;
        for (int l = 1; l <= 16; ++l) {
            const int nb = h.bits[tid][l - 1];
            h.maxcode[tid][l] = -1;
            h.delta[tid][l] = 0;
            if (nb) {
                h.delta[tid][l] = k - code;
                code += nb; k += nb;
                h.maxcode[tid][l] = code - 1;
            }
            code <<= 1;
        }
    }
    __syncthreads();
    for (uint32_t x = tid; x < 4u * 256u; x += threads) {
        const uint32_t t = x >> 8;
        const int j = (int)(x & 255u);
        if (j >= h.count[t]) continue;
        int k = 0;
        for (int l = 1; l <= DEC_LOOK; ++l) {
            const int nb = h.bits[t][l - 1];
            if (j < k + nb) {
                const int code = j - h.delta[t][l];
                if (code >= 0 && code < (1 << l)) {
                    const uint16_t e = (uint16_t)((l << 8) | h.vals[t][j]);
                    const int first = code << (DEC_LOOK - l);
                    for (int i = 0; i < (1 << (DEC_LOOK - l)); ++i) h.look[t][first + i] = e;
                }
                break;
            }
            k += nb;
        }
    }
    __syncthreads();
}

// The code at the top of a 16-bit window, from table ``slot`` -> its length; *sym its symbol (0 with a flag), *flag 0 or what is wrong
// (``st_code``: no such code, ``st_table``: a symbol index outside the table).
__device__ __forceinline__ uint32_t dec_huff_code(const HuffLds& h, int slot, uint32_t top, uint32_t st_code, uint32_t st_table, uint32_t* sym, uint32_t* flag) {
    uint32_t length;
    *sym = 0; *flag = 0;
    const uint32_t e = h.look[slot][top >> (16 - DEC_LOOK)];
    if (e) {
        length = e >> 8; *sym = e & 255u;
    } else {
        length = 16; *flag = st_code;
        for (int l = 1; l <= 16; ++l) {
            const int code = (int)(top >> (16 - l));
            if (code <= h.maxcode[slot][l]) {
                const int k = code + h.delta[slot][l];
                length = (uint32_t)l;
                if (k >= 0 && k < h.count[slot]) { *sym = h.vals[slot][k]; *flag = 0; } else *flag = st_table;
                break;
            }
        }
    }
    return length;
}

// ---------------------------------------------------------------------------------------------- the entropy-coded segment's bytes
// every byte of a segment is read through this: zero past its end
__device__ __forceinline__ uint32_t dec_rd(const uint8_t* scan, uint32_t len, uint32_t r) { return r < len ? (uint32_t)scan[r] : 0u; }

// The window at bit ``pos`` of the raw segment: five data bytes from byte pos >> 3 on (``w``, 40 bits), the raw index of each; behind
// a 0xFF byte a 0x00 is skipped; 0xFF followed by RSTm is a marker: it and everything behind it read as zero, ``mbit`` is the bit of
// the window at which it stands (-1: none) and ``mraw`` its raw index; ``ebit``: the bit of the window at which the segment ends (-1:
// not within it).
struct DecWindow { unsigned long long w; uint32_t idx[5], mraw; int mbit, ebit; };

__device__ __forceinline__ DecWindow dec_window(const uint8_t* scan, uint32_t len, uint32_t pos) {
    DecWindow d;
    uint32_t r = pos >> 3;
    d.mraw = 0; d.mbit = -1; d.ebit = -1; d.w = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        d.idx[j] = r;
        if (r >= len && d.ebit < 0 && d.mbit < 0) d.ebit = 8 * j;
        uint32_t v = dec_rd(scan, len, r);
        if (d.mbit >= 0) {
            v = 0;
        } else if (v == 0xFFu) {
            const uint32_t nxt = dec_rd(scan, len, r + 1u);
            if (nxt == 0u) r += 1u;
            else if ((nxt & 0xF8u) == 0xD0u) { d.mbit = 8 * j; d.mraw = r; v = 0; }
        }
        d.w = (d.w << 8) | v;
        if (d.mbit < 0) r += 1u;
    }
    return d;
}

// the bit position ``q`` bits (o + n <= 7 + 32: at most byte 4) into the window that starts at bit 0 of byte idx[0]
__device__ __forceinline__ uint32_t dec_window_pos(const DecWindow& d, uint32_t q) {
    const uint32_t at = q >> 3;
    uint32_t ri = d.idx[0];
#pragma unroll
    for (int j = 1; j < 5; ++j) ri = at == (uint32_t)j ? d.idx[j] : ri;
    return ri * 8u + (q & 7u);
}

// inclusive sum over the wave
__device__ __forceinline__ uint32_t dec_wave_scan(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// --------------------------------------------------------------------------------------------------------------------- the DC sums
// One workgroup of DEC_DC_THREADS per component.  Its ``n`` blocks in coding order (``block_of``: the t-th of them -> its index in the
// coefficient array), a stretch per lane: (cut seen, sum since the cut or the stretch's start) folded per stretch, scanned across the
// lanes (Hillis-Steele in LDS: ``s_sum`` and ``s_cut``, DEC_DC_THREADS words each, the caller's), then each stretch written with the
// sum that flows into it.
template <class BlockOf>
__device__ __forceinline__ void dec_dc_sum(uint32_t n, BlockOf block_of, int16_t* coef, const uint8_t* flags, int* s_sum, uint32_t* s_cut) {
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (n + DEC_DC_THREADS - 1) / DEC_DC_THREADS;
    const uint32_t t0 = tid * per < n ? tid * per : n, t1 = t0 + per < n ? t0 + per : n;
    int sum = 0;
    uint32_t cut = 0;
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t k = block_of(t);
        const int d = coef[(size_t)k * 64];
        if (flags[k]) { sum = d; cut = 1; } else sum += d;
    }
    s_sum[tid] = sum;
    s_cut[tid] = cut;
    __syncthreads();
    for (uint32_t d = 1; d < (uint32_t)DEC_DC_THREADS; d <<= 1) {
        int ps = 0;
        uint32_t pc = 0;
        if (tid >= d) { ps = s_sum[tid - d]; pc = s_cut[tid - d]; }
        __syncthreads();
        if (tid >= d) {
            if (!s_cut[tid]) s_sum[tid] += ps;
            s_cut[tid] |= pc;
        }
        __syncthreads();
    }
    int running = tid ? s_sum[tid - 1u] : 0;
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t k = block_of(t);
        const int d = coef[(size_t)k * 64];
        running = flags[k] ? d : running + d;
        coef[(size_t)k * 64] = (int16_t)running;
    }
}

// component ``comp`` of a frame whose blocks were coded in MCU order (one interleaved scan)
__device__ __forceinline__ void dec_dc_body(const Plan& plan, uint32_t comp, int16_t* coef, const uint8_t* flags) {
    __shared__ int s_sum[DEC_DC_THREADS];
    __shared__ uint32_t s_cut[DEC_DC_THREADS];
    const uint32_t bpm = (uint32_t)plan.blocks_per_mcu, luma = plan.components == 3 ? (uint32_t)(plan.hs * plan.vs) : 1u;
    const uint32_t mcus = (uint32_t)plan.mcus_x * (uint32_t)plan.mcus_y;
    const uint32_t n = comp == 0 ? mcus * luma : mcus;          // blocks of this component
    dec_dc_sum(n, [&](uint32_t t) { return comp == 0 ? (t / luma) * bpm + t % luma : t * bpm + luma + comp - 1u; }, coef, flags, s_sum, s_cut);
}

// ---------------------------------------------------------------------------------------------------------------------- the IDCT
// jidctint's 8-point pass (CONST_BITS 13): x in, the eight outputs descaled by SHIFT.  The sums are formed in uint32_t: the same bits as
// int for every sound file (|sum| < 2^31), and a defined wrap instead of a signed overflow for the coefficients of a damaged one.
template <int SHIFT>
__device__ __forceinline__ void idct_1d(const int (&xi)[8], int (&y)[8]) {
    using U = uint32_t;
    U x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = (U)xi[k];
    constexpr U N_0_899 = (U)-7373, N_2_562 = (U)-20995, N_1_961 = (U)-16069, N_0_390 = (U)-3196;
    U z1 = (x[2] + x[6]) * 4433u;
    const U tmp2 = z1 - x[6] * 15137u, tmp3 = z1 + x[2] * 6270u;
    const U tmp0 = (x[0] + x[4]) * 8192u, tmp1 = (x[0] - x[4]) * 8192u;
    const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    U t0 = x[7], t1 = x[5], t2 = x[3], t3 = x[1];
    z1 = t0 + t3;
    U z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const U z5 = (z3 + z4) * 9633u;
    t0 *= 2446u; t1 *= 16819u; t2 *= 25172u; t3 *= 12299u;
    z1 *= N_0_899; z2 *= N_2_562; z3 = z3 * N_1_961 + z5; z4 = z4 * N_0_390 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    constexpr U HALF = 1u << (SHIFT - 1);
    y[0] = (int)(tmp10 + t3 + HALF) >> SHIFT; y[7] = (int)(tmp10 - t3 + HALF) >> SHIFT;
    y[1] = (int)(tmp11 + t2 + HALF) >> SHIFT; y[6] = (int)(tmp11 - t2 + HALF) >> SHIFT;
    y[2] = (int)(tmp12 + t1 + HALF) >> SHIFT; y[5] = (int)(tmp12 - t1 + HALF) >> SHIFT;
    y[3] = (int)(tmp13 + t0 + HALF) >> SHIFT; y[4] = (int)(tmp13 - t0 + HALF) >> SHIFT;
}

// Eight lanes per block: lane = column in the first pass, row in the second; the 8x8 intermediate through LDS (row stride 9).
__device__ __forceinline__ void dec_idct_body(const uint8_t* file, const Plan& plan, const int16_t* coef, const DecPlanes planes, uint32_t group) {
    __shared__ int s_ws[DEC_IDCT_BLOCKS][72];
    __shared__ uint16_t s_q[3][64];                             // natural order
    const uint32_t tid = threadIdx.x, sub = tid >> 3, lane = tid & 7u;
    for (uint32_t x = tid; x < (uint32_t)plan.components * 64u; x += DEC_IDCT_THREADS)
        s_q[x >> 6][DEC_ZIGZAG.at[x & 63u]] = file[plan.dqt_off[x >> 6] + (x & 63u)];
    __syncthreads();
    const unsigned long long blk = (unsigned long long)group * DEC_IDCT_BLOCKS + sub;
    const bool live = blk < plan.expected_blocks;
    const uint32_t bpm = (uint32_t)plan.blocks_per_mcu, luma = plan.components == 3 ? (uint32_t)(plan.hs * plan.vs) : 1u;
    const uint32_t m = live ? (uint32_t)(blk / bpm) : 0u, b = live ? (uint32_t)(blk % bpm) : 0u;
    const uint32_t comp = b < luma ? 0u : b - luma + 1u;
    if (live) {
        const int16_t* src = coef + (size_t)blk * 64;
        int x[8], y[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) x[r] = (int)src[8 * r + lane] * (int)s_q[comp][8 * r + lane];
        idct_1d<11>(x, y);
#pragma unroll
        for (int r = 0; r < 8; ++r) s_ws[sub][9 * r + lane] = y[r];
    }
    __syncthreads();
    if (live) {
        int x[8], y[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = s_ws[sub][9 * lane + k];
        idct_1d<18>(x, y);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int v = y[k] + 128;
            const uint32_t u = (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
            if (k < 4) lo |= u << (8 * k); else hi |= u << (8 * (k - 4));
        }
        const uint32_t my = m / (uint32_t)plan.mcus_x, mx = m - my * (uint32_t)plan.mcus_x;
        const uint32_t by = comp == 0 ? my * (uint32_t)plan.vs + b / (uint32_t)plan.hs : my;
        const uint32_t bx = comp == 0 ? mx * (uint32_t)plan.hs + b % (uint32_t)plan.hs : mx;
        uint8_t* plane = comp == 0 ? planes.p[0] : (comp == 1 ? planes.p[1] : planes.p[2]);
        const int pw = comp == 0 ? planes.pw[0] : (comp == 1 ? planes.pw[1] : planes.pw[2]);
        uint32_t* dst = reinterpret_cast<uint32_t*>(plane + ((size_t)by * 8 + lane) * (size_t)pw + (size_t)bx * 8);
        dst[0] = lo;                                            // (planes are 16-byte aligned, their widths multiples of 8)
        dst[1] = hi;
    }
}

// ------------------------------------------------------------------------------------------------------------ upsampling, colour
// a chroma sample at full size: libjpeg's fancy upsampling (ycc_common.h); a plane of width <= 2 is replicated
__device__ __forceinline__ int dec_chroma(const uint8_t* plane, int pw, const Plan& plan, int x, int y) {
    if (plan.hs == 1) return plane[(size_t)y * pw + x];
    const int n = (plan.w + 1) >> 1, i = x >> 1;
    if (plan.vs == 1) {
        const uint8_t* s = plane + (size_t)y * pw;
        return n <= 2 ? s[i] : fancy_h2v1(s, n, x);
    }
    const uint8_t* near = plane + (size_t)(y >> 1) * pw;
    if (n <= 2) return near[i];
    return fancy_h2v2(near, plane + (size_t)fancy_far_row(y, (plan.h + 1) >> 1) * pw, n, x);
}

__device__ __forceinline__ void dec_colour_body(const Plan& plan, const DecPlanes planes, int bgr, uint8_t* out, int x, int y) {
    if (x >= plan.w || y >= plan.h) return;
    const int lum = planes.p[0][(size_t)y * planes.pw[0] + x];
    int r = lum, g = lum, b = lum;
    if (plan.components == 3) {
        const int cb = dec_chroma(planes.p[1], planes.pw[1], plan, x, y) - 128, cr = dec_chroma(planes.p[2], planes.pw[2], plan, x, y) - 128;
        jfif_ycc_to_rgb(lum, cb, cr, &r, &g, &b);
    }
    uint8_t* p = out + ((size_t)y * (size_t)plan.w + (size_t)x) * 3;
    p[0] = (uint8_t)(bgr ? b : r);
    p[1] = (uint8_t)g;
    p[2] = (uint8_t)(bgr ? r : b);
}

}  // namespace
}  // namespace frcnn
