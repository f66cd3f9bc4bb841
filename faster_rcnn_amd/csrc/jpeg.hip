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
#include "jpeg_common.h"

namespace frcnn {
namespace {


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
    int comp[3];
    jfif_rgb_to_ycc(r, g, b, &comp[0], &comp[1], &comp[2]);     // (ycc_common.h)
    comp[0] -= 128; comp[1] -= 128; comp[2] -= 128;

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
    gather_interval(src, n, dst, tid);
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
    const JpegQuant quant = jpeg_quant(quality);
    const uint32_t nint = (uint32_t)jpeg_intervals(h, w);
    uint32_t* meta = static_cast<uint32_t*>(workspace);
    uint8_t* slots = static_cast<uint8_t*>(workspace) + jpeg_meta_bytes(h, w);
    hipStream_t s = as_stream(stream);
    k_jpeg_interval<<<nint, JPEG_THREADS, 0, s>>>(frame, h, w, bgr ? 1 : 0, quant, slots, meta, nint);
    k_jpeg_finish<<<1, JPEG_COPY_THREADS, 0, s>>>(h, w, quant, meta, nint, out, out_len);
    k_jpeg_gather<<<nint, JPEG_COPY_THREADS, 0, s>>>(slots, meta, nint, out);
    return check_launch("jpeg_encode_u8");
}
