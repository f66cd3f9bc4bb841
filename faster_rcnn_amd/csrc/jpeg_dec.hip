// JPEG files decoded on the device (include/ext/frcnn_hip_jpeg_dec.h): the bytes of a baseline .jpg file in device memory -> an (h, w, 3)
// uint8 frame, the counterpart of the encoder (jpeg.hip).  Four launches that allocate nothing, synchronise nothing and read nothing on
// the host; the plan (the host's marker parse, frcnn_jpeg_dec_plan) travels BY VALUE.  gfx950 (CDNA4) only, wave64 throughout.  Integer
// arithmetic throughout: the frame is a function of the file alone, tests/jpeg_dec_ref.py states the same rules in Python, and the two
// agree byte for byte (and with libjpeg's default decoder: ISLOW IDCT, fancy upsampling).
//
//   k_jpeg_dec_entropy  ONE workgroup per file, one lane per subsequence of S raw bytes.  The four Huffman tables are built in LDS from
//                       the DHT payloads in the file: a lookahead table over 9 bits (length << 8 | symbol) and maxcode / delta per
//                       length for the longer codes.  A decoder state is (bit of the raw segment, block within the MCU, zigzag index,
//                       restart pending).  Lane i guesses that a symbol starts at its first bit, decodes to the end of its stretch and
//                       hands its exit state to lane i + 1; every lane whose entry state changed decodes again; the loop ends when no
//                       entry changed (a workgroup-wide flag) and after N rounds at the latest, since round r fixes entry r for good.
//                       Then an exclusive scan of the blocks each lane completed and a last walk that writes the coefficients (natural
//                       order, int16, DC as differences, zeros where the stream skips) and a restart flag per block.
//   k_jpeg_dec_dc       one workgroup per component: the DC differences summed along the component's blocks, cut at the restart flags.
//   k_jpeg_dec_idct     dequantise + jidctint's ISLOW passes, a lane per column, then per row, through LDS; 32 blocks per workgroup; the
//                       samples go to component planes at padded size.
//   k_jpeg_dec_colour   a lane per pixel: the triangle-filter chroma upsampling (h2v1, h2v2) from real rows and columns only, the
//                       colour conversion with 16 fractional bits, three bytes out.
//
// Bounds.  Every byte of the segment is read through rd() (zero past its end); a block index is checked against the plan's total before
// a coefficient is written; a zigzag index never passes 63; table indices are checked; the planes hold whole MCUs.  So a damaged scan
// yields a status word, not a fault.  One workgroup per file leaves the entropy stage on ONE CU: it is the batch that fills the chip.
//
// The batched form (include/ext/frcnn_hip_jpeg_dec_batch.h): k_jpeg_dec_*_batch run the SAME __device__ bodies for n files in one launch
// each.  A table of items (plan + where the file, the frame and the workspace region lie) in device memory replaces the by-value plan;
// a workgroup finds its item from its grid index and returns as a whole where the grid, sized by the batch's largest item, reaches past
// its own.  Every bound above holds per item: its status word, its workspace region, its output range.
#include "common.h"
#include "../../include/ext/frcnn_hip_jpeg_dec.h"
#include "../../include/ext/frcnn_hip_jpeg_dec_batch.h"

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
using Item = frcnn_jpeg_dec_batch_item_t;

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

// nullptr when the plan's fields agree with each other (what the kernels' bounds rest on), else what is wrong
inline const char* dec_plan_fault(const Plan& p) {
    if (p.h < 1 || p.w < 1 || p.h > 65535 || p.w > 65535) return "sides outside 1..65535";
    if (p.components != 1 && p.components != 3) return "components";
    if (!((p.hs == 1 && p.vs == 1) || (p.components == 3 && p.hs == 2 && (p.vs == 1 || p.vs == 2)))) return "sampling factors";
    if (p.mcus_x != (p.w + 8 * p.hs - 1) / (8 * p.hs) || p.mcus_y != (p.h + 8 * p.vs - 1) / (8 * p.vs)) return "MCU counts";
    if (p.blocks_per_mcu != (p.components == 3 ? p.hs * p.vs + 2 : 1)) return "blocks per MCU";
    if ((unsigned long long)p.expected_blocks != (unsigned long long)p.mcus_x * p.mcus_y * p.blocks_per_mcu) return "block total";
    if (p.scan_len >= DEC_MAX_SCAN || p.scan_off > p.file_len || p.scan_len > p.file_len - p.scan_off) return "scan outside the file";
    if (p.subsequence_bytes < DEC_MIN_S || p.subsequence_bytes % 4 || p.subsequences < 1 || p.subsequences > (uint32_t)DEC_MAX_LANES ||
        (unsigned long long)p.subsequence_bytes * p.subsequences < p.scan_len) return "subsequences";
    for (int c = 0; c < p.components; ++c) {
        if (p.dqt_off[c] > p.file_len || 64 > p.file_len - p.dqt_off[c]) return "quantisation table outside the file";
        if (p.comp_dc[c] > 1 || p.comp_ac[c] > 1 || !p.dht_off[0][p.comp_dc[c]] || !p.dht_off[1][p.comp_ac[c]]) return "Huffman table ids";
    }
    for (int t = 0; t < 4; ++t) {
        const uint32_t off = p.dht_off[t >> 1][t & 1], n = p.dht_count[t >> 1][t & 1];
        if (off && (n > 256 || off > p.file_len || 16 + n > p.file_len - off)) return "Huffman table outside the file";
    }
    return nullptr;
}

// ------------------------------------------------------------------------------------------------------------- entropy decoding
constexpr uint32_t ST_BLOCKS = FRCNN_JPEG_DEC_BLOCKS, ST_ZIGZAG = FRCNN_JPEG_DEC_ZIGZAG, ST_CODE = FRCNN_JPEG_DEC_CODE, ST_TABLE = FRCNN_JPEG_DEC_TABLE;

struct HuffLds {
    uint16_t look[4][1 << DEC_LOOK];    // [class * 2 + id]
    uint8_t vals[4][256];
    uint8_t bits[4][16];
    int maxcode[4][17], delta[4][17];   // per length 1..16: the largest code (-1: none), symbol index = code + delta
    int count[4];
};

struct EntropyCtx {
    const uint8_t* scan;
    uint32_t len;                       // bytes of the segment
    const HuffLds* huff;
    int16_t* coef;
    uint8_t* flags;
    uint32_t nblk;
    int bpm, luma;
    uint32_t tables;                    // bit c: the DC table id of component c, bit 4 + c: its AC table id
};

// state word: zigzag index | block within the MCU << 8 | restart pending << 16
struct DecState { uint32_t pos, bz; };

__device__ __forceinline__ uint32_t rd(const EntropyCtx& c, uint32_t r) { return r < c.len ? (uint32_t)c.scan[r] : 0u; }

// F_i: whole symbols from ``st`` until the next would start at or past ``end`` (a bit position); -> blocks completed.  WRITE: the final
// walk, ``blk`` the index of the block the entry state stands in.
template <bool WRITE>
__device__ uint32_t dec_run(const EntropyCtx& c, uint32_t end, DecState& st, uint32_t blk, uint32_t* status) {
    uint32_t pos = st.pos, z = st.bz & 255u, b = (st.bz >> 8) & 255u, rst = (st.bz >> 16) & 1u, done = 0, flagged = 0;
    while (pos < end) {
        // ---- the window: five data bytes from byte pos >> 3 on, the raw index of each, the bit at which an RSTm marker stands
        uint32_t r = pos >> 3, idx[5], mraw = 0;
        int mbit = -1, ebit = -1;
        unsigned long long w = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            idx[j] = r;
            if (r >= c.len && ebit < 0 && mbit < 0) ebit = 8 * j;
            uint32_t v = rd(c, r);
            if (mbit >= 0) {
                v = 0;
            } else if (v == 0xFFu) {
                const uint32_t nxt = rd(c, r + 1u);
                if (nxt == 0u) r += 1u;
                else if ((nxt & 0xF8u) == 0xD0u) { mbit = 8 * j; mraw = r; v = 0; }
            }
            w = (w << 8) | v;
            if (mbit < 0) r += 1u;
        }
        const uint32_t o = pos & 7u;
        const int comp = (int)b < c.luma ? 0 : (int)b - c.luma + 1;
        const int slot = z == 0 ? (int)((c.tables >> comp) & 1u) : 2 + (int)((c.tables >> (4 + comp)) & 1u);
        // ---- the code
        const uint32_t top = (uint32_t)(w >> (24u - o)) & 0xFFFFu;
        uint32_t length, sym = 0, flag = 0;
        const uint32_t e = c.huff->look[slot][top >> (16 - DEC_LOOK)];
        if (e) {
            length = e >> 8; sym = e & 255u;
        } else {
            length = 16; flag = ST_CODE;
            for (int l = 1; l <= 16; ++l) {
                const int code = (int)(top >> (16 - l));
                if (code <= c.huff->maxcode[slot][l]) {
                    const int k = code + c.huff->delta[slot][l];
                    length = (uint32_t)l;
                    if (k >= 0 && k < c.huff->count[slot]) { sym = c.huff->vals[slot][k]; flag = 0; } else flag = ST_TABLE;
                    break;
                }
            }
        }
        const uint32_t size = sym & 15u;
        if ((z == 0 && sym > 11u) || (z > 0 && size > 10u)) flag |= ST_TABLE;
        const uint32_t n = length + size;
        if (mbit >= 0 && o + n > (uint32_t)mbit) {              // the symbol reaches into a restart marker: abandoned
            if (z > 0) {
                if (WRITE && blk < c.nblk)
                    for (uint32_t k = z; k < 64u; ++k) c.coef[(size_t)blk * 64 + DEC_ZIGZAG.at[k]] = 0;
                ++blk; ++done;
            }
            pos = (mraw + 2u) * 8u; b = 0; z = 0; rst = 1;
            continue;
        }
        if (ebit >= 0 && o + n > (uint32_t)ebit) {              // ... past the end of the segment (the last padding): abandoned, the end
            pos = pos > c.len * 8u ? pos : c.len * 8u;
            break;
        }
        flagged |= flag;
        int v = size ? (int)((uint32_t)(w >> (40u - o - n)) & ((1u << size) - 1u)) : 0;
        if (size && v < (1 << (size - 1))) v -= (1 << size) - 1;
        if (z == 0) {
            if (WRITE && blk < c.nblk) {
                c.coef[(size_t)blk * 64] = (int16_t)v;
                c.flags[blk] = (uint8_t)((b == 0 || (int)b >= c.luma) ? rst : 0u);
            }
            z = 1;
        } else {
            uint32_t run = sym >> 4, keep = 1;
            if (size == 0) { run = run == 15u ? 16u : 64u - z; keep = 0; }      // ZRL; EOB
            if (z + run + keep > 64u) { flagged |= ST_ZIGZAG; run = 64u - z; keep = 0; }
            if (WRITE && blk < c.nblk) {
                int16_t* dst = c.coef + (size_t)blk * 64;
                for (uint32_t k = z; k < z + run; ++k) dst[DEC_ZIGZAG.at[k]] = 0;
                if (keep) dst[DEC_ZIGZAG.at[z + run]] = (int16_t)v;
            }
            z += run + keep;
        }
        if (z >= 64u) {
            ++blk; ++done; z = 0;
            b = (int)b + 1 < c.bpm ? b + 1u : 0u;
            rst = b ? rst : 0u;
        }
        const uint32_t q = o + n, at = q >> 3;                  // (q <= 7 + 31: at <= 4)
        uint32_t ri = idx[0];
#pragma unroll
        for (int j = 1; j < 5; ++j) ri = at == (uint32_t)j ? idx[j] : ri;
        pos = ri * 8u + (q & 7u);
    }
    st.pos = pos;
    st.bz = z | (b << 8) | (rst << 16);
    if (WRITE) *status |= flagged;
    return done;
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

// The entropy stage of ONE file by the whole workgroup (blockDim.x a multiple of 64, >= plan.subsequences; lanes past the file's
// subsequences idle through every barrier: ``active`` is false for them, so they never change the round loop's flag).
__device__ __forceinline__ void dec_entropy_body(const uint8_t* file, const Plan& plan, int16_t* coef, uint8_t* flags, int32_t* status) {
    __shared__ HuffLds s_huff;
    __shared__ uint32_t s_xpos[DEC_MAX_LANES], s_xbz[DEC_MAX_LANES];
    __shared__ uint32_t s_part[DEC_MAX_LANES / 64];
    __shared__ uint32_t s_changed, s_status;
    const uint32_t tid = threadIdx.x, threads = blockDim.x;

    // ---- the Huffman tables: BITS and HUFFVAL from the file, maxcode / delta per length (one lane per table), then the lookahead
    // table: one lane per symbol finds its code and fills the 2^(9 - length) entries that start with it
    for (uint32_t x = tid; x < 4u << DEC_LOOK; x += threads) s_huff.look[x >> DEC_LOOK][x & ((1u << DEC_LOOK) - 1u)] = 0;
    for (uint32_t x = tid; x < 4u * 256u; x += threads) {
        const uint32_t t = x >> 8, j = x & 255u, off = plan.dht_off[t >> 1][t & 1], n = off ? plan.dht_count[t >> 1][t & 1] : 0u;
        s_huff.vals[t][j] = j < n ? file[off + 16u + j] : (uint8_t)0;
        if (j < 16u) s_huff.bits[t][j] = off ? file[off + j] : (uint8_t)0;
    }
    if (tid == 0) { s_changed = 0; s_status = 0; }
    __syncthreads();
    if (tid < 4u) {
        int code = 0, k = 0;
        s_huff.count[tid] = plan.dht_off[tid >> 1][tid & 1] ? (int)plan.dht_count[tid >> 1][tid & 1] : 0;
        for (int l = 1; l <= 16; ++l) {
            const int nb = s_huff.bits[tid][l - 1];
            s_huff.maxcode[tid][l] = -1;
            s_huff.delta[tid][l] = 0;
            if (nb) {
                s_huff.delta[tid][l] = k - code;
                code += nb; k += nb;
                s_huff.maxcode[tid][l] = code - 1;
            }
            code <<= 1;
        }
    }
    __syncthreads();
    for (uint32_t x = tid; x < 4u * 256u; x += threads) {
        const uint32_t t = x >> 8;
        const int j = (int)(x & 255u);
        if (j >= s_huff.count[t]) continue;
        int k = 0;
        for (int l = 1; l <= DEC_LOOK; ++l) {
            const int nb = s_huff.bits[t][l - 1];
            if (j < k + nb) {
                const int code = j - s_huff.delta[t][l];
                if (code >= 0 && code < (1 << l)) {
                    const uint16_t e = (uint16_t)((l << 8) | s_huff.vals[t][j]);
                    const int first = code << (DEC_LOOK - l);
                    for (int i = 0; i < (1 << (DEC_LOOK - l)); ++i) s_huff.look[t][first + i] = e;
                }
                break;
            }
            k += nb;
        }
    }
    __syncthreads();

    EntropyCtx c;
    c.scan = file + plan.scan_off;
    c.len = plan.scan_len;
    c.huff = &s_huff;
    c.coef = coef;
    c.flags = flags;
    c.nblk = plan.expected_blocks;
    c.bpm = plan.blocks_per_mcu;
    c.luma = plan.components == 3 ? plan.hs * plan.vs : 1;
    c.tables = 0;
    for (int k = 0; k < 3; ++k) c.tables |= (uint32_t)(plan.comp_dc[k] & 1) << k | (uint32_t)(plan.comp_ac[k] & 1) << (4 + k);

    // ---- rounds: exit[i] = F_i(entry[i]) for every lane whose entry changed, entry[i + 1] = exit[i], until nothing changes
    const uint32_t N = plan.subsequences, S = plan.subsequence_bytes;
    const bool active = tid < N;
    const uint32_t last = (tid + 1u) * S < c.len ? (tid + 1u) * S : c.len;
    const uint32_t end = last * 8u;
    DecState entry = {tid * S * 8u, 0u};
    uint32_t count = 0, unused = 0;
    bool changed = active;
    for (uint32_t round = 0; round < N; ++round) {
        if (changed) {
            DecState st = entry;
            count = dec_run<false>(c, end, st, 0u, &unused);
            s_xpos[tid] = st.pos;
            s_xbz[tid] = st.bz;
        }
        __syncthreads();
        changed = false;
        if (active && tid > 0u) {
            const uint32_t p = s_xpos[tid - 1u], bz = s_xbz[tid - 1u];
            if (p != entry.pos || bz != entry.bz) { entry.pos = p; entry.bz = bz; changed = true; }
        }
        if (changed) atomicOr(&s_changed, 1u);
        __syncthreads();
        const uint32_t any = s_changed;
        __syncthreads();
        if (!any) break;
        if (tid == 0) s_changed = 0;                           // (read again only behind the next round's barriers)
    }

    // ---- every lane's first block, the total, the final walk
    const uint32_t incl = dec_wave_scan(active ? count : 0u);
    if ((tid & 63u) == 63u) s_part[tid >> 6] = incl;
    __syncthreads();
    uint32_t before = incl - (active ? count : 0u), total = 0;
    for (uint32_t k = 0; k < (threads + 63u) / 64u; ++k) {
        const uint32_t p = s_part[k];
        total += p;
        if (k < (tid >> 6)) before += p;
    }
    uint32_t flagged = 0;
    if (active) {
        DecState st = entry;
        dec_run<true>(c, end, st, before, &flagged);
    }
    if (flagged) atomicOr(&s_status, flagged);
    __syncthreads();
    if (tid == 0) {
        const uint32_t s = s_status | (total != plan.expected_blocks ? ST_BLOCKS : 0u);
        if (s) *status = (int32_t)((uint32_t)*status | s);
    }
}

__global__ void __launch_bounds__(DEC_MAX_LANES) k_jpeg_dec_entropy(const uint8_t* file, Plan plan, int16_t* coef, uint8_t* flags, int32_t* status) {
    dec_entropy_body(file, plan, coef, flags, status);
}

// The batched kernels: grid index -> item.  The item lies in device memory at an address that is uniform over the workgroup and that
// nothing written here aliases (__restrict__): its fields are scalar loads, as the by-value plan's are from the kernel arguments.
struct DecItemArrays { const uint8_t* file; int16_t* coef; uint8_t* flags; DecPlanes planes; };

__device__ __forceinline__ DecItemArrays dec_item_arrays(const Item& it, const uint8_t* files, uint8_t* workspace) {
    const DecLayout l = dec_layout(it.plan);
    uint8_t* ws = workspace + it.ws_off;
    DecItemArrays a = {};
    a.file = files + it.file_off;
    a.coef = reinterpret_cast<int16_t*>(ws + l.coef);
    a.flags = ws + l.flags;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        if (c < it.plan.components) { a.planes.p[c] = ws + l.plane[c]; a.planes.pw[c] = l.pw[c]; }
    return a;
}

// grid.x = item; the block is the batch's largest ``subsequences`` rounded up to 64
__global__ void __launch_bounds__(DEC_MAX_LANES) k_jpeg_dec_entropy_batch(const uint8_t* files, const Item* __restrict__ items, uint8_t* workspace, int32_t* status) {
    const Item& it = items[blockIdx.x];
    const DecItemArrays a = dec_item_arrays(it, files, workspace);
    dec_entropy_body(a.file, it.plan, a.coef, a.flags, status + blockIdx.x);
}

// One workgroup per component.  Its blocks in coding order, a stretch per lane: (cut seen, sum since the cut or the stretch's start)
// folded per stretch, scanned across the lanes (Hillis-Steele in LDS), then each stretch written with the sum that flows into it.
__device__ __forceinline__ void dec_dc_body(const Plan& plan, uint32_t comp, int16_t* coef, const uint8_t* flags) {
    __shared__ int s_sum[DEC_DC_THREADS];
    __shared__ uint32_t s_cut[DEC_DC_THREADS];
    const uint32_t tid = threadIdx.x;
    const uint32_t bpm = (uint32_t)plan.blocks_per_mcu, luma = plan.components == 3 ? (uint32_t)(plan.hs * plan.vs) : 1u;
    const uint32_t mcus = (uint32_t)plan.mcus_x * (uint32_t)plan.mcus_y;
    const uint32_t n = comp == 0 ? mcus * luma : mcus;          // blocks of this component
    const uint32_t per = (n + DEC_DC_THREADS - 1) / DEC_DC_THREADS;
    const uint32_t t0 = tid * per < n ? tid * per : n, t1 = t0 + per < n ? t0 + per : n;
    auto block_of = [&](uint32_t t) { return comp == 0 ? (t / luma) * bpm + t % luma : t * bpm + luma + comp - 1u; };
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

__global__ void __launch_bounds__(DEC_DC_THREADS) k_jpeg_dec_dc(Plan plan, int16_t* coef, const uint8_t* flags) {
    dec_dc_body(plan, blockIdx.x, coef, flags);
}

// grid = (3, items): a workgroup whose component the item does not have returns as a whole
__global__ void __launch_bounds__(DEC_DC_THREADS) k_jpeg_dec_dc_batch(const Item* __restrict__ items, uint8_t* workspace) {
    const Item& it = items[blockIdx.y];
    if ((int)blockIdx.x >= it.plan.components) return;
    const DecItemArrays a = dec_item_arrays(it, nullptr, workspace);
    dec_dc_body(it.plan, blockIdx.x, a.coef, a.flags);
}

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

__global__ void __launch_bounds__(DEC_IDCT_THREADS) k_jpeg_dec_idct(const uint8_t* file, Plan plan, const int16_t* coef, DecPlanes planes) {
    dec_idct_body(file, plan, coef, planes, blockIdx.x);
}

// grid = (ceil(the batch's most blocks / 32), items): workgroups past the item's blocks return
__global__ void __launch_bounds__(DEC_IDCT_THREADS) k_jpeg_dec_idct_batch(const uint8_t* files, const Item* __restrict__ items, uint8_t* workspace) {
    const Item& it = items[blockIdx.y];
    if ((unsigned long long)blockIdx.x * DEC_IDCT_BLOCKS >= it.plan.expected_blocks) return;
    const DecItemArrays a = dec_item_arrays(it, files, workspace);
    dec_idct_body(a.file, it.plan, a.coef, a.planes, blockIdx.x);
}

// a chroma sample at full size: libjpeg's fancy upsampling; a plane of width <= 2 is replicated
__device__ __forceinline__ int dec_chroma(const uint8_t* plane, int pw, const Plan& plan, int x, int y) {
    if (plan.hs == 1) return plane[(size_t)y * pw + x];
    const int n = (plan.w + 1) >> 1, i = x >> 1;
    if (plan.vs == 1) {
        const uint8_t* s = plane + (size_t)y * pw;
        if (n <= 2 || x == 0 || x == 2 * n - 1) return s[i];
        return (x & 1) ? (3 * s[i] + s[i + 1] + 2) >> 2 : (3 * s[i] + s[i - 1] + 1) >> 2;
    }
    const int rows = (plan.h + 1) >> 1, yr = y >> 1;
    const uint8_t* near = plane + (size_t)yr * pw;
    if (n <= 2) return near[i];
    const int yf = (y & 1) ? (yr + 1 < rows ? yr + 1 : rows - 1) : (yr > 0 ? yr - 1 : 0);
    const uint8_t* far = plane + (size_t)yf * pw;
    const int cs = 3 * near[i] + far[i];
    if (x == 0) return (4 * cs + 8) >> 4;
    if (x == 2 * n - 1) return (4 * cs + 7) >> 4;
    return (x & 1) ? (3 * cs + 3 * near[i + 1] + far[i + 1] + 7) >> 4 : (3 * cs + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
}

__device__ __forceinline__ void dec_colour_body(const Plan& plan, const DecPlanes planes, int bgr, uint8_t* out, int x, int y) {
    if (x >= plan.w || y >= plan.h) return;
    const int lum = planes.p[0][(size_t)y * planes.pw[0] + x];
    int r = lum, g = lum, b = lum;
    if (plan.components == 3) {
        const int cb = dec_chroma(planes.p[1], planes.pw[1], plan, x, y) - 128, cr = dec_chroma(planes.p[2], planes.pw[2], plan, x, y) - 128;
        r = lum + ((91881 * cr + 32768) >> 16);
        b = lum + ((116130 * cb + 32768) >> 16);
        g = lum + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
        r = r < 0 ? 0 : (r > 255 ? 255 : r);
        g = g < 0 ? 0 : (g > 255 ? 255 : g);
        b = b < 0 ? 0 : (b > 255 ? 255 : b);
    }
    uint8_t* p = out + ((size_t)y * (size_t)plan.w + (size_t)x) * 3;
    p[0] = (uint8_t)(bgr ? b : r);
    p[1] = (uint8_t)g;
    p[2] = (uint8_t)(bgr ? r : b);
}

__global__ void __launch_bounds__(DEC_COLOUR_THREADS) k_jpeg_dec_colour(Plan plan, DecPlanes planes, int bgr, uint8_t* out) {
    dec_colour_body(plan, planes, bgr, out, (int)(blockIdx.x * DEC_COLOUR_THREADS + threadIdx.x), (int)blockIdx.y);
}

// grid = (ceil(the batch's largest w / 256), its largest h, items): rows and columns past the item's own return
__global__ void __launch_bounds__(DEC_COLOUR_THREADS) k_jpeg_dec_colour_batch(const Item* __restrict__ items, uint8_t* workspace, int bgr, uint8_t* out) {
    const Item& it = items[blockIdx.z];
    if ((int)(blockIdx.x * DEC_COLOUR_THREADS) >= it.plan.w || (int)blockIdx.y >= it.plan.h) return;
    const DecItemArrays a = dec_item_arrays(it, nullptr, workspace);
    dec_colour_body(it.plan, a.planes, bgr, out + it.out_off, (int)(blockIdx.x * DEC_COLOUR_THREADS + threadIdx.x), (int)blockIdx.y);
}

// ------------------------------------------------------------------------------------------------------------------ the planner
#define DEC_UNSUPPORTED(...) return fail(FRCNN_E_UNSUPPORTED, "jpeg_dec_plan: " __VA_ARGS__)

int dec_plan(const uint8_t* d, size_t n, Plan* out) {
    Plan p = {};
    if (n == 0) DEC_UNSUPPORTED("empty file");
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) DEC_UNSUPPORTED("not a JPEG file (no SOI)");
    if (n > 0xFFFFFFFFull) DEC_UNSUPPORTED("a file of %zu bytes", n);
    p.file_len = (uint32_t)n;
    uint32_t dqt[4] = {0, 0, 0, 0};
    size_t sof = 0, pos = 2;
    int jfif = 0, adobe = -1;
    for (;;) {
        if (pos + 4 > n) DEC_UNSUPPORTED("truncated: the headers end at byte %zu before SOS", pos);
        if (d[pos] != 0xFF) DEC_UNSUPPORTED("no marker at byte %zu", pos);
        const int m = d[pos + 1];
        if (m == 0xFF) { pos += 1; continue; }
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) { pos += 2; continue; }
        if (m == 0xD9) DEC_UNSUPPORTED("EOI before SOS");
        const size_t seg = ((size_t)d[pos + 2] << 8) | d[pos + 3];
        if (seg < 2 || pos + 2 + seg > n) DEC_UNSUPPORTED("truncated: segment 0x%02X at byte %zu runs past the file", m, pos);
        const size_t a = pos + 4, e = pos + 2 + seg;
        if (m == 0xC0) {
            if (sof) DEC_UNSUPPORTED("two frame headers");
            if (e - a < 6 || e - a != 6 + 3 * (size_t)d[a + 5]) DEC_UNSUPPORTED("malformed SOF0");
            if (d[a] != 8) DEC_UNSUPPORTED("%d-bit samples", d[a]);
            sof = a;
        } else if (m == 0xC2) {
            DEC_UNSUPPORTED("progressive");
        } else if (m == 0xC9 || m == 0xCC) {
            DEC_UNSUPPORTED("arithmetic coding");
        } else if (m == 0xC1) {
            DEC_UNSUPPORTED("extended sequential");
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8) {
            DEC_UNSUPPORTED("frame type 0x%02X", m);
        } else if (m == 0xDB) {
            for (size_t q = a; q < e; q += 65) {
                if (d[q] >> 4) DEC_UNSUPPORTED("16-bit DQT");
                if ((d[q] & 15) > 3 || q + 65 > e) DEC_UNSUPPORTED("malformed DQT");
                dqt[d[q] & 15] = (uint32_t)(q + 1);
            }
        } else if (m == 0xC4) {
            for (size_t q = a; q < e;) {
                if (q + 17 > e) DEC_UNSUPPORTED("malformed DHT");
                const int tc = d[q] >> 4, th = d[q] & 15;
                size_t cnt = 0;
                for (int l = 0; l < 16; ++l) cnt += d[q + 1 + l];
                if (tc > 1 || th > 1) DEC_UNSUPPORTED("Huffman table class %d id %d outside baseline", tc, th);
                if (cnt > 256 || q + 17 + cnt > e) DEC_UNSUPPORTED("malformed DHT");
                uint32_t code = 0;
                for (int l = 1; l <= 16; ++l) {
                    code += d[q + l];
                    if (code > (1u << l)) DEC_UNSUPPORTED("malformed DHT: codes overflow length %d", l);
                    code <<= 1;
                }
                p.dht_off[tc][th] = (uint32_t)(q + 1);
                p.dht_count[tc][th] = (uint32_t)cnt;
                q += 17 + cnt;
            }
        } else if (m == 0xDD) {
            if (seg != 4) DEC_UNSUPPORTED("malformed DRI");
            p.restart_interval = ((uint32_t)d[a] << 8) | d[a + 1];
        } else if (m == 0xE0 && e - a >= 5 && d[a] == 'J' && d[a + 1] == 'F' && d[a + 2] == 'I' && d[a + 3] == 'F' && d[a + 4] == 0) {
            jfif = 1;
        } else if (m == 0xEE && e - a >= 12 && d[a] == 'A' && d[a + 1] == 'd' && d[a + 2] == 'o' && d[a + 3] == 'b' && d[a + 4] == 'e') {
            adobe = d[a + 11];
        } else if (m == 0xDA) {
            break;
        }
        pos = e;
    }
    if (!sof) DEC_UNSUPPORTED("SOS before a frame header");
    const int nc = d[sof + 5];
    p.h = (d[sof + 1] << 8) | d[sof + 2];
    p.w = (d[sof + 3] << 8) | d[sof + 4];
    p.components = nc;
    if (p.h < 1 || p.w < 1) DEC_UNSUPPORTED("frame %dx%d: both sides must be at least 1", p.h, p.w);
    if (nc == 4) DEC_UNSUPPORTED("4 components (CMYK / YCCK)");
    if (nc != 1 && nc != 3) DEC_UNSUPPORTED("%d components", nc);
    const uint8_t* comps = d + sof + 6;                         // (id, h << 4 | v, quantisation table) per component
    if (nc == 3) {
        if (!jfif) {
            if (adobe >= 0 && adobe != 1) DEC_UNSUPPORTED("Adobe transform %d (not Y Cb Cr)", adobe);
            if (adobe < 0 && comps[0] == 'R' && comps[3] == 'G' && comps[6] == 'B') DEC_UNSUPPORTED("component ids R G B (not Y Cb Cr)");
        }
        const int s0 = comps[1];
        if ((s0 != 0x11 && s0 != 0x21 && s0 != 0x22) || comps[4] != 0x11 || comps[7] != 0x11)
            DEC_UNSUPPORTED("sampling factors %dx%d,%dx%d,%dx%d", comps[1] >> 4, comps[1] & 15, comps[4] >> 4, comps[4] & 15, comps[7] >> 4, comps[7] & 15);
        p.hs = s0 >> 4;
        p.vs = s0 & 15;
    } else {
        p.hs = p.vs = 1;                                        // (a single component is coded block by block whatever its factors say)
    }
    const size_t a = pos + 4, e = pos + 2 + (((size_t)d[pos + 2] << 8) | d[pos + 3]);
    if (e - a < 1) DEC_UNSUPPORTED("malformed SOS");
    if (e - a != 4 + 2 * (size_t)d[a] || d[a] != nc) DEC_UNSUPPORTED("a scan of %d of the %d components (multiple scans)", d[a], nc);
    for (int c = 0; c < nc; ++c) {
        if (d[a + 1 + 2 * c] != comps[3 * c]) DEC_UNSUPPORTED("scan components out of frame order");
        const int td = d[a + 2 + 2 * c] >> 4, ta = d[a + 2 + 2 * c] & 15;
        if (td > 1 || ta > 1 || !p.dht_off[0][td] || !p.dht_off[1][ta]) DEC_UNSUPPORTED("component %d names a Huffman table that is not defined", c);
        if (comps[3 * c + 2] > 3 || !dqt[comps[3 * c + 2]]) DEC_UNSUPPORTED("component %d names a quantisation table that is not defined", c);
        p.comp_dc[c] = (uint8_t)td;
        p.comp_ac[c] = (uint8_t)ta;
        p.dqt_off[c] = dqt[comps[3 * c + 2]];
    }
    if (d[e - 3] != 0 || d[e - 2] != 63 || d[e - 1] != 0) DEC_UNSUPPORTED("spectral selection / successive approximation in a baseline scan");
    p.scan_off = (uint32_t)e;
    size_t q = e;
    for (; q < n; ++q)
        if (d[q] == 0xFF && q + 1 < n && d[q + 1] != 0 && !(d[q + 1] >= 0xD0 && d[q + 1] <= 0xD7)) break;
    if (q - e >= DEC_MAX_SCAN) DEC_UNSUPPORTED("entropy-coded segment of %zu bytes", q - e);
    if (q == e) DEC_UNSUPPORTED("truncated: no entropy-coded data behind SOS");
    p.scan_len = (uint32_t)(q - e);
    p.mcus_x = (p.w + 8 * p.hs - 1) / (8 * p.hs);
    p.mcus_y = (p.h + 8 * p.vs - 1) / (8 * p.vs);
    p.blocks_per_mcu = nc == 3 ? p.hs * p.vs + 2 : 1;
    p.expected_blocks = (uint32_t)p.mcus_x * (uint32_t)p.mcus_y * (uint32_t)p.blocks_per_mcu;
    dec_subsequences(p.scan_len, &p.subsequence_bytes, &p.subsequences);
    *out = p;
    return FRCNN_OK;
}

}  // namespace
}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_jpeg_dec_version(void) { return FRCNN_JPEG_DEC_VERSION; }

extern "C" int frcnn_jpeg_dec_plan(const uint8_t* file_host, size_t len, frcnn_jpeg_dec_plan_t* plan) {
    if (!plan || (!file_host && len)) return fail(FRCNN_E_ARG, "jpeg_dec_plan: null pointer");
    return dec_plan(file_host, len, plan);
}

extern "C" size_t frcnn_jpeg_dec_workspace_bytes(const frcnn_jpeg_dec_plan_t* plan) {
    if (!plan || dec_plan_fault(*plan)) return 0;
    return dec_layout(*plan).total;
}

extern "C" int frcnn_jpeg_decode_u8(const uint8_t* file_dev, const frcnn_jpeg_dec_plan_t* plan, int bgr, uint8_t* out, size_t out_capacity,
                                    int32_t* status_dev, void* workspace, void* stream) {
    if (!file_dev || !plan || !out || !status_dev || !workspace) return fail(FRCNN_E_ARG, "jpeg_decode_u8: null pointer");
    if (const char* what = dec_plan_fault(*plan)) return fail(FRCNN_E_ARG, "jpeg_decode_u8: the plan contradicts itself (%s)", what);
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return fail(FRCNN_E_ARG, "jpeg_decode_u8: workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(status_dev) & 3u) return fail(FRCNN_E_ARG, "jpeg_decode_u8: status_dev must be 4-byte aligned");
    const Plan& p = *plan;
    const size_t need = (size_t)p.h * (size_t)p.w * 3;
    if (out_capacity < need) return fail(FRCNN_E_ARG, "jpeg_decode_u8: out_capacity=%zu below %d * %d * 3 = %zu", out_capacity, p.h, p.w, need);
    const DecLayout l = dec_layout(p);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    int16_t* coef = reinterpret_cast<int16_t*>(ws + l.coef);
    uint8_t* flags = ws + l.flags;
    DecPlanes planes = {};
    for (int c = 0; c < p.components; ++c) { planes.p[c] = ws + l.plane[c]; planes.pw[c] = l.pw[c]; }
    hipStream_t s = as_stream(stream);
    const unsigned lanes = (p.subsequences + 63u) / 64u * 64u;
    k_jpeg_dec_entropy<<<1, lanes, 0, s>>>(file_dev, p, coef, flags, status_dev);
    k_jpeg_dec_dc<<<p.components, DEC_DC_THREADS, 0, s>>>(p, coef, flags);
    k_jpeg_dec_idct<<<(p.expected_blocks + DEC_IDCT_BLOCKS - 1) / DEC_IDCT_BLOCKS, DEC_IDCT_THREADS, 0, s>>>(file_dev, p, coef, planes);
    k_jpeg_dec_colour<<<dim3((p.w + DEC_COLOUR_THREADS - 1) / DEC_COLOUR_THREADS, p.h), DEC_COLOUR_THREADS, 0, s>>>(p, planes, bgr ? 1 : 0, out);
    return check_launch("jpeg_decode_u8");
}

// ---------------------------------------------------------------------------------------------------------------- the batched form
extern "C" int frcnn_jpeg_dec_batch_version(void) { return FRCNN_JPEG_DEC_BATCH_VERSION; }

extern "C" size_t frcnn_jpeg_dec_batch_layout(const frcnn_jpeg_dec_plan_t* plans, int n, uint64_t* ws_off) {
    if (!plans || !ws_off || n < 1 || n > FRCNN_JPEG_DEC_BATCH_MAX) return 0;
    for (int i = 0; i < n; ++i)
        if (dec_plan_fault(plans[i])) return 0;
    size_t at = 0;
    for (int i = 0; i < n; ++i) { ws_off[i] = at; at += dec_layout(plans[i]).total; }
    return at;
}

extern "C" int frcnn_jpeg_decode_batch_u8(const frcnn_jpeg_dec_batch_item_t* items_host, const frcnn_jpeg_dec_batch_item_t* items_dev, int n,
                                          const uint8_t* files_dev, size_t files_capacity, int bgr, uint8_t* out_dev, size_t out_capacity,
                                          int32_t* status_dev, void* workspace, size_t workspace_capacity, void* stream) {
    if (!items_host || !items_dev || !files_dev || !out_dev || !status_dev || !workspace) return fail(FRCNN_E_ARG, "jpeg_decode_batch_u8: null pointer");
    if (n < 1 || n > FRCNN_JPEG_DEC_BATCH_MAX) return fail(FRCNN_E_ARG, "jpeg_decode_batch_u8: n=%d outside 1..%d", n, FRCNN_JPEG_DEC_BATCH_MAX);
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return fail(FRCNN_E_ARG, "jpeg_decode_batch_u8: workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(status_dev) & 3u) return fail(FRCNN_E_ARG, "jpeg_decode_batch_u8: status_dev must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(items_dev) & 7u) return fail(FRCNN_E_ARG, "jpeg_decode_batch_u8: items_dev must be 8-byte aligned");
    Range outs[FRCNN_JPEG_DEC_BATCH_MAX], regions[FRCNN_JPEG_DEC_BATCH_MAX];
    uint32_t lanes = 64, blocks = 1;
    int max_w = 1, max_h = 1;
    for (int i = 0; i < n; ++i) {
        const Item& it = items_host[i];
        const Plan& p = it.plan;
        if (const char* what = dec_plan_fault(p)) return fail(FRCNN_E_ARG, "jpeg_decode_batch_u8: item %d: the plan contradicts itself (%s)", i, what);
        const unsigned long long frame = (unsigned long long)p.h * p.w * 3, need = dec_layout(p).total;
        if (it.file_off > files_capacity || p.file_len > files_capacity - it.file_off)
            return fail(FRCNN_E_ARG, "jpeg_decode_batch_u8: item %d: file_off=%llu + file_len=%u beyond files_capacity=%zu", i, (unsigned long long)it.file_off, p.file_len, files_capacity);
        if (it.out_off > out_capacity || frame > out_capacity - it.out_off)
            return fail(FRCNN_E_ARG, "jpeg_decode_batch_u8: item %d: out_off=%llu + %d * %d * 3 beyond out_capacity=%zu", i, (unsigned long long)it.out_off, p.h, p.w, out_capacity);
        if (it.ws_off & 15u) return fail(FRCNN_E_ARG, "jpeg_decode_batch_u8: item %d: ws_off=%llu must be 16-byte aligned", i, (unsigned long long)it.ws_off);
        if (it.ws_off > workspace_capacity || need > workspace_capacity - it.ws_off)
            return fail(FRCNN_E_ARG, "jpeg_decode_batch_u8: item %d: ws_off=%llu + %llu beyond workspace_capacity=%zu", i, (unsigned long long)it.ws_off, need, workspace_capacity);
        outs[i] = {it.out_off, it.out_off + frame, i};
        regions[i] = {it.ws_off, it.ws_off + need, i};
        const uint32_t l = (p.subsequences + 63u) / 64u * 64u;
        lanes = l > lanes ? l : lanes;
        blocks = p.expected_blocks > blocks ? p.expected_blocks : blocks;
        max_w = p.w > max_w ? p.w : max_w;
        max_h = p.h > max_h ? p.h : max_h;
    }
    int k = range_overlap(outs, n);
    if (k >= 0) return fail(FRCNN_E_ARG, "jpeg_decode_batch_u8: the output ranges of items %d and %d overlap", outs[k].item, outs[k + 1].item);
    k = range_overlap(regions, n);
    if (k >= 0) return fail(FRCNN_E_ARG, "jpeg_decode_batch_u8: the workspace regions of items %d and %d overlap", regions[k].item, regions[k + 1].item);
    hipStream_t s = as_stream(stream);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    k_jpeg_dec_entropy_batch<<<n, lanes, 0, s>>>(files_dev, items_dev, ws, status_dev);
    k_jpeg_dec_dc_batch<<<dim3(3, n), DEC_DC_THREADS, 0, s>>>(items_dev, ws);
    k_jpeg_dec_idct_batch<<<dim3((blocks + DEC_IDCT_BLOCKS - 1) / DEC_IDCT_BLOCKS, n), DEC_IDCT_THREADS, 0, s>>>(files_dev, items_dev, ws);
    k_jpeg_dec_colour_batch<<<dim3((max_w + DEC_COLOUR_THREADS - 1) / DEC_COLOUR_THREADS, max_h, n), DEC_COLOUR_THREADS, 0, s>>>(items_dev, ws, bgr ? 1 : 0, out_dev);
    return check_launch("jpeg_decode_batch_u8");
}
