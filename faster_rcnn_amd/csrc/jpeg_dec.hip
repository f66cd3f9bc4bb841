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
//
// The table build, the code lookup, the byte-stuffing / RSTm window and the __device__ bodies of the DC, IDCT and colour kernels live in
// jpeg_dec_common.h: the decoder of progressive files (jpeg_dec_full.hip) runs the same ones.
#include "jpeg_dec_common.h"
#include "../../include/ext/frcnn_hip_jpeg_dec_batch.h"

namespace frcnn {
namespace {

using Item = frcnn_jpeg_dec_batch_item_t;

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

// F_i: whole symbols from ``st`` until the next would start at or past ``end`` (a bit position); -> blocks completed.  WRITE: the final
// walk, ``blk`` the index of the block the entry state stands in.
template <bool WRITE>
__device__ uint32_t dec_run(const EntropyCtx& c, uint32_t end, DecState& st, uint32_t blk, uint32_t* status) {
    uint32_t pos = st.pos, z = st.bz & 255u, b = (st.bz >> 8) & 255u, rst = (st.bz >> 16) & 1u, done = 0, flagged = 0;
    while (pos < end) {
        const DecWindow win = dec_window(c.scan, c.len, pos);           // (the window, its marker and its end: jpeg_dec_common.h)
        const unsigned long long w = win.w;
        const int mbit = win.mbit, ebit = win.ebit;
        const uint32_t o = pos & 7u;
        const int comp = (int)b < c.luma ? 0 : (int)b - c.luma + 1;
        const int slot = z == 0 ? (int)((c.tables >> comp) & 1u) : 2 + (int)((c.tables >> (4 + comp)) & 1u);
        // ---- the code
        const uint32_t top = (uint32_t)(w >> (24u - o)) & 0xFFFFu;
        uint32_t sym, flag;
        const uint32_t length = dec_huff_code(*c.huff, slot, top, ST_CODE, ST_TABLE, &sym, &flag);
        const uint32_t size = sym & 15u;
        if ((z == 0 && sym > 11u) || (z > 0 && size > 10u)) flag |= ST_TABLE;
        const uint32_t n = length + size;
        if (mbit >= 0 && o + n > (uint32_t)mbit) {              // the symbol reaches into a restart marker: abandoned
            if (z > 0) {
                if (WRITE && blk < c.nblk)
                    for (uint32_t k = z; k < 64u; ++k) c.coef[(size_t)blk * 64 + DEC_ZIGZAG.at[k]] = 0;
                ++blk; ++done;
            }
            pos = (win.mraw + 2u) * 8u; b = 0; z = 0; rst = 1;
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
        pos = dec_window_pos(win, o + n);                       // (o + n <= 7 + 31)
    }
    st.pos = pos;
    st.bz = z | (b << 8) | (rst << 16);
    if (WRITE) *status |= flagged;
    return done;
}

// The entropy stage of ONE file by the whole workgroup (blockDim.x a multiple of 64, >= plan.subsequences; lanes past the file's
// subsequences idle through every barrier: ``active`` is false for them, so they never change the round loop's flag).
__device__ __forceinline__ void dec_entropy_body(const uint8_t* file, const Plan& plan, int16_t* coef, uint8_t* flags, int32_t* status) {
    __shared__ HuffLds s_huff;
    __shared__ uint32_t s_xpos[DEC_MAX_LANES], s_xbz[DEC_MAX_LANES];
    __shared__ uint32_t s_part[DEC_MAX_LANES / 64];
    __shared__ uint32_t s_changed, s_status;
    const uint32_t tid = threadIdx.x, threads = blockDim.x;

    // ---- the Huffman tables (slot = class * 2 + id), from the DHT payloads in the file
    if (tid == 0) { s_changed = 0; s_status = 0; }
    const uint32_t t_off[4] = {plan.dht_off[0][0], plan.dht_off[0][1], plan.dht_off[1][0], plan.dht_off[1][1]};
    const uint32_t t_n[4] = {plan.dht_count[0][0], plan.dht_count[0][1], plan.dht_count[1][0], plan.dht_count[1][1]};
    dec_huff_build(s_huff, file, t_off, t_n);

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
