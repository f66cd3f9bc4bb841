// Progressive JPEG files decoded on the device (include/ext/frcnn_hip_jpeg_dec_full.h): the sibling of jpeg_dec.hip for SOF2 files.
// Everything behind the coefficients is the baseline's (jpeg_dec_common.h: DC sums, ISLOW IDCT, fancy upsampling, colour) on the
// baseline's coefficient layout (int16, natural order, 64 per block, blocks in MCU order padded to whole MCUs); what is new is filling
// that array from several scans.  gfx950 (CDNA4) only, wave64.  tests/jpeg_prog_ref.py states the same rules in Python.
//
//   k_jpeg_full_zero     the coefficient array zeroed: an AC scan never visits the padding blocks of partial MCUs, and a first scan
//                        writes only the coefficients it finds.
//   k_jpeg_full_entropy  ONE workgroup of 1024 lanes per file walks the file's scans in order (a barrier and a fence between scans: a
//                        later scan reads what an earlier one wrote).  Per scan: the Huffman tables of THAT scan into LDS (slot =
//                        frame component), then the baseline's rounds over the scan's subsequences: lane i guesses an entry state,
//                        decodes its stretch, hands its exit state to lane i + 1, until no entry changed, then a last walk that writes.
//                        The four kinds of scan differ in their state:
//                          DC first       (bit, block within the scan's MCU, restart pending); self-synchronising; blocks counted, an
//                                         exclusive scan gives every lane its first block; writes diff << Al and the restart flag;
//                                         behind the scan the workgroup sums the differences per component in the SCAN's block order
//                                         (dec_dc_sum), so the sum sees this scan's differences only.
//                          AC first       (bit, zigzag index k in Ss..Se); an EOBn symbol completes its blocks at once (they consume no
//                                         bits), so no run is carried; self-synchronising like the DC scan.
//                          DC refinement  (bit, block): one bit per block, ORed in at 1 << Al.
//                          AC refinement  (bit, k, EOB run left, block): jdphuff's walk; a correction bit for every non-zero coefficient
//                                         passed, inside EOB runs too.  The block index is part of the state that is compared, for both
//                                         refinement kinds: a guessed entry is never right, so the rounds fix one lane each (the
//                                         header's cost paragraph).  Restarts are taken where they are due (block index known); the
//                                         first kinds find them in the window, as the baseline does.
//   k_jpeg_full_idct, k_jpeg_full_colour   the baseline's bodies on the plan's frame.
//
// Block order.  An interleaved scan visits blocks in MCU order, padding included; a scan of ONE component visits that component's own
// ceil(w_c / 8) x ceil(h_c / 8) blocks in raster order (w_c, h_c: the image size, divided by the sampling factors and rounded up for
// chroma), and its restart interval counts blocks.  full_block() maps a scan's t-th block to its index in the MCU-order array.
//
// Bounds.  Every byte of a segment is read through dec_rd (zero past its end); full_block() answers FULL_NONE for a block past the
// scan's count and every coefficient access is behind that check; k never passes Se <= 63; table slots are 0..2; every loop advances
// the bit position or the block index, both bounded by the plan (full_plan_fault is what that rests on).  A damaged scan yields a
// status word, never a fault or a hang.
#include "jpeg_dec_common.h"
#include "../../include/ext/frcnn_hip_jpeg_dec_full.h"

namespace frcnn {
namespace {

using FullPlan = frcnn_jpeg_dec_full_plan_t;
using FullScan = frcnn_jpeg_dec_full_scan_t;
using FullItem = frcnn_jpeg_dec_full_batch_item_t;

constexpr int FULL_MAX_SCANS = FRCNN_JPEG_DEC_FULL_MAX_SCANS;
constexpr uint32_t FULL_NONE = 0xFFFFFFFFu;
constexpr uint32_t FT_BLOCKS = FRCNN_JPEG_DEC_FULL_BLOCKS, FT_ZIGZAG = FRCNN_JPEG_DEC_FULL_ZIGZAG, FT_CODE = FRCNN_JPEG_DEC_FULL_CODE,
                   FT_TABLE = FRCNN_JPEG_DEC_FULL_TABLE, FT_EOBRUN = FRCNN_JPEG_DEC_FULL_EOBRUN;
enum { K_DC_FIRST = 0, K_DC_REFINE = 1, K_AC_FIRST = 2, K_AC_REFINE = 3 };

__host__ __device__ inline int full_kind(const FullScan& s) { return (s.ss ? 2 : 0) + (s.ah ? 1 : 0); }

// blocks a scan visits, and per MCU of the scan (1 for a single component)
__host__ __device__ inline uint32_t full_scan_blocks(const Plan& f, const FullScan& s, uint32_t* per_mcu, uint32_t* row) {
    const uint32_t m = s.comps;
    const uint32_t luma = f.components == 3 ? (uint32_t)(f.hs * f.vs) : 1u;
    if (m & (m - 1u)) {                                         // interleaved: whole MCUs
        const uint32_t bps = ((m & 1u) ? luma : 0u) + ((m >> 1) & 1u) + ((m >> 2) & 1u);
        *per_mcu = bps; *row = 0;
        return (uint32_t)f.mcus_x * (uint32_t)f.mcus_y * bps;
    }
    const bool chroma = f.components == 3 && !(m & 1u);
    const uint32_t wc = chroma ? ((uint32_t)f.w + (uint32_t)f.hs - 1u) / (uint32_t)f.hs : (uint32_t)f.w;
    const uint32_t hc = chroma ? ((uint32_t)f.h + (uint32_t)f.vs - 1u) / (uint32_t)f.vs : (uint32_t)f.h;
    *per_mcu = 1; *row = (wc + 7u) / 8u;
    return *row * ((hc + 7u) / 8u);
}

// nullptr when the plan's fields agree with each other (what the kernels' bounds rest on), else what is wrong
inline const char* full_plan_fault(const FullPlan& fp) {
    const Plan& p = fp.frame;
    if (p.h < 1 || p.w < 1 || p.h > 65535 || p.w > 65535) return "sides outside 1..65535";
    if (p.components != 1 && p.components != 3) return "components";
    if (!((p.hs == 1 && p.vs == 1) || (p.components == 3 && p.hs == 2 && (p.vs == 1 || p.vs == 2)))) return "sampling factors";
    if (p.mcus_x != (p.w + 8 * p.hs - 1) / (8 * p.hs) || p.mcus_y != (p.h + 8 * p.vs - 1) / (8 * p.vs)) return "MCU counts";
    if (p.blocks_per_mcu != (p.components == 3 ? p.hs * p.vs + 2 : 1)) return "blocks per MCU";
    if ((unsigned long long)p.expected_blocks != (unsigned long long)p.mcus_x * p.mcus_y * p.blocks_per_mcu) return "block total";
    for (int c = 0; c < p.components; ++c)
        if (p.dqt_off[c] > p.file_len || 64 > p.file_len - p.dqt_off[c]) return "quantisation table outside the file";
    if (fp.scans < 1 || fp.scans > (uint32_t)FULL_MAX_SCANS) return "scan count";
    unsigned long long total = 0;
    for (uint32_t i = 0; i < fp.scans; ++i) {
        const FullScan& s = fp.scan[i];
        if (s.len >= DEC_MAX_SCAN || s.off > p.file_len || s.len > p.file_len - s.off) return "scan outside the file";
        total += s.len;
        if (s.subsequence_bytes < DEC_MIN_S || s.subsequence_bytes % 4 || s.subsequences < 1 || s.subsequences > (uint32_t)DEC_MAX_LANES ||
            (unsigned long long)s.subsequence_bytes * s.subsequences < s.len) return "subsequences";
        if (s.comps == 0 || s.comps >= (1u << p.components)) return "scan components";
        if (s.ss == 0 ? s.se != 0 : (s.ss > s.se || s.se > 63 || (s.comps & (s.comps - 1)))) return "spectral selection";
        if (s.al > 13 || s.ah > 13) return "successive approximation";
        if (s.restart_interval > 65535u) return "restart interval";
        const int kind = full_kind(s);
        for (int c = 0; c < 3; ++c) {
            const bool in = (s.comps >> c) & 1;
            const uint32_t need_dc = in && kind == K_DC_FIRST, need_ac = in && kind >= K_AC_FIRST;
            if (need_dc != (s.dc_off[c] != 0) || need_ac != (s.ac_off[c] != 0)) return "Huffman tables of a scan";
            if (s.dc_off[c] && (s.dc_count[c] > 256 || s.dc_off[c] > p.file_len || 16 + s.dc_count[c] > p.file_len - s.dc_off[c])) return "Huffman table outside the file";
            if (s.ac_off[c] && (s.ac_count[c] > 256 || s.ac_off[c] > p.file_len || 16 + s.ac_count[c] > p.file_len - s.ac_off[c])) return "Huffman table outside the file";
        }
    }
    if (total >= DEC_MAX_SCAN) return "entropy-coded bytes";
    return nullptr;
}

// ------------------------------------------------------------------------------------------------------------- entropy decoding
struct FullCtx {
    const uint8_t* scan;
    uint32_t len;                       // bytes of the segment
    const HuffLds* huff;
    int16_t* coef;
    uint8_t* flags;
    uint32_t bpm, luma, hs, vs, mcus_x; // the frame
    uint32_t mask, bps, row, nblk;      // the scan: components, blocks per MCU of the scan, single component: blocks per row; its blocks
    uint32_t single;                    // the component of a single-component scan (interleaved: unused)
    uint32_t ri;                        // restart interval in BLOCKS of the scan (0: none)
    uint32_t ss, se, al;
};

// block j of an MCU of an interleaved scan -> its component; *at: its place in the frame's MCU
__device__ __forceinline__ uint32_t full_mcu_block(const FullCtx& c, uint32_t j, uint32_t* at) {
    uint32_t jc = j;
    if (c.mask & 1u) {
        if (j < c.luma) { *at = j; return 0u; }
        jc = j - c.luma;
    }
    const uint32_t comp = (jc == 0u && (c.mask & 2u)) ? 1u : 2u;
    *at = c.luma + comp - 1u;
    return comp;
}

// the scan's t-th block -> its index in the MCU-order array (FULL_NONE past the scan's blocks)
__device__ __forceinline__ uint32_t full_block(const FullCtx& c, uint32_t t) {
    if (t >= c.nblk) return FULL_NONE;
    if (c.row == 0u) {
        uint32_t at;
        full_mcu_block(c, t % c.bps, &at);
        return (t / c.bps) * c.bpm + at;
    }
    const uint32_t by = t / c.row, bx = t - by * c.row;
    if (c.single == 0u) return ((by / c.vs) * c.mcus_x + bx / c.hs) * c.bpm + (by % c.vs) * c.hs + bx % c.hs;
    return (by * c.mcus_x + bx) * c.bpm + c.luma + c.single - 1u;
}

// state: pos = a bit of the raw segment; bz = DC first: block within the scan's MCU << 8 | restart pending << 16; AC: k | EOB run << 8;
// blk = the scan's block the state stands in (refinement kinds; the first kinds count from 0 and get it from the scan over the lanes)
struct FullState { uint32_t pos, bz, blk; };

// F_i for the kinds that re-synchronise: whole symbols from ``st`` until the next would start at or past ``end``; st.blk advances by the
// blocks completed.  WRITE: the final walk.
template <int KIND, bool WRITE>
__device__ void full_run_first(const FullCtx& c, uint32_t end, FullState& st, uint32_t* status) {
    uint32_t pos = st.pos, blk = st.blk, flagged = 0;
    uint32_t k = KIND == K_AC_FIRST ? (st.bz & 255u) : 0u, j = (st.bz >> 8) & 255u, rst = (st.bz >> 16) & 1u;
    while (pos < end) {
        const DecWindow win = dec_window(c.scan, c.len, pos);
        const uint32_t o = pos & 7u;
        uint32_t at = 0, comp = c.single;
        if (KIND == K_DC_FIRST && c.row == 0u) comp = full_mcu_block(c, j, &at);
        const uint32_t top = (uint32_t)(win.w >> (24u - o)) & 0xFFFFu;
        uint32_t sym, flag;
        const uint32_t length = dec_huff_code(*c.huff, (int)comp, top, FT_CODE, FT_TABLE, &sym, &flag);
        const uint32_t size = sym & 15u, run = sym >> 4;
        const bool eob = KIND == K_AC_FIRST && size == 0u && run < 15u;
        const uint32_t extra = eob ? run : size;                // value bits, or the bits of an EOB run's length
        if (KIND == K_DC_FIRST ? sym > 11u : size > 10u) flag |= FT_TABLE;
        const uint32_t n = length + extra;                      // (<= 16 + 15)
        if (win.mbit >= 0 && o + n > (uint32_t)win.mbit) {      // the symbol reaches into a restart marker: abandoned
            if (KIND == K_AC_FIRST && k != c.ss) ++blk;         // (a block left unfinished: a damaged scan)
            pos = (win.mraw + 2u) * 8u; j = 0; k = c.ss; rst = 1;
            continue;
        }
        if (win.ebit >= 0 && o + n > (uint32_t)win.ebit) {      // ... past the end of the segment: abandoned, the end
            pos = pos > c.len * 8u ? pos : c.len * 8u;
            break;
        }
        flagged |= flag;
        const uint32_t raw = extra ? (uint32_t)(win.w >> (40u - o - n)) & ((1u << extra) - 1u) : 0u;
        int v = (int)raw;
        if (size && v < (1 << (size - 1))) v -= (1 << size) - 1;
        const int16_t value = (int16_t)(uint16_t)((uint32_t)v << c.al);
        if (KIND == K_DC_FIRST) {
            if (WRITE) {
                const uint32_t b = full_block(c, blk);
                if (b != FULL_NONE) {
                    c.coef[(size_t)b * 64] = value;
                    c.flags[b] = (uint8_t)((comp != 0u || j == 0u || c.row != 0u) ? rst : 0u);
                }
            }
            ++blk;
            j = j + 1u < c.bps ? j + 1u : 0u;
            rst = j ? rst : 0u;
        } else if (eob) {                                       // EOBn: this block and run - 1 more are complete
            const uint32_t blocks = (1u << run) + raw;
            if (WRITE && (blk >= c.nblk || blocks > c.nblk - blk)) flagged |= FT_EOBRUN;
            blk += blocks;
            k = c.ss;
        } else {
            bool done = false;
            if (size) {
                k += run;
                if (k > c.se) { flagged |= FT_ZIGZAG; done = true; }
                else {
                    if (WRITE) {
                        const uint32_t b = full_block(c, blk);
                        if (b != FULL_NONE) c.coef[(size_t)b * 64 + DEC_ZIGZAG.at[k]] = value;
                    }
                    done = ++k > c.se;
                }
            } else {                                            // ZRL
                k += 16u;
                if (k > c.se + 1u) flagged |= FT_ZIGZAG;
                done = k > c.se;
            }
            if (done) { ++blk; k = c.ss; }
        }
        pos = dec_window_pos(win, o + n);
    }
    st.pos = pos;
    st.blk = blk;
    st.bz = KIND == K_AC_FIRST ? k : (j << 8) | (rst << 16);
    if (WRITE) *status |= flagged;
}

// The refinement kinds read bit by bit.  ``cur``: the data byte at pos >> 3 (a 0x00 behind 0xFF is skipped when the position crosses
// into it; an RSTm marker and what lies past the segment read as zero, and the position does not move into a marker).
struct FullBits { uint32_t pos, cur, marker; };

__device__ __forceinline__ void full_load(const FullCtx& c, FullBits& b) {
    const uint32_t r = b.pos >> 3;
    uint32_t v = dec_rd(c.scan, c.len, r);
    b.marker = 0;
    if (v == 0xFFu && (dec_rd(c.scan, c.len, r + 1u) & 0xF8u) == 0xD0u) { b.marker = 1; v = 0; }
    b.cur = v;
}

__device__ __forceinline__ uint32_t full_bit(const FullCtx& c, FullBits& b) {
    if (b.marker) return 0u;
    const uint32_t bit = (b.cur >> (7u - (b.pos & 7u))) & 1u;
    b.pos += 1u;
    if ((b.pos & 7u) == 0u) {
        if (b.cur == 0xFFu && dec_rd(c.scan, c.len, b.pos >> 3) == 0u) b.pos += 8u;
        full_load(c, b);
    }
    return bit;
}

// a restart is due: the padding of the byte is dropped, the marker behind it skipped (FT_CODE where none stands there)
__device__ __forceinline__ uint32_t full_restart(const FullCtx& c, FullBits& b) {
    uint32_t r = b.pos >> 3, flag = 0;
    if (b.pos & 7u) r += (dec_rd(c.scan, c.len, r) == 0xFFu && dec_rd(c.scan, c.len, r + 1u) == 0u) ? 2u : 1u;
    if (dec_rd(c.scan, c.len, r) == 0xFFu && (dec_rd(c.scan, c.len, r + 1u) & 0xF8u) == 0xD0u) r += 2u; else flag = FT_CODE;
    b.pos = r * 8u;
    full_load(c, b);
    return flag;
}

// one correction bit for a non-zero coefficient (jdphuff: away from zero by 1 << Al when the bit is set and that bit is still clear)
__device__ __forceinline__ void full_correct(const FullCtx& c, FullBits& b, int16_t* at, bool write) {
    if (!full_bit(c, b) || !write) return;
    const int v = *at, p1 = 1 << c.al;
    if ((v & p1) == 0) *at = (int16_t)(v >= 0 ? v + p1 : v - p1);
}

// F_i for the refinement kinds: from ``st`` until the next symbol (DC: bit; AC: symbol, or block of an EOB run) would start at or past
// ``end`` or the scan's blocks are done (the last stretch: until an EOB run that reaches past the bits is done too).
template <int KIND, bool WRITE>
__device__ void full_run_refine(const FullCtx& c, uint32_t end, FullState& st, uint32_t* status) {
    FullBits b;
    b.pos = st.pos;
    full_load(c, b);
    uint32_t blk = st.blk, k = st.bz & 255u, eobrun = st.bz >> 8, flagged = 0;
    const int slot = (int)c.single;
    const bool tail = end >= c.len * 8u;                        // the scan's last stretch also ends the blocks of an EOB run that take no bits
    while ((b.pos < end || (tail && eobrun)) && blk < c.nblk) {
        const uint32_t at = full_block(c, blk);                 // (blk < nblk: never FULL_NONE)
        int16_t* dst = c.coef + (size_t)at * 64;
        bool done;
        if (KIND == K_DC_REFINE) {
            const uint32_t bit = full_bit(c, b);
            if (WRITE && bit) dst[0] = (int16_t)(dst[0] | (1 << c.al));
            done = true;
        } else if (eobrun) {                                    // the rest of a block inside an EOB run: correction bits only
            for (; k <= c.se; ++k) {
                int16_t* p = dst + DEC_ZIGZAG.at[k];
                if (*p) full_correct(c, b, p, WRITE);
            }
            --eobrun;
            done = true;
        } else {
            uint32_t code = 0, sym = 0, flag = FT_CODE;         // the code, bit by bit (at most 16)
            for (int l = 1; l <= 16; ++l) {
                code = (code << 1) | full_bit(c, b);
                if ((int)code <= c.huff->maxcode[slot][l]) {
                    const int i = (int)code + c.huff->delta[slot][l];
                    if (i >= 0 && i < c.huff->count[slot]) { sym = c.huff->vals[slot][i]; flag = 0; } else flag = FT_TABLE;
                    break;
                }
            }
            flagged |= flag;
            int run = (int)(sym >> 4);
            const uint32_t size = sym & 15u;
            int16_t fresh = 0;
            done = false;
            if (size) {
                if (size != 1u) flagged |= FT_TABLE;
                fresh = (int16_t)(full_bit(c, b) ? (1 << c.al) : -(1 << c.al));
            } else if (run != 15) {                             // EOBn: the run counts this block
                eobrun = 1u << run;
                for (int i = 0; i < run; ++i) eobrun += full_bit(c, b) << (run - 1 - i);
                if (WRITE && eobrun > c.nblk - blk) flagged |= FT_EOBRUN;
                run = -1;                                       // (handled by the branch above, at the same k)
            }
            if (run >= 0) {
                // pass ``run`` coefficients whose history is zero, correcting the non-zero ones in between
                for (; k <= c.se; ++k) {
                    int16_t* p = dst + DEC_ZIGZAG.at[k];
                    if (*p) full_correct(c, b, p, WRITE);
                    else if (--run < 0) break;
                }
                if (fresh) {
                    if (k <= c.se) { if (WRITE) dst[DEC_ZIGZAG.at[k]] = fresh; }
                    else flagged |= FT_ZIGZAG;
                }
                ++k;
                done = k > c.se;
            }
        }
        if (done) {
            ++blk;
            k = c.ss;
            if (c.ri && blk < c.nblk && blk % c.ri == 0u) { flagged |= full_restart(c, b); eobrun = 0; }
        }
    }
    st.pos = b.pos;
    st.blk = blk;
    st.bz = k | (eobrun << 8);
    if (WRITE) *status |= flagged;
}

template <bool WRITE>
__device__ __forceinline__ void full_run(int kind, const FullCtx& c, uint32_t end, FullState& st, uint32_t* status) {
    if (kind == K_DC_FIRST) full_run_first<K_DC_FIRST, WRITE>(c, end, st, status);
    else if (kind == K_AC_FIRST) full_run_first<K_AC_FIRST, WRITE>(c, end, st, status);
    else if (kind == K_DC_REFINE) full_run_refine<K_DC_REFINE, WRITE>(c, end, st, status);
    else full_run_refine<K_AC_REFINE, WRITE>(c, end, st, status);
}

struct FullItemArrays { const uint8_t* file; int16_t* coef; uint8_t* flags; DecPlanes planes; };

__device__ __forceinline__ FullItemArrays full_item_arrays(const FullItem& it, const uint8_t* files, uint8_t* workspace) {
    const DecLayout l = dec_layout(it.plan.frame);
    uint8_t* ws = workspace + it.ws_off;
    FullItemArrays a = {};
    a.file = files + it.file_off;
    a.coef = reinterpret_cast<int16_t*>(ws + l.coef);
    a.flags = ws + l.flags;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        if (c < it.plan.frame.components) { a.planes.p[c] = ws + l.plane[c]; a.planes.pw[c] = l.pw[c]; }
    return a;
}

// grid = (ceil(the batch's most blocks / 32), items), 256 lanes: 16 bytes per lane
__global__ void __launch_bounds__(DEC_IDCT_THREADS) k_jpeg_full_zero(const FullItem* __restrict__ items, uint8_t* workspace) {
    const FullItem& it = items[blockIdx.y];
    const unsigned long long at = ((unsigned long long)blockIdx.x * DEC_IDCT_THREADS + threadIdx.x) * 16ull;
    if (at >= (unsigned long long)it.plan.frame.expected_blocks * 128ull) return;
    uint4* dst = reinterpret_cast<uint4*>(workspace + it.ws_off + dec_layout(it.plan.frame).coef + at);     // (16-byte aligned: ws_off and the layout)
    *dst = make_uint4(0u, 0u, 0u, 0u);
}

// grid.x = item; DEC_MAX_LANES lanes whatever the scans' subsequences are (the DC sums want them all)
__global__ void __launch_bounds__(DEC_MAX_LANES) k_jpeg_full_entropy(const uint8_t* files, const FullItem* __restrict__ items, uint8_t* workspace, int32_t* status) {
    __shared__ HuffLds s_huff;
    __shared__ uint32_t s_xpos[DEC_MAX_LANES], s_xbz[DEC_MAX_LANES], s_xblk[DEC_MAX_LANES];
    __shared__ uint32_t s_part[DEC_MAX_LANES / 64];
    __shared__ uint32_t s_changed, s_status, s_last;
    const FullItem& it = items[blockIdx.x];
    const Plan& f = it.plan.frame;
    const FullItemArrays a = full_item_arrays(it, files, workspace);
    const uint32_t tid = threadIdx.x;
    if (tid == 0) { s_changed = 0; s_status = 0; }

    FullCtx c;
    c.huff = &s_huff;
    c.coef = a.coef;
    c.flags = a.flags;
    c.bpm = (uint32_t)f.blocks_per_mcu;
    c.luma = f.components == 3 ? (uint32_t)(f.hs * f.vs) : 1u;
    c.hs = (uint32_t)f.hs; c.vs = (uint32_t)f.vs; c.mcus_x = (uint32_t)f.mcus_x;
    const uint32_t scans = it.plan.scans < (uint32_t)FULL_MAX_SCANS ? it.plan.scans : (uint32_t)FULL_MAX_SCANS;

    for (uint32_t si = 0; si < scans; ++si) {
        const FullScan& sc = it.plan.scan[si];
        const int kind = full_kind(sc);
        // ---- this scan's tables (slot = frame component) and geometry
        const uint32_t t_off[4] = {kind == K_DC_FIRST ? sc.dc_off[0] : sc.ac_off[0], kind == K_DC_FIRST ? sc.dc_off[1] : sc.ac_off[1],
                                   kind == K_DC_FIRST ? sc.dc_off[2] : sc.ac_off[2], 0u};
        const uint32_t t_n[4] = {kind == K_DC_FIRST ? sc.dc_count[0] : sc.ac_count[0], kind == K_DC_FIRST ? sc.dc_count[1] : sc.ac_count[1],
                                 kind == K_DC_FIRST ? sc.dc_count[2] : sc.ac_count[2], 0u};
        if (tid == 0) s_changed = 0;
        dec_huff_build(s_huff, a.file, t_off, t_n);             // (barriers inside: the previous scan's LDS reads are behind them)
        c.scan = a.file + sc.off;
        c.len = sc.len;
        c.mask = sc.comps;
        c.nblk = full_scan_blocks(f, sc, &c.bps, &c.row);
        c.single = (sc.comps & 1u) ? 0u : ((sc.comps & 2u) ? 1u : 2u);
        c.ri = sc.restart_interval * c.bps;
        c.ss = sc.ss; c.se = sc.se; c.al = sc.al;

        // ---- rounds: exit[i] = F_i(entry[i]) for every lane whose entry changed, entry[i + 1] = exit[i], until nothing changes
        const uint32_t N = sc.subsequences, S = sc.subsequence_bytes;
        const bool active = tid < N, carried = (kind & 1) != 0;  // carried: the block index is part of the state
        const uint32_t last = (tid + 1u) * S < c.len ? (tid + 1u) * S : c.len;
        const uint32_t end = last * 8u;
        // A first kind guesses: every lane starts at its stretch's first bit.  A carried kind does not (a guessed block index is never
        // right, and a walk from a wrong one reads history that is not its own): lane 0 starts, every other lane waits for its
        // predecessor's exit to differ from the FULL_NONE it holds, so exactly one lane decodes per round.
        FullState entry = {tid * S * 8u, kind >= K_AC_FIRST ? c.ss : 0u, 0u};
        if (carried && tid > 0u) entry = {FULL_NONE, 0u, 0u};
        if (carried) { s_xpos[tid] = FULL_NONE; s_xbz[tid] = 0u; s_xblk[tid] = 0u; }
        uint32_t count = 0, unused = 0;
        bool changed = carried ? tid == 0u : active;
        __syncthreads();
        for (uint32_t round = 0; round < N; ++round) {
            if (changed) {
                FullState st = entry;
                if (!carried) st.blk = 0;
                full_run<false>(kind, c, end, st, &unused);
                count = st.blk;
                s_xpos[tid] = st.pos;
                s_xbz[tid] = st.bz;
                s_xblk[tid] = carried ? st.blk : 0u;
            }
            __syncthreads();
            changed = false;
            if (active && tid > 0u) {
                const uint32_t p = s_xpos[tid - 1u], bz = s_xbz[tid - 1u], bk = s_xblk[tid - 1u];
                if (p != entry.pos || bz != entry.bz || bk != entry.blk) { entry.pos = p; entry.bz = bz; entry.blk = bk; changed = true; }
            }
            if (changed) atomicOr(&s_changed, 1u);
            __syncthreads();
            const uint32_t any = s_changed;
            __syncthreads();
            if (!any) break;
            if (tid == 0) s_changed = 0;                       // (read again only behind the next round's barriers)
        }

        // ---- every lane's first block (the first kinds: from the counts), the final walk, the scan's total
        uint32_t total = 0;
        if (!carried) {
            const uint32_t incl = dec_wave_scan(active ? count : 0u);
            if ((tid & 63u) == 63u) s_part[tid >> 6] = incl;
            __syncthreads();
            uint32_t before = incl - (active ? count : 0u);
            for (uint32_t k = 0; k < (uint32_t)DEC_MAX_LANES / 64u; ++k) {
                const uint32_t p = s_part[k];
                total += p;
                if (k < (tid >> 6)) before += p;
            }
            entry.blk = before;
        }
        uint32_t flagged = 0;
        if (active && entry.pos != FULL_NONE) {
            FullState st = entry;
            full_run<true>(kind, c, end, st, &flagged);
            if (tid == N - 1u) s_last = st.blk;
        }
        if (flagged) atomicOr(&s_status, flagged);
        __threadfence();
        __syncthreads();
        if (tid == 0 && (carried ? s_last : total) != c.nblk) atomicOr(&s_status, FT_BLOCKS);

        // ---- behind a DC-first scan: the differences summed per component, in the scan's block order, cut at the restart flags
        if (kind == K_DC_FIRST) {
            for (uint32_t comp = 0; comp < 3u; ++comp) {
                if (!((sc.comps >> comp) & 1u)) continue;
                const uint32_t mcus = c.mcus_x * (uint32_t)f.mcus_y, n = c.row ? c.nblk : (comp == 0 ? mcus * c.luma : mcus);
                dec_dc_sum(n, [&](uint32_t t) {
                    if (c.row) return full_block(c, t);
                    return comp == 0 ? (t / c.luma) * c.bpm + t % c.luma : t * c.bpm + c.luma + comp - 1u;
                }, a.coef, a.flags, reinterpret_cast<int*>(s_xpos), s_xbz);     // (the rounds' exchange arrays are free here)
                __syncthreads();
            }
            __threadfence();
            __syncthreads();
        }
    }
    if (tid == 0 && s_status) status[blockIdx.x] = (int32_t)((uint32_t)status[blockIdx.x] | s_status);
}

// grid = (ceil(the batch's most blocks / 32), items): workgroups past the item's blocks return
__global__ void __launch_bounds__(DEC_IDCT_THREADS) k_jpeg_full_idct(const uint8_t* files, const FullItem* __restrict__ items, uint8_t* workspace) {
    const FullItem& it = items[blockIdx.y];
    if ((unsigned long long)blockIdx.x * DEC_IDCT_BLOCKS >= it.plan.frame.expected_blocks) return;
    const FullItemArrays a = full_item_arrays(it, files, workspace);
    dec_idct_body(a.file, it.plan.frame, a.coef, a.planes, blockIdx.x);
}

// grid = (ceil(the batch's largest w / 256), its largest h, items): rows and columns past the item's own return
__global__ void __launch_bounds__(DEC_COLOUR_THREADS) k_jpeg_full_colour(const FullItem* __restrict__ items, uint8_t* workspace, int bgr, uint8_t* out) {
    const FullItem& it = items[blockIdx.z];
    if ((int)(blockIdx.x * DEC_COLOUR_THREADS) >= it.plan.frame.w || (int)blockIdx.y >= it.plan.frame.h) return;
    const FullItemArrays a = full_item_arrays(it, nullptr, workspace);
    dec_colour_body(it.plan.frame, a.planes, bgr, out + it.out_off, (int)(blockIdx.x * DEC_COLOUR_THREADS + threadIdx.x), (int)blockIdx.y);
}

// ------------------------------------------------------------------------------------------------------------------ the planner
#define FULL_UNSUPPORTED(...) return fail(FRCNN_E_UNSUPPORTED, "jpeg_dec_full_plan: " __VA_ARGS__)

int full_plan(const uint8_t* d, size_t n, FullPlan* out) {
    static thread_local FullPlan fp;                            // (5 KB: kept off the stack of a caller's thread)
    fp = FullPlan{};
    Plan& p = fp.frame;
    if (n == 0) FULL_UNSUPPORTED("empty file");
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) FULL_UNSUPPORTED("not a JPEG file (no SOI)");
    if (n > 0xFFFFFFFFull) FULL_UNSUPPORTED("a file of %zu bytes", n);
    p.file_len = (uint32_t)n;
    uint32_t dqt[4] = {0, 0, 0, 0}, dht_off[2][4] = {}, dht_count[2][4] = {}, restart = 0;
    int8_t prog[3][64];                                         // per coefficient: the Al it stands at, -1: not coded yet
    for (int c = 0; c < 3; ++c) for (int k = 0; k < 64; ++k) prog[c][k] = -1;
    size_t sof = 0, pos = 2;
    int jfif = 0, adobe = -1, nc = 0;
    const uint8_t* comps = nullptr;
    unsigned long long total = 0;
    for (;;) {
        if (pos + 4 > n) {
            if (pos + 2 <= n && d[pos] == 0xFF && d[pos + 1] == 0xD9 && fp.scans) break;
            FULL_UNSUPPORTED("truncated: the file ends at byte %zu before EOI", pos);
        }
        if (d[pos] != 0xFF) FULL_UNSUPPORTED("no marker at byte %zu", pos);
        const int m = d[pos + 1];
        if (m == 0xFF) { pos += 1; continue; }
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) { pos += 2; continue; }
        if (m == 0xD9) {
            if (!fp.scans) FULL_UNSUPPORTED("EOI before SOS");
            break;
        }
        const size_t seg = ((size_t)d[pos + 2] << 8) | d[pos + 3];
        if (seg < 2 || pos + 2 + seg > n) FULL_UNSUPPORTED("truncated: segment 0x%02X at byte %zu runs past the file", m, pos);
        const size_t a = pos + 4, e = pos + 2 + seg;
        if (m == 0xC2) {
            if (sof) FULL_UNSUPPORTED("two frame headers");
            if (e - a < 6 || e - a != 6 + 3 * (size_t)d[a + 5]) FULL_UNSUPPORTED("malformed SOF2");
            if (d[a] != 8) FULL_UNSUPPORTED("%d-bit samples", d[a]);
            sof = a;
        } else if (m == 0xC0) {
            FULL_UNSUPPORTED("baseline (SOF0): the baseline planner's file");
        } else if (m == 0xC9 || m == 0xCA || m == 0xCC) {
            FULL_UNSUPPORTED("arithmetic coding");
        } else if (m == 0xC1) {
            FULL_UNSUPPORTED("extended sequential");
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8) {
            FULL_UNSUPPORTED("frame type 0x%02X", m);
        } else if (m == 0xDB) {
            for (size_t q = a; q < e; q += 65) {
                if (d[q] >> 4) FULL_UNSUPPORTED("16-bit DQT");
                if ((d[q] & 15) > 3 || q + 65 > e) FULL_UNSUPPORTED("malformed DQT");
                dqt[d[q] & 15] = (uint32_t)(q + 1);
            }
        } else if (m == 0xC4) {
            for (size_t q = a; q < e;) {
                if (q + 17 > e) FULL_UNSUPPORTED("malformed DHT");
                const int tc = d[q] >> 4, th = d[q] & 15;
                size_t cnt = 0;
                for (int l = 0; l < 16; ++l) cnt += d[q + 1 + l];
                if (tc > 1 || th > 3) FULL_UNSUPPORTED("Huffman table class %d id %d", tc, th);
                if (cnt > 256 || q + 17 + cnt > e) FULL_UNSUPPORTED("malformed DHT");
                uint32_t code = 0;
                for (int l = 1; l <= 16; ++l) {
                    code += d[q + l];
                    if (code > (1u << l)) FULL_UNSUPPORTED("malformed DHT: codes overflow length %d", l);
                    code <<= 1;
                }
                dht_off[tc][th] = (uint32_t)(q + 1);
                dht_count[tc][th] = (uint32_t)cnt;
                q += 17 + cnt;
            }
        } else if (m == 0xDD) {
            if (seg != 4) FULL_UNSUPPORTED("malformed DRI");
            restart = ((uint32_t)d[a] << 8) | d[a + 1];
        } else if (m == 0xE0 && e - a >= 5 && d[a] == 'J' && d[a + 1] == 'F' && d[a + 2] == 'I' && d[a + 3] == 'F' && d[a + 4] == 0) {
            jfif = 1;
        } else if (m == 0xEE && e - a >= 12 && d[a] == 'A' && d[a + 1] == 'd' && d[a + 2] == 'o' && d[a + 3] == 'b' && d[a + 4] == 'e') {
            adobe = d[a + 11];
        }
        if (m != 0xDA) { pos = e; continue; }

        // ---- a scan
        if (!sof) FULL_UNSUPPORTED("SOS before a frame header");
        if (!fp.scans) {                                        // the frame, as the baseline planner judges it
            nc = d[sof + 5];
            comps = d + sof + 6;                                // (id, h << 4 | v, quantisation table) per component
            p.h = (d[sof + 1] << 8) | d[sof + 2];
            p.w = (d[sof + 3] << 8) | d[sof + 4];
            p.components = nc;
            if (p.h < 1 || p.w < 1) FULL_UNSUPPORTED("frame %dx%d: both sides must be at least 1", p.h, p.w);
            if (nc == 4) FULL_UNSUPPORTED("4 components (CMYK / YCCK)");
            if (nc != 1 && nc != 3) FULL_UNSUPPORTED("%d components", nc);
            if (nc == 3) {
                if (!jfif) {
                    if (adobe >= 0 && adobe != 1) FULL_UNSUPPORTED("Adobe transform %d (not Y Cb Cr)", adobe);
                    if (adobe < 0 && comps[0] == 'R' && comps[3] == 'G' && comps[6] == 'B') FULL_UNSUPPORTED("component ids R G B (not Y Cb Cr)");
                }
                const int s0 = comps[1];
                if ((s0 != 0x11 && s0 != 0x21 && s0 != 0x22) || comps[4] != 0x11 || comps[7] != 0x11)
                    FULL_UNSUPPORTED("sampling factors %dx%d,%dx%d,%dx%d", comps[1] >> 4, comps[1] & 15, comps[4] >> 4, comps[4] & 15, comps[7] >> 4, comps[7] & 15);
                p.hs = s0 >> 4;
                p.vs = s0 & 15;
            } else {
                p.hs = p.vs = 1;                                // (a single component is coded block by block whatever its factors say)
            }
            p.mcus_x = (p.w + 8 * p.hs - 1) / (8 * p.hs);
            p.mcus_y = (p.h + 8 * p.vs - 1) / (8 * p.vs);
            p.blocks_per_mcu = nc == 3 ? p.hs * p.vs + 2 : 1;
            p.expected_blocks = (uint32_t)p.mcus_x * (uint32_t)p.mcus_y * (uint32_t)p.blocks_per_mcu;
            p.restart_interval = restart;
        }
        if (fp.scans == (uint32_t)FULL_MAX_SCANS) FULL_UNSUPPORTED("more than %d scans", FULL_MAX_SCANS);
        if (e - a < 1 || d[a] < 1 || d[a] > nc || e - a != 4 + 2 * (size_t)d[a]) FULL_UNSUPPORTED("malformed SOS");
        const int ns = d[a];
        FullScan& s = fp.scan[fp.scans];
        s.ss = d[e - 3]; s.se = d[e - 2]; s.ah = d[e - 1] >> 4; s.al = d[e - 1] & 15;
        if (s.ss == 0) {
            if (s.se != 0) FULL_UNSUPPORTED("illegal script: scan %u mixes DC and AC (Ss=0 Se=%d)", fp.scans, s.se);
        } else {
            if (s.ss > s.se || s.se > 63) FULL_UNSUPPORTED("illegal script: scan %u has Ss=%d Se=%d", fp.scans, s.ss, s.se);
            if (ns != 1) FULL_UNSUPPORTED("illegal script: AC scan %u holds %d components", fp.scans, ns);
        }
        if (s.al > 13 || s.ah > 13) FULL_UNSUPPORTED("illegal script: scan %u has Ah=%d Al=%d", fp.scans, s.ah, s.al);
        const int kind = full_kind(s);
        int prev = -1;
        for (int i = 0; i < ns; ++i) {
            int c = 0;
            while (c < nc && comps[3 * c] != d[a + 1 + 2 * i]) ++c;
            if (c == nc || c <= prev) FULL_UNSUPPORTED("scan components out of frame order");
            prev = c;
            s.comps |= (uint8_t)(1u << c);
            const int td = d[a + 2 + 2 * i] >> 4, ta = d[a + 2 + 2 * i] & 15;
            if (kind == K_DC_FIRST) {
                if (td > 3 || !dht_off[0][td]) FULL_UNSUPPORTED("component %d names a Huffman table that is not defined", c);
                s.dc_off[c] = dht_off[0][td]; s.dc_count[c] = dht_count[0][td];
            } else if (kind >= K_AC_FIRST) {
                if (ta > 3 || !dht_off[1][ta]) FULL_UNSUPPORTED("component %d names a Huffman table that is not defined", c);
                s.ac_off[c] = dht_off[1][ta]; s.ac_count[c] = dht_count[1][ta];
            }
            if (s.ss && prog[c][0] < 0) FULL_UNSUPPORTED("illegal script: AC scan %u of component %d before its DC scan", fp.scans, c);
            for (int k = s.ss; k <= s.se; ++k) {
                if (prog[c][k] < 0 ? s.ah != 0 : (s.ah != prog[c][k] || s.al + 1 != s.ah))
                    FULL_UNSUPPORTED("illegal script: scan %u has Ah=%d Al=%d for coefficient %d of component %d, which stands at %d", fp.scans, s.ah, s.al, k, c, prog[c][k]);
                prog[c][k] = (int8_t)s.al;
            }
            if (kind == K_DC_FIRST) {                           // the component's first scan: its quantisation table is latched here
                if (comps[3 * c + 2] > 3 || !dqt[comps[3 * c + 2]]) FULL_UNSUPPORTED("component %d names a quantisation table that is not defined", c);
                p.dqt_off[c] = dqt[comps[3 * c + 2]];
            }
        }
        s.restart_interval = restart;
        s.off = (uint32_t)e;
        size_t q = e;
        for (; q < n; ++q)
            if (d[q] == 0xFF && q + 1 < n && d[q + 1] != 0 && !(d[q + 1] >= 0xD0 && d[q + 1] <= 0xD7)) break;
        if (q == n) FULL_UNSUPPORTED("truncated: scan %u runs to the end of the file (no EOI)", fp.scans);
        if (q == e) FULL_UNSUPPORTED("truncated: no entropy-coded data behind SOS");
        total += q - e;
        if (total >= DEC_MAX_SCAN) FULL_UNSUPPORTED("entropy-coded segments of %llu bytes", total);
        s.len = (uint32_t)(q - e);
        dec_subsequences(s.len, &s.subsequence_bytes, &s.subsequences);
        if (!fp.scans) p.scan_off = s.off;
        if (s.subsequences > p.subsequences || (s.subsequences == p.subsequences && s.subsequence_bytes > p.subsequence_bytes)) {
            p.subsequences = s.subsequences; p.subsequence_bytes = s.subsequence_bytes;
        }
        ++fp.scans;
        pos = q;
    }
    p.scan_len = (uint32_t)total;
    for (int c = 0; c < nc; ++c)
        for (int k = 0; k < 64; ++k)
            if (prog[c][k] != 0)
                FULL_UNSUPPORTED("incomplete script: coefficient %d of component %d %s", k, c, prog[c][k] < 0 ? "is never coded" : "is not refined to its last bit");
    *out = fp;
    return FRCNN_OK;
}

}  // namespace
}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_jpeg_dec_full_version(void) { return FRCNN_JPEG_DEC_FULL_VERSION; }

extern "C" int frcnn_jpeg_dec_full_plan(const uint8_t* file_host, size_t len, frcnn_jpeg_dec_full_plan_t* plan) {
    if (!plan || (!file_host && len)) return fail(FRCNN_E_ARG, "jpeg_dec_full_plan: null pointer");
    return full_plan(file_host, len, plan);
}

extern "C" size_t frcnn_jpeg_dec_full_workspace_bytes(const frcnn_jpeg_dec_full_plan_t* plan) {
    if (!plan || full_plan_fault(*plan)) return 0;
    return dec_layout(plan->frame).total;
}

extern "C" size_t frcnn_jpeg_dec_full_batch_layout(const frcnn_jpeg_dec_full_plan_t* plans, int n, uint64_t* ws_off) {
    if (!plans || !ws_off || n < 1 || n > FRCNN_JPEG_DEC_BATCH_MAX) return 0;
    for (int i = 0; i < n; ++i)
        if (full_plan_fault(plans[i])) return 0;
    size_t at = 0;
    for (int i = 0; i < n; ++i) { ws_off[i] = at; at += dec_layout(plans[i].frame).total; }
    return at;
}

extern "C" int frcnn_jpeg_decode_full_batch_u8(const frcnn_jpeg_dec_full_batch_item_t* items_host, const frcnn_jpeg_dec_full_batch_item_t* items_dev, int n,
                                               const uint8_t* files_dev, size_t files_capacity, int bgr, uint8_t* out_dev, size_t out_capacity,
                                               int32_t* status_dev, void* workspace, size_t workspace_capacity, void* stream) {
    if (!items_host || !items_dev || !files_dev || !out_dev || !status_dev || !workspace) return fail(FRCNN_E_ARG, "jpeg_decode_full_batch_u8: null pointer");
    if (n < 1 || n > FRCNN_JPEG_DEC_BATCH_MAX) return fail(FRCNN_E_ARG, "jpeg_decode_full_batch_u8: n=%d outside 1..%d", n, FRCNN_JPEG_DEC_BATCH_MAX);
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return fail(FRCNN_E_ARG, "jpeg_decode_full_batch_u8: workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(status_dev) & 3u) return fail(FRCNN_E_ARG, "jpeg_decode_full_batch_u8: status_dev must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(items_dev) & 7u) return fail(FRCNN_E_ARG, "jpeg_decode_full_batch_u8: items_dev must be 8-byte aligned");
    Range outs[FRCNN_JPEG_DEC_BATCH_MAX], regions[FRCNN_JPEG_DEC_BATCH_MAX];
    uint32_t blocks = 1;
    int max_w = 1, max_h = 1;
    for (int i = 0; i < n; ++i) {
        const FullItem& it = items_host[i];
        const Plan& p = it.plan.frame;
        if (const char* what = full_plan_fault(it.plan)) return fail(FRCNN_E_ARG, "jpeg_decode_full_batch_u8: item %d: the plan contradicts itself (%s)", i, what);
        const unsigned long long frame = (unsigned long long)p.h * p.w * 3, need = dec_layout(p).total;
        if (it.file_off > files_capacity || p.file_len > files_capacity - it.file_off)
            return fail(FRCNN_E_ARG, "jpeg_decode_full_batch_u8: item %d: file_off=%llu + file_len=%u beyond files_capacity=%zu", i, (unsigned long long)it.file_off, p.file_len, files_capacity);
        if (it.out_off > out_capacity || frame > out_capacity - it.out_off)
            return fail(FRCNN_E_ARG, "jpeg_decode_full_batch_u8: item %d: out_off=%llu + %d * %d * 3 beyond out_capacity=%zu", i, (unsigned long long)it.out_off, p.h, p.w, out_capacity);
        if (it.ws_off & 15u) return fail(FRCNN_E_ARG, "jpeg_decode_full_batch_u8: item %d: ws_off=%llu must be 16-byte aligned", i, (unsigned long long)it.ws_off);
        if (it.ws_off > workspace_capacity || need > workspace_capacity - it.ws_off)
            return fail(FRCNN_E_ARG, "jpeg_decode_full_batch_u8: item %d: ws_off=%llu + %llu beyond workspace_capacity=%zu", i, (unsigned long long)it.ws_off, need, workspace_capacity);
        outs[i] = {it.out_off, it.out_off + frame, i};
        regions[i] = {it.ws_off, it.ws_off + need, i};
        blocks = p.expected_blocks > blocks ? p.expected_blocks : blocks;
        max_w = p.w > max_w ? p.w : max_w;
        max_h = p.h > max_h ? p.h : max_h;
    }
    int k = range_overlap(outs, n);
    if (k >= 0) return fail(FRCNN_E_ARG, "jpeg_decode_full_batch_u8: the output ranges of items %d and %d overlap", outs[k].item, outs[k + 1].item);
    k = range_overlap(regions, n);
    if (k >= 0) return fail(FRCNN_E_ARG, "jpeg_decode_full_batch_u8: the workspace regions of items %d and %d overlap", regions[k].item, regions[k + 1].item);
    hipStream_t s = as_stream(stream);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    const unsigned groups = (blocks + DEC_IDCT_BLOCKS - 1) / DEC_IDCT_BLOCKS;
    k_jpeg_full_zero<<<dim3(groups, n), DEC_IDCT_THREADS, 0, s>>>(items_dev, ws);
    k_jpeg_full_entropy<<<n, DEC_MAX_LANES, 0, s>>>(files_dev, items_dev, ws, status_dev);
    k_jpeg_full_idct<<<dim3(groups, n), DEC_IDCT_THREADS, 0, s>>>(files_dev, items_dev, ws);
    k_jpeg_full_colour<<<dim3((max_w + DEC_COLOUR_THREADS - 1) / DEC_COLOUR_THREADS, max_h, n), DEC_COLOUR_THREADS, 0, s>>>(items_dev, ws, bgr ? 1 : 0, out_dev);
    return check_launch("jpeg_decode_full_batch_u8");
}

extern "C" int frcnn_jpeg_decode_full_u8(const uint8_t* file_dev, const frcnn_jpeg_dec_full_plan_t* plan, const frcnn_jpeg_dec_full_batch_item_t* item_dev,
                                         int bgr, uint8_t* out, size_t out_capacity, int32_t* status_dev, void* workspace, size_t workspace_capacity,
                                         void* stream) {
    if (!plan) return fail(FRCNN_E_ARG, "jpeg_decode_full_u8: null pointer");
    static thread_local FullItem item;
    item = FullItem{};
    item.plan = *plan;
    return frcnn_jpeg_decode_full_batch_u8(&item, item_dev, 1, file_dev, plan->frame.file_len, bgr, out, out_capacity, status_dev, workspace,
                                           workspace_capacity, stream);
}
