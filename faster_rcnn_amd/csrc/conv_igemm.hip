// Implicit-GEMM NHWC convolution on the CDNA4 matrix cores (gfx950), f32 in / f32 accumulate.
//
// Replaces Keras Conv2D (+bias) / BatchNormalization(training=False) / Scale / Activation /
// add in resnet.py:150-176, 218-247, 408-412, 464-474, 508-533 and vgg.py:96-137, 172-185,
// 233-247 (Dense = 1x1 conv on a 1x1 map).
//
// GEMM view:  Y[m][n] = sum_k A[m][k] * Wt[n][k]
//   m = (img, ho, wo) output pixel, n = output channel, k = (channel chunk, filter tap (r,s), channel in chunk).
//   A is never materialised (no im2col): for one 32-wide k-chunk inside a single filter tap
//   (r,s) the A row of pixel m is the 128 contiguous bytes x[img][ho*st+r-pt][wo*st+s-pl][c0..c0+32)
//   of the NHWC input, or zeros in the padding halo.
//   Wt is the filter pre-packed to [Cout][Kpad] (k contiguous), so both operands are
//   "row-major, k contiguous" and share one LDS image + one fragment-read pattern.
//
// Workgroup = 256 threads = 4 wave64 in a 2x2 arrangement; each wave owns TM x TN tiles of
// 32x32 outputs (v_mfma_f32_32x32x2_f32: lane l supplies A[i=l&31][k=l>>5], B[k=l>>5][j=l&31],
// 16 accumulator VGPRs per tile).  One ds_read_b128 per operand tile yields FOUR mfma k-steps
// (lane half h reads k = 8*kk + 4h .. +3; step j multiplies k=8kk+j (h=0) and 8kk+4+j (h=1)),
// so a 32-deep chunk costs (TM+TN)*4 LDS reads for TM*TN*16 MFMAs.  LDS rows are padded to 36
// floats (144 B): the 16-lane ds_read_b128 groups then hit 16 distinct 4-bank slots.
// Global->LDS staging is register double-buffered: loads for chunk t+1 are issued before
// the MFMAs of chunk t and written to the other LDS buffer after them; one barrier per chunk.
// The blockIdx -> tile map is XCD-aware (8 XCDs round-robin on blockIdx): each XCD walks a
// contiguous run of m-tiles of ONE n-tile so that n-tile's filter slice stays in its 4 MB L2.
//
// Epilogue (fused, in registers): v = acc*scale[n] + shift[n] (folded bias+BN(+Scale)),
// + residual[m][n], activation (none / relu / sigmoid), store NHWC.
#include "conv_f32_common.h"
#include "conv_policy.h"
#include "../../include/ext/frcnn_hip_roi_res.h"
#include "../../include/ext/frcnn_hip_pool_epilogue.h"
#include "../../include/ext/frcnn_hip_rowmap.h"

namespace frcnn {

template <int TM, int TN, bool GENERIC_A>
__global__ void __launch_bounds__(256) k_conv_igemm_f32(const ConvArgs p) {
    constexpr int BM = 64 * TM, BN = 64 * TN;
    constexpr int PA = BM / 32, PB = BN / 32;          // float4 rows staged per thread
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                                   // [2][BM][LDS_STRIDE]
    float* Bs = smem + 2 * BM * LDS_STRIDE;             // [2][BN][LDS_STRIDE]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, lh = lane >> 5;

    const int nwg = p.tiles_m * p.tiles_n;
    const int logical = xcd_remap(blockIdx.x, nwg);
    const int tile_n = logical / p.tiles_m, tile_m = logical - tile_n * p.tiles_m;
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    // ---- per-thread staging coordinates
    const int lrow = tid >> 3, lcol = (tid & 7) * 4;
    int a_h[PA], a_w[PA];
    size_t a_img[PA];
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        const int m = m0 + lrow + 32 * i;
        if (m < p.M) {
            const int wo = m % p.Wo, t = m / p.Wo, ho = t % p.Ho, img = t / p.Ho;
            a_h[i] = ho * p.stride - p.pad_top;
            a_w[i] = wo * p.stride - p.pad_left;
            a_img[i] = (size_t)img * p.H * p.W * p.Cin;
        } else {
            a_h[i] = -(1 << 28); a_w[i] = 0; a_img[i] = 0;
        }
    }
    const float* b_ptr[PB];
    bool b_ok[PB];
#pragma unroll
    for (int i = 0; i < PB; ++i) {
        const int n = n0 + lrow + 32 * i;
        b_ok[i] = n < p.Cout;
        b_ptr[i] = p.w + (size_t)(b_ok[i] ? n : 0) * p.Kpad + lcol;
    }

    f32x4 ra[PA], rb[PB];
    int r_tap = 0, s_tap = 0, c0 = 0;                   // filter tap / channel offset of the NEXT chunk to load

    auto load_chunk = [&](int kc) {
#pragma unroll
        for (int i = 0; i < PB; ++i)
            rb[i] = b_ok[i] ? *reinterpret_cast<const f32x4*>(b_ptr[i] + kc * BK) : f32x4{0, 0, 0, 0};
        if constexpr (!GENERIC_A) {
#pragma unroll
            for (int i = 0; i < PA; ++i) {
                const int hi = a_h[i] + r_tap, wi = a_w[i] + s_tap;
                const bool ok = (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
                const float* src = p.x + a_img[i] + ((size_t)hi * p.W + wi) * p.Cin + c0 + lcol;
                ra[i] = ok ? *reinterpret_cast<const f32x4*>(src) : f32x4{0, 0, 0, 0};
            }
            // k order = [channel chunk][tap][32 channels]: consecutive chunks re-read the SAME 128-byte
            // channel slice of neighbouring pixels, so the 9 taps of a 3x3 hit L1/L2 instead of streaming
            // the whole input tile 9 times (measured: 46 % L2 hit rate and ~1 GB fetched per launch before)
            if (++s_tap == p.S) { s_tap = 0; if (++r_tap == p.R) { r_tap = 0; c0 += BK; } }
        } else {
            // small-Cin path (stem, Cin=3): decode every k separately
#pragma unroll
            for (int i = 0; i < PA; ++i) {
                f32x4 v = {0, 0, 0, 0};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = kc * BK + lcol + e;
                    if (k < p.K) {
                        const int c = k % p.Cin, rs = k / p.Cin, s = rs % p.S, r = rs / p.S;
                        const int hi = a_h[i] + r, wi = a_w[i] + s;
                        if ((unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W)
                            v[e] = p.x[a_img[i] + ((size_t)hi * p.W + wi) * p.Cin + c];
                    }
                }
                ra[i] = v;
            }
        }
    };
    auto store_chunk = [&](int buf) {
        float* a = As + buf * BM * LDS_STRIDE;
        float* b = Bs + buf * BN * LDS_STRIDE;
#pragma unroll
        for (int i = 0; i < PA; ++i) *reinterpret_cast<f32x4*>(a + (lrow + 32 * i) * LDS_STRIDE + lcol) = ra[i];
#pragma unroll
        for (int i = 0; i < PB; ++i) *reinterpret_cast<f32x4*>(b + (lrow + 32 * i) * LDS_STRIDE + lcol) = rb[i];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

    const int nk = p.Kpad / BK;
    load_chunk(0);
    store_chunk(0);
    __syncthreads();

    for (int kc = 0; kc < nk; ++kc) {
        const int buf = kc & 1;
        if (kc + 1 < nk) load_chunk(kc + 1);
        const float* a = As + buf * BM * LDS_STRIDE + (wm * TM * 32 + li) * LDS_STRIDE + lh * 4;
        const float* b = Bs + buf * BN * LDS_STRIDE + (wn * TN * 32 + li) * LDS_STRIDE + lh * 4;
#pragma unroll
        for (int kk = 0; kk < BK / 8; ++kk) {
            f32x4 fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[i] = *reinterpret_cast<const f32x4*>(a + i * 32 * LDS_STRIDE + kk * 8);
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = *reinterpret_cast<const f32x4*>(b + j * 32 * LDS_STRIDE + kk * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][e], fb[j][e], acc[i][j], 0, 0, 0);
        }
        if (kc + 1 < nk) store_chunk(buf ^ 1);
        __syncthreads();
    }

    epilogue<TM, TN>(acc, p, m0, n0, wm, wn, li, lh);
}

// ------------------------------------------------------------------------------------
// v2 main loop: branch-free and software-pipelined inside ONE wave.
//   * operands come through buffer loads (SRD + 32-bit offsets): padding halo, m >= M and
//     n >= Cout rows simply carry an out-of-range offset and read back zeros, so the loop
//     body is a single basic block the scheduler may interleave freely;
//   * sched_group_barrier pins the interleave: the next chunk's 8 global loads ride behind
//     the first MFMAs, each kk-step's fragment reads behind the previous step's MFMAs and
//     the LDS stores behind the last MFMAs.  A 32x32x2 f32 MFMA occupies the matrix pipe
//     for 64 cycles but the wave's issue port only briefly, so those VALU/VMEM/DS
//     instructions issue in the shadow of the wave's own MFMAs instead of in a separate
//     phase (v1: matrix pipe 79 % busy on a 2-wave SIMD, both waves stalling in lockstep).
// Lab builds (scripts/micro/conv_lab.hip) compile this file with FRCNN_LAB_STAMPS: every workgroup then records
// the 100 MHz wall clock at its phase boundaries.  The product library never defines it.
#ifdef FRCNN_LAB_STAMPS
__device__ unsigned long long* g_lab_stamps = nullptr;
#define LAB_STAMP(i) do { if (g_lab_stamps && threadIdx.x == 0) g_lab_stamps[(size_t)blockIdx.x * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define LAB_STAMP(i) do { } while (0)
#endif
//
// SPLITK: small grids (stage 4, the RPN heads, the dense layers: <= 152 tiles for 256 CUs and a long k loop)
// cut K into `splits` slices, one workgroup each.  Every slice writes its f32 partial tile to a slab, publishes
// it with ONE agent-scope release and draws a ticket; the workgroup that draws the last ticket acquires, sums
// the slabs in slice order (fixed order: two runs are bitwise equal) and runs the fused epilogue.  One launch,
// no atomics on data (cdna guide s5 "in-launch split-K reduction").
//
// CIN3: the 3-channel stems (ResNet conv1 7x7, VGG block1_conv1 3x3).  The filter is packed as if the image had FOUR
// channels (k = tap*4 + c, c == 3 a zero column, see packed_k), so a 32-wide chunk is eight taps and each of the eight
// lanes that stage a row fetches ITS tap of its pixel with one 12-byte buffer load (per-lane r, s instead of the
// wave-uniform tap walk) and appends a zero.  Taps beyond R*S load nothing.  Replaces the per-element gather of the
// v1 kernel for these layers.
template <int TM, int TN, int VARIANT = 0, int WM = 2, int WN = 2, bool SPLITK = false, bool CIN3 = false>
__global__ void __launch_bounds__(64 * WM * WN) k_conv_igemm_f32_v2(const ConvArgs p) {
    // WM x WN waves, each owning TM x TN 32x32 tiles.  2x2 waves (256 threads) is the base shape; 4x2 waves
    // (512 threads) on the same 128x128 tile halves the registers per wave so FOUR waves share a SIMD
    // instead of two and a wave's barrier / LDS-latency gaps are covered by three partners.
    constexpr int NT = 64 * WM * WN;
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    constexpr int RPP = NT / 8;                          // tile rows staged per pass (8 lanes x 16 B per row)
    constexpr int PA = BM / RPP, PB = BN / RPP;
    static_assert(BM % RPP == 0 && BN % RPP == 0, "tile rows must be a multiple of the staging pass");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;
    float* Bs = smem + 2 * BM * LDS_STRIDE;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int li = lane & 31, lh = lane >> 5;
    LAB_STAMP(0);

    const int splits = SPLITK ? p.splits : 1;
    const int nwg = p.tiles_m * p.tiles_n * splits;
    const int logical = xcd_remap(blockIdx.x, nwg);
    const int tile = SPLITK ? logical / splits : logical;          // a tile's slices are neighbours on one XCD
    const int slice = SPLITK ? logical - tile * splits : 0;
    int tile_n = tile / p.tiles_m, tile_m = tile - tile_n * p.tiles_m;
    if (p.group_m > 0) {
        // Grouped order.  An XCD's workgroups hold a contiguous run of ids (xcd_remap), ~128 tiles at a time.  In the plain
        // order those are 128 ROW tiles of one column tile: the filter slice is shared, every A tile is its own
        // (1x1 512->2048 on the head's 14 700 rows: 128 x 128 KB = 16 MB live per 4 MB L2, A streamed from beyond L2 once
        // per column tile, ~0.9 GB per launch).  Grouped, the run is g row tiles x 128/g column tiles: (g + 128/g) tiles of
        // operands live, each fetched once per group.
        const int per = p.group_m * p.tiles_n, g = tile / per, m_base = g * p.group_m;
        const int gm = min(p.group_m, p.tiles_m - m_base), r = tile - g * per;
        tile_n = r / gm;
        tile_m = m_base + r - tile_n * gm;
    }
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.x), 0, (int)((size_t)p.n_img * p.H * p.W * p.Cin * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.w), 0, (int)((size_t)p.Cout * p.Kpad * 4), 0x00020000);

    const int lrow = tid >> 3, lcol = (tid & 7) * 4;
    int a_h[PA], a_w[PA], a_off[PA];
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        const int m = m0 + lrow + RPP * i;
        if (m < p.M) {
            int wo, ho, img;
            if (p.layout) { img = m % p.n_img; const int pos = m / p.n_img; ho = pos / p.Wo; wo = pos - ho * p.Wo; }
            else { wo = m % p.Wo; const int t = m / p.Wo; ho = t % p.Ho; img = t / p.Ho; }
            a_h[i] = ho * p.stride - p.pad_top;
            a_w[i] = wo * p.stride - p.pad_left;
            a_off[i] = (img * p.img_stride + (a_h[i] * p.W + a_w[i]) * p.pix_stride + (CIN3 ? 0 : lcol)) * 4;     // may be "negative" in the halo
        } else {
            a_h[i] = -(1 << 28); a_w[i] = 0; a_off[i] = 0;
        }
    }
    unsigned b_off[PB];
#pragma unroll
    for (int i = 0; i < PB; ++i) {
        const int n = n0 + lrow + RPP * i;
        b_off[i] = n < p.Cout ? (unsigned)((n * p.Kpad + lcol) * 4) : OOB_OFFSET;
    }

    // Filter taps this tile needs, one bit per tap.  With position-major rows (layout 1: the detector head's
    // [7][7][roi][c] tensors) a 128-row tile spans one or two output positions, so the taps that fall into the
    // zero padding for ALL of them -- 14 % of the chunks of a 3x3 SAME conv on 7x7 maps -- are skipped outright;
    // they would only add exact zeros, so the result is bit-identical.
    const int RS = p.R * p.S;
    const unsigned all_taps = RS >= 32 ? 0xffffffffu : (1u << RS) - 1u;
    unsigned tap_mask = all_taps;
    if (p.layout) {
        const int pos_lo = m0 / p.n_img, pos_hi = (min(m0 + BM, p.M) - 1) / p.n_img;
        if (pos_hi - pos_lo < 8) {
            unsigned mk = 0;
            for (int pos = pos_lo; pos <= pos_hi; ++pos) {
                const int ho = pos / p.Wo, wo = pos - ho * p.Wo;
                const int h0 = ho * p.stride - p.pad_top, w0 = wo * p.stride - p.pad_left;
                for (int r = 0; r < p.R; ++r)
                    for (int sx = 0; sx < p.S; ++sx)
                        if ((unsigned)(h0 + r) < (unsigned)p.H && (unsigned)(w0 + sx) < (unsigned)p.W) mk |= 1u << (r * p.S + sx);
            }
            if (mk) tap_mask = mk;
        }
    }
    const int n_taps = __popc(tap_mask);

    // this workgroup's chunk range [kb, ke) of the (channel group, needed tap) sequence
    const int nk_all = CIN3 ? p.Kpad / BK : (p.Kpad / (BK * RS)) * n_taps;
    const int kb = SPLITK ? (int)((long long)slice * nk_all / splits) : 0;
    const int ke = SPLITK ? (int)((long long)(slice + 1) * nk_all / splits) : nk_all;

    unsigned rem = tap_mask;                                 // taps of the current channel group still to load
    int c0 = 0, w_grp = 0;                                   // channel offset / byte offset of the group's filter chunks
    if (SPLITK) {
        const int grp = kb / n_taps;
        c0 = grp * BK; w_grp = grp * RS * (BK * 4);
        for (int t = kb - grp * n_taps; t > 0; --t) rem &= rem - 1;
    }
    int kc3 = kb;                                            // CIN3: next chunk (of eight taps) to load
    // the NEXT chunk of this workgroup's sequence -> a set of staging registers (calls walk the sequence in order; calls
    // past the end of the range fetch in-bounds or zero data that is never multiplied)
    auto load_into = [&](i32x4 (&xa)[PA], i32x4 (&xb)[PB]) {
        if constexpr (CIN3) {
            const int tap = kc3 * 8 + (tid & 7);             // per lane: this lane's tap of the chunk
            const int r_tap = (tap * p.inv_S) >> 16, s_tap = tap - r_tap * p.S;
            const int tap_off = (r_tap * p.W + s_tap) * 12;  // 3 channels x 4 bytes per pixel
#pragma unroll
            for (int i = 0; i < PB; ++i)
                xb[i] = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, b_off[i], kc3 * (BK * 4), 0);
#pragma unroll
            for (int i = 0; i < PA; ++i) {
                const int hi = a_h[i] + r_tap, wi = a_w[i] + s_tap;
                const bool ok = tap < RS && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
                const i32x3 v = __builtin_amdgcn_raw_buffer_load_b96(xrsrc, ok ? (unsigned)(a_off[i] + tap_off) : OOB_OFFSET, 0, 0);
                xa[i] = i32x4{v[0], v[1], v[2], 0};
            }
            ++kc3;
            return;
        }
        const int tap = __builtin_ctz(rem);                  // wave-uniform
        const int r_tap = (tap * p.inv_S) >> 16, s_tap = tap - r_tap * p.S;
        const int tap_off = ((r_tap * p.W + s_tap) * p.pix_stride + c0) * 4;
        const int w_off = w_grp + tap * (BK * 4);
#pragma unroll
        for (int i = 0; i < PB; ++i)
            xb[i] = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, b_off[i], w_off, 0);
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            const int hi = a_h[i] + r_tap, wi = a_w[i] + s_tap;
            const bool ok = (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
            xa[i] = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, ok ? (unsigned)(a_off[i] + tap_off) : OOB_OFFSET, 0, 0);
        }
        // branch-free walk to the next needed tap (a scalar branch here would split the loop body into two
        // scheduling regions and undo the interleave below)
        rem &= rem - 1;
        const int wrap = (rem == 0);
        rem |= wrap ? tap_mask : 0u;
        c0 += wrap * BK;
        w_grp += wrap * (RS * BK * 4);
    };
    auto store_from = [&](const i32x4 (&xa)[PA], const i32x4 (&xb)[PB], int buf) {
        float* a = As + buf * BM * LDS_STRIDE;
        float* b = Bs + buf * BN * LDS_STRIDE;
#pragma unroll
        for (int i = 0; i < PA; ++i) *reinterpret_cast<i32x4*>(a + (lrow + RPP * i) * LDS_STRIDE + lcol) = xa[i];
#pragma unroll
        for (int i = 0; i < PB; ++i) *reinterpret_cast<i32x4*>(b + (lrow + RPP * i) * LDS_STRIDE + lcol) = xb[i];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

    // the residual pieces this thread will add in the vector epilogue, requested now: a 64x64 tile's main loop is a few
    // microseconds, about as long as the fetch
    using EV = EpiVec<TM, TN, WM, WN>;
    constexpr bool EPI_PRE = EV::fits && !SPLITK && TM * TN == 1;
    f32x4 rpre[EPI_PRE ? EV::PASSES : 1];
    if constexpr (EPI_PRE) {
        if (p.vec_epi) epi_prefetch_residual<TM, TN, WM, WN>(p, m0, n0, tid, rpre);
    }

    constexpr int MF = TM * TN * 4;        // MFMAs per kk-step
    constexpr int NL = PA + PB;            // global loads == LDS stores per chunk per thread
    constexpr int NF = TM + TN;            // fragment reads per kk-step
    if constexpr (VARIANT == 2) {
        // ---- VARIANT 2: the barrier sits in the MIDDLE of a chunk and nothing waits behind it.
        // In VARIANTs 0/1 every chunk ends [LDS stores -> barrier -> first fragment reads -> first MFMA]: a wave alone
        // on its SIMD (stage-4 grids: one or two workgroups per CU) idles the matrix pipe for that whole chain -- timed
        // at 1 700 cycles per 1 024-cycle chunk (scripts/micro/conv_lab.hip, stamps).  Here chunk T is multiplied as
        //   first half : MFMAs of k-steps 0,1 (step-0 fragments were read during chunk T-1); fragment reads of steps 1..3
        //   barrier    : all waves have finished READING buffer T%2 and their stores of chunk T+1 (made during the
        //                second half of chunk T-1) are visible
        //   second half: MFMAs of k-steps 2,3; LDS stores of chunk T+2 into buffer T%2; fragment reads of chunk T+1's
        //                step 0; global loads of chunk T+4
        // so the operands of the MFMAs that follow the barrier are already in registers, the stores and the next reads
        // ride in the shadow of k-steps 2,3, and a chunk's global loads have TWO chunks of MFMA time to land (two
        // staging register sets; same two LDS buffers as before).
        // staging register sets: two for the 64-wide tiles (a chunk's loads get two chunks of MFMA time), one for the
        // big tiles (a 128x128 chunk is 4 096 MFMA cycles per wave: one chunk of lead is plenty, and the registers are needed)
        constexpr int SETS = TM * TN == 1 ? 2 : 1;
        i32x4 sa0[PA], sb0[PB], sa1[SETS == 2 ? PA : 1], sb1[SETS == 2 ? PB : 1];
        f32x4 na[TM], nb[TN];                                  // step-0 fragments of the chunk about to start
        load_into(sa0, sb0);                                   // chunk 0
        if constexpr (SETS == 2) {
            load_into(sa1, sb1);                               // chunk 1
            store_from(sa0, sb0, 0);
            load_into(sa0, sb0);                               // chunk 2
            store_from(sa1, sb1, 1);
            load_into(sa1, sb1);                               // chunk 3
        } else {
            store_from(sa0, sb0, 0);
            load_into(sa0, sb0);                               // chunk 1
            store_from(sa0, sb0, 1);
            load_into(sa0, sb0);                               // chunk 2
        }
        __syncthreads();
        LAB_STAMP(1);
        {
            const float* a = As + (wm * TM * 32 + li) * LDS_STRIDE + lh * 4;
            const float* b = Bs + (wn * TN * 32 + li) * LDS_STRIDE + lh * 4;
#pragma unroll
            for (int i = 0; i < TM; ++i) na[i] = *reinterpret_cast<const f32x4*>(a + i * 32 * LDS_STRIDE);
#pragma unroll
            for (int j = 0; j < TN; ++j) nb[j] = *reinterpret_cast<const f32x4*>(b + j * 32 * LDS_STRIDE);
        }
        auto chunk = [&](auto parity, auto& xa, auto& xb) {
            constexpr int P = decltype(parity)::value;
            const float* a = As + P * BM * LDS_STRIDE + (wm * TM * 32 + li) * LDS_STRIDE + lh * 4;
            const float* b = Bs + P * BN * LDS_STRIDE + (wn * TN * 32 + li) * LDS_STRIDE + lh * 4;
            const float* an = As + (P ^ 1) * BM * LDS_STRIDE + (wm * TM * 32 + li) * LDS_STRIDE + lh * 4;
            const float* bn = Bs + (P ^ 1) * BN * LDS_STRIDE + (wn * TN * 32 + li) * LDS_STRIDE + lh * 4;
            f32x4 fa[BK / 8][TM], fb[BK / 8][TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[0][i] = na[i];
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[0][j] = nb[j];
#pragma unroll
            for (int kk = 1; kk < BK / 8; ++kk) {
#pragma unroll
                for (int i = 0; i < TM; ++i) fa[kk][i] = *reinterpret_cast<const f32x4*>(a + i * 32 * LDS_STRIDE + kk * 8);
#pragma unroll
                for (int j = 0; j < TN; ++j) fb[kk][j] = *reinterpret_cast<const f32x4*>(b + j * 32 * LDS_STRIDE + kk * 8);
            }
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[kk][i][e], fb[kk][j][e], acc[i][j], 0, 0, 0);
            SGB(SG_DS_RD, NF);                                       // step-1 fragments first
#pragma unroll
            for (int q = 0; q < MF; ++q) {                           // k-step 0: the step-2,3 fragment reads behind its MFMAs
                SGB(SG_MFMA, 1);
                if (q < NF) SGB(SG_DS_RD, 2);
            }
#pragma unroll
            for (int q = 0; q < MF; ++q) SGB(SG_MFMA, 1);            // k-step 1
            __builtin_amdgcn_sched_barrier(0);                       // k-steps 0,1 stay in FRONT of the barrier: its wait then falls behind 8 queued MFMAs
            __syncthreads();
            store_from(xa, xb, P);                                   // chunk T+2 -> the buffer every wave has just finished reading
            load_into(xa, xb);                                       // chunk T+4
#pragma unroll
            for (int i = 0; i < TM; ++i) na[i] = *reinterpret_cast<const f32x4*>(an + i * 32 * LDS_STRIDE);
#pragma unroll
            for (int j = 0; j < TN; ++j) nb[j] = *reinterpret_cast<const f32x4*>(bn + j * 32 * LDS_STRIDE);
#pragma unroll
            for (int kk = 2; kk < BK / 8; ++kk)
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[kk][i][e], fb[kk][j][e], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int q = 0; q < MF; ++q) {                           // k-step 2: LDS stores, then the next chunk's step-0 reads
                SGB(SG_MFMA, 1);
                if (q < NL) SGB(SG_DS_WR, 1);
            }
            if (NL > MF) SGB(SG_DS_WR, NL - MF);
            SGB(SG_DS_RD, NF);
#pragma unroll
            for (int q = 0; q < MF; ++q) {                           // k-step 3: global loads
                SGB(SG_MFMA, 1);
                if (q < NL) { SGB(SG_VALU, 4); SGB(SG_VMEM_RD, 1); }
            }
        };
        int kc = kb;
        for (; kc + 1 < ke; kc += 2) {
            chunk(std::integral_constant<int, 0>{}, sa0, sb0);
            if constexpr (SETS == 2) chunk(std::integral_constant<int, 1>{}, sa1, sb1);
            else chunk(std::integral_constant<int, 1>{}, sa0, sb0);
        }
        if (kc < ke) chunk(std::integral_constant<int, 0>{}, sa0, sb0);
        __syncthreads();                                             // the epilogue reuses the buffers
    } else {
    i32x4 ra[PA], rb[PB];
    auto load_chunk = [&](int) { load_into(ra, rb); };
    auto store_chunk = [&](int buf) { store_from(ra, rb, buf); };
    // Two-deep operand pipeline: chunk t+2 travels global->registers while chunk t+1 travels
    // registers->LDS and chunk t feeds the MFMAs.  The loads issued in iteration t are consumed
    // (ds_write) at the top of iteration t+1, so they have a whole chunk of MFMA time to land and
    // the compiler cannot sink them next to their use.
    load_chunk(kb);
    store_chunk(0);
    load_chunk(kb + 1 < ke ? kb + 1 : kb);
    __syncthreads();
    LAB_STAMP(1);

    for (int kc = kb; kc < ke; ++kc) {
        const int buf = (kc - kb) & 1;
        if constexpr (VARIANT == 0) {
            store_chunk(buf ^ 1);                              // chunk kc+1 (harmless duplicate at the tail)
            load_chunk(kc + 2 < ke ? kc + 2 : ke - 1);         // always in range: keeps the body branch-free
        }
        const float* a = As + buf * BM * LDS_STRIDE + (wm * TM * 32 + li) * LDS_STRIDE + lh * 4;
        const float* b = Bs + buf * BN * LDS_STRIDE + (wn * TN * 32 + li) * LDS_STRIDE + lh * 4;
        f32x4 fa[BK / 8][TM], fb[BK / 8][TN];
#pragma unroll
        for (int kk = 0; kk < BK / 8; ++kk) {
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[kk][i] = *reinterpret_cast<const f32x4*>(a + i * 32 * LDS_STRIDE + kk * 8);
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[kk][j] = *reinterpret_cast<const f32x4*>(b + j * 32 * LDS_STRIDE + kk * 8);
        }
#pragma unroll
        for (int kk = 0; kk < BK / 8; ++kk)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[kk][i][e], fb[kk][j][e], acc[i][j], 0, 0, 0);

        if constexpr (VARIANT == 0) {
            // ---- pinned interleave (per wave, per chunk): everything that is not an MFMA issues in
            // the shadow of the wave's own MFMAs
            SGB(SG_DS_RD, NF);                                       // kk = 0 fragments
#pragma unroll
            for (int q = 0; q < MF; ++q) {                           // kk-step 0: LDS stores, then kk=1 fragments
                SGB(SG_MFMA, 1);
                if (q < NL) SGB(SG_DS_WR, 1);
                else if (q - NL < NF) SGB(SG_DS_RD, 1);
            }
#pragma unroll
            for (int q = 0; q < MF; ++q) {                           // kk-step 1: global loads, then kk=2 fragments
                SGB(SG_MFMA, 1);
                if (q < NL) { SGB(SG_VALU, 4); SGB(SG_VMEM_RD, 1); }
                else if (q - NL < NF) SGB(SG_DS_RD, 1);
            }
#pragma unroll
            for (int q = 0; q < MF; ++q) {                           // kk-step 2: kk=3 fragments
                SGB(SG_MFMA, 1);
                if (q < NF) SGB(SG_DS_RD, 1);
            }
#pragma unroll
            for (int q = 0; q < MF; ++q) SGB(SG_MFMA, 1);            // kk-step 3
        } else {
            // VARIANT 1: the LDS stores come AFTER all fragment reads in program order (the compiler keeps
            // may-alias LDS accesses ordered), so they can ride behind the last MFMAs instead of sitting in
            // front of the first one; the next loads follow the stores (register reuse) at the tail.
            store_chunk(buf ^ 1);
            load_chunk(kc + 2 < ke ? kc + 2 : ke - 1);
            SGB(SG_DS_RD, NF);
#pragma unroll
            for (int kk = 0; kk < BK / 8 - 1; ++kk) {
#pragma unroll
                for (int q = 0; q < MF; ++q) {
                    SGB(SG_MFMA, 1);
                    if (q < NF) SGB(SG_DS_RD, 1);
                    else if (kk == BK / 8 - 2 && q - NF < NL) SGB(SG_DS_WR, 1);
                }
            }
#pragma unroll
            for (int q = 0; q < MF; ++q) {
                SGB(SG_MFMA, 1);
                if (MF - NF < NL && q < NL - (MF - NF)) SGB(SG_DS_WR, 1);
                else if (q < NL + (MF - NF < NL ? NL - (MF - NF) : 0)) { SGB(SG_VALU, 4); SGB(SG_VMEM_RD, 1); }
            }
        }
        __syncthreads();
    }
    }
    LAB_STAMP(2);
    if constexpr (SPLITK) {
        // publish this slice's partial tile WRITE-THROUGH (sc1 stores need no release fence: cdna guide G16 R1);
        // thread-major 16-B rows, so the stores and the reducer's loads coalesce
        const __amdgpu_buffer_rsrc_t srsrc = __builtin_amdgcn_make_buffer_rsrc(
            p.slabs, 0, (int)((size_t)p.tiles_m * p.tiles_n * splits * (BM * BN) * 4), 0x00020000);
        const unsigned slab_off = (unsigned)((tile * splits + slice) * (BM * BN) * 4 + tid * 16);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    f32x4 v = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, v), srsrc,
                                                           slab_off + ((i * TN + j) * 4 + q) * (NT * 16), 0, 16 /* sc1 */);
                }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // every storing wave drains ...
        __syncthreads();                                       // ... before ONE lane draws the ticket
        int* last = reinterpret_cast<int*>(smem);              // the main loop is done with the (one) LDS array
        if (tid == 0) {
            const unsigned t = __hip_atomic_fetch_add(&p.tickets[tile], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int is_last = (t == (unsigned)(splits - 1));
            if (is_last) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");                 // drop this CU's stale L1 lines
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(&p.tickets[tile], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
            }
            *last = is_last;
        }
        __syncthreads();
        LAB_STAMP(3);
        if (!*last) return;
        const float4* base = reinterpret_cast<const float4*>(p.slabs + (size_t)tile * splits * (BM * BN));
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
        for (int sl = 0; sl < splits; ++sl) {
            const float4* sp = base + (size_t)sl * (BM * BN / 4);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 v = sp[((i * TN + j) * 4 + q) * NT + tid];
                        acc[i][j][4 * q] += v.x; acc[i][j][4 * q + 1] += v.y; acc[i][j][4 * q + 2] += v.z; acc[i][j][4 * q + 3] += v.w;
                    }
        }
        LAB_STAMP(4);
    }
    if constexpr (EV::fits) {
        if (p.vec_epi) epilogue_vec<TM, TN, WM, WN, EPI_PRE>(acc, p, m0, n0, tid, wm, wn, li, lh, smem, rpre);
        else epilogue<TM, TN>(acc, p, m0, n0, wm, wn, li, lh);
    } else {
        epilogue<TM, TN>(acc, p, m0, n0, wm, wn, li, lh);
    }
#ifdef FRCNN_LAB_STAMPS
    LAB_STAMP(5);                                            // stores issued
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    LAB_STAMP(6);                                            // stores done
    if (g_lab_stamps && threadIdx.x == 0) {
        unsigned hw; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        unsigned xcc; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        g_lab_stamps[(size_t)blockIdx.x * 8 + 7] = ((unsigned long long)xcc << 32) | hw;
    }
#endif
}

// ------------------------------------------------------------------------------------
// Balanced ("stream-K") launch form of the v2 kernel, late-store variant, 2x2 waves.
//
// A launch of T tiles on S concurrent workgroup slots runs ceil(T/S) rounds whatever T is: the detector head's
// 460 128x128 tiles on 512 slots leave 52 CUs with one workgroup while 204 carry two, and the launch lasts as long
// as the loaded ones (0.90 of the slots' work; a bare MFMA + LDS loop of this shape measures 127 vs 141 TFLOP/s,
// scripts/micro/mfma_ladder.hip).  Here the launch has G = rounds x S workgroups and the UNIT of work is a k-chunk:
// the tiles' chunks, tile after tile (a tile's count depends on its row range only: position-major rows skip
// padding-only taps), form one sequence of U units and workgroup w takes units [w*U/G, (w+1)*U/G).  A range covers
// the tail of one tile, possibly whole tiles, and the head of another.  A tile covered by ONE workgroup goes straight
// to the epilogue; otherwise each contributor publishes its f32 partial tile in slot (w - first contributor) with
// write-through stores and adds its chunk count to the tile's ticket -- the one that completes the count sums the
// slots in slot order (deterministic) and runs the epilogue, exactly the split-K protocol with unequal slices.
// (SK_SLOTS, conv_policy.h: partial-tile slots per output tile; the policy keeps ranges long enough)

template <int TM, int TN>
__global__ void __launch_bounds__(256) k_conv_igemm_f32_sk(const ConvArgs p) {
    constexpr int WM = 2, WN = 2, NT = 256;
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    constexpr int RPP = NT / 8;
    constexpr int PA = BM / RPP, PB = BN / RPP;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;
    float* Bs = smem + 2 * BM * LDS_STRIDE;
    int* pref = reinterpret_cast<int*>(smem + 2 * (BM + BN) * LDS_STRIDE);       // [tiles_m + 1] chunk-count prefix over row tiles

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int li = lane & 31, lh = lane >> 5;
    const int lrow = tid >> 3, lcol = (tid & 7) * 4;
    const int RS = p.R * p.S;
    const unsigned all_taps = RS >= 32 ? 0xffffffffu : (1u << RS) - 1u;
    const int groups = p.Kpad / (BK * RS);

    auto taps_of = [&](int tile_m) -> unsigned {
        if (!p.layout) return all_taps;
        const int m0 = tile_m * BM;
        const int pos_lo = m0 / p.n_img, pos_hi = (min(m0 + BM, p.M) - 1) / p.n_img;
        if (pos_hi - pos_lo >= 8) return all_taps;
        unsigned mk = 0;
        for (int pos = pos_lo; pos <= pos_hi; ++pos) {
            const int ho = pos / p.Wo, wo = pos - ho * p.Wo;
            const int h0 = ho * p.stride - p.pad_top, w0 = wo * p.stride - p.pad_left;
            for (int r = 0; r < p.R; ++r)
                for (int sx = 0; sx < p.S; ++sx)
                    if ((unsigned)(h0 + r) < (unsigned)p.H && (unsigned)(w0 + sx) < (unsigned)p.W) mk |= 1u << (r * p.S + sx);
        }
        return mk ? mk : all_taps;
    };
    for (int m = tid; m < p.tiles_m; m += NT) pref[m + 1] = groups * __popc(taps_of(m));
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        pref[0] = 0;
        for (int m = 1; m <= p.tiles_m; ++m) { run += pref[m]; pref[m] = run; }
    }
    __syncthreads();
    const int Pm = pref[p.tiles_m];
    const long long U = (long long)Pm * p.tiles_n;
    const int G = gridDim.x;
    const int w = xcd_remap(blockIdx.x, G);
    long long u = (long long)w * U / G;
    const long long u_end = (long long)(w + 1) * U / G;

    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.x), 0, (int)((size_t)p.n_img * p.H * p.W * p.Cin * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.w), 0, (int)((size_t)p.Cout * p.Kpad * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t srsrc = __builtin_amdgcn_make_buffer_rsrc(
        p.slabs, 0, (int)((size_t)p.tiles_m * p.tiles_n * SK_SLOTS * (BM * BN) * 4), 0x00020000);

    while (u < u_end) {
        __syncthreads();                                     // the previous segment is done with the LDS (operands, flag)
        const int tile_n = (int)(u / Pm);
        const int r_u = (int)(u - (long long)tile_n * Pm);
        int lo = 0, hi = p.tiles_m;                          // largest tile_m with pref[tile_m] <= r_u
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (pref[mid] <= r_u) lo = mid; else hi = mid; }
        const int tile_m = lo;
        const int nk_t = pref[tile_m + 1] - pref[tile_m];
        const int kb = r_u - pref[tile_m];
        const int ke = (int)min((long long)nk_t, kb + (u_end - u));
        const int tile = tile_n * p.tiles_m + tile_m;
        const int m0 = tile_m * BM, n0 = tile_n * BN;
        const unsigned tap_mask = taps_of(tile_m);
        const int n_taps = __popc(tap_mask);

        int a_h[PA], a_w[PA], a_off[PA];
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            const int m = m0 + lrow + RPP * i;
            if (m < p.M) {
                int wo, ho, img;
                if (p.layout) { img = m % p.n_img; const int pos = m / p.n_img; ho = pos / p.Wo; wo = pos - ho * p.Wo; }
                else { wo = m % p.Wo; const int t = m / p.Wo; ho = t % p.Ho; img = t / p.Ho; }
                a_h[i] = ho * p.stride - p.pad_top;
                a_w[i] = wo * p.stride - p.pad_left;
                a_off[i] = (img * p.img_stride + (a_h[i] * p.W + a_w[i]) * p.pix_stride + lcol) * 4;
            } else {
                a_h[i] = -(1 << 28); a_w[i] = 0; a_off[i] = 0;
            }
        }
        unsigned b_off[PB];
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            const int n = n0 + lrow + RPP * i;
            b_off[i] = n < p.Cout ? (unsigned)((n * p.Kpad + lcol) * 4) : OOB_OFFSET;
        }

        i32x4 ra[PA], rb[PB];
        unsigned rem = tap_mask;
        const int grp0 = kb / n_taps;
        int c0 = grp0 * BK, w_grp = grp0 * RS * (BK * 4);
        for (int t = kb - grp0 * n_taps; t > 0; --t) rem &= rem - 1;
        auto load_chunk = [&]() {
            const int tap = __builtin_ctz(rem);
            const int r_tap = (tap * p.inv_S) >> 16, s_tap = tap - r_tap * p.S;
            const int tap_off = ((r_tap * p.W + s_tap) * p.pix_stride + c0) * 4;
            const int w_off = w_grp + tap * (BK * 4);
#pragma unroll
            for (int i = 0; i < PB; ++i)
                rb[i] = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, b_off[i], w_off, 0);
#pragma unroll
            for (int i = 0; i < PA; ++i) {
                const int hi2 = a_h[i] + r_tap, wi = a_w[i] + s_tap;
                const bool ok = (unsigned)hi2 < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
                ra[i] = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, ok ? (unsigned)(a_off[i] + tap_off) : OOB_OFFSET, 0, 0);
            }
            rem &= rem - 1;
            const int wrap = (rem == 0);
            rem |= wrap ? tap_mask : 0u;
            c0 += wrap * BK;
            w_grp += wrap * (RS * BK * 4);
        };
        auto store_chunk = [&](int buf) {
            float* a = As + buf * BM * LDS_STRIDE;
            float* b = Bs + buf * BN * LDS_STRIDE;
#pragma unroll
            for (int i = 0; i < PA; ++i) *reinterpret_cast<i32x4*>(a + (lrow + RPP * i) * LDS_STRIDE + lcol) = ra[i];
#pragma unroll
            for (int i = 0; i < PB; ++i) *reinterpret_cast<i32x4*>(b + (lrow + RPP * i) * LDS_STRIDE + lcol) = rb[i];
        };

        f32x16 acc[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

        load_chunk();
        store_chunk(0);
        load_chunk();                                        // past the range's end at most: loaded, never multiplied
        __syncthreads();

        constexpr int MF = TM * TN * 4, NL = PA + PB, NF = TM + TN;
        for (int kc = kb; kc < ke; ++kc) {
            const int buf = (kc - kb) & 1;
            const float* a = As + buf * BM * LDS_STRIDE + (wm * TM * 32 + li) * LDS_STRIDE + lh * 4;
            const float* b = Bs + buf * BN * LDS_STRIDE + (wn * TN * 32 + li) * LDS_STRIDE + lh * 4;
            f32x4 fa[BK / 8][TM], fb[BK / 8][TN];
#pragma unroll
            for (int kk = 0; kk < BK / 8; ++kk) {
#pragma unroll
                for (int i = 0; i < TM; ++i) fa[kk][i] = *reinterpret_cast<const f32x4*>(a + i * 32 * LDS_STRIDE + kk * 8);
#pragma unroll
                for (int j = 0; j < TN; ++j) fb[kk][j] = *reinterpret_cast<const f32x4*>(b + j * 32 * LDS_STRIDE + kk * 8);
            }
#pragma unroll
            for (int kk = 0; kk < BK / 8; ++kk)
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[kk][i][e], fb[kk][j][e], acc[i][j], 0, 0, 0);
            store_chunk(buf ^ 1);
            load_chunk();
            SGB(SG_DS_RD, NF);
#pragma unroll
            for (int kk = 0; kk < BK / 8 - 1; ++kk) {
#pragma unroll
                for (int q = 0; q < MF; ++q) {
                    SGB(SG_MFMA, 1);
                    if (q < NF) SGB(SG_DS_RD, 1);
                    else if (kk == BK / 8 - 2 && q - NF < NL) SGB(SG_DS_WR, 1);
                }
            }
#pragma unroll
            for (int q = 0; q < MF; ++q) {
                SGB(SG_MFMA, 1);
                if (MF - NF < NL && q < NL - (MF - NF)) SGB(SG_DS_WR, 1);
                else if (q < NL + (MF - NF < NL ? NL - (MF - NF) : 0)) { SGB(SG_VALU, 4); SGB(SG_VMEM_RD, 1); }
            }
            __syncthreads();
        }
        u += ke - kb;

        if (kb != 0 || ke != nk_t) {
            // partial tile: which contributors does this tile have?  first = the workgroup whose range holds the tile's
            // first unit, last = the one holding its last (w*U/G <= x  <=>  w <= ((x+1)*G - 1) / U)
            const long long ts = (long long)tile_n * Pm + pref[tile_m];
            const int w_first = (int)(((ts + 1) * G - 1) / U);
            const int w_last = (int)(((ts + nk_t) * G - 1) / U);
            const unsigned slab_off = (unsigned)(((size_t)tile * SK_SLOTS + (w - w_first)) * (BM * BN) * 4 + tid * 16);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        f32x4 v = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, v), srsrc,
                                                               slab_off + ((i * TN + j) * 4 + q) * (NT * 16), 0, 16 /* sc1 */);
                    }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            int* last = reinterpret_cast<int*>(smem);
            if (tid == 0) {
                const unsigned mine = (unsigned)(ke - kb);
                const unsigned t = __hip_atomic_fetch_add(&p.tickets[tile], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int is_last = (t + mine == (unsigned)nk_t);
                if (is_last) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __hip_atomic_store(&p.tickets[tile], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                *last = is_last;
            }
            __syncthreads();
            if (!*last) continue;                             // somebody else finishes this tile
            const float4* base = reinterpret_cast<const float4*>(p.slabs + (size_t)tile * SK_SLOTS * (BM * BN));
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
            for (int sl = 0; sl <= w_last - w_first; ++sl) {
                const float4* sp = base + (size_t)sl * (BM * BN / 4);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float4 v = sp[((i * TN + j) * 4 + q) * NT + tid];
                            acc[i][j][4 * q] += v.x; acc[i][j][4 * q + 1] += v.y; acc[i][j][4 * q + 2] += v.z; acc[i][j][4 * q + 3] += v.w;
                        }
            }
        }
        if (p.vec_epi) epilogue_vec<TM, TN, WM, WN, false>(acc, p, m0, n0, tid, wm, wn, li, lh, smem, nullptr);
        else epilogue<TM, TN>(acc, p, m0, n0, wm, wn, li, lh);
    }
}

// filter packing, Keras HWIO -> [Cout][Kpad] (the layout: conv_f32_common.h packed_k / pack_hwio_elem)
__global__ void k_pack_hwio(const float* w, int RS, int Cin, int Cout, int Kpad, float* out) {
    const size_t total = (size_t)Cout * Kpad;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        out[i] = pack_hwio_elem(w, RS, Cin, Cout, Kpad, i);
}

template <int TM, int TN, bool G>
static int launch_conv(const ConvArgs& a, hipStream_t s) {
    constexpr int BM = 64 * TM, BN = 64 * TN;
    ConvArgs p = a;
    p.tiles_m = (p.M + BM - 1) / BM;
    p.tiles_n = (p.Cout + BN - 1) / BN;
    const size_t lds = (size_t)2 * (BM + BN) * LDS_STRIDE * sizeof(float);
    static std::atomic<uint64_t> lds_seen{0};
    if (int e = raise_lds_once(lds_seen, (const void*)k_conv_igemm_f32<TM, TN, G>, lds, "conv2d")) return e;
    k_conv_igemm_f32<TM, TN, G><<<p.tiles_m * p.tiles_n, 256, lds, s>>>(p);
    return check_launch("conv2d_fwd");
}

template <int TM, int TN, int VARIANT = 0, int WM = 2, int WN = 2>
static int launch_conv_v2(const ConvArgs& a, hipStream_t s) {
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    ConvArgs p = a;
    p.tiles_m = (p.M + BM - 1) / BM;
    p.tiles_n = (p.Cout + BN - 1) / BN;
    const size_t lds = (size_t)2 * (BM + BN) * LDS_STRIDE * sizeof(float);
    static std::atomic<uint64_t> lds_seen{0};
    if (int e = raise_lds_once(lds_seen, (const void*)k_conv_igemm_f32_v2<TM, TN, VARIANT, WM, WN>, lds, "conv2d")) return e;
    k_conv_igemm_f32_v2<TM, TN, VARIANT, WM, WN><<<p.tiles_m * p.tiles_n, 64 * WM * WN, lds, s>>>(p);
    return check_launch("conv2d_fwd");
}

static int launch_conv_cin3(const ConvArgs& a, hipStream_t s, bool variant2) {
    ConvArgs p = a;
    p.tiles_m = (p.M + 63) / 64;
    p.tiles_n = (p.Cout + 63) / 64;
    const size_t lds = (size_t)2 * (64 + 64) * LDS_STRIDE * sizeof(float);
    if (variant2) k_conv_igemm_f32_v2<1, 1, 2, 2, 2, false, true><<<p.tiles_m * p.tiles_n, 256, lds, s>>>(p);
    else k_conv_igemm_f32_v2<1, 1, 1, 2, 2, false, true><<<p.tiles_m * p.tiles_n, 256, lds, s>>>(p);
    return check_launch("conv2d_fwd (3-channel stem)");
}


template <int TM, int TN, int VARIANT = 0, int WM = 2, int WN = 2>
static int launch_conv_v2_splitk(const ConvArgs& a, hipStream_t s) {
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    ConvArgs p = a;
    p.tiles_m = (p.M + BM - 1) / BM;
    p.tiles_n = (p.Cout + BN - 1) / BN;
    const size_t lds = (size_t)2 * (BM + BN) * LDS_STRIDE * sizeof(float);
    static std::atomic<uint64_t> lds_seen{0};
    if (int e = raise_lds_once(lds_seen, (const void*)k_conv_igemm_f32_v2<TM, TN, VARIANT, WM, WN, true>, lds, "conv2d")) return e;
    k_conv_igemm_f32_v2<TM, TN, VARIANT, WM, WN, true><<<p.tiles_m * p.tiles_n * p.splits, 64 * WM * WN, lds, s>>>(p);
    return check_launch("conv2d_fwd (split-K)");
}

template <int TM, int TN>
static int launch_conv_sk(const ConvArgs& a, int G, hipStream_t s) {
    constexpr int BM = 64 * TM, BN = 64 * TN;
    ConvArgs p = a;
    p.tiles_m = (p.M + BM - 1) / BM;
    p.tiles_n = (p.Cout + BN - 1) / BN;
    const size_t lds = (size_t)2 * (BM + BN) * LDS_STRIDE * sizeof(float) + (size_t)(p.tiles_m + 1) * sizeof(int);
    static std::atomic<size_t> attr_lds[64];                 // per device ordinal (the limit is a per-device function attribute); grows with tiles_m
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(FRCNN_E_HIP, "conv2d: no current HIP device");
    if (lds > attr_lds[dev & 63].load(std::memory_order_acquire)) {
        if (hipFuncSetAttribute((const void*)k_conv_igemm_f32_sk<TM, TN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return fail(FRCNN_E_HIP, "conv2d: cannot raise dynamic LDS to %zu", lds);
        attr_lds[dev & 63].store(lds, std::memory_order_release);
    }
    k_conv_igemm_f32_sk<TM, TN><<<G, 256, lds, s>>>(p);
    return check_launch("conv2d_fwd (balanced)");
}

}  // namespace frcnn

using namespace frcnn;

struct DualOut { int n1; int act1; float* y2; int act2; };      // frcnn_conv2d_fwd_dual: the launch's second layer
static int roi_res_available(const frcnn_conv_desc* d, int engine, bool x_is_planes);
static int pool_available(const frcnn_conv_desc* d, int engine, bool x_is_planes, int window);
static int rowmap_available(const frcnn_conv_desc* d, int engine, bool x_is_planes);
static int conv_h3_planes_impl(const frcnn_conv_desc* d, const float* x, const frcnn_h3_planes* x_planes, const float* x_amax, const void* w_planes_f16,
                               const float* scale, const float* shift, const float* residual, const frcnn_h3_planes* residual_planes,
                               const frcnn_roi_res* gathered, const float* residual_amax, float* y, float* y_amax, const frcnn_h3_planes* y_planes,
                               float bound_c, float bound_d, void* stream, const frcnn_rowmap* rowmap = nullptr);

// the magnitude records of a launch (ConvArgs.x_amax / y_amax / y2_amax), every other field zero
static ConvArgs amax_args(const float* x_amax, float* y_amax, float* y2_amax = nullptr) {
    ConvArgs a = {};
    a.x_amax = x_amax; a.y_amax = y_amax; a.y2_amax = y2_amax;
    return a;
}

// Every frcnn_conv2d_fwd* entry point: one launch on `engine` (FRCNN_ENGINE_*) of what the policy (conv_policy.hip) picks for the
// descriptor.  `a` arrives with the magnitude records and the f16x3 engine's fp16 planes set (all null: nothing is tracked); the rest
// of the launch arguments come from the descriptor here.
static int conv_fwd_impl(const frcnn_conv_desc* d, const float* x, const float* w_packed,
                         const float* scale, const float* shift, const float* residual, const float* mask, float* y,
                         const DualOut* dual, void* workspace, size_t workspace_bytes, void* stream, int engine = FRCNN_ENGINE_NATIVE,
                         ConvArgs a = {}) {
    const bool planes_io = a.x_planes || a.y_planes;
    if (!d || !w_packed || (!planes_io && (!x || !y))) return fail(FRCNN_E_ARG, "conv2d_fwd: null pointer");
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->cin <= 0 || d->cout <= 0 || d->kh <= 0 || d->kw <= 0 || d->stride <= 0 || d->ho <= 0 || d->wo <= 0)
        return fail(FRCNN_E_ARG, "conv2d_fwd: bad shape");
    const long long M = (long long)d->n * d->ho * d->wo;
    if (M > 0x7fffffffLL) return fail(FRCNN_E_ARG, "conv2d_fwd: too many output pixels");
    a.x = x; a.w = w_packed; a.scale = scale; a.shift = shift; a.residual = residual; a.y = y; a.mask = mask;
    a.n_img = d->n; a.H = d->h; a.W = d->w; a.Cin = d->cin; a.Cout = d->cout; a.R = d->kh; a.S = d->kw;
    a.stride = d->stride; a.pad_top = d->pad_top; a.pad_left = d->pad_left; a.Ho = d->ho; a.Wo = d->wo;
    a.M = (int)M; a.K = d->kh * d->kw * d->cin; a.Kpad = frcnn_conv_packed_k(d->kh, d->kw, d->cin);
    a.act = d->act; a.ldy = d->ldy > 0 ? d->ldy : d->cout; a.ldres = d->ldres > 0 ? d->ldres : d->cout;
    if (dual) { a.n_split = dual->n1; a.act = dual->act1; a.ldy = dual->n1; a.y2 = dual->y2; a.ldy2 = d->cout - dual->n1; a.act2 = dual->act2; }
    a.splits = 1;
    a.layout = d->layout ? 1 : 0;
    a.pix_stride = a.layout ? d->n * d->cin : d->cin;
    a.img_stride = a.layout ? d->cin : d->h * d->w * d->cin;
    a.inv_S = (65536 + d->kw - 1) / d->kw;
    // the vector epilogue addresses rows in 16-byte pieces through 32-bit buffer offsets
    auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    a.vec_epi = !conv_knobs().scalar_epilogue && (d->cout & 3) == 0 && (a.ldy & 3) == 0 && al16(y) && (size_t)M * a.ldy * 4 < 0x7fffffffull
             && (!residual || ((a.ldres & 3) == 0 && al16(residual) && (size_t)M * a.ldres * 4 < 0x7fffffffull))
             && (!mask || (al16(mask) && (size_t)M * d->cout * 4 < 0x7fffffffull)) && (!scale || al16(scale)) && (!shift || al16(shift));
    // the 16-byte epilogue picks the output per TILE: the boundary between the layers of a paired launch must be a tile boundary and
    // both outputs 16-byte addressable; otherwise every lane picks per column (the 4-byte epilogue)
    auto dual_vec_epi = [&](int bn) {
        return a.vec_epi && dual->n1 % bn == 0 && (a.ldy2 & 3) == 0 && al16(dual->y2) && (size_t)M * a.ldy2 * 4 < 0x7fffffffull;
    };
    auto use_workspace = [&]() { a.tickets = (unsigned*)workspace; a.slabs = (float*)((char*)workspace + SPLITK_TICKET_BYTES); };
    hipStream_t s = as_stream(stream);
    const bool generic = (d->cin % BK) != 0;
    if (engine != FRCNN_ENGINE_NATIVE) {
        // the split engines: w_packed points at the three bf16 filter planes (conv_x6.hip) / the header + two fp16 planes (conv_h3.hip)
        const bool h3 = engine == FRCNN_ENGINE_H3;
        const SplitRule& r = split_rule(engine);
        int (*launch)(const ConvArgs&, int, hipStream_t) = h3 ? launch_conv_h3 : launch_conv_x6;
        if (generic || d->kh * d->kw > 32) return fail(FRCNN_E_UNSUPPORTED, "conv2d_fwd_%s: cin %% 32 == 0 and at most 32 taps", r.name);
        if ((size_t)r.planes * d->cout * a.Kpad * 2 >= 0x7fffffffull) return fail(FRCNN_E_UNSUPPORTED, "conv2d_fwd_%s: filter planes over 2 GiB", r.name);
        if (h3 && (reinterpret_cast<uintptr_t>(w_packed) & 15)) return fail(FRCNN_E_ARG, "conv2d_fwd_h3: 16-byte aligned filter planes required");
        const int cfg = split_config(r, d, dual ? dual->n1 : 0), bn = r.tile_width(cfg);
        if (a.res_map) {
            // the residual gathered by RoI taps (include/ext/frcnn_hip_roi_res.h): what frcnn_conv2d_roi_res_available admits, nothing else
            if (roi_res_available(d, engine, a.x_planes != nullptr) != 1 || dual || mask || residual || a.res_planes || workspace)
                return fail(FRCNN_E_UNSUPPORTED, "conv2d_fwd_h3_roi_res: not available for this launch (frcnn_conv2d_roi_res_available)");
            if (y && !a.vec_epi) return fail(FRCNN_E_ARG, "conv2d_fwd_h3_roi_res: 16-byte addressable output rows required");
            if ((long long)a.res_map_rows * d->cout * 4 >= 0x7fffffffLL || M * 32 >= 0x7fffffffLL) return fail(FRCNN_E_UNSUPPORTED, "conv2d_fwd_h3_roi_res: map or tap table over 2 GiB");
        }
        if (a.pool_rows) {
            // the output averaged over groups of rows (include/ext/frcnn_hip_pool_epilogue.h): what frcnn_conv2d_pool_available admits, nothing else
            if (pool_available(d, engine, a.x_planes != nullptr, a.pool_rows) != 1 || dual || mask || a.res_planes || a.res_map || a.y_planes || workspace || !y)
                return fail(FRCNN_E_UNSUPPORTED, "conv2d_fwd_h3_pool: not available for this launch (frcnn_conv2d_pool_available)");
            if (!a.vec_epi) return fail(FRCNN_E_ARG, "conv2d_fwd_h3_pool: 16-byte addressable output and residual rows required");
            a.pool_groups = 256 / a.pool_rows < 1024 / 128 ? 256 / a.pool_rows : 1024 / 128;      // whole groups in a 256-row tile, one thread per group and column
        }
        if (a.row_map) {
            // rows assigned to tiles by a map (include/ext/frcnn_hip_rowmap.h): what frcnn_conv2d_rowmap_available admits, nothing else
            if (rowmap_available(d, engine, a.x_planes != nullptr) != 1 || dual || mask || residual || a.res_planes || a.res_map || a.pool_rows || workspace)
                return fail(FRCNN_E_UNSUPPORTED, "conv2d_fwd_h3_rowmap: not available for this launch (frcnn_conv2d_rowmap_available)");
            if (y && !a.vec_epi) return fail(FRCNN_E_ARG, "conv2d_fwd_h3_rowmap: 16-byte addressable output rows required");
            if (a.map_rows < 256 || a.map_rows % 256 || a.map_rows < M) return fail(FRCNN_E_ARG, "conv2d_fwd_h3_rowmap: the map holds whole 256-row tiles and at least every output row");
        }
        if (planes_io) {
            // activations as fp16 planes (f16x3 only): the double-buffered 256x128 forms only, 16-byte epilogue, one layer, no mask
            if ((cfg != 86 && cfg != 85 && cfg != 82) || dual || mask || (!a.vec_epi && y) || d->ldy > 0)
                return fail(FRCNN_E_UNSUPPORTED, "conv2d_fwd_h3_planes: needs the 256x128 tile (>= 256 output tiles of 128x128; frcnn_conv2d_h3_config 86 / 82), a dense single-layer launch without a mask");
            if ((d->cout & 3) || (d->cin & 7)) return fail(FRCNN_E_UNSUPPORTED, "conv2d_fwd_h3_planes: cin %% 8 == 0 and cout %% 4 == 0");
            if (a.res_planes && (residual || (y && !a.vec_epi))) return fail(FRCNN_E_ARG, "conv2d_fwd_h3_planes: residual planes exclude an f32 residual and need 16-byte addressable output rows");
            if ((size_t)M * d->cout * 4 >= 0x7fffffffull || (size_t)d->n * d->h * d->w * d->cin * 4 >= 0x7fffffffull)
                return fail(FRCNN_E_UNSUPPORTED, "conv2d_fwd_h3_planes: tensor planes over 2 GiB");
            if (!y) a.vec_epi = 1;
        } else if (workspace && !dual) {
            if (const size_t need = split_workspace_bytes(r, d)) {
                if (workspace_bytes < need) return fail(FRCNN_E_WORKSPACE, "conv2d_fwd_%s: workspace needs %zu bytes", r.name, need);
                a.splits = split_slices(r, d);
                use_workspace();
                a.group_m = 0;
                return launch(a, split_sk_code(r, d), s);
            }
        }
        if (dual) a.vec_epi = dual_vec_epi(bn);
        a.group_m = split_group_m(d, bn);
        return launch(a, cfg, s);
    }
    int cfg = choose_config(d);
    if (dual) {
        cfg = dual_config(cfg);
        a.vec_epi = dual_vec_epi(native_tile_width(cfg));
    }
    a.group_m = native_group_m(d, cfg);
    cfg = workspace_config(d, cfg, workspace != nullptr);
    if (a.layout && (generic || cfg < 11 || d->kh * d->kw > 32))
        return fail(FRCNN_E_UNSUPPORTED, "conv2d_fwd: position-major layout needs cin %% 32 == 0, a tensor under 2 GiB and at most 32 taps");
    if (d->cin == 3) {                                          // the stems: filter packed 4 wide, eight taps per chunk
        if (a.layout) return fail(FRCNN_E_UNSUPPORTED, "conv2d_fwd: position-major layout needs cin %% 32 == 0");
        if ((size_t)d->n * d->h * d->w * 12 >= 0x7fffffffull) return fail(FRCNN_E_UNSUPPORTED, "conv2d_fwd: 3-channel input over 2 GiB");
        return launch_conv_cin3(a, s, d->tile % 100 != 32);      // the mid-chunk-barrier loop (conv1 50.6 -> 49.4 us); 32: dev code, the late-store loop
    }
    if (!generic && workspace) {
        const size_t need = dual ? frcnn_conv2d_dual_workspace_bytes(d) : frcnn_conv2d_workspace_bytes(d);
        if (need) {
            if (workspace_bytes < need) return fail(FRCNN_E_WORKSPACE, "conv2d_fwd: workspace needs %zu bytes", need);
            use_workspace();
            if (const int G = dual ? 0 : choose_streamk(d, cfg))
                return streamk_edge(cfg) == 128 ? launch_conv_sk<2, 2>(a, G, s) : launch_conv_sk<1, 1>(a, G, s);
            a.splits = choose_splits(d, cfg);
            return cfg == 23 ? launch_conv_v2_splitk<1, 1, 2>(a, s) : launch_conv_v2_splitk<1, 1, 1>(a, s);
        }
    }
    if (generic) return cfg == 2 ? launch_conv<1, 1, true>(a, s) : launch_conv<2, 1, true>(a, s);
    switch (plain_config(cfg)) {                                // (61 / 62 without a workspace: the plain launch)
        case 41: return launch_conv_v2<1, 2, 1, 4, 2>(a, s);     // 128x128, 8 waves
        case 42: return launch_conv_v2<2, 1, 1, 2, 4>(a, s);     // 128x128, 8 waves (2x4)
        case 43: return launch_conv_v2<1, 1, 1, 4, 2>(a, s);     // 128x64, 8 waves
        case 21: return launch_conv_v2<2, 2, 1>(a, s);
        case 22: return launch_conv_v2<1, 1, 1>(a, s);
        case 23: return launch_conv_v2<1, 1, 2>(a, s);           // 64x64, mid-chunk barrier main loop
        case 24: return launch_conv_v2<1, 2, 2>(a, s);           // 64x128
        case 25: return launch_conv_v2<2, 1, 2>(a, s);           // 128x64
        case 26: return launch_conv_v2<2, 2, 2>(a, s);           // 128x128
        case 11: return launch_conv_v2<2, 2>(a, s);
        case 12: return launch_conv_v2<1, 1>(a, s);
        case 13: return launch_conv_v2<2, 1>(a, s);
        case 14: return launch_conv_v2<4, 2>(a, s);
        case 1: return launch_conv<2, 2, false>(a, s);
        case 2: return launch_conv<1, 1, false>(a, s);
        case 3: return launch_conv<2, 1, false>(a, s);
        case 4: return launch_conv<4, 2, false>(a, s);
        default: return fail(FRCNN_E_ARG, "conv2d_fwd: unknown tile config %d", cfg);
    }
}

// frcnn_conv2d_roi_res_available (the launch asks the same question): 1 / 0
static int roi_res_available(const frcnn_conv_desc* d, int engine, bool x_is_planes) {
    if (engine != FRCNN_ENGINE_H3) return 0;
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->cin <= 0 || d->cout <= 0 || d->kh <= 0 || d->kw <= 0 || d->stride <= 0 || d->ho <= 0 || d->wo <= 0) return 0;
    if ((d->cin % BK) != 0 || d->kh * d->kw > 32 || (d->cout & 3) || d->ldy > 0 || d->ldres > 0) return 0;
    const SplitRule& r = split_rule(engine);
    const int cfg = split_config(r, d, 0);
    if (cfg != 86 && cfg != 85) return 0;                   // 256x128 on sixteen waves; an explicit split-K code (184 / 181) maps to 84 / 81 here
    if (x_is_planes && h3_takes_ring(cfg, frcnn_conv_packed_k(d->kh, d->kw, d->cin))) return 0;
    const long long M = (long long)d->n * d->ho * d->wo;
    if (M * d->cout * 4 >= 0x7fffffffLL || (long long)d->n * d->h * d->w * d->cin * 4 >= 0x7fffffffLL) return 0;
    return 1;
}

// frcnn_conv2d_pool_available (the launch asks the same question): 1 / 0
static int pool_available(const frcnn_conv_desc* d, int engine, bool x_is_planes, int window) {
    if (engine != FRCNN_ENGINE_H3 || !x_is_planes) return 0;
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->cin <= 0 || d->cout <= 0 || d->kh <= 0 || d->kw <= 0 || d->stride <= 0 || d->ho <= 0 || d->wo <= 0) return 0;
    if (d->kh != 1 || d->kw != 1 || d->stride != 1 || d->pad_top || d->pad_left || d->ho != d->h || d->wo != d->w || d->layout) return 0;
    if ((d->cin % BK) != 0 || (d->cout & 3) || d->ldy > 0 || d->ldres > 0) return 0;
    const SplitRule& r = split_rule(engine);
    const int cfg = split_config(r, d, 0);
    if (cfg != 86 && cfg != 85) return 0;                   // 256x128 on sixteen waves; an explicit split-K code (184 / 181) maps to 84 / 81 here
    if (h3_takes_ring(cfg, frcnn_conv_packed_k(d->kh, d->kw, d->cin))) return 0;
    const long long M = (long long)d->n * d->ho * d->wo;
    if (window < 1 || window > 256 || M % window) return 0;
    if (M * d->cout * 4 >= 0x7fffffffLL || (long long)d->n * d->h * d->w * d->cin * 4 >= 0x7fffffffLL) return 0;
    return 1;
}

// frcnn_conv2d_rowmap_available (the launch asks the same question): 1 / 0
static int rowmap_available(const frcnn_conv_desc* d, int engine, bool x_is_planes) {
    if (engine != FRCNN_ENGINE_H3 || !x_is_planes) return 0;
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->cin <= 0 || d->cout <= 0 || d->kh <= 0 || d->kw <= 0 || d->stride <= 0 || d->ho <= 0 || d->wo <= 0) return 0;
    if (d->layout || (d->cin % BK) != 0 || d->kh * d->kw > 32 || (d->cout & 3) || d->ldy > 0 || d->ldres > 0) return 0;
    const SplitRule& r = split_rule(engine);
    if (split_config(r, d, 0) != 86) return 0;              // 256x128 on sixteen waves, the ring allowed (85 keeps the two buffers); a split-K code maps to 84 / 81 here
    const long long M = (long long)d->n * d->ho * d->wo;
    if (M * d->cout * 4 >= 0x7fffffffLL || (long long)d->n * d->h * d->w * d->cin * 4 >= 0x7fffffffLL) return 0;
    return 1;
}

extern "C" {

int frcnn_conv2d_rowmap_available(const frcnn_conv_desc* d, int engine, int x_is_planes) {
    if (!d) return fail(FRCNN_E_ARG, "conv2d_rowmap_available: null descriptor");
    if (engine != FRCNN_ENGINE_NATIVE && engine != FRCNN_ENGINE_X6 && engine != FRCNN_ENGINE_H3) return fail(FRCNN_E_ARG, "conv2d_rowmap_available: unknown engine %d", engine);
    return rowmap_available(d, engine, x_is_planes != 0);
}

int frcnn_conv2d_fwd_h3_rowmap(const frcnn_conv_desc* d, const frcnn_h3_planes* x_planes, const float* x_amax, const void* w_planes_f16,
                               const float* scale, const float* shift, float* y, float* y_amax, const frcnn_h3_planes* y_planes,
                               float bound_c, float bound_d, const frcnn_rowmap* map, void* stream) {
    if (!d || !w_planes_f16 || !map) return fail(FRCNN_E_ARG, "conv2d_fwd_h3_rowmap: null pointer");
    if (!map->row_map || !map->tile_taps || map->rows <= 0 || map->reserved != 0 || (reinterpret_cast<uintptr_t>(map->row_map) & 3) || (reinterpret_cast<uintptr_t>(map->tile_taps) & 3))
        return fail(FRCNN_E_ARG, "conv2d_fwd_h3_rowmap: row map, tap words and rows > 0 required (reserved = 0)");
    if (rowmap_available(d, FRCNN_ENGINE_H3, x_planes != nullptr) != 1)
        return fail(FRCNN_E_UNSUPPORTED, "conv2d_fwd_h3_rowmap: not available for this launch (frcnn_conv2d_rowmap_available)");
    return conv_h3_planes_impl(d, nullptr, x_planes, x_amax, w_planes_f16, scale, shift, nullptr, nullptr, nullptr, nullptr, y, y_amax, y_planes, bound_c, bound_d, stream, map);
}

int frcnn_pool_epilogue_version(void) { return FRCNN_POOL_EPILOGUE_VERSION; }

int frcnn_conv2d_pool_available(const frcnn_conv_desc* d, int engine, int x_is_planes, int window) {
    if (!d) return fail(FRCNN_E_ARG, "conv2d_pool_available: null descriptor");
    if (engine != FRCNN_ENGINE_NATIVE && engine != FRCNN_ENGINE_X6 && engine != FRCNN_ENGINE_H3) return fail(FRCNN_E_ARG, "conv2d_pool_available: unknown engine %d", engine);
    return pool_available(d, engine, x_is_planes != 0, window);
}

int frcnn_conv2d_fwd_h3_pool(const frcnn_conv_desc* d, const float* x, const frcnn_h3_planes* x_planes, const float* x_amax,
                             const void* w_planes_f16, const float* scale, const float* shift, const float* residual,
                             const frcnn_h3_planes* residual_planes, const float* mask, int window, float* y, float* y_amax,
                             const frcnn_h3_planes* y_planes, void* stream) {
    if (!d || !w_planes_f16 || !y) return fail(FRCNN_E_ARG, "conv2d_fwd_h3_pool: null pointer");
    if (!x_amax) return fail(FRCNN_E_ARG, "conv2d_fwd_h3_pool: the input's magnitude record is required");
    if (x || residual_planes || mask || y_planes)
        return fail(FRCNN_E_UNSUPPORTED, "conv2d_fwd_h3_pool: plane input, an f32 residual or none, no mask and no plane output (frcnn_conv2d_pool_available)");
    if (pool_available(d, FRCNN_ENGINE_H3, x_planes != nullptr, window) != 1)
        return fail(FRCNN_E_UNSUPPORTED, "conv2d_fwd_h3_pool: not available for this launch (frcnn_conv2d_pool_available)");
    if (!x_planes->planes || !x_planes->exponent || (reinterpret_cast<uintptr_t>(x_planes->planes) & 15))
        return fail(FRCNN_E_ARG, "conv2d_fwd_h3_pool: incomplete or misaligned input planes");
    ConvArgs rg = amax_args(x_amax, y_amax);
    rg.x_planes = x_planes->planes; rg.x_pexp = x_planes->exponent;
    rg.pool_rows = window;
    return conv_fwd_impl(d, nullptr, reinterpret_cast<const float*>(w_planes_f16), scale, shift, residual, nullptr, y, nullptr, nullptr, 0, stream, FRCNN_ENGINE_H3, rg);
}

int frcnn_conv_packed_k(int kh, int kw, int cin) { return packed_k(kh * kw, cin); }

int frcnn_pack_conv_weights(const float* w_hwio, int kh, int kw, int cin, int cout, float* packed, void* stream) {
    if (!w_hwio || !packed || kh <= 0 || kw <= 0 || cin <= 0 || cout <= 0) return fail(FRCNN_E_ARG, "pack_conv_weights: bad argument");
    const int Kpad = frcnn_conv_packed_k(kh, kw, cin);
    const size_t total = (size_t)cout * Kpad;
    int grid = (int)((total + 255) / 256);
    if (grid > 4096) grid = 4096;
    k_pack_hwio<<<grid, 256, 0, as_stream(stream)>>>(w_hwio, kh * kw, cin, cout, Kpad, packed);
    return check_launch("pack_conv_weights");
}

int frcnn_conv2d_fwd(const frcnn_conv_desc* d, const float* x, const float* w_packed,
                     const float* scale, const float* shift, const float* residual, float* y, void* stream) {
    return frcnn_conv2d_fwd_masked(d, x, w_packed, scale, shift, residual, nullptr, y, stream);
}

int frcnn_conv2d_fwd_masked(const frcnn_conv_desc* d, const float* x, const float* w_packed,
                            const float* scale, const float* shift, const float* residual, const float* mask, float* y, void* stream) {
    return frcnn_conv2d_fwd_ws(d, x, w_packed, scale, shift, residual, mask, y, nullptr, 0, stream);
}

int frcnn_conv2d_fwd_ws(const frcnn_conv_desc* d, const float* x, const float* w_packed,
                        const float* scale, const float* shift, const float* residual, const float* mask, float* y,
                        void* workspace, size_t workspace_bytes, void* stream) {
    return conv_fwd_impl(d, x, w_packed, scale, shift, residual, mask, y, nullptr, workspace, workspace_bytes, stream);
}

// the native launches of frcnn_conv2d_fwd_ws / frcnn_conv2d_fwd_dual that also leave max|y| in a magnitude record: what feeds an
// f16x3 launch from a layer that stays on the native kernels (the 3-channel stem, stage 4's 256-column 1x1 layers)
int frcnn_conv2d_fwd_ws_amax(const frcnn_conv_desc* d, const float* x, const float* w_packed,
                             const float* scale, const float* shift, const float* residual, const float* mask, float* y, float* y_amax,
                             void* workspace, size_t workspace_bytes, void* stream) {
    return conv_fwd_impl(d, x, w_packed, scale, shift, residual, mask, y, nullptr, workspace, workspace_bytes, stream, FRCNN_ENGINE_NATIVE,
                         amax_args(nullptr, y_amax));
}

int frcnn_conv2d_fwd_dual(const frcnn_conv_desc* d, const float* x, const float* w_packed, const float* scale, const float* shift,
                          float* y1, int n1, int act1, float* y2, int act2,
                          void* workspace, size_t workspace_bytes, void* stream) {
    if (!d || !y2 || n1 <= 0 || n1 >= d->cout) return fail(FRCNN_E_ARG, "conv2d_fwd_dual: need 0 < n1 < cout and two outputs");
    if (d->ldy > 0 || d->ldres > 0) return fail(FRCNN_E_ARG, "conv2d_fwd_dual: dense outputs only (ldy = ldres = 0)");
    if ((d->cin % BK) != 0 || d->kh * d->kw > 32) return fail(FRCNN_E_UNSUPPORTED, "conv2d_fwd_dual: cin %% 32 == 0 and at most 32 taps");
    const DualOut dual = {n1, act1, y2, act2};
    return conv_fwd_impl(d, x, w_packed, scale, shift, nullptr, nullptr, y1, &dual, workspace, workspace_bytes, stream);
}

int frcnn_conv2d_fwd_x6(const frcnn_conv_desc* d, const float* x, const void* w_planes_bf16,
                        const float* scale, const float* shift, const float* residual, const float* mask, float* y,
                        void* workspace, size_t workspace_bytes, void* stream) {
    return conv_fwd_impl(d, x, reinterpret_cast<const float*>(w_planes_bf16), scale, shift, residual, mask, y, nullptr, workspace, workspace_bytes, stream, FRCNN_ENGINE_X6);
}

int frcnn_conv2d_fwd_dual_x6(const frcnn_conv_desc* d, const float* x, const void* w_planes_bf16, const float* scale, const float* shift,
                             float* y1, int n1, int act1, float* y2, int act2, void* stream) {
    if (!d || !y2 || n1 <= 0 || n1 >= d->cout) return fail(FRCNN_E_ARG, "conv2d_fwd_dual_x6: need 0 < n1 < cout and two outputs");
    if (d->ldy > 0 || d->ldres > 0) return fail(FRCNN_E_ARG, "conv2d_fwd_dual_x6: dense outputs only (ldy = ldres = 0)");
    const DualOut dual = {n1, act1, y2, act2};
    return conv_fwd_impl(d, x, reinterpret_cast<const float*>(w_planes_bf16), scale, shift, nullptr, nullptr, y1, &dual, nullptr, 0, stream, FRCNN_ENGINE_X6);
}

int frcnn_conv2d_fwd_h3(const frcnn_conv_desc* d, const float* x, const float* x_amax, const void* w_planes_f16,
                        const float* scale, const float* shift, const float* residual, const float* mask, float* y, float* y_amax,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (!x_amax) return fail(FRCNN_E_ARG, "conv2d_fwd_h3: the input's magnitude record is required (frcnn_amax_f32 makes one)");
    return conv_fwd_impl(d, x, reinterpret_cast<const float*>(w_planes_f16), scale, shift, residual, mask, y, nullptr, workspace, workspace_bytes, stream, FRCNN_ENGINE_H3,
                         amax_args(x_amax, y_amax));
}

int frcnn_conv2d_fwd_dual_h3(const frcnn_conv_desc* d, const float* x, const float* x_amax, const void* w_planes_f16, const float* scale, const float* shift,
                             float* y1, int n1, int act1, float* y1_amax, float* y2, int act2, float* y2_amax, void* stream) {
    if (!d || !y2 || n1 <= 0 || n1 >= d->cout) return fail(FRCNN_E_ARG, "conv2d_fwd_dual_h3: need 0 < n1 < cout and two outputs");
    if (d->ldy > 0 || d->ldres > 0) return fail(FRCNN_E_ARG, "conv2d_fwd_dual_h3: dense outputs only (ldy = ldres = 0)");
    if (!x_amax) return fail(FRCNN_E_ARG, "conv2d_fwd_dual_h3: the input's magnitude record is required");
    const DualOut dual = {n1, act1, y2, act2};
    return conv_fwd_impl(d, x, reinterpret_cast<const float*>(w_planes_f16), scale, shift, nullptr, nullptr, y1, &dual, nullptr, 0, stream, FRCNN_ENGINE_H3,
                         amax_args(x_amax, y1_amax, y2_amax));
}

int frcnn_conv2d_fwd_h3_planes(const frcnn_conv_desc* d, const float* x, const frcnn_h3_planes* x_planes, const float* x_amax, const void* w_planes_f16,
                               const float* scale, const float* shift, const float* residual, const float* residual_amax,
                               float* y, float* y_amax, const frcnn_h3_planes* y_planes, float bound_c, float bound_d, void* stream) {
    return frcnn_conv2d_fwd_h3_planes_res(d, x, x_planes, x_amax, w_planes_f16, scale, shift, residual, nullptr, residual_amax, y, y_amax, y_planes, bound_c, bound_d, stream);
}

int frcnn_conv2d_roi_res_available(const frcnn_conv_desc* d, int engine, int x_is_planes) {
    if (!d) return fail(FRCNN_E_ARG, "conv2d_roi_res_available: null descriptor");
    if (engine != FRCNN_ENGINE_NATIVE && engine != FRCNN_ENGINE_X6 && engine != FRCNN_ENGINE_H3) return fail(FRCNN_E_ARG, "conv2d_roi_res_available: unknown engine %d", engine);
    return roi_res_available(d, engine, x_is_planes != 0);
}

int frcnn_conv2d_fwd_h3_roi_res(const frcnn_conv_desc* d, const float* x, const frcnn_h3_planes* x_planes, const float* x_amax,
                                const void* w_planes_f16, const float* scale, const float* shift, const frcnn_roi_res* res,
                                const float* residual_amax, float* y, float* y_amax, const frcnn_h3_planes* y_planes,
                                float bound_c, float bound_d, void* stream) {
    return conv_h3_planes_impl(d, x, x_planes, x_amax, w_planes_f16, scale, shift, nullptr, nullptr, res, residual_amax, y, y_amax, y_planes, bound_c, bound_d, stream);
}

int frcnn_conv2d_fwd_h3_planes_res(const frcnn_conv_desc* d, const float* x, const frcnn_h3_planes* x_planes, const float* x_amax, const void* w_planes_f16,
                                   const float* scale, const float* shift, const float* residual, const frcnn_h3_planes* residual_planes,
                                   const float* residual_amax, float* y, float* y_amax, const frcnn_h3_planes* y_planes, float bound_c, float bound_d,
                                   void* stream) {
    return conv_h3_planes_impl(d, x, x_planes, x_amax, w_planes_f16, scale, shift, residual, residual_planes, nullptr, residual_amax, y, y_amax, y_planes, bound_c, bound_d, stream);
}

}  // extern "C"

// frcnn_conv2d_fwd_h3_planes_res / frcnn_conv2d_fwd_h3_roi_res: the residual as an f32 tensor, as planes or (`gathered`) resampled from a map
static int conv_h3_planes_impl(const frcnn_conv_desc* d, const float* x, const frcnn_h3_planes* x_planes, const float* x_amax, const void* w_planes_f16,
                               const float* scale, const float* shift, const float* residual, const frcnn_h3_planes* residual_planes,
                               const frcnn_roi_res* gathered, const float* residual_amax, float* y, float* y_amax, const frcnn_h3_planes* y_planes,
                               float bound_c, float bound_d, void* stream, const frcnn_rowmap* rowmap) {
    if (gathered) {
        auto a16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
        if (!gathered->map || !gathered->taps || gathered->map_rows <= 0 || gathered->reserved != 0)
            return fail(FRCNN_E_ARG, "conv2d_fwd_h3_roi_res: map, tap table and map_rows > 0 required (reserved = 0)");
        if (!a16(gathered->map) || !a16(gathered->taps) || !a16(gathered->fill)) return fail(FRCNN_E_ARG, "conv2d_fwd_h3_roi_res: 16-byte aligned map, tap table and fill required");
    }
    if (!x_amax) return fail(FRCNN_E_ARG, "conv2d_fwd_h3_planes: the input's magnitude record is required");
    if (residual && residual_planes) return fail(FRCNN_E_ARG, "conv2d_fwd_h3_planes: the residual as an f32 tensor OR as planes");
    if (residual_planes && (!residual_planes->planes || !residual_planes->exponent || (reinterpret_cast<uintptr_t>(residual_planes->planes) & 15)))
        return fail(FRCNN_E_ARG, "conv2d_fwd_h3_planes: incomplete or misaligned residual planes");
    if ((x != nullptr) == (x_planes != nullptr)) return fail(FRCNN_E_ARG, "conv2d_fwd_h3_planes: exactly one of x / x_planes");
    if (!y && !y_planes) return fail(FRCNN_E_ARG, "conv2d_fwd_h3_planes: no output");
    if (x_planes && (!x_planes->planes || !x_planes->exponent)) return fail(FRCNN_E_ARG, "conv2d_fwd_h3_planes: incomplete input planes");
    if (y_planes && (!y_planes->planes || !y_planes->exponent || !(bound_c >= 0.0f) || !(bound_d >= 0.0f) || ((residual || residual_planes || gathered) && !residual_amax)))
        return fail(FRCNN_E_ARG, "conv2d_fwd_h3_planes: output planes need their buffers, the filter's bound constants and, with a residual, its magnitude record");
    auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    if ((x_planes && !al16(x_planes->planes)) || (y_planes && !al16(y_planes->planes))) return fail(FRCNN_E_ARG, "conv2d_fwd_h3_planes: 16-byte aligned planes required");
    ConvArgs rg = amax_args(x_amax, y_amax);
    if (x_planes) { rg.x_planes = x_planes->planes; rg.x_pexp = x_planes->exponent; }
    if (y_planes) { rg.y_planes = y_planes->planes; rg.y_pexp = y_planes->exponent; rg.res_amax = (residual || residual_planes || gathered) ? residual_amax : nullptr; rg.bound_c = bound_c; rg.bound_d = bound_d; }
    if (residual_planes) { rg.res_planes = residual_planes->planes; rg.res_pexp = residual_planes->exponent; }
    if (gathered) { rg.res_map = gathered->map; rg.res_taps = gathered->taps; rg.res_fill = gathered->fill; rg.res_map_rows = gathered->map_rows; }
    if (rowmap) { rg.row_map = rowmap->row_map; rg.tile_taps = rowmap->tile_taps; rg.map_rows = rowmap->rows; }
    return conv_fwd_impl(d, x, reinterpret_cast<const float*>(w_planes_f16), scale, shift, residual, nullptr, y, nullptr, nullptr, 0, stream, FRCNN_ENGINE_H3, rg);
}
