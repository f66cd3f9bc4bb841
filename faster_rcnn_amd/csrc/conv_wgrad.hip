// Training-side companions of the f32 convolution (conv_igemm.hip): the input-gradient filter pack, the batched refresh of every
// layer's packed forms after an optimiser step, bias gradients (column sums) and the weight gradient on the matrix cores -- one
// layer at a time (frcnn_conv2d_wgrad*) or every layer of a step in batched launches (frcnn_conv2d_wgrad_batch).
#include "conv_f32_common.h"

namespace frcnn {

// ------------------------------------------------------------------------------------
// Backward of a stride-1 convolution w.r.t. its input = a forward convolution of the output
// gradient with the filter transposed (Cin <-> Cout) and flipped in both taps.  The per-channel
// epilogue scale s[co] of the forward layer (folded BatchNorm) multiplies the incoming gradient,
// which is the same as scaling the transposed filter's INPUT channel co, so it is folded here and
// the dgrad launch is an ordinary frcnn_conv2d_fwd on these weights.
//   w'[r'][s'][co][ci] = w[R-1-r'][S-1-s'][ci][co] * s[co]      (conv' has Cin' = Cout, Cout' = Cin)
__device__ __forceinline__ float pack_dgrad_elem(const float* w, const float* scale, int R, int S, int Cin, int Cout, int Kpad, size_t i) {
    const int RS = R * S;                                   // rows = Cout' = Cin, k over (co chunk, tap', co)
    const int k = (int)(i % Kpad), ci = (int)(i / Kpad);
    int tap, co;
    if ((Cout % BK) == 0) { const int j = k % BK, kc = k / BK; tap = kc % RS; co = (kc / RS) * BK + j; }
    else if (Cout == 3) { tap = k >> 2; co = k & 3; if (co == 3 || tap >= RS) return 0.0f; }
    else { if (k >= RS * Cout) return 0.0f; tap = k / Cout; co = k % Cout; }
    const int r = R - 1 - tap / S, sx = S - 1 - tap % S;
    return w[((size_t)(r * S + sx) * Cin + ci) * Cout + co] * (scale ? scale[co] : 1.0f);
}
__global__ void k_pack_dgrad(const float* w, const float* scale, int R, int S, int Cin, int Cout, int Kpad, float* out) {
    const size_t total = (size_t)Cin * Kpad;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        out[i] = pack_dgrad_elem(w, scale, R, S, Cin, Cout, Kpad, i);
}

// One launch re-derives EVERY trainable layer's device-side forms from the fp32 master weights after an
// optimiser step: forward pack, input-gradient pack and the folded epilogue shift.  The job table rides in
// the kernel arguments (no table upload); blockIdx.y = job.
constexpr int REFRESH_JOBS = 32;
// Workgroups are dealt out in proportion to each job's size (first_block: prefix over the jobs): with a fixed 96 per job
// the 4.7 M-element RPN filter kept 96 workgroups busy long after the 1x1 layers' had left (159 us per fp32 RPN step).
struct RefreshTable { frcnn_pack_job job[REFRESH_JOBS]; int first_block[REFRESH_JOBS + 1]; int n; };
static int refresh_blocks(const frcnn_pack_job& j) {
    const long long elems = (long long)j.kh * j.kw * j.cin * j.cout;
    long long g = (elems + 2047) / 2048;              // (round 6: 8192 per workgroup left the dense layer's element-wise input-gradient pack on 26 workgroups)
    // (at least 16 workgroups: the small f32 layers of a mixed-precision step -- rpn_out_cls / rpn_out_bbreg, 512 -> 9 / 36 -- are a
    //  launch of their own whose 16 transposing tiles went through 4 workgroups one after the other: 24-33 us of a 1.2 ms step)
    return (int)(g < 16 ? 16 : (g > 2048 ? 2048 : g));
}
__global__ void __launch_bounds__(256) k_refresh_packed(const RefreshTable t) {
    int ji = 0;
    while (ji + 1 < t.n && (int)blockIdx.x >= t.first_block[ji + 1]) ++ji;
    const frcnn_pack_job& j = t.job[ji];
    const int bx = (int)blockIdx.x - t.first_block[ji], gsz = t.first_block[ji + 1] - t.first_block[ji];
    const int RS = j.kh * j.kw;
    const size_t stride = (size_t)gsz * blockDim.x, first = (size_t)bx * blockDim.x + threadIdx.x;
    if (j.packed && (j.cin % BK) == 0) {
        // HWIO has cout fastest, the packed rows have the 32 channels of a chunk fastest: transpose 32 x 64
        // (channel x cout) tiles through LDS so both the reads (256 B) and the writes (128 B) are whole segments
        __shared__ float tile[BK][65];
        const int Kpad = RS * j.cin, nblk = (j.cout + 63) / 64, ntiles = RS * (j.cin / BK) * nblk;
        const int lane = threadIdx.x & 63, jr = threadIdx.x >> 6, wn = threadIdx.x >> 3, j4 = (threadIdx.x & 7) * 4;
        for (int tl = bx; tl < ntiles; tl += gsz) {
            const int nb = tl % nblk, kc = tl / nblk, tap = kc % RS, cc = kc / RS, n0 = nb * 64;
#pragma unroll
            for (int pp = 0; pp < 8; ++pp) {
                const int c = jr + 4 * pp;
                tile[c][lane] = n0 + lane < j.cout ? j.w_hwio[((size_t)tap * j.cin + cc * BK + c) * j.cout + n0 + lane] : 0.0f;
            }
            __syncthreads();
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
                const int n = wn + 32 * pass;
                if (n0 + n < j.cout)
                    *reinterpret_cast<float4*>(j.packed + (size_t)(n0 + n) * Kpad + kc * BK + j4) =
                        make_float4(tile[j4][n], tile[j4 + 1][n], tile[j4 + 2][n], tile[j4 + 3][n]);
            }
            __syncthreads();
        }
    } else if (j.packed) {
        const int Kpad = packed_k(RS, j.cin);
        const size_t total = (size_t)j.cout * Kpad;
        for (size_t i = first; i < total; i += stride) j.packed[i] = pack_hwio_elem(j.w_hwio, RS, j.cin, j.cout, Kpad, i);
    }
    if (j.packed_dgrad) {
        const int Kpad = packed_k(RS, j.cout);
        const size_t total = (size_t)j.cin * Kpad;
        for (size_t i = first; i < total; i += stride) j.packed_dgrad[i] = pack_dgrad_elem(j.w_hwio, j.scale, j.kh, j.kw, j.cin, j.cout, Kpad, i);
    }
    if (j.shift)
        for (size_t i = first; i < (size_t)j.cout; i += stride)
            j.shift[i] = (j.bias ? j.bias[i] : 0.0f) * (j.scale ? j.scale[i] : 1.0f) + (j.shift_const ? j.shift_const[i] : 0.0f);
}

// Bias gradients of many layers in ONE launch: out[co] = scale[co] * sum_m g[m][co].  A 1024-thread workgroup
// owns 64 columns of one job; its 16 waves stride over the rows (256-B coalesced reads) and are summed in a
// fixed order, so the result is reproducible.  blockIdx.x walks the (job, column group) pairs.
constexpr int COLSUM_JOBS = 64;
struct ColsumTable { frcnn_colsum_job job[COLSUM_JOBS]; int first_block[COLSUM_JOBS + 1]; int n; };
__global__ void __launch_bounds__(1024) k_colsum_batch(const ColsumTable t) {
    __shared__ float part[16][64];
    int ji = 0;
    while (ji + 1 < t.n && (int)blockIdx.x >= t.first_block[ji + 1]) ++ji;
    const frcnn_colsum_job& j = t.job[ji];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int co = ((int)blockIdx.x - t.first_block[ji]) * 64 + lane;
    float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f, v3 = 0.0f;
    if (co < j.cout && !j.g_is_bf16) {
        const float* g = reinterpret_cast<const float*>(j.g) + co;
        int m = wave;
        for (; m + 48 < j.m; m += 64) {
            v0 += g[(size_t)m * j.cout]; v1 += g[(size_t)(m + 16) * j.cout];
            v2 += g[(size_t)(m + 32) * j.cout]; v3 += g[(size_t)(m + 48) * j.cout];
        }
        for (; m < j.m; m += 16) v0 += g[(size_t)m * j.cout];
    } else if (co < j.cout) {
        const __bf16* g = reinterpret_cast<const __bf16*>(j.g) + co;
        int m = wave;
        for (; m + 48 < j.m; m += 64) {
            v0 += (float)g[(size_t)m * j.cout]; v1 += (float)g[(size_t)(m + 16) * j.cout];
            v2 += (float)g[(size_t)(m + 32) * j.cout]; v3 += (float)g[(size_t)(m + 48) * j.cout];
        }
        for (; m < j.m; m += 16) v0 += (float)g[(size_t)m * j.cout];
    }
    part[wave][lane] = (v0 + v1) + (v2 + v3);
    __syncthreads();
    if (wave == 0 && co < j.cout) {
        float s = 0.0f;
#pragma unroll
        for (int w = 0; w < 16; ++w) s += part[w][lane];
        j.out[co] = j.scale ? s * j.scale[co] : s;
    }
}

// ------------------------------------------------------------------------------------
// Weight gradient on the matrix cores:  dW[tap][ci][co] = s[co] * sum_m A[m][(tap,ci)] * G[m][co]
// (A = implicit im2col of the layer input x, G = gradient w.r.t. the layer's pre-activation
// output, m = output pixel).  The reduction index is the PIXEL, so both operands are staged
// [pixel][channel] exactly as they lie in HBM (NHWC) and the 32x32x2 MFMA reads them with
// conflict-free ds_read_b32 (lane = channel).  Workgroup = 4 waves = 64 (ci) x 64 (co) outputs of
// one filter tap; grid.z splits the pixel range, each slice writes its own partial slab and a
// second kernel reduces the slabs in a fixed order (bitwise reproducible; no float atomics).
struct WgradArgs {
    const void* x; const void* g; float* partial;            // x / g: f32, or bf16 for the IN_BF16 instantiation
    int n_img, H, W, Cin, Cout, R, S, stride, pad_top, pad_left, Ho, Wo, M;
    int m_per_slice;
};

constexpr int WG_MC = 32;                 // pixels per staged chunk
constexpr int WG_LD = 64 + 4;             // LDS row stride in floats (272 B keeps 16-B alignment for the b128 stores)

// IN_BF16: activations and gradients arrive in bf16 (mixed-precision training); they are widened while being
// staged, the products accumulate in f32 on the same f32-input MFMA, dW leaves in f32 for the master weights.
__device__ __forceinline__ f32x4 load4_bf16(const __bf16* p) {
    const uint2 raw = *reinterpret_cast<const uint2*>(p);                 // 4 x bf16 = 8 bytes
    f32x4 v;
    v[0] = __uint_as_float(raw.x << 16); v[1] = __uint_as_float(raw.x & 0xffff0000u);
    v[2] = __uint_as_float(raw.y << 16); v[3] = __uint_as_float(raw.y & 0xffff0000u);
    return v;
}

template <bool IN_BF16>
__device__ __forceinline__ void wgrad_body_f32(const WgradArgs& p, int bx, int by, int bz) {
    __shared__ __attribute__((aligned(16))) float Xs[2][WG_MC][WG_LD];
    __shared__ __attribute__((aligned(16))) float Gs[2][WG_MC][WG_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wk = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
    const int ci_tiles = (p.Cin + 63) / 64;
    const int tap = bx / ci_tiles, ci0 = (bx % ci_tiles) * 64;
    const int r_tap = tap / p.S, s_tap = tap % p.S;
    const int co0 = by * 64;
    const int m_begin = bz * p.m_per_slice, m_end = min(p.M, m_begin + p.m_per_slice);

    // staging: 256 threads move 32 pixels x 64 channels (16 float4 per pixel) per operand per chunk
    const int srow = tid >> 4, scol = (tid & 15) * 4;      // rows srow and srow+16
    f32x4 rx[2], rg[2];
    auto load = [&](int mc) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int m = mc + srow + 16 * q;
            f32x4 vx = {0, 0, 0, 0}, vg = {0, 0, 0, 0};
            if (m < m_end) {
                const int wo = m % p.Wo, t = m / p.Wo, ho = t % p.Ho, img = t / p.Ho;
                const int hi = ho * p.stride - p.pad_top + r_tap, wi = wo * p.stride - p.pad_left + s_tap;
                if ((unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W) {
                    const size_t off = (((size_t)img * p.H + hi) * p.W + wi) * p.Cin + ci0 + scol;
                    if constexpr (IN_BF16) {
                        const __bf16* src = reinterpret_cast<const __bf16*>(p.x) + off;
                        if (ci0 + scol + 3 < p.Cin) vx = load4_bf16(src);
                        else for (int e = 0; e < 4; ++e) if (ci0 + scol + e < p.Cin) vx[e] = (float)src[e];
                    } else {
                        const float* src = reinterpret_cast<const float*>(p.x) + off;
                        if (ci0 + scol + 3 < p.Cin) vx = *reinterpret_cast<const f32x4*>(src);
                        else for (int e = 0; e < 4; ++e) if (ci0 + scol + e < p.Cin) vx[e] = src[e];
                    }
                }
                const size_t goff = (size_t)m * p.Cout + co0 + scol;
                if constexpr (IN_BF16) {
                    const __bf16* gs = reinterpret_cast<const __bf16*>(p.g) + goff;
                    if (co0 + scol + 3 < p.Cout && (p.Cout & 3) == 0) vg = load4_bf16(gs);
                    else for (int e = 0; e < 4; ++e) if (co0 + scol + e < p.Cout) vg[e] = (float)gs[e];
                } else {
                    const float* gs = reinterpret_cast<const float*>(p.g) + goff;
                    if (co0 + scol + 3 < p.Cout && (p.Cout & 3) == 0) vg = *reinterpret_cast<const f32x4*>(gs);
                    else for (int e = 0; e < 4; ++e) if (co0 + scol + e < p.Cout) vg[e] = gs[e];
                }
            }
            rx[q] = vx; rg[q] = vg;
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            *reinterpret_cast<f32x4*>(&Xs[buf][srow + 16 * q][scol]) = rx[q];
            *reinterpret_cast<f32x4*>(&Gs[buf][srow + 16 * q][scol]) = rg[q];
        }
    };

    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;

    const int n_chunks = (m_end - m_begin + WG_MC - 1) / WG_MC;
    if (n_chunks > 0) {
        load(m_begin);
        store(0);
        __syncthreads();
        for (int c = 0; c < n_chunks; ++c) {
            const int buf = c & 1;
            if (c + 1 < n_chunks) load(m_begin + (c + 1) * WG_MC);
#pragma unroll
            for (int st = 0; st < WG_MC / 2; ++st) {
                const float a = Xs[buf][2 * st + lh][wk * 32 + li];
                const float b = Gs[buf][2 * st + lh][wn * 32 + li];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
            }
            if (c + 1 < n_chunks) store(buf ^ 1);
            __syncthreads();
        }
    }
    // partial slab layout = HWIO: [slice][tap][ci][co]
    const int co = co0 + wn * 32 + li;
    if (co < p.Cout) {
        float* dst = p.partial + ((size_t)bz * p.R * p.S + tap) * p.Cin * p.Cout;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int ci = ci0 + wk * 32 + 4 * lh + (e & 3) + 8 * (e >> 2);
            if (ci < p.Cin) dst[(size_t)ci * p.Cout + co] = acc[e];
        }
    }
}

template <bool IN_BF16>
__global__ void __launch_bounds__(256) k_conv_wgrad_f32(const WgradArgs p) {
    wgrad_body_f32<IN_BF16>(p, blockIdx.x, blockIdx.y, blockIdx.z);
}

// The 128 (ci) x 128 (co) form of the f32 weight gradient, for layers with cin, cout >= 128 (every trainable layer of the
// ResNet stages 3-5, the RPN and VGG from block 2 on).  The 64x64 body above reads one A and one B value per MFMA
// (ds_read_b32, and its 68-float rows put the two k-rows of a read 4 banks apart: 2-way conflicts) and moves 16 KB of
// operands per 262 kFLOP -- ~70 TFLOP/s on the training steps' layers (profiles/round2_lab/train_trace_by_grid_f32_*).
// Here each wave owns 64 x 64: its two 32-wide row tiles are the EVEN and the ODD channels of its 64 (the output-row
// permutation is free, the epilogue undoes it), so ONE ds_read_b64 per operand feeds four MFMAs; a b64 read is served
// half-wave by half-wave, each half one unpadded 128-float row segment = every bank once.  Operand traffic per FLOP
// halves, the chunk (32 pixels) is 64 MFMAs = 4096 cycles per wave against 8 + 8 staging copies per thread, two
// workgroups (64 KB of LDS each) share a CU.  Pixel coordinates advance incrementally (no division in the loop);
// halo / tail / channel edges ride on the buffer descriptors.  Slab layout and the fixed-order slice reduction are
// unchanged; the pixel order inside a slice is the 64x64 body's, only the slice boundaries move with the tile count.
constexpr int WGB_LD = 128;
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void wgrad_body_f32_big(const WgradArgs& p, int bx, int by, int bz) {
    __shared__ __attribute__((aligned(16))) float Xs[2][WG_MC][WGB_LD];
    __shared__ __attribute__((aligned(16))) float Gs[2][WG_MC][WGB_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wk = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
    const int ci_tiles = (p.Cin + 127) / 128;
    const int tap = bx / ci_tiles, ci0 = (bx % ci_tiles) * 128;
    const int r_tap = tap / p.S, s_tap = tap % p.S;
    const int co0 = by * 128;
    const int m_begin = bz * p.m_per_slice, m_end = min(p.M, m_begin + p.m_per_slice);

    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(p.x), 0, (int)((size_t)p.n_img * p.H * p.W * p.Cin * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t grsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(p.g), 0, (int)((size_t)p.M * p.Cout * 4), 0x00020000);

    // staging: 256 threads move 32 pixels x 128 channels per operand per chunk: 8 rows per pass, 4 passes
    const int srow = tid >> 5, scol = (tid & 31) * 4;
    const bool ci_ok = ci0 + scol < p.Cin, co_ok = co0 + scol < p.Cout;
    const float inv_wo = 1.0f / (float)p.Wo, inv_ho = 1.0f / (float)p.Ho;
    // n / d for 0 <= n < 2^23 (the host keeps M below that): the float product is within one of the quotient
    auto divmod = [](int n, int d, float inv, int& q, int& r) {
        q = (int)((float)n * inv); r = n - q * d;
        if (r < 0) { r += d; --q; }
        if (r >= d) { r -= d; ++q; }
    };
    int mc = m_begin;
    i32x4 rx[4], rg[4];
    auto load = [&]() {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int m = mc + srow + 8 * q;
            int wo, t, ho, img;
            divmod(m, p.Wo, inv_wo, t, wo);
            divmod(t, p.Ho, inv_ho, img, ho);
            const int hi = ho * p.stride - p.pad_top + r_tap, wi = wo * p.stride - p.pad_left + s_tap;
            const bool in = m < m_end && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
            const unsigned xoff = (unsigned)(((img * p.H + hi) * p.W + wi) * p.Cin + ci0 + scol) * 4u;
            rx[q] = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, in && ci_ok ? xoff : OOB_OFFSET, 0, 0);
            const unsigned goff = (unsigned)(m * p.Cout + co0 + scol) * 4u;
            rg[q] = __builtin_amdgcn_raw_buffer_load_b128(grsrc, m < m_end && co_ok ? goff : OOB_OFFSET, 0, 0);
        }
        mc += WG_MC;
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            *reinterpret_cast<i32x4*>(&Xs[buf][srow + 8 * q][scol]) = rx[q];
            *reinterpret_cast<i32x4*>(&Gs[buf][srow + 8 * q][scol]) = rg[q];
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

    // chunk c multiplies from LDS buffer c & 1 while chunk c+1 (in registers since the previous iteration) moves into the
    // other buffer and chunk c+2 is requested: every global load has a whole chunk (64 MFMAs = 4096 cycles) to land.
    // Loads past the slice carry m >= m_end: zeros.
    const int n_chunks = (m_end - m_begin + WG_MC - 1) / WG_MC;
    if (n_chunks > 0) {
        load();
        store(0);
        load();
        __syncthreads();
        for (int c = 0; c < n_chunks; ++c) {
            const int buf = c & 1;
            store(buf ^ 1);
            load();
            const float* xa = &Xs[buf][lh][wk * 64 + 2 * li];
            const float* gb = &Gs[buf][lh][wn * 64 + 2 * li];
            f32x2 fa[WG_MC / 2], fb[WG_MC / 2];
#pragma unroll
            for (int st = 0; st < WG_MC / 2; ++st) {
                fa[st] = *reinterpret_cast<const f32x2*>(xa + 2 * st * WGB_LD);
                fb[st] = *reinterpret_cast<const f32x2*>(gb + 2 * st * WGB_LD);
            }
#pragma unroll
            for (int st = 0; st < WG_MC / 2; ++st) {
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[st][0], fb[st][0], acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[st][0], fb[st][1], acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[st][1], fb[st][0], acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[st][1], fb[st][1], acc[1][1], 0, 0, 0);
            }
            // issue order: fragment reads run ahead of the MFMAs that need them, the LDS stores ride behind the first
            // MFMAs, the address arithmetic and the eight global loads behind the middle ones
            SGB(SG_DS_RD, 4);
#pragma unroll
            for (int q = 0; q < 8; ++q) { SGB(SG_MFMA, 1); SGB(SG_DS_WR, 1); SGB(SG_DS_RD, 1); }
#pragma unroll
            for (int q = 8; q < 28; ++q) { SGB(SG_MFMA, 1); SGB(SG_DS_RD, 1); }
#pragma unroll
            for (int q = 28; q < 36; ++q) { SGB(SG_MFMA, 1); SGB(SG_VALU, 16); SGB(SG_VMEM_RD, 1); }
#pragma unroll
            for (int q = 36; q < 64; ++q) SGB(SG_MFMA, 1);
            __syncthreads();
        }
    }
    // partial slab layout = HWIO: [slice][tap][ci][co]; tile (i, j) of this wave = channels 2*row + i, 2*col + j
    float* dst = p.partial + ((size_t)bz * p.R * p.S + tap) * p.Cin * p.Cout;
    const int co = co0 + wn * 64 + 2 * li;
    if (co < p.Cout) {                               // cout is a multiple of 4: the pair is inside together
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int ci = ci0 + wk * 64 + 2 * (4 * lh + (e & 3) + 8 * (e >> 2)) + i;
                if (ci < p.Cin) {
                    f32x2 v; v[0] = acc[i][0][e]; v[1] = acc[i][1][e];
                    *reinterpret_cast<f32x2*>(dst + (size_t)ci * p.Cout + co) = v;
                }
            }
    }
}

// Weight gradient on the bf16 matrix cores (mixed-precision training): x and g arrive in bf16, [pixel][channel] as
// they lie in NHWC.  The reduction index is the PIXEL, i.e. both MFMA operands are k-strided in memory; they are
// staged untransposed (coalesced 16-byte copies, 192-byte LDS rows) and read back with ds_read_b64_tr_b16, the
// gfx950 transposing LDS read: a 16-lane group fetches 4 pixel rows x 16 channels and each lane receives one
// channel's 4 pixels, so two reads form the 8-pixel operand of v_mfma_f32_32x32x16_bf16.  The 192-byte row stride
// puts the 4 rows of a half-wave's block on disjoint 16-bank groups (conflict-free).  Same grid, slabs and
// fixed-order reduction as the f32 kernel; 16x its MFMA rate.
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef short i16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8w __attribute__((ext_vector_type(8)));
constexpr int WB_MC = 64;                 // pixels per staged chunk
constexpr int WB_ROW = 192;               // LDS row stride in bytes (128 B of channels + 64 B)

__device__ __forceinline__ void wgrad_body_bf16(const WgradArgs& p, int bx, int by, int bz) {
    __shared__ __attribute__((aligned(16))) char Xs[2][WB_MC][WB_ROW];
    __shared__ __attribute__((aligned(16))) char Gs[2][WB_MC][WB_ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wk = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
    const int ci_tiles = (p.Cin + 63) / 64;
    const int tap = bx / ci_tiles, ci0 = (bx % ci_tiles) * 64;
    const int r_tap = tap / p.S, s_tap = tap % p.S;
    const int co0 = by * 64;
    const int m_begin = bz * p.m_per_slice, m_end = min(p.M, m_begin + p.m_per_slice);
    const __bf16* xg = reinterpret_cast<const __bf16*>(p.x);
    const __bf16* gg = reinterpret_cast<const __bf16*>(p.g);

    // staging: 256 threads move 64 pixels x 64 channels (8 x 16 B per pixel) per operand per chunk, two passes of 32 rows
    const int srow = tid >> 3, scol = (tid & 7) * 8;       // channel offset inside the 64-wide tile
    i32x4 rx[2], rg[2];
    auto load = [&](int mc) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int m = mc + srow + 32 * q;
            i32x4 vx = {0, 0, 0, 0}, vg = {0, 0, 0, 0};
            if (m < m_end) {
                const int wo = m % p.Wo, t = m / p.Wo, ho = t % p.Ho, img = t / p.Ho;
                const int hi = ho * p.stride - p.pad_top + r_tap, wi = wo * p.stride - p.pad_left + s_tap;
                if ((unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W && ci0 + scol < p.Cin)
                    vx = *reinterpret_cast<const i32x4*>(xg + (((size_t)img * p.H + hi) * p.W + wi) * p.Cin + ci0 + scol);
                if (co0 + scol < p.Cout) vg = *reinterpret_cast<const i32x4*>(gg + (size_t)m * p.Cout + co0 + scol);
            }
            rx[q] = vx; rg[q] = vg;
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            *reinterpret_cast<i32x4*>(&Xs[buf][srow + 32 * q][scol * 2]) = rx[q];
            *reinterpret_cast<i32x4*>(&Gs[buf][srow + 32 * q][scol * 2]) = rg[q];
        }
    };

    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;

    // transposed-read addressing: lane 4q+p of a 16-lane group supplies (row q, channels 4p..4p+3) of its block;
    // lanes 0-15 / 16-31 take channels 0-15 / 16-31 of the wave's 32, lanes 32-63 the next 8 pixels (lh)
    const int g16 = lane & 15, tq = g16 >> 2, tp = g16 & 3, cblk = ((lane >> 4) & 1) * 16;
    const int a_byte = (8 * lh + tq) * WB_ROW + (wk * 32 + cblk + 4 * tp) * 2;
    const int b_byte = (8 * lh + tq) * WB_ROW + (wn * 32 + cblk + 4 * tp) * 2;
    typedef i16x4 __attribute__((address_space(3))) * lds_i16x4;

    const int n_chunks = (m_end - m_begin + WB_MC - 1) / WB_MC;
    if (n_chunks > 0) {
        load(m_begin);
        store(0);
        __syncthreads();
        for (int c = 0; c < n_chunks; ++c) {
            const int buf = c & 1;
            if (c + 1 < n_chunks) load(m_begin + (c + 1) * WB_MC);
            const char* xa = &Xs[buf][0][0] + a_byte;
            const char* gb = &Gs[buf][0][0] + b_byte;
#pragma unroll
            for (int st = 0; st < WB_MC / 16; ++st) {       // 16 pixels per MFMA
                const i16x4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4)(xa + (16 * st) * WB_ROW));
                const i16x4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4)(xa + (16 * st + 4) * WB_ROW));
                const i16x4 b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4)(gb + (16 * st) * WB_ROW));
                const i16x4 b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4)(gb + (16 * st + 4) * WB_ROW));
                const i16x8 av = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
                const i16x8 bv = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8w, av), __builtin_bit_cast(bf16x8w, bv), acc, 0, 0, 0);
            }
            if (c + 1 < n_chunks) store(buf ^ 1);
            __syncthreads();
        }
    }
    const int co = co0 + wn * 32 + li;
    if (co < p.Cout) {
        float* dst = p.partial + ((size_t)bz * p.R * p.S + tap) * p.Cin * p.Cout;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int ci = ci0 + wk * 32 + 4 * lh + (e & 3) + 8 * (e >> 2);
            if (ci < p.Cin) dst[(size_t)ci * p.Cout + co] = acc[e];
        }
    }
}

__global__ void __launch_bounds__(256) k_conv_wgrad_bf16(const WgradArgs p) {
    wgrad_body_bf16(p, blockIdx.x, blockIdx.y, blockIdx.z);
}

// Weight gradient of an f32 layer on the bf16 matrix cores by exact three-way operand splitting (the forward engine of
// conv_x6.hip, for dW = X^T . G): BOTH operands arrive in f32 ([pixel][channel] as they lie in NHWC) and are split as they move
// into LDS -- x = x1 + x2 + x3 with bf16 pieces, each subtraction exact -- into three planes of 32 pixels x 128 channels
// (320-byte rows: the four pixel rows of a transposing read land on disjoint 16-bank groups).  The reduction index is the pixel,
// so fragments come back through ds_read_b64_tr_b16 as in the bf16 body above; the six partial products with i + j <= 4 go
// through v_mfma_f32_32x32x16_bf16, smallest first, into the same f32 accumulators.  Tile, grid, slabs, slice boundaries and
// the fixed-order reduction are those of the 128x128 f32 body (kind 3); ONE LDS buffer of 60 KB (two workgroups per CU), the
// next chunk's operands wait in registers.  Error against fp64: the native f32 kernel's level (tests/test_conv_bwd_gpu.py).
constexpr int WX_ROW = 320;               // LDS row stride in bytes: 128 channels x 2 B + 64
typedef int i32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void wg_split3(const f32x4 v, i32x2& h, i32x2& m, i32x2& l) {
    typedef __bf16 bf16x4s __attribute__((ext_vector_type(4)));
    bf16x4s hh, mm, ll;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        hh[e] = (__bf16)v[e];
        const float r1 = v[e] - (float)hh[e];
        mm[e] = (__bf16)r1;
        ll[e] = (__bf16)(r1 - (float)mm[e]);
    }
    h = __builtin_bit_cast(i32x2, hh); m = __builtin_bit_cast(i32x2, mm); l = __builtin_bit_cast(i32x2, ll);
}

__device__ __forceinline__ void wgrad_body_x6_big(const WgradArgs& p, int bx, int by, int bz) {
    __shared__ __attribute__((aligned(16))) char Xp[3][WG_MC][WX_ROW];
    __shared__ __attribute__((aligned(16))) char Gp[3][WG_MC][WX_ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wk = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
    const int ci_tiles = (p.Cin + 127) / 128;
    const int tap = bx / ci_tiles, ci0 = (bx % ci_tiles) * 128;
    const int r_tap = tap / p.S, s_tap = tap % p.S;
    const int co0 = by * 128;
    const int m_begin = bz * p.m_per_slice, m_end = min(p.M, m_begin + p.m_per_slice);

    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(p.x), 0, (int)((size_t)p.n_img * p.H * p.W * p.Cin * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t grsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(p.g), 0, (int)((size_t)p.M * p.Cout * 4), 0x00020000);

    // staging: 256 threads move 32 pixels x 128 channels per operand per chunk: 8 rows per pass, 4 passes (the f32 body's walk)
    const int srow = tid >> 5, scol = (tid & 31) * 4;
    const bool ci_ok = ci0 + scol < p.Cin, co_ok = co0 + scol < p.Cout;
    const float inv_wo = 1.0f / (float)p.Wo, inv_ho = 1.0f / (float)p.Ho;
    auto divmod = [](int n, int d, float inv, int& q, int& r) {
        q = (int)((float)n * inv); r = n - q * d;
        if (r < 0) { r += d; --q; }
        if (r >= d) { r -= d; ++q; }
    };
    int mc = m_begin;
    i32x4 rx[4], rg[4];
    auto load = [&]() {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int m = mc + srow + 8 * q;
            int wo, t, ho, img;
            divmod(m, p.Wo, inv_wo, t, wo);
            divmod(t, p.Ho, inv_ho, img, ho);
            const int hi = ho * p.stride - p.pad_top + r_tap, wi = wo * p.stride - p.pad_left + s_tap;
            const bool in = m < m_end && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
            const unsigned xoff = (unsigned)(((img * p.H + hi) * p.W + wi) * p.Cin + ci0 + scol) * 4u;
            rx[q] = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, in && ci_ok ? xoff : OOB_OFFSET, 0, 0);
            const unsigned goff = (unsigned)(m * p.Cout + co0 + scol) * 4u;
            rg[q] = __builtin_amdgcn_raw_buffer_load_b128(grsrc, m < m_end && co_ok ? goff : OOB_OFFSET, 0, 0);
        }
        mc += WG_MC;
    };
    auto store = [&]() {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            i32x2 h, m, l;
            wg_split3(__builtin_bit_cast(f32x4, rx[q]), h, m, l);
            *reinterpret_cast<i32x2*>(&Xp[0][srow + 8 * q][scol * 2]) = h;
            *reinterpret_cast<i32x2*>(&Xp[1][srow + 8 * q][scol * 2]) = m;
            *reinterpret_cast<i32x2*>(&Xp[2][srow + 8 * q][scol * 2]) = l;
            wg_split3(__builtin_bit_cast(f32x4, rg[q]), h, m, l);
            *reinterpret_cast<i32x2*>(&Gp[0][srow + 8 * q][scol * 2]) = h;
            *reinterpret_cast<i32x2*>(&Gp[1][srow + 8 * q][scol * 2]) = m;
            *reinterpret_cast<i32x2*>(&Gp[2][srow + 8 * q][scol * 2]) = l;
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

    // transposed-read addressing (wgrad_body_bf16): lane 4q+p of a 16-lane group supplies (pixel row q, channels 4p..4p+3) of its
    // block; lanes 0-15 / 16-31 take channels 0-15 / 16-31 of a 32-channel tile, lanes 32-63 the next 8 pixels (lh)
    const int g16 = lane & 15, tq = g16 >> 2, tp = g16 & 3, cblk = ((lane >> 4) & 1) * 16;
    const int a_byte = (8 * lh + tq) * WX_ROW + (wk * 64 + cblk + 4 * tp) * 2;
    const int b_byte = (8 * lh + tq) * WX_ROW + (wn * 64 + cblk + 4 * tp) * 2;
    typedef i16x4 __attribute__((address_space(3))) * lds_i16x4;
    auto frag = [&](const char* base) {
        const i16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4)base);
        const i16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4)(base + 4 * WX_ROW));
        return __builtin_bit_cast(bf16x8w, __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7));
    };

    const int n_chunks = (m_end - m_begin + WG_MC - 1) / WG_MC;
    if (n_chunks > 0) {
        load();
        store();
        load();                                              // chunk 1 (zeros past the slice)
        __syncthreads();
        for (int c = 0; c < n_chunks; ++c) {
#pragma unroll
            for (int st = 0; st < WG_MC / 16; ++st) {        // 16 pixels per MFMA
                bf16x8w fa[3][2], fb[3][2];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl)
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        fa[pl][i] = frag(&Xp[pl][0][0] + a_byte + (16 * st) * WX_ROW + i * 64);
                        fb[pl][i] = frag(&Gp[pl][0][0] + b_byte + (16 * st) * WX_ROW + i * 64);
                    }
                constexpr int IA[6] = {2, 0, 1, 1, 0, 0}, IB[6] = {0, 2, 1, 0, 1, 0};      // smallest terms first
#pragma unroll
                for (int t = 0; t < 6; ++t)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[IA[t]][i], fb[IB[t]][j], acc[i][j], 0, 0, 0);
            }
            __syncthreads();                                 // everybody is done reading chunk c
            if (c + 1 < n_chunks) {
                store();                                     // chunk c + 1 (in registers since the previous iteration)
                load();                                      // chunk c + 2
            }
            __syncthreads();
        }
    }
    // partial slab layout = HWIO: [slice][tap][ci][co]; tile (i, j) of this wave = channels 32 i + row, 32 j + column
    float* dst = p.partial + ((size_t)bz * p.R * p.S + tap) * p.Cin * p.Cout;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int co = co0 + wn * 64 + 32 * j + li;
        if (co >= p.Cout) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int ci = ci0 + wk * 64 + 32 * i + 4 * lh + (e & 3) + 8 * (e >> 2);
                if (ci < p.Cin) dst[(size_t)ci * p.Cout + co] = acc[i][j][e];
            }
    }
}

// The 128 (ci) x 128 (co) form of the bf16 weight gradient (mixed-precision steps; layers with cin, cout >= 128): the tile and
// wave layout of the split-engine body above with ONE plane per operand -- each wave owns 64 x 64, eight transposing reads feed four
// MFMAs per 16 pixels (the 64x64 body: four reads per MFMA) -- 64 pixels per chunk in ONE 40 KB LDS buffer, the next chunk's
// operands waiting in registers.  Slabs, slice boundaries and the fixed-order reduction as everywhere.
constexpr int WB2_MC = 64;
__device__ __forceinline__ void wgrad_body_bf16_big(const WgradArgs& p, int bx, int by, int bz) {
    __shared__ __attribute__((aligned(16))) char Xb[WB2_MC][WX_ROW];
    __shared__ __attribute__((aligned(16))) char Gb[WB2_MC][WX_ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wk = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
    const int ci_tiles = (p.Cin + 127) / 128;
    const int tap = bx / ci_tiles, ci0 = (bx % ci_tiles) * 128;
    const int r_tap = tap / p.S, s_tap = tap % p.S;
    const int co0 = by * 128;
    const int m_begin = bz * p.m_per_slice, m_end = min(p.M, m_begin + p.m_per_slice);
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(p.x), 0, (int)((size_t)p.n_img * p.H * p.W * p.Cin * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t grsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(p.g), 0, (int)((size_t)p.M * p.Cout * 2), 0x00020000);

    // staging: 256 threads move 64 pixels x 128 channels (16 x 16 B per pixel) per operand per chunk: 16 rows per pass, 4 passes
    const int srow = tid >> 4, scol = (tid & 15) * 8;
    const bool ci_ok = ci0 + scol < p.Cin, co_ok = co0 + scol < p.Cout;
    const float inv_wo = 1.0f / (float)p.Wo, inv_ho = 1.0f / (float)p.Ho;
    auto divmod = [](int n, int d, float inv, int& q, int& r) {
        q = (int)((float)n * inv); r = n - q * d;
        if (r < 0) { r += d; --q; }
        if (r >= d) { r -= d; ++q; }
    };
    int mc = m_begin;
    i32x4 rx[4], rg[4];
    auto load = [&]() {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int m = mc + srow + 16 * q;
            int wo, t, ho, img;
            divmod(m, p.Wo, inv_wo, t, wo);
            divmod(t, p.Ho, inv_ho, img, ho);
            const int hi = ho * p.stride - p.pad_top + r_tap, wi = wo * p.stride - p.pad_left + s_tap;
            const bool in = m < m_end && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
            const unsigned xoff = (unsigned)(((img * p.H + hi) * p.W + wi) * p.Cin + ci0 + scol) * 2u;
            rx[q] = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, in && ci_ok ? xoff : OOB_OFFSET, 0, 0);
            const unsigned goff = (unsigned)(m * p.Cout + co0 + scol) * 2u;
            rg[q] = __builtin_amdgcn_raw_buffer_load_b128(grsrc, m < m_end && co_ok ? goff : OOB_OFFSET, 0, 0);
        }
        mc += WB2_MC;
    };
    auto store = [&]() {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            *reinterpret_cast<i32x4*>(&Xb[srow + 16 * q][scol * 2]) = rx[q];
            *reinterpret_cast<i32x4*>(&Gb[srow + 16 * q][scol * 2]) = rg[q];
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

    const int g16 = lane & 15, tq = g16 >> 2, tp = g16 & 3, cblk = ((lane >> 4) & 1) * 16;
    const int a_byte = (8 * lh + tq) * WX_ROW + (wk * 64 + cblk + 4 * tp) * 2;
    const int b_byte = (8 * lh + tq) * WX_ROW + (wn * 64 + cblk + 4 * tp) * 2;
    typedef i16x4 __attribute__((address_space(3))) * lds_i16x4;
    auto frag = [&](const char* base) {
        const i16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4)base);
        const i16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4)(base + 4 * WX_ROW));
        return __builtin_bit_cast(bf16x8w, __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7));
    };

    const int n_chunks = (m_end - m_begin + WB2_MC - 1) / WB2_MC;
    if (n_chunks > 0) {
        load();
        store();
        load();
        __syncthreads();
        for (int c = 0; c < n_chunks; ++c) {
#pragma unroll
            for (int st = 0; st < WB2_MC / 16; ++st) {
                bf16x8w fa[2], fb[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    fa[i] = frag(&Xb[0][0] + a_byte + (16 * st) * WX_ROW + i * 64);
                    fb[i] = frag(&Gb[0][0] + b_byte + (16 * st) * WX_ROW + i * 64);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
            }
            __syncthreads();
            if (c + 1 < n_chunks) {
                store();
                load();
            }
            __syncthreads();
        }
    }
    float* dst = p.partial + ((size_t)bz * p.R * p.S + tap) * p.Cin * p.Cout;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int co = co0 + wn * 64 + 32 * j + li;
        if (co >= p.Cout) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int ci = ci0 + wk * 64 + 32 * i + 4 * lh + (e & 3) + 8 * (e >> 2);
                if (ci < p.Cin) dst[(size_t)ci * p.Cout + co] = acc[i][j][e];
            }
    }
}

__global__ void __launch_bounds__(256) k_conv_wgrad_bf16_big(const WgradArgs p) {
    wgrad_body_bf16_big(p, blockIdx.x, blockIdx.y, blockIdx.z);
}

// dW = s[co] * sum over slices (fixed order); dbias[co] handled by k_colsum
__global__ void k_wgrad_reduce(const float* partial, int slices, size_t elems, int Cout, const float* scale, float* dw) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < elems; i += (size_t)gridDim.x * blockDim.x) {
        float v = 0.0f;
        for (int sidx = 0; sidx < slices; ++sidx) v += partial[(size_t)sidx * elems + i];
        dw[i] = scale ? v * scale[i % Cout] : v;
    }
}

// ------------------------------------------------------------------------------------
// The weight gradients of ALL trainable layers of a training step in one launch per operand kind, plus one launch for
// their slice reductions.  A step of the RPN / detector model has 22 / 32 trainable convolutions whose weight
// gradients are tiny GEMMs (stage 4: 1.25 - 2.8 GFLOP over 2 394 pixels): launched one by one, each paid its own
// ramp and tail (2 launches per layer, 28 us + 19 us on average for the 1x1 layers, the chip half empty) -- 1.4 ms of a
// 3.9 ms step.  Nothing reads a weight gradient before the optimiser, so the host queues them during the backward
// pass and issues them together: ~30 000 workgroups of mixed shapes keep every CU's four slots turning over.  The
// job table rides in the kernel arguments; a workgroup finds its job by scanning the block prefix.  Arithmetic, slab
// layout and the fixed slice order are those of the single-layer kernels: results are bit-identical.
constexpr int WGRAD_BATCH = 32;
struct WgradBatch { WgradArgs job[WGRAD_BATCH]; int first_block[WGRAD_BATCH + 1]; int gx[WGRAD_BATCH]; int gy[WGRAD_BATCH]; int n; };
struct WgradReduceJob { const float* partial; const float* scale; float* dw; unsigned long long elems; int slices, cout; };
struct WgradReduceBatch { WgradReduceJob job[2 * WGRAD_BATCH]; int first_block[2 * WGRAD_BATCH + 1]; int n; };   // workgroups in proportion to job size

template <int KIND>          // 0: f32 operands; 1: bf16 operands on the bf16 MFMA; 2: bf16 operands widened onto the f32 MFMA; 3: f32, 128x128 tiles; 4: f32 operands split onto the bf16 MFMA, 128x128 tiles; 5: bf16 operands, 128x128 tiles
__global__ void __launch_bounds__(256) k_conv_wgrad_batch(const WgradBatch t) {
    int j = 0;
    while (j + 1 < t.n && (int)blockIdx.x >= t.first_block[j + 1]) ++j;
    const int local = (int)blockIdx.x - t.first_block[j];
    const int bx = local % t.gx[j], r = local / t.gx[j], by = r % t.gy[j], bz = r / t.gy[j];
    if constexpr (KIND == 1) wgrad_body_bf16(t.job[j], bx, by, bz);
    else if constexpr (KIND == 3) wgrad_body_f32_big(t.job[j], bx, by, bz);
    else if constexpr (KIND == 4) wgrad_body_x6_big(t.job[j], bx, by, bz);
    else if constexpr (KIND == 5) wgrad_body_bf16_big(t.job[j], bx, by, bz);
    else wgrad_body_f32<KIND == 2>(t.job[j], bx, by, bz);
}

__global__ void __launch_bounds__(256) k_conv_wgrad_f32_big(const WgradArgs p) {
    wgrad_body_f32_big(p, blockIdx.x, blockIdx.y, blockIdx.z);
}

__global__ void __launch_bounds__(256) k_conv_wgrad_x6_big(const WgradArgs p) {
    wgrad_body_x6_big(p, blockIdx.x, blockIdx.y, blockIdx.z);
}

__global__ void __launch_bounds__(256) k_wgrad_reduce_batch(const WgradReduceBatch t) {
    int ji = 0;
    while (ji + 1 < t.n && (int)blockIdx.x >= t.first_block[ji + 1]) ++ji;
    const WgradReduceJob& j = t.job[ji];
    const size_t bx = (size_t)((int)blockIdx.x - t.first_block[ji]), gsz = (size_t)(t.first_block[ji + 1] - t.first_block[ji]);
    for (size_t i = bx * blockDim.x + threadIdx.x; i < j.elems; i += gsz * blockDim.x) {
        float v = 0.0f;
        for (int sidx = 0; sidx < j.slices; ++sidx) v += j.partial[(size_t)sidx * j.elems + i];
        j.dw[i] = j.scale ? v * j.scale[i % j.cout] : v;
    }
}

// dbias[co] = s[co] * sum_m G[m][co], two stages: (64 columns x 1 row slice) per workgroup into a
// partial table, then a fixed-order sum over the slices (reproducible).
constexpr int COLSUM_SLICES = 64;
__global__ void __launch_bounds__(256) k_colsum_partial(const float* g, int M, int Cout, int rows_per_slice, float* partial) {
    __shared__ float part[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int co = blockIdx.x * 64 + lane;
    const int m0 = blockIdx.y * rows_per_slice, m1 = min(M, m0 + rows_per_slice);
    float v = 0.0f;
    if (co < Cout) for (int m = m0 + wave; m < m1; m += 4) v += g[(size_t)m * Cout + co];
    part[wave][lane] = v;
    __syncthreads();
    if (wave == 0 && co < Cout) partial[(size_t)blockIdx.y * Cout + co] = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
}
__global__ void k_colsum_final(const float* partial, int slices, int Cout, const float* scale, float* out) {
    const int co = blockIdx.x * blockDim.x + threadIdx.x;
    if (co >= Cout) return;
    float t = 0.0f;
    for (int sidx = 0; sidx < slices; ++sidx) t += partial[(size_t)sidx * Cout + co];
    out[co] = scale ? t * scale[co] : t;
}

}  // namespace frcnn

using namespace frcnn;

extern "C" {

int frcnn_pack_conv_weights_dgrad(const float* w_hwio, const float* scale, int kh, int kw, int cin, int cout, float* packed, void* stream) {
    if (!w_hwio || !packed || kh <= 0 || kw <= 0 || cin <= 0 || cout <= 0) return fail(FRCNN_E_ARG, "pack_conv_weights_dgrad: bad argument");
    const int Kpad = frcnn_conv_packed_k(kh, kw, cout);
    const size_t total = (size_t)cin * Kpad;
    int grid = (int)((total + 255) / 256);
    if (grid > 4096) grid = 4096;
    k_pack_dgrad<<<grid, 256, 0, as_stream(stream)>>>(w_hwio, scale, kh, kw, cin, cout, Kpad, packed);
    return check_launch("pack_conv_weights_dgrad");
}

// f32 operands, cin and cout >= 128: the 128x128-tile kernel (dev knob FRCNN_WGRAD_BIG=0: the 64x64 kernel everywhere)
// frcnn_conv_desc.tile 71..77 on an f32 job asks for the split-bf16 engine (kind 4) where the 128x128 form applies
static bool wgrad_wants_x6(const frcnn_conv_desc* d) { const int t = d->tile % 100; return t >= 71 && t <= 77; }

static bool wgrad_big(const frcnn_conv_desc* d, bool in_bf16) {
    static const bool on = !(getenv("FRCNN_WGRAD_BIG") && atoi(getenv("FRCNN_WGRAD_BIG")) == 0);
    if (!on || in_bf16 || d->cin < 128 || d->cout < 128 || (d->cin & 3) || (d->cout & 3)) return false;
    const size_t xb = (size_t)d->n * d->h * d->w * d->cin * 4, gb = (size_t)d->n * d->ho * d->wo * d->cout * 4;
    return xb < 0x80000000ull && gb < 0x80000000ull && (long long)d->n * d->ho * d->wo < (1 << 23);         // 32-bit buffer offsets, float-exact pixel index
}

// the 128x128 bf16 form (kind 5): both channel counts >= 128 and multiples of 8, 32-bit byte offsets, float-exact pixel index
static bool wgrad_big_bf16(const frcnn_conv_desc* d) {
    static const bool on = !(getenv("FRCNN_WGRAD_BIG_BF16") && atoi(getenv("FRCNN_WGRAD_BIG_BF16")) == 0);
    if (!on || d->cin < 128 || d->cout < 128 || (d->cin & 7) || (d->cout & 7)) return false;
    const size_t xb = (size_t)d->n * d->h * d->w * d->cin * 2, gb = (size_t)d->n * d->ho * d->wo * d->cout * 2;
    return xb < 0x80000000ull && gb < 0x80000000ull && (long long)d->n * d->ho * d->wo < (1 << 23);
}

static int wgrad_slices(const frcnn_conv_desc* d, bool big, bool fast = false) {
    const long long M = (long long)d->n * d->ho * d->wo;
    const int tw = big ? 128 : 64;
    const long long tiles = (long long)d->kh * d->kw * ((d->cin + tw - 1) / tw) * ((d->cout + tw - 1) / tw);
    // ~256 workgroups per layer: the layers of a step are launched together (frcnn_conv2d_wgrad_batch), so the chip is
    // filled by the batch, not by one layer, and fewer slices mean fewer partial slabs to write and re-read (measured,
    // scripts/micro/train_ab2.py, target 2048 -> 256: mixed RPN step 2.36 -> 2.08 ms, detector step 3.30 -> 2.85 ms)
    static const long long target = getenv("FRCNN_WGRAD_TARGET") ? atoll(getenv("FRCNN_WGRAD_TARGET")) : 256;   // dev knob
    static const long long target_big = getenv("FRCNN_WGRAD_TARGET_BIG") ? atoll(getenv("FRCNN_WGRAD_TARGET_BIG")) : 256;
    // the split-bf16 form's workgroups finish sooner: fewer, longer slices (bench_train.py: 2.18 / 4.02 ms at 256, 2.12 / 3.96 at 96-128,
    // 2.10 / 3.93 at 48, 2.19 / 4.04 at 32)
    static const long long target_x6 = getenv("FRCNN_WGRAD_TARGET_X6") ? atoll(getenv("FRCNN_WGRAD_TARGET_X6")) : 96;
    const long long tg = big ? ((fast || wgrad_wants_x6(d)) ? target_x6 : target_big) : target;
    long long s = (tg + tiles - 1) / tiles;
    const long long max_s = (M + 4 * WG_MC - 1) / (4 * WG_MC); // at least 4 chunks per slice
    if (s > max_s) s = max_s;
    if (s < 1) s = 1;
    if (s > 64) s = 64;
    return (int)s;
}
static int wgrad_slices_max(const frcnn_conv_desc* d) {
    const int a = wgrad_slices(d, false), b = wgrad_big(d, false) ? wgrad_slices(d, true) : 0;
    const int c = (wgrad_big(d, false) || wgrad_big_bf16(d)) ? wgrad_slices(d, true, true) : 0;
    return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

size_t frcnn_conv2d_wgrad_workspace_bytes(const frcnn_conv_desc* d) {
    if (!d) return 0;
    const size_t dw = (size_t)wgrad_slices_max(d) * d->kh * d->kw * d->cin * d->cout * sizeof(float);
    const size_t db = (size_t)COLSUM_SLICES * d->cout * sizeof(float);
    return align_up(dw > db ? dw : db, 256);
}

static int wgrad_impl(const frcnn_conv_desc* d, const void* x, const void* g, bool in_bf16, const float* scale,
                      float* dw_hwio, float* dbias, void* workspace, size_t workspace_bytes, void* stream);

int frcnn_conv2d_wgrad(const frcnn_conv_desc* d, const float* x, const float* g, const float* scale,
                       float* dw_hwio, float* dbias, void* workspace, size_t workspace_bytes, void* stream) {
    return wgrad_impl(d, x, g, false, scale, dw_hwio, dbias, workspace, workspace_bytes, stream);
}

int frcnn_conv2d_wgrad_bf16(const frcnn_conv_desc* d, const void* x_bf16, const void* g_bf16, const float* scale,
                            float* dw_hwio, float* dbias, void* workspace, size_t workspace_bytes, void* stream) {
    return wgrad_impl(d, x_bf16, g_bf16, true, scale, dw_hwio, dbias, workspace, workspace_bytes, stream);
}

static int wgrad_impl(const frcnn_conv_desc* d, const void* x, const void* g, bool in_bf16, const float* scale,
                      float* dw_hwio, float* dbias, void* workspace, size_t workspace_bytes, void* stream) {
    if (!d || !x || !g || !dw_hwio) return fail(FRCNN_E_ARG, "conv2d_wgrad: null pointer");
    if ((d->cin & 3) && d->cin >= 4) return fail(FRCNN_E_UNSUPPORTED, "conv2d_wgrad: cin must be a multiple of 4 (or < 4)");
    if (in_bf16 && ((d->cin & 3) || (d->cout & 3))) return fail(FRCNN_E_UNSUPPORTED, "conv2d_wgrad_bf16: cin and cout must be multiples of 4");
    if (!workspace || workspace_bytes < frcnn_conv2d_wgrad_workspace_bytes(d))
        return fail(FRCNN_E_WORKSPACE, "conv2d_wgrad: workspace needs %zu bytes", frcnn_conv2d_wgrad_workspace_bytes(d));
    WgradArgs a;
    a.x = x; a.g = g; a.partial = (float*)workspace;
    a.n_img = d->n; a.H = d->h; a.W = d->w; a.Cin = d->cin; a.Cout = d->cout; a.R = d->kh; a.S = d->kw;
    a.stride = d->stride; a.pad_top = d->pad_top; a.pad_left = d->pad_left; a.Ho = d->ho; a.Wo = d->wo;
    a.M = d->n * d->ho * d->wo;
    const bool big16 = in_bf16 && wgrad_big_bf16(d);
    const bool big = wgrad_big(d, in_bf16) || big16;
    const int slices = wgrad_slices(d, big, big16);
    a.m_per_slice = ((a.M + slices - 1) / slices + WG_MC - 1) / WG_MC * WG_MC;
    hipStream_t s = as_stream(stream);
    const int tw = big ? 128 : 64;
    dim3 grid(d->kh * d->kw * ((d->cin + tw - 1) / tw), (d->cout + tw - 1) / tw, slices);
    if (big16) k_conv_wgrad_bf16_big<<<grid, 256, 0, s>>>(a);
    else if (big && wgrad_wants_x6(d)) k_conv_wgrad_x6_big<<<grid, 256, 0, s>>>(a);
    else if (big) k_conv_wgrad_f32_big<<<grid, 256, 0, s>>>(a);
    else if (in_bf16 && (d->cin & 7) == 0 && (d->cout & 7) == 0) k_conv_wgrad_bf16<<<grid, 256, 0, s>>>(a);      // bf16 MFMA
    else if (in_bf16) k_conv_wgrad_f32<true><<<grid, 256, 0, s>>>(a);                                          // widened, f32 MFMA
    else k_conv_wgrad_f32<false><<<grid, 256, 0, s>>>(a);
    if (int e = check_launch("conv2d_wgrad")) return e;
    const size_t elems = (size_t)d->kh * d->kw * d->cin * d->cout;
    int rgrid = (int)((elems + 255) / 256);
    if (rgrid > 4096) rgrid = 4096;
    k_wgrad_reduce<<<rgrid, 256, 0, s>>>((const float*)workspace, slices, elems, d->cout, scale, dw_hwio);
    if (int e = check_launch("conv2d_wgrad reduce")) return e;
    if (dbias && in_bf16) {
        frcnn_colsum_job job;
        job.g = g; job.scale = scale; job.out = dbias; job.m = a.M; job.cout = d->cout; job.g_is_bf16 = 1; job.reserved = 0;
        return frcnn_colsum_batch(&job, 1, stream);
    }
    if (dbias) {                                   // the slab workspace is free again after the reduce (stream order)
        int cs = (a.M + 63) / 64;
        if (cs > COLSUM_SLICES) cs = COLSUM_SLICES;
        if (cs < 1) cs = 1;
        const int rows_per_slice = (a.M + cs - 1) / cs;
        k_colsum_partial<<<dim3((d->cout + 63) / 64, cs), 256, 0, s>>>((const float*)g, a.M, d->cout, rows_per_slice, (float*)workspace);
        if (int e = check_launch("conv2d_wgrad bias")) return e;
        k_colsum_final<<<(d->cout + 255) / 256, 256, 0, s>>>((const float*)workspace, cs, d->cout, scale, dbias);
        if (int e = check_launch("conv2d_wgrad bias")) return e;
    }
    return FRCNN_OK;
}

static int wgrad_kind(const frcnn_wgrad_job& j) {
    if (!j.in_bf16) return wgrad_big(&j.d, false) ? (wgrad_wants_x6(&j.d) ? 4 : 3) : 0;
    if (wgrad_big_bf16(&j.d)) return 5;
    return ((j.d.cin & 7) == 0 && (j.d.cout & 7) == 0) ? 1 : 2;
}

static size_t wgrad_slab_bytes(const frcnn_conv_desc* d) {
    return align_up((size_t)wgrad_slices_max(d) * d->kh * d->kw * d->cin * d->cout * sizeof(float), 256);
}

size_t frcnn_conv2d_wgrad_batch_workspace_bytes(const frcnn_wgrad_job* jobs, int n_jobs) {
    size_t tot = 0;
    for (int i = 0; jobs && i < n_jobs; ++i) tot += wgrad_slab_bytes(&jobs[i].d);
    return tot;
}

int frcnn_conv2d_wgrad_batch(const frcnn_wgrad_job* jobs, int n_jobs, void* workspace, size_t workspace_bytes, void* stream) {
    if (n_jobs < 0 || (n_jobs > 0 && !jobs)) return fail(FRCNN_E_ARG, "conv2d_wgrad_batch: bad argument");
    if (n_jobs == 0) return FRCNN_OK;
    if (!workspace || workspace_bytes < frcnn_conv2d_wgrad_batch_workspace_bytes(jobs, n_jobs))
        return fail(FRCNN_E_WORKSPACE, "conv2d_wgrad_batch: workspace needs %zu bytes", frcnn_conv2d_wgrad_batch_workspace_bytes(jobs, n_jobs));
    hipStream_t s = as_stream(stream);
    // every job's slab region, in job order
    size_t off = 0;
    static thread_local float* slab[1024];
    if (n_jobs > 1024) return fail(FRCNN_E_ARG, "conv2d_wgrad_batch: more than 1024 jobs");
    for (int i = 0; i < n_jobs; ++i) {
        const frcnn_wgrad_job& j = jobs[i];
        if (!j.x || !j.g || !j.dw) return fail(FRCNN_E_ARG, "conv2d_wgrad_batch: job %d has a null pointer", i);
        if ((j.d.cin & 3) && j.d.cin >= 4) return fail(FRCNN_E_UNSUPPORTED, "conv2d_wgrad_batch: job %d: cin must be a multiple of 4 (or < 4)", i);
        if (j.in_bf16 && ((j.d.cin & 3) || (j.d.cout & 3))) return fail(FRCNN_E_UNSUPPORTED, "conv2d_wgrad_batch: job %d: bf16 operands need cin, cout multiples of 4", i);
        slab[i] = (float*)((char*)workspace + off);
        off += wgrad_slab_bytes(&j.d);
    }
    for (int kind = 0; kind < 6; ++kind) {
        WgradBatch t;
        t.n = 0;
        int blocks = 0;
        auto flush = [&]() -> int {
            if (t.n == 0) return FRCNN_OK;
            t.first_block[t.n] = blocks;
            for (int q = t.n; q < WGRAD_BATCH; ++q) { t.job[q] = t.job[0]; t.gx[q] = t.gy[q] = 1; t.first_block[q + 1] = blocks; }
            if (kind == 0) k_conv_wgrad_batch<0><<<blocks, 256, 0, s>>>(t);
            else if (kind == 1) k_conv_wgrad_batch<1><<<blocks, 256, 0, s>>>(t);
            else if (kind == 2) k_conv_wgrad_batch<2><<<blocks, 256, 0, s>>>(t);
            else if (kind == 3) k_conv_wgrad_batch<3><<<blocks, 256, 0, s>>>(t);
            else if (kind == 4) k_conv_wgrad_batch<4><<<blocks, 256, 0, s>>>(t);
            else k_conv_wgrad_batch<5><<<blocks, 256, 0, s>>>(t);
            t.n = 0; blocks = 0;
            return check_launch("conv2d_wgrad_batch");
        };
        for (int i = 0; i < n_jobs; ++i) {
            const frcnn_wgrad_job& j = jobs[i];
            if (wgrad_kind(j) != kind) continue;
            const frcnn_conv_desc* d = &j.d;
            WgradArgs& a = t.job[t.n];
            a.x = j.x; a.g = j.g; a.partial = slab[i];
            a.n_img = d->n; a.H = d->h; a.W = d->w; a.Cin = d->cin; a.Cout = d->cout; a.R = d->kh; a.S = d->kw;
            a.stride = d->stride; a.pad_top = d->pad_top; a.pad_left = d->pad_left; a.Ho = d->ho; a.Wo = d->wo;
            a.M = d->n * d->ho * d->wo;
            const int slices = wgrad_slices(d, kind >= 3, kind == 5);
            a.m_per_slice = ((a.M + slices - 1) / slices + WG_MC - 1) / WG_MC * WG_MC;
            const int tw = kind >= 3 ? 128 : 64;
            t.gx[t.n] = d->kh * d->kw * ((d->cin + tw - 1) / tw);
            t.gy[t.n] = (d->cout + tw - 1) / tw;
            t.first_block[t.n] = blocks;
            blocks += t.gx[t.n] * t.gy[t.n] * slices;
            if (++t.n == WGRAD_BATCH) if (int e = flush()) return e;
        }
        if (int e = flush()) return e;
    }
    // the slice reductions of all jobs: grid.y = job
    for (int b = 0; b < n_jobs; b += 2 * WGRAD_BATCH) {
        WgradReduceBatch r;
        r.n = n_jobs - b < 2 * WGRAD_BATCH ? n_jobs - b : 2 * WGRAD_BATCH;
        for (int i = 0; i < 2 * WGRAD_BATCH; ++i) {
            const int q = b + (i < r.n ? i : 0);
            const frcnn_conv_desc* d = &jobs[q].d;
            r.job[i].partial = slab[q]; r.job[i].scale = jobs[q].scale; r.job[i].dw = jobs[q].dw;
            r.job[i].elems = (unsigned long long)d->kh * d->kw * d->cin * d->cout;
            r.job[i].slices = wgrad_slices(d, wgrad_kind(jobs[q]) >= 3, wgrad_kind(jobs[q]) == 5); r.job[i].cout = d->cout;
        }
        int rblocks = 0;
        for (int i = 0; i <= 2 * WGRAD_BATCH; ++i) {
            r.first_block[i] = rblocks;
            if (i < r.n) {
                const unsigned long long g = (r.job[i].elems + 2047) / 2048;       // 8 elements (x slices) per thread
                rblocks += (int)(g < 4 ? 4 : (g > 2048 ? 2048 : g));
            }
        }
        k_wgrad_reduce_batch<<<rblocks, 256, 0, s>>>(r);
        if (int e = check_launch("conv2d_wgrad_batch reduce")) return e;
    }
    return FRCNN_OK;
}

int frcnn_refresh_packed(const frcnn_pack_job* jobs, int n_jobs, void* stream) {
    if (n_jobs < 0 || (n_jobs > 0 && !jobs)) return fail(FRCNN_E_ARG, "refresh_packed: bad argument");
    for (int i = 0; i < n_jobs; ++i)
        if (!jobs[i].w_hwio || jobs[i].kh <= 0 || jobs[i].kw <= 0 || jobs[i].cin <= 0 || jobs[i].cout <= 0)
            return fail(FRCNN_E_ARG, "refresh_packed: job %d is malformed", i);
    for (int b = 0; b < n_jobs; b += REFRESH_JOBS) {
        RefreshTable t;
        const int n = n_jobs - b < REFRESH_JOBS ? n_jobs - b : REFRESH_JOBS;
        int blocks = 0;
        for (int i = 0; i < n; ++i) { t.job[i] = jobs[b + i]; t.first_block[i] = blocks; blocks += refresh_blocks(jobs[b + i]); }
        for (int i = n; i < REFRESH_JOBS; ++i) { t.job[i] = jobs[b]; t.first_block[i] = blocks; }        // never indexed
        t.first_block[REFRESH_JOBS] = blocks;
        t.n = n;
        k_refresh_packed<<<blocks, 256, 0, as_stream(stream)>>>(t);
        if (int e = check_launch("refresh_packed")) return e;
    }
    return FRCNN_OK;
}

int frcnn_colsum_batch(const frcnn_colsum_job* jobs, int n_jobs, void* stream) {
    if (n_jobs < 0 || (n_jobs > 0 && !jobs)) return fail(FRCNN_E_ARG, "colsum_batch: bad argument");
    for (int i = 0; i < n_jobs; ++i)
        if (!jobs[i].g || !jobs[i].out || jobs[i].m <= 0 || jobs[i].cout <= 0) return fail(FRCNN_E_ARG, "colsum_batch: job %d is malformed", i);
    for (int b = 0; b < n_jobs; b += COLSUM_JOBS) {
        ColsumTable t;
        t.n = n_jobs - b < COLSUM_JOBS ? n_jobs - b : COLSUM_JOBS;
        int blocks = 0;
        for (int i = 0; i < t.n; ++i) { t.job[i] = jobs[b + i]; t.first_block[i] = blocks; blocks += (jobs[b + i].cout + 63) / 64; }
        for (int i = t.n; i < COLSUM_JOBS; ++i) { t.job[i] = jobs[b]; t.first_block[i] = blocks; }
        t.first_block[COLSUM_JOBS] = blocks;
        k_colsum_batch<<<blocks, 1024, 0, as_stream(stream)>>>(t);
        if (int e = check_launch("colsum_batch")) return e;
    }
    return FRCNN_OK;
}

}  // extern "C"
