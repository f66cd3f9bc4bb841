// Objects painted out with a learned background: a per-pixel plate learned over a sequence's frames and copied into the boxes of chosen
// classes (include/ext/frcnn_hip_plate.h states the rule, DESIGN §8 "Plate rule").  gfx950 (CDNA4) only.  Integers throughout, no atomics
// on memory.
// k_plate_update: one pass over the pixels in tiles of 128 x 8, 256 threads; the kernel streams 8 B of state in and out and 3 B of frame
// in per pixel and is bound by that.  The workgroup walks the frame's rows 256 at a time: the boxes that meet the tile are compacted into
// LDS by wave64 ballots (a round, as csrc/heat.hip's), and every thread marks which of its pixels they cover.  A thread owns 4 consecutive
// pixels of one row: 32 B of state, two 16-byte accesses where the run starts on an even pixel (every run of an even-width frame, every
// other row of an odd one), four 8-byte ones elsewhere and at the right border; half a wave on a row of the tile is 1 KiB of state.  The
// 12 frame bytes of the run start at any byte: the thread reads the 3 or 4 ALIGNED words that hold them -- a wave's loads are consecutive
// words, each fetched once from memory -- and shifts the pixels out; a word that reaches over an end of the frame is put together from
// its bytes inside.  The tile's count of known pixels goes to the tile's scratch word behind the pixels.
// k_plate_finish: one workgroup adds the scratch words in a fixed order and writes `frames` and `known`.  Both kernels return before their
// first store when the frame is not real (*n_frames, *gate), so a captured pass can be replayed with no frames of its own.
// k_plate_fill: tiles of 256 byte columns x 16 rows with threads as bytes, as k_heat_draw and for its reason; the FILL boxes that meet the
// tile are staged by the same rounds, a thread keeps a bit per row of its column, and a tile that meets no box reads no state at all.
#include "plate.h"                                                          // (the tile, plate_real, plate_round, plate_word)

namespace frcnn {

constexpr int PL_FILL_ROWS = 16;

__device__ inline int plate_absdiff(uint32_t a, uint32_t b) { return abs((int)(a & 255u) - (int)(b & 255u)); }

// One pixel's step: (word 0, word 1) of the state, x its three bytes in the frame's order.
__device__ inline void plate_step(uint32_t& w0, uint32_t& w1, uint32_t x, bool blocked, uint32_t S, int T) {
    if (blocked) {
        w1 &= 0x00ffffffu;
        return;
    }
    uint32_t N = w1 >> 24;
    const int d = max(max(plate_absdiff(x, w1), plate_absdiff(x >> 8, w1 >> 8)), plate_absdiff(x >> 16, w1 >> 16));
    if (N >= 1u && d <= T) {
        N = min(N + 1u, 255u);
        w1 = (w1 & 0x00ffffffu) | (N << 24);
    } else {
        N = 1u;
        w1 = x | (1u << 24);
    }
    if (N >= S) w0 = x | (1u << 24);
}

__global__ void __launch_bounds__(PL_THREADS) k_plate_update(int32_t* state, int h, int w, const uint8_t* frame, const int32_t* det, int rows,
                                                               int M, int S, int T, int f, const int32_t* n_frames, const int32_t* gate,
                                                               const int32_t* cut) {
    __shared__ int4 s_box[PL_THREADS];                                      // (xa, xb, ya, yb) of a round's boxes that meet this tile
    __shared__ int s_cnt[PL_WAVES], s_known[PL_WAVES];
    if (!plate_real(f, n_frames, gate)) return;
    const bool wipe = cut && *cut != 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx0 = blockIdx.x * PL_TILE_W, ty0 = blockIdx.y * PL_TILE_H;
    const int tx1 = min(tx0 + PL_TILE_W, w) - 1, ty1 = min(ty0 + PL_TILE_H, h) - 1;
    const int x0 = tx0 + PL_RUN * (tid % (PL_TILE_W / PL_RUN)), y = ty0 + tid / (PL_TILE_W / PL_RUN);
    const bool mine = x0 <= tx1 && y <= ty1;
    const int nd = min(max(det[0], 0), rows);                               // n_dets, or n_rows of a tracked buffer: the held rows too
    const int32_t *bbox = det + 4, *cls = det + 4 + 4 * (size_t)rows;
    unsigned blocked = 0;                                                   // bit k: pixel x0 + k is under a BLOCK box
    for (int base = 0; base < nd; base += PL_THREADS) {                     // a round
        const int total = plate_round(s_box, s_cnt, base, nd, bbox, cls, nullptr, 0, M, h, w, tx0, tx1, ty0, ty1);
        if (mine)
            for (int s = 0; s < total; ++s) {
                const int4 b = s_box[s];
                if (y < b.z || y > b.w) continue;
#pragma unroll
                for (int k = 0; k < PL_RUN; ++k) blocked |= (unsigned)(x0 + k >= b.x && x0 + k <= b.y) << k;
            }
        __syncthreads();                                                    // (the next round writes s_cnt and s_box)
    }
    int known = 0;
    if (mine) {
        const int n = min(PL_RUN, w - x0);                                  // pixels of the run inside the frame
        const size_t p = (size_t)y * w + x0;
        int32_t* at = state + 4 + 2 * p;
        const bool wide = n == PL_RUN && (p & 1) == 0;                      // (the state is 16-byte aligned, and so is its pixel 0)
        uint32_t w0[PL_RUN] = {0, 0, 0, 0}, w1[PL_RUN] = {0, 0, 0, 0};
        if (!wipe) {
            if (wide) {
                const int4 a = *reinterpret_cast<const int4*>(at), b = *reinterpret_cast<const int4*>(at + 4);
                w0[0] = a.x, w1[0] = a.y, w0[1] = a.z, w1[1] = a.w, w0[2] = b.x, w1[2] = b.y, w0[3] = b.z, w1[3] = b.w;
            } else {
#pragma unroll
                for (int k = 0; k < PL_RUN; ++k)
                    if (k < n) {
                        const int2 a = *reinterpret_cast<const int2*>(at + 2 * k);
                        w0[k] = a.x, w1[k] = a.y;
                    }
            }
        }
        // the run's 3n bytes start at byte `sh` of the aligned word at q
        const uint8_t *lo = frame, *hi = frame + 3 * (size_t)h * (size_t)w, *a = frame + 3 * p;
        const int sh = (int)(reinterpret_cast<uintptr_t>(a) & 3u);
        const uint8_t* q = a - sh;
        uint32_t d[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * k < sh + 3 * n) d[k] = plate_word(q + 4 * k, lo, hi);
        uint32_t e[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) e[k] = (uint32_t)((((uint64_t)d[k + 1] << 32) | d[k]) >> (8 * sh));
        const uint32_t x[PL_RUN] = {e[0] & 0x00ffffffu, ((e[0] >> 24) | (e[1] << 8)) & 0x00ffffffu, ((e[1] >> 16) | (e[2] << 16)) & 0x00ffffffu,
                                    e[2] >> 8};
#pragma unroll
        for (int k = 0; k < PL_RUN; ++k)
            if (k < n) {
                plate_step(w0[k], w1[k], x[k], (blocked >> k) & 1u, (uint32_t)S, T);
                known += (w0[k] >> 24) != 0u;
            }
        if (wide) {
            *reinterpret_cast<int4*>(at) = make_int4((int)w0[0], (int)w1[0], (int)w0[1], (int)w1[1]);
            *reinterpret_cast<int4*>(at + 4) = make_int4((int)w0[2], (int)w1[2], (int)w0[3], (int)w1[3]);
        } else {
#pragma unroll
            for (int k = 0; k < PL_RUN; ++k)
                if (k < n) *reinterpret_cast<int2*>(at + 2 * k) = make_int2((int)w0[k], (int)w1[k]);
        }
    }
    for (int o = 32; o > 0; o >>= 1) known += __shfl_xor(known, o);
    if (lane == 0) s_known[wave] = known;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < PL_WAVES; ++k) known += s_known[k];
        state[4 + 2 * (size_t)h * w + (size_t)blockIdx.y * gridDim.x + blockIdx.x] = known;
    }
}

__global__ void __launch_bounds__(PL_THREADS) k_plate_finish(int32_t* state, size_t hw, int tiles, int f, const int32_t* n_frames,
                                                               const int32_t* gate) {
    __shared__ int s_sum[PL_WAVES];
    if (!plate_real(f, n_frames, gate)) return;
    const int32_t* part = state + 4 + 2 * hw;
    int sum = 0;                                                            // (at most 2^30 pixels: no overflow)
    for (int i = threadIdx.x; i < tiles; i += PL_THREADS) sum += part[i];
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < PL_WAVES; ++k) sum += s_sum[k];
        state[0] += 1;
        state[1] = sum;
    }
}

__global__ void __launch_bounds__(PL_THREADS) k_plate_fill(uint8_t* frame, int h, int w, const int32_t* state, const int32_t* det, int rows,
                                                             const uint8_t* table, int num_classes, int M, int keep) {
    __shared__ int4 s_box[PL_THREADS];
    __shared__ int s_cnt[PL_WAVES];
    const int rowbytes = 3 * w, j0 = blockIdx.x * PL_THREADS, j = j0 + threadIdx.x;
    const int y0 = blockIdx.y * PL_FILL_ROWS, y1 = min(y0 + PL_FILL_ROWS, h) - 1;
    const int tx0 = j0 / 3, tx1 = min(j0 + PL_THREADS - 1, rowbytes - 1) / 3;
    const int x = min(j, rowbytes - 1) / 3, c = j - 3 * x;                  // (j >= rowbytes: a thread that only helps staging)
    const int nd = min(max(det[0], 0), rows);
    const int32_t *bbox = det + 4, *cls = det + 4 + 4 * (size_t)rows;
    unsigned cover = 0;                                                     // bit i: row y0 + i of this column is under a FILL box
    for (int base = 0; base < nd; base += PL_THREADS) {
        const int total = plate_round(s_box, s_cnt, base, nd, bbox, cls, table, num_classes, M, h, w, tx0, tx1, y0, y1);
        for (int s = 0; s < total; ++s) {
            const int4 b = s_box[s];
            if (x < b.x || x > b.y) continue;
            const int ia = max(b.z, y0) - y0, ib = min(b.w, y1) - y0;      // (the box meets the tile: 0 <= ia <= ib <= 15)
            cover |= ((2u << ib) - 1u) & ~((1u << ia) - 1u);
        }
        __syncthreads();
    }
    if (j >= rowbytes || cover == 0) return;
    const int32_t* px = state + 4;
    for (int y = y0; y <= y1; ++y) {
        if (!((cover >> (y - y0)) & 1u)) continue;
        const uint32_t w0 = (uint32_t)px[2 * ((size_t)y * w + x)];
        uint8_t* at = frame + (size_t)y * rowbytes + j;
        if (w0 >> 24)
            *at = (uint8_t)(w0 >> (8 * c));
        else if (!keep)
            *at = 0;
    }
}

static bool plate_sides_ok(int h, int w) { return h >= 1 && h <= FRCNN_REDACT_MAX_SIDE && w >= 1 && w <= FRCNN_REDACT_MAX_SIDE; }

static int plate_tiles_x(int w) { return (w + PL_TILE_W - 1) / PL_TILE_W; }
static int plate_tiles_y(int h) { return (h + PL_TILE_H - 1) / PL_TILE_H; }

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_plate_version(void) { return FRCNN_PLATE_VERSION; }

extern "C" size_t frcnn_plate_state_bytes(int h, int w) {
    if (!plate_sides_ok(h, w)) return 0;
    return sizeof(int32_t) * (4 + 2 * (size_t)h * (size_t)w + (size_t)plate_tiles_x(w) * (size_t)plate_tiles_y(h));
}

extern "C" int frcnn_plate_update(int32_t* state, int h, int w, const uint8_t* frame, const int32_t* det, int rows, int tracked, int margin,
                                  int settle, int tol, int frame_index, const int32_t* n_frames, const int32_t* gate, const int32_t* cut,
                                  void* stream) {
    const char* who = "plate_update";
    (void)tracked;                                                          // (both buffers count their BLOCK rows in word 0)
    if (!state || !frame || !det || !n_frames) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (reinterpret_cast<uintptr_t>(state) & 15u) return fail(FRCNN_E_ARG, "%s: the state is not 16-byte aligned", who);
    if (!plate_sides_ok(h, w)) return fail(FRCNN_E_ARG, "%s: frame %dx%d out of range (sides 1..%d)", who, h, w, FRCNN_REDACT_MAX_SIDE);
    if (rows < 1 || rows > FRCNN_REDACT_MAX_ROWS) return fail(FRCNN_E_ARG, "%s: rows=%d not in [1, %d]", who, rows, FRCNN_REDACT_MAX_ROWS);
    if (margin < 0 || margin > FRCNN_PLATE_MAX_MARGIN)
        return fail(FRCNN_E_ARG, "%s: margin=%d not in [0, %d]", who, margin, FRCNN_PLATE_MAX_MARGIN);
    if (settle < 1 || settle > FRCNN_PLATE_MAX_SETTLE)
        return fail(FRCNN_E_ARG, "%s: settle=%d not in [1, %d]", who, settle, FRCNN_PLATE_MAX_SETTLE);
    if (tol < 0 || tol > 255) return fail(FRCNN_E_ARG, "%s: tol=%d not in [0, 255]", who, tol);
    if (frame_index < 0 || frame_index >= FRCNN_PLATE_MAX_FRAMES)
        return fail(FRCNN_E_ARG, "%s: frame_index=%d not in [0, %d]", who, frame_index, FRCNN_PLATE_MAX_FRAMES - 1);
    hipStream_t st = as_stream(stream);
    const int gx = plate_tiles_x(w), gy = plate_tiles_y(h);
    k_plate_update<<<dim3(gx, gy), PL_THREADS, 0, st>>>(state, h, w, frame, det, rows, margin, settle, tol, frame_index, n_frames, gate, cut);
    if (int rc = check_launch("plate_update (tiles)")) return rc;
    k_plate_finish<<<1, PL_THREADS, 0, st>>>(state, (size_t)h * (size_t)w, gx * gy, frame_index, n_frames, gate);
    return check_launch(who);
}

extern "C" int frcnn_plate_fill_u8(uint8_t* frame, int h, int w, const int32_t* state, const int32_t* det, int rows, int tracked,
                                   const uint8_t* table, int num_classes, int margin, int keep_unknown, void* stream) {
    const char* who = "plate_fill_u8";
    (void)tracked;
    if (!frame || !state || !det || !table) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (!plate_sides_ok(h, w)) return fail(FRCNN_E_ARG, "%s: frame %dx%d out of range (sides 1..%d)", who, h, w, FRCNN_REDACT_MAX_SIDE);
    if (rows < 1 || rows > FRCNN_REDACT_MAX_ROWS) return fail(FRCNN_E_ARG, "%s: rows=%d not in [1, %d]", who, rows, FRCNN_REDACT_MAX_ROWS);
    if (num_classes < 1 || num_classes > 256) return fail(FRCNN_E_ARG, "%s: num_classes=%d not in [1, 256]", who, num_classes);
    if (margin < 0 || margin > FRCNN_PLATE_MAX_MARGIN)
        return fail(FRCNN_E_ARG, "%s: margin=%d not in [0, %d]", who, margin, FRCNN_PLATE_MAX_MARGIN);
    if (keep_unknown != 0 && keep_unknown != 1) return fail(FRCNN_E_ARG, "%s: keep_unknown=%d is neither 0 nor 1", who, keep_unknown);
    k_plate_fill<<<dim3((3 * w + PL_THREADS - 1) / PL_THREADS, (h + PL_FILL_ROWS - 1) / PL_FILL_ROWS), PL_THREADS, 0, as_stream(stream)>>>(
        frame, h, w, state, det, rows, table, num_classes, margin, keep_unknown);
    return check_launch(who);
}
