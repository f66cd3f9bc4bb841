// Where objects have been: an occupancy heat map accumulated over a sequence's frames and blended into them (include/ext/frcnn_hip_heat.h
// states the rule, DESIGN §8 "Heat rule").  gfx950 (CDNA4) only.  Integers throughout, no atomics on memory.
// k_heat_update: one pass over the map in tiles of 64 x 16 pixels, 256 threads.  Threads are pixels here -- the map is int32, a wave on a
// row of the tile is one 256-byte access -- and a thread owns the 4 pixels of its column that its wave's rows hold.  The workgroup walks
// the frame's rows 256 at a time: the boxes of the heat classes that meet the tile are compacted into LDS by wave64 ballots (a round),
// every thread counts those that cover its pixels, and the next round follows; most tiles meet no box and only decay.  Then each pixel is
// decayed, raised, clamped and stored where it changed, and the tile's maximum goes to the tile's scratch word behind the map.
// k_heat_finish: one workgroup reduces the scratch words and writes `frames` and `peak`.  Both kernels return before their first store
// when the frame is not real (*n_frames, *gate), so a captured pass can be replayed with no frames of its own.
// k_heat_draw: tiles of 256 byte columns x 16 rows with threads as bytes, as csrc/redact.hip's phase two and for its reason; the three
// bytes of a pixel read the same map word and each blends its own channel of the ramp.
#include "common.h"
#include "../../include/ext/frcnn_hip_redact.h"
#include "../../include/ext/frcnn_hip_heat.h"

namespace frcnn {

constexpr int HT_THREADS = 256, HT_WAVES = HT_THREADS / 64;
constexpr int HT_TILE_W = FRCNN_HEAT_TILE_W, HT_TILE_H = FRCNN_HEAT_TILE_H, HT_PER = HT_TILE_H / HT_WAVES;    // a thread's pixels
constexpr int HT_DRAW_ROWS = 16;
static_assert(HT_TILE_W == 64 && HT_TILE_H % HT_WAVES == 0, "a wave is a row of the tile");

__device__ inline bool heat_real(int f, const int32_t* n_frames, const int32_t* gate) {
    return f < max(*n_frames, 0) && !(gate && *gate == 0);
}

__device__ inline int heat_wave_max(int v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

__global__ void __launch_bounds__(HT_THREADS) k_heat_update(int32_t* state, int h, int w, const int32_t* det, int rows, int tracked,
                                                              const uint8_t* table, int num_classes, int S, int f, const int32_t* n_frames,
                                                              const int32_t* gate) {
    __shared__ int4 s_box[HT_THREADS];                                      // (xa, xb, ya, yb) of a round's boxes that meet this tile
    __shared__ int s_cnt[HT_WAVES], s_max[HT_WAVES];
    if (!heat_real(f, n_frames, gate)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx0 = blockIdx.x * HT_TILE_W, ty0 = blockIdx.y * HT_TILE_H;
    const int tx1 = min(tx0 + HT_TILE_W, w) - 1, ty1 = min(ty0 + HT_TILE_H, h) - 1;
    const int x = tx0 + lane;
    const int nd = min(max(det[tracked ? 1 : 0], 0), rows);                 // a tracked buffer: its LIVE rows only
    const int32_t *bbox = det + 4, *cls = det + 4 + 4 * (size_t)rows;
    int cnt[HT_PER];
#pragma unroll
    for (int j = 0; j < HT_PER; ++j) cnt[j] = 0;
    for (int base = 0; base < nd; base += HT_THREADS) {                     // a round
        const int r = base + tid;
        bool hit = false;
        int4 q = make_int4(0, 0, 0, 0);
        if (r < nd) {
            const int c = cls[r];
            if (c >= 0 && c < num_classes && table[c]) {
                const int x1 = bbox[4 * r], y1 = bbox[4 * r + 1], x2 = bbox[4 * r + 2], y2 = bbox[4 * r + 3];
                q = make_int4(max(min(x1, x2), 0), min(max(x1, x2), w - 1), max(min(y1, y2), 0), min(max(y1, y2), h - 1));
                hit = q.x <= q.y && q.z <= q.w && q.y >= tx0 && q.x <= tx1 && q.w >= ty0 && q.z <= ty1;
            }
        }
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) s_cnt[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
        for (int k = 0; k < HT_WAVES; ++k) {
            const int c = s_cnt[k];
            before += k < wave ? c : 0;
            total += c;
        }
        if (hit) s_box[before + __popcll(mask & ((1ull << lane) - 1ull))] = q;
        __syncthreads();
        if (x <= tx1)
            for (int s = 0; s < total; ++s) {
                const int4 b = s_box[s];
                if (x < b.x || x > b.y) continue;
#pragma unroll
                for (int j = 0; j < HT_PER; ++j) {
                    const int y = ty0 + wave + HT_WAVES * j;
                    cnt[j] += y >= b.z && y <= b.w;
                }
            }
        __syncthreads();                                                    // (the next round writes s_cnt and s_box)
    }
    int32_t* map = state + 4;
    int m = 0;
    bool clamped = false;
    if (x <= tx1) {
#pragma unroll
        for (int j = 0; j < HT_PER; ++j) {
            const int y = ty0 + wave + HT_WAVES * j;
            if (y > ty1) continue;
            const size_t at = (size_t)y * w + x;
            const int v0 = map[at];
            int v = v0;
            if (S > 0) v -= (v + (1 << S) - 1) >> S;
            v += 256 * cnt[j];                                              // (at most 2^30 + 2^17: no overflow)
            if (v > FRCNN_HEAT_MAX) {
                v = FRCNN_HEAT_MAX;
                clamped = true;
            }
            if (v != v0) map[at] = v;
            m = max(m, v);
        }
    }
    if (clamped) state[2] = 1;                                              // (every writer stores the same value)
    m = heat_wave_max(m);
    if (lane == 0) s_max[wave] = m;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < HT_WAVES; ++k) m = max(m, s_max[k]);
        map[(size_t)h * w + (size_t)blockIdx.y * gridDim.x + blockIdx.x] = m;
    }
}

__global__ void __launch_bounds__(HT_THREADS) k_heat_finish(int32_t* state, size_t hw, int tiles, int f, const int32_t* n_frames,
                                                              const int32_t* gate) {
    __shared__ int s_max[HT_WAVES];
    if (!heat_real(f, n_frames, gate)) return;
    const int32_t* part = state + 4 + hw;
    int m = 0;
    for (int i = threadIdx.x; i < tiles; i += HT_THREADS) m = max(m, part[i]);
    m = heat_wave_max(m);
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < HT_WAVES; ++k) m = max(m, s_max[k]);
        state[0] += 1;
        state[1] = m;
    }
}

__global__ void __launch_bounds__(HT_THREADS) k_heat_draw(uint8_t* frame, int h, int w, const int32_t* state, int A, int rgb) {
    const int p = state[1];
    if (p <= 0) return;
    const int rowbytes = 3 * w, j = blockIdx.x * HT_THREADS + threadIdx.x;
    if (j >= rowbytes) return;
    const int x = j / 3, c = j - 3 * x, ch = rgb ? c : 2 - c;              // ch: 0 R, 1 G, 2 B
    const int y0 = blockIdx.y * HT_DRAW_ROWS, y1 = min(y0 + HT_DRAW_ROWS, h) - 1;
    const int32_t* map = state + 4;
    const bool narrow = p <= (1 << 24);                                     // v x 255 then fits 32 bits: the short division
    for (int y = y0; y <= y1; ++y) {
        const int v = min(map[(size_t)y * w + x], p);
        if (v <= 0) continue;
        const int t = narrow ? (int)((uint32_t)v * 255u / (uint32_t)p) : (int)((uint64_t)v * 255u / (uint64_t)p);
        const int a = A * t / 255;
        if (a == 0) continue;
        const int C = min(max(3 * t - 255 * ch, 0), 255);
        uint8_t* at = frame + (size_t)y * rowbytes + j;
        *at = (uint8_t)(((int)*at * (255 - a) + C * a + 127) / 255);
    }
}

static bool heat_sides_ok(int h, int w) { return h >= 1 && h <= FRCNN_REDACT_MAX_SIDE && w >= 1 && w <= FRCNN_REDACT_MAX_SIDE; }

static int heat_tiles_x(int w) { return (w + HT_TILE_W - 1) / HT_TILE_W; }
static int heat_tiles_y(int h) { return (h + HT_TILE_H - 1) / HT_TILE_H; }

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_heat_version(void) { return FRCNN_HEAT_VERSION; }

extern "C" size_t frcnn_heat_state_bytes(int h, int w) {
    if (!heat_sides_ok(h, w)) return 0;
    return sizeof(int32_t) * (4 + (size_t)h * (size_t)w + (size_t)heat_tiles_x(w) * (size_t)heat_tiles_y(h));
}

extern "C" int frcnn_heat_update(int32_t* state, int h, int w, const int32_t* det, int rows, int tracked, const uint8_t* table,
                                 int num_classes, int decay, int frame_index, const int32_t* n_frames, const int32_t* gate, void* stream) {
    const char* who = "heat_update";
    if (!state || !det || !table || !n_frames) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (!heat_sides_ok(h, w)) return fail(FRCNN_E_ARG, "%s: frame %dx%d out of range (sides 1..%d)", who, h, w, FRCNN_REDACT_MAX_SIDE);
    if (rows < 1 || rows > FRCNN_REDACT_MAX_ROWS) return fail(FRCNN_E_ARG, "%s: rows=%d not in [1, %d]", who, rows, FRCNN_REDACT_MAX_ROWS);
    if (num_classes < 1 || num_classes > 256) return fail(FRCNN_E_ARG, "%s: num_classes=%d not in [1, 256]", who, num_classes);
    if (decay < 0 || decay > FRCNN_HEAT_MAX_DECAY) return fail(FRCNN_E_ARG, "%s: decay=%d not in [0, %d]", who, decay, FRCNN_HEAT_MAX_DECAY);
    if (frame_index < 0 || frame_index >= FRCNN_HEAT_MAX_FRAMES)
        return fail(FRCNN_E_ARG, "%s: frame_index=%d not in [0, %d]", who, frame_index, FRCNN_HEAT_MAX_FRAMES - 1);
    hipStream_t st = as_stream(stream);
    const int gx = heat_tiles_x(w), gy = heat_tiles_y(h);
    k_heat_update<<<dim3(gx, gy), HT_THREADS, 0, st>>>(state, h, w, det, rows, tracked ? 1 : 0, table, num_classes, decay, frame_index, n_frames,
                                                       gate);
    if (int rc = check_launch("heat_update (tiles)")) return rc;
    k_heat_finish<<<1, HT_THREADS, 0, st>>>(state, (size_t)h * (size_t)w, gx * gy, frame_index, n_frames, gate);
    return check_launch(who);
}

extern "C" int frcnn_heat_draw_u8(uint8_t* frame, int h, int w, const int32_t* state, int alpha, int rgb, void* stream) {
    const char* who = "heat_draw_u8";
    if (!frame || !state) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (!heat_sides_ok(h, w)) return fail(FRCNN_E_ARG, "%s: frame %dx%d out of range (sides 1..%d)", who, h, w, FRCNN_REDACT_MAX_SIDE);
    if (alpha < 1 || alpha > 255) return fail(FRCNN_E_ARG, "%s: alpha=%d not in [1, 255]", who, alpha);
    k_heat_draw<<<dim3((3 * w + HT_THREADS - 1) / HT_THREADS, (h + HT_DRAW_ROWS - 1) / HT_DRAW_ROWS), HT_THREADS, 0, as_stream(stream)>>>(
        frame, h, w, state, alpha, rgb ? 1 : 0);
    return check_launch(who);
}
