// Whatever differs from the learned background hidden, detected or not (include/ext/frcnn_hip_redact_moving.h states the rule, DESIGN §8
// "Moving rule"): per frame, inside the captured pass, the plate state and the untouched frame become a plane of weights in exactly the
// region extension's layout, which that extension's prepare and apply calls then blend under.  gfx950 (CDNA4) only.  Integers throughout.
//   build, three launches per frame:
//     1. k_moving_cells: csrc/plate.hip's update tiling -- 128 x 8 pixels, one row of 16 cells, 256 threads, a thread owns 4 consecutive
//        pixels: the plate words by 16-byte loads, the frame as aligned words (plate.h).  The EXCEPT boxes that meet the tile are staged
//        in LDS by plate.h's rounds.  A cell is two threads wide and eight rows high: the foreground counts are added across the thread
//        pair and the two rows of a wave by shuffles, across the four waves through LDS; thread c < 16 then owns cell c of the tile: it
//        alone reads and writes the cell's `left` byte and writes its `moving` byte, and the tile's count of moving cells goes to the
//        tile's scratch word.
//     2. k_moving_finish: one workgroup adds the scratch words in a fixed order, writes `frames` and `cells_now`, the plane's header
//        (counts zeroed: launch 3 sums into them) and the frame's stats.
//     3. k_moving_weights: in the tiles of the apply kernel (256 byte columns x 16 rows).  The moving bytes of the cells within reach
//        G + F <= 64 of the tile become one 32-bit word per cell row in LDS (ballots); a thread owns one pixel column and every other row
//        of the tile: per cell row its horizontal distance to the nearest moving cell from the word's bits (two bit scans), then the
//        minimum over the cell rows of max(horizontal, vertical).  W from a table of F + 2 entries in LDS; the tile's flag is a workgroup
//        OR with one writer; covered and full by a wave sum and one integer atomic per wave, count and place (header and stats).  A tile
//        with no moving cell in reach writes its zeros and leaves.
// No kernel writes a word of state, W or scratch when the frame is not real; launches 2 and 3 then write the header and the flags as zeros.
#include "plate.h"
#include "redact_region.h"
#include "../../include/ext/frcnn_hip_redact_moving.h"

namespace frcnn {

constexpr int MV_CELL = FRCNN_REDACT_MOVING_CELL;                           // 8: a cell is 8 x 8 pixels
constexpr int MV_TILE_CELLS = PL_TILE_W / MV_CELL;                          // 16 cells in a tile of launch 1
constexpr int MV_REACH = FRCNN_REDACT_MOVING_GROW_MAX + FRCNN_REDACT_MOVING_FEATHER_MAX;       // 64
constexpr int MV_PX = (RD_THREADS + 2) / 3 + 1;                             // pixel columns an apply tile can touch: 86 + 1 spare
constexpr int MV_COLS = 128;                                                // threads of launch 3 along x (>= MV_PX), two rows of them
constexpr int MV_ROWS = 20;                                                 // cell rows staged by launch 3: (16 + 2 * 64 - 1) / 8 + 2 = 19 at most
static_assert(MV_CELL == 8 && PL_TILE_H == MV_CELL && PL_RUN * 2 == MV_CELL, "a cell is two threads wide and a tile high");
static_assert((MV_PX + 2 * MV_REACH - 1) / MV_CELL + 2 <= 32, "the cells in reach of a tile's columns are the bits of one word");
static_assert((RD_TILE_ROWS + 2 * MV_REACH - 1) / MV_CELL + 2 <= MV_ROWS && MV_PX <= MV_COLS && 2 * MV_COLS == RD_THREADS, "staging");

__host__ __device__ inline int mv_cells(int n) { return (n + MV_CELL - 1) / MV_CELL; }

// where the pieces of a state buffer lie, in bytes from its start: [int32 frames, cells_now, 0, 0 | left | moving | int32 part[tiles]]
struct MovingLayout { size_t left_at, moving_at, part_at, total; };

__host__ __device__ inline MovingLayout moving_layout(int h, int w) {
    MovingLayout L;
    const size_t cells = (size_t)mv_cells(h) * mv_cells(w);
    const size_t tiles = (size_t)((w + PL_TILE_W - 1) / PL_TILE_W) * ((h + PL_TILE_H - 1) / PL_TILE_H);
    L.left_at = 16;
    L.moving_at = align16(L.left_at + cells);
    L.part_at = align16(L.moving_at + cells);
    L.total = align16(L.part_at + 4 * tiles);
    return L;
}

__device__ inline int mv_floor_cell(int v) { return v >= 0 ? v / MV_CELL : -((-v + MV_CELL - 1) / MV_CELL); }

// launch 1: foreground, vote and hold of a tile's 16 cells
__global__ void __launch_bounds__(PL_THREADS) k_moving_cells(uint8_t* state, int h, int w, const uint8_t* frame, const int32_t* plate,
                                                               const int32_t* det, int rows, const uint8_t* table, int num_classes, int M,
                                                               int D, int K, int H, int unknown, int f, const int32_t* n_frames,
                                                               const int32_t* gate, const int32_t* cut) {
    __shared__ int4 s_box[PL_THREADS];                                      // (xa, xb, ya, yb) of a round's EXCEPT boxes that meet this tile
    __shared__ int s_cnt[PL_WAVES];
    __shared__ int s_fg[PL_WAVES][MV_TILE_CELLS];
    if (!plate_real(f, n_frames, gate)) return;
    const bool wipe = cut && *cut != 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx0 = blockIdx.x * PL_TILE_W, ty0 = blockIdx.y * PL_TILE_H;
    const int tx1 = min(tx0 + PL_TILE_W, w) - 1, ty1 = min(ty0 + PL_TILE_H, h) - 1;
    const int x0 = tx0 + PL_RUN * (tid % (PL_TILE_W / PL_RUN)), y = ty0 + tid / (PL_TILE_W / PL_RUN);
    const bool mine = x0 <= tx1 && y <= ty1;
    const int nd = min(max(det[0], 0), rows);
    const int32_t *bbox = det + 4, *cls = det + 4 + 4 * (size_t)rows;
    unsigned except = 0;                                                    // bit k: pixel x0 + k is under an EXCEPT box
    for (int base = 0; base < nd; base += PL_THREADS) {                     // a round
        const int total = plate_round(s_box, s_cnt, base, nd, bbox, cls, table, num_classes, M, h, w, tx0, tx1, ty0, ty1);
        if (mine)
            for (int s = 0; s < total; ++s) {
                const int4 b = s_box[s];
                if (y < b.z || y > b.w) continue;
#pragma unroll
                for (int k = 0; k < PL_RUN; ++k) except |= (unsigned)(x0 + k >= b.x && x0 + k <= b.y) << k;
            }
        __syncthreads();                                                    // (the next round writes s_cnt and s_box)
    }
    int fg = 0;
    if (mine) {
        const int n = min(PL_RUN, w - x0);                                  // pixels of the run inside the frame
        const size_t p = (size_t)y * w + x0;
        const int32_t* at = plate + 4 + 2 * p;
        uint32_t w0[PL_RUN] = {0, 0, 0, 0};                                 // P0, P1, P2, V of the run's pixels
        if (n == PL_RUN && (p & 1) == 0) {                                  // (the plate state is 16-byte aligned, and so is its pixel 0)
            const int4 a = *reinterpret_cast<const int4*>(at), b = *reinterpret_cast<const int4*>(at + 4);
            w0[0] = a.x, w0[1] = a.z, w0[2] = b.x, w0[3] = b.z;
        } else {
#pragma unroll
            for (int k = 0; k < PL_RUN; ++k)
                if (k < n) w0[k] = (uint32_t)at[2 * k];
        }
        // the run's 3n bytes start at byte `sh` of the aligned word at q, as in k_plate_update
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
            if (k < n && !((except >> k) & 1u)) {
                if (w0[k] >> 24) {
                    const int d0 = abs((int)(x[k] & 255u) - (int)(w0[k] & 255u));
                    const int d1 = abs((int)((x[k] >> 8) & 255u) - (int)((w0[k] >> 8) & 255u));
                    const int d2 = abs((int)((x[k] >> 16) & 255u) - (int)((w0[k] >> 16) & 255u));
                    fg += max(max(d0, d1), d2) > D;
                } else {
                    fg += unknown;
                }
            }
    }
    // a cell: lanes 2c and 2c + 1 of both rows of a wave, in all four waves
    fg += __shfl_xor(fg, 1);
    fg += __shfl_xor(fg, 32);
    if (lane < 32 && !(lane & 1)) s_fg[wave][lane >> 1] = fg;
    __syncthreads();
    if (tid < 64) {                                                         // (a whole wave: the ballot below)
        const int cx = blockIdx.x * MV_TILE_CELLS + tid, cy = blockIdx.y, cw = mv_cells(w);
        bool moving = false;
        if (tid < MV_TILE_CELLS && cx < cw) {
            const int count = s_fg[0][tid] + s_fg[1][tid] + s_fg[2][tid] + s_fg[3][tid];
            const int px = (min(MV_CELL * cx + MV_CELL, w) - MV_CELL * cx) * (ty1 - ty0 + 1);      // pixels of the clipped cell
            const MovingLayout L = moving_layout(h, w);
            uint8_t* left = state + L.left_at + (size_t)cy * cw + cx;
            int l = wipe ? 0 : *left;
            if (count >= min(K, px)) {
                l = H;
                moving = true;
            } else if (l > 0) {
                l -= 1;
                moving = true;
            }
            *left = (uint8_t)l;
            state[L.moving_at + (size_t)cy * cw + cx] = moving ? 1 : 0;
        }
        const unsigned long long votes = __ballot(moving);
        if (tid == 0)
            *reinterpret_cast<int32_t*>(state + moving_layout(h, w).part_at + 4 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x)) = __popcll(votes);
    }
}

// launch 2: the state's two counts, the plane's header and the frame's stats
__global__ void __launch_bounds__(PL_THREADS) k_moving_finish(uint8_t* state, int32_t* plane, int32_t* stats, int h, int w, int F, int tiles,
                                                                int f, const int32_t* n_frames, const int32_t* gate) {
    __shared__ int s_sum[PL_WAVES];
    const bool real = plate_real(f, n_frames, gate);
    int sum = 0;
    if (real) {
        const int32_t* part = reinterpret_cast<const int32_t*>(state + moving_layout(h, w).part_at);
        for (int i = threadIdx.x; i < tiles; i += PL_THREADS) sum += part[i];
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x < RR_HEAD) {
        const int t = threadIdx.x;
        plane[t] = t == RR_H ? h : t == RR_W ? w : t == RR_F ? F : t == RR_ONE ? 1 : 0;
    }
    if (threadIdx.x == 0) {
        for (int k = 1; k < PL_WAVES; ++k) sum += s_sum[k];
        if (real) {
            int32_t* head = reinterpret_cast<int32_t*>(state);
            head[0] += 1;
            head[1] = sum;
        }
        stats[0] = real ? 1 : 0;
        stats[1] = sum;                                                     // (0 for a frame that is not real)
        stats[2] = stats[3] = 0;                                            // (launch 3 sums into them)
    }
}

// launch 3: W, the tile flags and the counts, in the tiles of k_region_apply
__global__ void __launch_bounds__(RD_THREADS) k_moving_weights(const uint8_t* state, uint8_t* plane, int32_t* stats, int h, int w, int G, int F,
                                                                 int f, const int32_t* n_frames, const int32_t* gate) {
    __shared__ uint32_t s_bits[MV_ROWS];                                    // bit i of word r: cell (cx0 + i, cy0 + r) is moving
    __shared__ uint16_t s_weight[MV_REACH + 2];                             // W of e0 = 0 .. G + F + 1
    const RegionLayout L = region_layout(h, w);
    uint8_t* flag = plane + L.flags_at + (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    const int tid = threadIdx.x;
    if (!plate_real(f, n_frames, gate)) {
        if (tid == 0) *flag = 0;
        return;
    }
    const int R = G + F, rowbytes = 3 * w, j0 = blockIdx.x * RD_THREADS, y0 = blockIdx.y * RD_TILE_ROWS;
    const int y1 = min(y0 + RD_TILE_ROWS, h) - 1;
    const int tx0 = j0 / 3, tx1 = min(j0 + RD_THREADS - 1, rowbytes - 1) / 3;   // the pixel columns with a byte in this tile
    const int cw = mv_cells(w), ch = mv_cells(h);
    const int cx0 = mv_floor_cell(tx0 - R), cy0 = mv_floor_cell(y0 - R);
    const uint8_t* moving = state + moving_layout(h, w).moving_at;
    for (int idx = tid; idx < MV_ROWS * 32; idx += RD_THREADS) {            // (three rounds in waves 0-1, two in waves 2-3: the same for a whole wave, as a ballot needs)
        const int r = idx >> 5, cx = cx0 + (idx & 31), cy = cy0 + r;
        const bool on = cx >= 0 && cx < cw && cy >= 0 && cy < ch && moving[(size_t)cy * cw + cx] != 0;
        const unsigned long long votes = __ballot(on);                      // a wave holds the cell rows r and r + 1
        if ((tid & 63) == 0) {
            s_bits[r] = (uint32_t)votes;
            s_bits[r + 1] = (uint32_t)(votes >> 32);
        }
    }
    if (tid <= R + 1) s_weight[tid] = (uint16_t)(tid <= G ? 256 : tid > R ? 0 : (256 * (F + 1 - (tid - G))) / (F + 1));
    __syncthreads();
    uint32_t any_bits = 0;
    for (int r = 0; r < MV_ROWS; ++r) any_bits |= s_bits[r];
    const int xl = tid & (MV_COLS - 1), x = tx0 + xl, ya = y0 + (tid >> 7);    // this thread: column x, rows ya, ya + 2, ...
    const bool active = x <= tx1;
    const bool owner = active && 3 * x >= j0;                               // (a pixel's first byte owns its word and its count)
    uint16_t* Wp = (uint16_t*)(plane + L.w_at);
    if (any_bits == 0) {                                                    // nothing moves within reach: zeros, and the apply skips the tile
        if (owner)
            for (int y = ya; y <= y1; y += 2) Wp[(size_t)y * w + x] = 0;
        if (tid == 0) *flag = 0;
        return;
    }
    int e0[RD_TILE_ROWS / 2];
#pragma unroll
    for (int k = 0; k < RD_TILE_ROWS / 2; ++k) e0[k] = R + 1;
    if (active) {
        const int ci = x / MV_CELL - cx0;                                   // 0..31: the bit of this column's cell
        for (int r = 0; r < MV_ROWS; ++r) {
            const uint32_t b = s_bits[r];
            if (b == 0) continue;                                           // (the same for the whole workgroup)
            int hd = R + 1;
            if ((b >> ci) & 1u) {
                hd = 0;
            } else {
                const uint32_t lower = b & ((1u << ci) - 1u), upper = ci == 31 ? 0u : b >> (ci + 1);
                if (lower) hd = min(hd, x - (MV_CELL * (cx0 + 31 - __clz((int)lower)) + MV_CELL - 1));
                if (upper) hd = min(hd, MV_CELL * (cx0 + ci + __ffs((int)upper)) - x);
            }
            const int top = MV_CELL * (cy0 + r), bottom = top + MV_CELL - 1;
#pragma unroll
            for (int k = 0; k < RD_TILE_ROWS / 2; ++k) {
                const int y = ya + 2 * k;
                const int vd = y < top ? top - y : y > bottom ? y - bottom : 0;
                e0[k] = min(e0[k], max(hd, vd));
            }
        }
    }
    int covered = 0, full = 0, any = 0;
    if (active) {
#pragma unroll
        for (int k = 0; k < RD_TILE_ROWS / 2; ++k) {
            const int y = ya + 2 * k;
            if (y > y1) continue;
            const int W = s_weight[e0[k]];
            any |= W;
            if (owner) {
                Wp[(size_t)y * w + x] = (uint16_t)W;
                covered += W > 0;
                full += W == 256;
            }
        }
    }
    const int flagged = __syncthreads_or(any);
    if (tid == 0) *flag = flagged ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) { covered += __shfl_xor(covered, o); full += __shfl_xor(full, o); }
    if ((tid & 63) == 0) {
        if (covered) { atomicAdd((int*)plane + RR_COVERED, covered); atomicAdd(stats + 2, covered); }
        if (full) { atomicAdd((int*)plane + RR_FULL, full); atomicAdd(stats + 3, full); }
    }
}

static bool moving_sides_ok(int h, int w) { return h >= 1 && h <= FRCNN_REDACT_MAX_SIDE && w >= 1 && w <= FRCNN_REDACT_MAX_SIDE; }

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_redact_moving_version(void) { return FRCNN_REDACT_MOVING_VERSION; }

extern "C" size_t frcnn_redact_moving_state_bytes(int h, int w) { return moving_sides_ok(h, w) ? moving_layout(h, w).total : 0; }

extern "C" int frcnn_redact_moving_build(void* state, void* plane, int32_t* stats, int h, int w, const uint8_t* frame, const int32_t* plate,
                                         const int32_t* det, int rows, int tracked, const uint8_t* table, int num_classes, int margin,
                                         int tol, int vote, int hold, int grow, int feather, int unknown, int frame_index,
                                         const int32_t* n_frames, const int32_t* gate, const int32_t* cut, void* stream) {
    const char* who = "redact_moving_build";
    (void)tracked;                                                          // (both buffers count their rows in word 0)
    if (!state || !plane || !stats || !frame || !plate || !det || !table || !n_frames) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if ((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(plane) | reinterpret_cast<uintptr_t>(plate)) & 15u)
        return fail(FRCNN_E_ARG, "%s: the state, the plane or the plate state is not 16-byte aligned", who);
    if (!moving_sides_ok(h, w)) return fail(FRCNN_E_ARG, "%s: frame %dx%d out of range (sides 1..%d)", who, h, w, FRCNN_REDACT_MAX_SIDE);
    if (rows < 1 || rows > FRCNN_REDACT_MAX_ROWS) return fail(FRCNN_E_ARG, "%s: rows=%d not in [1, %d]", who, rows, FRCNN_REDACT_MAX_ROWS);
    if (num_classes < 1 || num_classes > 256) return fail(FRCNN_E_ARG, "%s: num_classes=%d not in [1, 256]", who, num_classes);
    if (margin < 0 || margin > FRCNN_PLATE_MAX_MARGIN)
        return fail(FRCNN_E_ARG, "%s: margin=%d not in [0, %d]", who, margin, FRCNN_PLATE_MAX_MARGIN);
    if (tol < 0 || tol > 255) return fail(FRCNN_E_ARG, "%s: tol=%d not in [0, 255]", who, tol);
    if (vote < 1 || vote > MV_CELL * MV_CELL) return fail(FRCNN_E_ARG, "%s: vote=%d not in [1, %d]", who, vote, MV_CELL * MV_CELL);
    if (hold < 0 || hold > FRCNN_REDACT_MOVING_HOLD_MAX)
        return fail(FRCNN_E_ARG, "%s: hold=%d not in [0, %d]", who, hold, FRCNN_REDACT_MOVING_HOLD_MAX);
    if (grow < 0 || grow > FRCNN_REDACT_MOVING_GROW_MAX)
        return fail(FRCNN_E_ARG, "%s: grow=%d not in [0, %d]", who, grow, FRCNN_REDACT_MOVING_GROW_MAX);
    if (feather < 0 || feather > FRCNN_REDACT_MOVING_FEATHER_MAX)
        return fail(FRCNN_E_ARG, "%s: feather=%d not in [0, %d]", who, feather, FRCNN_REDACT_MOVING_FEATHER_MAX);
    if (unknown != 0 && unknown != 1) return fail(FRCNN_E_ARG, "%s: unknown=%d is neither 0 nor 1", who, unknown);
    if (frame_index < 0 || frame_index >= FRCNN_PLATE_MAX_FRAMES)
        return fail(FRCNN_E_ARG, "%s: frame_index=%d not in [0, %d]", who, frame_index, FRCNN_PLATE_MAX_FRAMES - 1);
    hipStream_t st = as_stream(stream);
    const int gx = (w + PL_TILE_W - 1) / PL_TILE_W, gy = (h + PL_TILE_H - 1) / PL_TILE_H;
    k_moving_cells<<<dim3(gx, gy), PL_THREADS, 0, st>>>((uint8_t*)state, h, w, frame, plate, det, rows, table, num_classes, margin, tol, vote,
                                                         hold, unknown, frame_index, n_frames, gate, cut);
    if (int rc = check_launch("redact_moving_build (cells)")) return rc;
    k_moving_finish<<<1, PL_THREADS, 0, st>>>((uint8_t*)state, (int32_t*)plane, stats, h, w, feather, gx * gy, frame_index, n_frames, gate);
    if (int rc = check_launch("redact_moving_build (counts)")) return rc;
    k_moving_weights<<<dim3((3 * w + RD_THREADS - 1) / RD_THREADS, (h + RD_TILE_ROWS - 1) / RD_TILE_ROWS), RD_THREADS, 0, st>>>(
        (const uint8_t*)state, (uint8_t*)plane, stats, h, w, grow, feather, frame_index, n_frames, gate);
    return check_launch("redact_moving_build (weights)");
}
