// A returning object given its old id back (include/ext/frcnn_hip_track_reid.h states the rule, DESIGN §8 "Re-identify rule").  gfx950
// (CDNA4) only.
// k_reid_signatures: a workgroup per (row, frame).  A row that gets no signature costs its workgroup one word; for the others threads are
// samples of the motion rule's grid, each adds one to one of 192 counters in LDS with an integer LDS atomic (integer sums do not depend on
// order), and the first 192 threads normalise and store.  Frame bytes are read where they lie, as the motion search reads them: a strided
// grid does not tile.
// k_reid_step: ONE workgroup walks the frames of a call in order -- frame f + 1 needs frame f's table.  The five head words of every entry
// live in LDS for the whole call; the 192-word signatures stay where they are, in the state: 256 x 192 words need no LDS, they are read
// once per (row, candidate) pair, by a wave with three words a lane and a shuffle sum.  A thread per entry scans the frame's ids for
// PRESENT and BOUND, a thread per row scans the tids for UNBOUND and OUT.  The unbound rows take their turns one after another (the rule
// is sequential there, and such rows are births: rare); the waves share a row's candidates and meet in one packed key, D << 32 | place,
// under a 64-bit minimum: the table is in pid order, so the lowest place among equal distances is the lowest pid.  Signature word k of
// every entry is moved by thread k alone when the table opens for an insert or closes over the removed, so the moves need no barrier
// between them.  Every word has one writer per phase, phases are separated by barriers, and there are no atomics on memory.
#include "common.h"
#include "../../include/ext/frcnn_hip_redact.h"
#include "../../include/ext/frcnn_hip_track.h"
#include "../../include/ext/frcnn_hip_track_motion.h"
#include "../../include/ext/frcnn_hip_track_reid.h"

namespace frcnn {

constexpr int RD_THREADS = 256, RD_WAVES = RD_THREADS / 64;
constexpr int RD_CAP = FRCNN_TRACK_REID_MAX, RD_ROWS = FRCNN_REDACT_MAX_ROWS, RD_SIG = FRCNN_TRACK_REID_SIG_WORDS;
constexpr int RD_BINS = FRCNN_TRACK_REID_BINS, RD_BANDS = FRCNN_TRACK_REID_BANDS, RD_GRID = FRCNN_TRACK_MOTION_GRID;
constexpr int RD_ENTRY = FRCNN_TRACK_REID_ENTRY_WORDS, RD_WS = 1 + RD_SIG, RD_EVENTS = FRCNN_TRACK_REID_MAX_EVENTS;
constexpr int RD_LIST = FRCNN_TRACK_REID_LIST_WORDS;
enum { RD_PID, RD_TID, RD_CLS, RD_SEEN, RD_HAS, RD_META };
static_assert(RD_CAP == RD_THREADS && RD_SIG <= RD_THREADS, "a thread per entry, and per word of a signature");
static_assert(RD_SIG == 3 * 64 && RD_SIG == RD_BANDS * RD_BINS && RD_ENTRY == RD_META + RD_SIG, "a lane holds three words of a signature");
static_assert(RD_LIST == 4 + 5 * RD_EVENTS && RD_BINS == 64, "a list is its head and 32 events; two bits a channel");

// The signature words of entry ``e`` of a state.
__device__ inline int32_t* rd_sig(int32_t* state, int e) { return state + 4 + (size_t)e * RD_ENTRY + RD_META; }

// Does any thread of the workgroup set ``flag``?  Every thread calls it; ``s_cnt`` is free again when it returns.
__device__ inline bool rd_any(bool flag, int* s_cnt) {
    const unsigned long long mask = __ballot(flag);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = mask != 0ull;
    __syncthreads();
    int any = 0;
    for (int k = 0; k < RD_WAVES; ++k) any |= s_cnt[k];
    __syncthreads();
    return any != 0;
}

__global__ void __launch_bounds__(RD_THREADS) k_reid_signatures(const uint8_t* frames_u8, long long frame_stride, int h, int w, int rgb,
                                                                  const int32_t* tracked, long long stride, int R, int frames,
                                                                  const int32_t* n_frames, const uint8_t* classes, int nc, int32_t* ws) {
    __shared__ int s_hist[RD_SIG];
    const int tid = threadIdx.x, r = blockIdx.x, f = blockIdx.y;
    if (f >= min(max(*n_frames, 0), frames)) return;                        // padding: nothing is written
    const int32_t* buf = tracked + (long long)f * stride;
    int32_t* o = ws + ((size_t)f * R + r) * RD_WS;
    const int nrows = min(max(buf[0], 0), R), nl = min(max(buf[1], 0), nrows);
    int sx = 1, sy = 1, x0 = 0, y0 = 0, cols = 0, rows = 0;
    if (r < nl && buf[4 + 6 * R + r] >= 1) {
        const int c = buf[4 + 4 * R + r];
        if (c >= 0 && c < nc && classes[c] != 0) {
            const int x1 = buf[4 + 4 * r], y1 = buf[4 + 4 * r + 1], x2 = buf[4 + 4 * r + 2], y2 = buf[4 + 4 * r + 3];
            const int xa = max(min(x1, x2), 0), xb = min(max(x1, x2), w - 1), ya = max(min(y1, y2), 0), yb = min(max(y1, y2), h - 1);
            if (xa <= xb && ya <= yb) {                                     // the motion rule's GRID
                sx = (xb - xa + 1 + RD_GRID - 1) / RD_GRID;
                sy = (yb - ya + 1 + RD_GRID - 1) / RD_GRID;
                x0 = xa + sx / 2;
                y0 = ya + sy / 2;
                cols = (xb - x0) / sx + 1;                                  // (x0 + (cols - 1) sx <= xb <= w - 1: every sample is in the frame)
                rows = (yb - y0) / sy + 1;
            }
        }
    }
    const int n = cols * rows;
    if (n < FRCNN_TRACK_MOTION_MIN_SAMPLES) {                               // (the whole workgroup)
        if (tid == 0) o[0] = 0;
        return;
    }
    if (tid < RD_SIG) s_hist[tid] = 0;
    __syncthreads();
    const uint8_t* src = frames_u8 + (long long)f * frame_stride;
    for (int i = tid; i < n; i += RD_THREADS) {
        const int j = i / cols, x = x0 + (i - j * cols) * sx, y = y0 + j * sy;
        const uint8_t* p = src + ((size_t)y * w + x) * 3;
        const int red = p[rgb ? 0 : 2], green = p[1], blue = p[rgb ? 2 : 0];
        atomicAdd(&s_hist[(3 * j / rows) * RD_BINS + ((red >> 6) << 4 | (green >> 6) << 2 | (blue >> 6))], 1);
    }
    __syncthreads();
    if (tid < RD_SIG) o[1 + tid] = (s_hist[tid] << 12) / n;
    if (tid == 0) o[0] = 1;
}

__global__ void __launch_bounds__(RD_THREADS) k_reid_step(int32_t* state, int cap, const int32_t* tracked, long long stride, int R, int frames,
                                                            const int32_t* n_frames, const int32_t* cuts, const uint8_t* classes, int nc,
                                                            int pct, int keep, const int32_t* ws, int32_t* out, long long ostride,
                                                            int32_t* lists) {
    __shared__ int s_m[RD_META][RD_CAP];                                    // the entries' head words
    __shared__ int s_gone[RD_CAP], s_lrow[RD_CAP], s_dead[RD_CAP];          // tid not PRESENT; the lowest live row of the tid; removed
    __shared__ int s_rid[RD_ROWS], s_unb[RD_ROWS];                          // the frame's ids (0: none); the row is unbound and takes a turn
    __shared__ int s_ev[5 * RD_EVENTS];
    __shared__ unsigned long long s_key[RD_WAVES];
    __shared__ int s_cnt[RD_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nf = min(max(*n_frames, 0), frames), words = 4 + 8 * R;
    for (int f = nf; f < frames; ++f) {                                     // padding frames: the buffer as it is, an empty list
        const int32_t* buf = tracked + (long long)f * stride;
        int32_t* obuf = out + (long long)f * ostride;
        for (int i = tid; i < words; i += RD_THREADS) obuf[i] = buf[i];
        for (int i = tid; i < RD_LIST; i += RD_THREADS) lists[(long long)f * RD_LIST + i] = 0;
    }
    if (nf <= 0) return;
    int ne = min(max(state[0], 0), cap), fr = state[1], dropped = state[2], reid = state[3], hi = ne;
    {
        const bool live = tid < ne;
        const int32_t* e = state + 4 + (size_t)(live ? tid : 0) * RD_ENTRY;
#pragma unroll
        for (int j = 0; j < RD_META; ++j) s_m[j][tid] = live ? e[j] : 0;
    }
    __syncthreads();
    for (int f = 0; f < nf; ++f) {
        const int32_t* buf = tracked + (long long)f * stride;
        int32_t* obuf = out + (long long)f * ostride;
        const int32_t *cls = buf + 4 + 4 * R, *ids = buf + 4 + 6 * R;
        const int32_t* wsf = ws + (size_t)f * R * RD_WS;
        const int nrows = min(max(buf[0], 0), R), nl = min(max(buf[1], 0), nrows);
        if (cuts && cuts[f] != 0) ne = 0;                                   // 0 CUT (the words are zeroed behind the last frame: `hi`)
        fr += 1;
        for (int r = tid; r < nrows; r += RD_THREADS) s_rid[r] = max(ids[r], 0);
        for (int i = tid; i < 5 * RD_EVENTS; i += RD_THREADS) s_ev[i] = 0;
        __syncthreads();
        // 2 PRESENT, and the row of step 3: a thread per entry
        if (tid < ne) {
            const int t = s_m[RD_TID][tid];
            int present = 0, lrow = -1;
            for (int r = 0; r < nrows; ++r)
                if (s_rid[r] == t && t >= 1) {
                    present = 1;
                    if (r < nl && lrow < 0) lrow = r;
                }
            s_gone[tid] = !present;
            s_lrow[tid] = lrow;
        }
        // the rows of step 4, against the table as the frame found it: a thread per row
        for (int r = tid; r < nl; r += RD_THREADS) {
            const int t = s_rid[r];
            int ok = 0;
            if (t >= 1) {
                const int c = cls[r];
                ok = c >= 0 && c < nc && classes[c] != 0;
                for (int e = 0; ok && e < ne; ++e) ok = s_m[RD_TID][e] != t;
            }
            s_unb[r] = ok;
        }
        __syncthreads();
        // 3 BOUND: a wave per entry
        for (int e = wave; e < ne; e += RD_WAVES) {
            const int lr = s_lrow[e];
            if (lr < 0) continue;
            const int32_t* s = wsf + (size_t)lr * RD_WS;
            if (s[0] == 0) continue;
            int32_t* g = rd_sig(state, e);
            const int has = s_m[RD_HAS][e];
            for (int k = lane; k < RD_SIG; k += 64) g[k] = has ? (3 * g[k] + s[1 + k] + 2) >> 2 : s[1 + k];
            if (lane == 0) {
                s_m[RD_HAS][e] = 1;
                s_m[RD_SEEN][e] = fr;
            }
        }
        __syncthreads();
        // 4 UNBOUND: the rows in order, one at a time
        int nev = 0;
        for (int r = 0; r < nl; ++r) {
            if (!s_unb[r]) continue;                                        // (the same word for every thread)
            const int t = s_rid[r], c = cls[r];
            if (rd_any(tid < ne && s_m[RD_TID][tid] == t, s_cnt)) continue;   // an earlier row of the frame has bound t
            const int32_t* s = wsf + (size_t)r * RD_WS;
            const bool has = s[0] != 0;
            unsigned long long best = ~0ull;
            if (has) {
                const int s0 = s[1 + lane], s1 = s[65 + lane], s2 = s[129 + lane];
                for (int e = wave; e < ne; e += RD_WAVES) {                 // (wave-uniform: the shuffles below see all 64 lanes)
                    if (s_m[RD_CLS][e] != c || !s_m[RD_HAS][e] || !s_gone[e] || fr - s_m[RD_SEEN][e] > keep) continue;
                    const int32_t* g = rd_sig(state, e);
                    int d = abs(g[lane] - s0) + abs(g[64 + lane] - s1) + abs(g[128 + lane] - s2);
                    for (int off = 32; off > 0; off >>= 1) d += __shfl_xor(d, off);
                    const unsigned long long key = ((unsigned long long)d << 32) | (unsigned)e;
                    best = key < best ? key : best;
                }
            }
            if (lane == 0) s_key[wave] = best;
            __syncthreads();
            best = s_key[0];
            for (int k = 1; k < RD_WAVES; ++k) best = s_key[k] < best ? s_key[k] : best;
            __syncthreads();
            const long long D = (long long)(best >> 32);
            if (best != ~0ull && D * 100 <= (long long)pct * FRCNN_TRACK_REID_MAX_DISTANCE) {
                const int e = (int)(best & 0xffffffffull);
                if (tid < RD_SIG) {
                    int32_t* g = rd_sig(state, e);
                    g[tid] = (3 * g[tid] + s[1 + tid] + 2) >> 2;            // (a candidate has a signature)
                }
                if (tid == 0) {
                    if (nev < RD_EVENTS) {
                        s_ev[5 * nev] = s_m[RD_PID][e];
                        s_ev[5 * nev + 1] = t;
                        s_ev[5 * nev + 2] = c;
                        s_ev[5 * nev + 3] = (int)D;
                        s_ev[5 * nev + 4] = fr - s_m[RD_SEEN][e];
                    }
                    s_m[RD_TID][e] = t;
                    s_m[RD_SEEN][e] = fr;
                    s_gone[e] = 0;                                          // t is present: nobody takes the entry again in this frame
                }
                nev += 1;
                reid += 1;
                __syncthreads();
            } else if (ne >= cap) {
                dropped += 1;
            } else {
                int pos = ne;                                               // behind the last entry with pid <= t: mostly the end
                if (ne > 0 && s_m[RD_PID][ne - 1] > t) {
                    pos = 0;
                    for (int e = 0; e < ne; ++e) pos += s_m[RD_PID][e] <= t;
                }
                int mv[RD_META], gone = 0;
                const bool up = tid >= pos && tid < ne;
                if (up) {
#pragma unroll
                    for (int j = 0; j < RD_META; ++j) mv[j] = s_m[j][tid];
                    gone = s_gone[tid];
                }
                __syncthreads();
                if (up) {                                                   // (tid + 1 <= ne < cap)
#pragma unroll
                    for (int j = 0; j < RD_META; ++j) s_m[j][tid + 1] = mv[j];
                    s_gone[tid + 1] = gone;
                }
                if (tid < RD_SIG) {
                    for (int e = ne - 1; e >= pos; --e) rd_sig(state, e + 1)[tid] = rd_sig(state, e)[tid];
                    rd_sig(state, pos)[tid] = has ? s[1 + tid] : 0;
                }
                if (tid == 0) {
                    s_m[RD_PID][pos] = t;
                    s_m[RD_TID][pos] = t;
                    s_m[RD_CLS][pos] = c;
                    s_m[RD_SEEN][pos] = fr;
                    s_m[RD_HAS][pos] = has;
                    s_gone[pos] = 0;
                }
                ne += 1;
                hi = max(hi, ne);
                __syncthreads();
            }
        }
        // 5 OUT: word for word, the ids of the rows through the table
        for (int i = tid; i < words; i += RD_THREADS) {
            int v = buf[i];
            const int k = i - (4 + 6 * R);
            if (k >= 0 && k < nrows && v >= 1)
                for (int e = 0; e < ne; ++e)
                    if (s_m[RD_TID][e] == v) {
                        v = s_m[RD_PID][e];
                        break;
                    }
            obuf[i] = v;
        }
        // 6 EXPIRE
        const bool dead = tid < ne && s_gone[tid] && fr - s_m[RD_SEEN][tid] > keep;
        s_dead[tid] = dead;
        if (rd_any(dead, s_cnt)) {                                          // (its barriers publish s_dead)
            int mv[RD_META], pos = 0, left = 0;
            const bool stays = tid < ne && !dead;
            for (int e = 0; e < ne; ++e) {
                pos += e < tid && !s_dead[e];
                left += !s_dead[e];
            }
            if (stays) {
#pragma unroll
                for (int j = 0; j < RD_META; ++j) mv[j] = s_m[j][tid];
            }
            __syncthreads();
            if (stays) {
#pragma unroll
                for (int j = 0; j < RD_META; ++j) s_m[j][pos] = mv[j];
            }
            if (tid < RD_SIG) {
                int p = 0;
                for (int e = 0; e < ne; ++e) {
                    if (s_dead[e]) continue;
                    if (p != e) rd_sig(state, p)[tid] = rd_sig(state, e)[tid];
                    p += 1;
                }
            }
            ne = left;
            __syncthreads();
        }
        // 7 LIST
        int32_t* L = lists + (long long)f * RD_LIST;
        for (int i = tid; i < RD_LIST; i += RD_THREADS) L[i] = i == 0 ? min(nev, RD_EVENTS) : i == 1 ? fr : i < 4 ? 0 : s_ev[i - 4];
        __syncthreads();
    }
    // the head, the entries' head words, and zeros behind the live entries as far as the table ever reached in this call
    const int total = 4 + hi * RD_ENTRY;
    for (int i = tid; i < total; i += RD_THREADS) {
        if (i < 4) {
            state[i] = i == 0 ? ne : i == 1 ? fr : i == 2 ? dropped : reid;
            continue;
        }
        const int e = (i - 4) / RD_ENTRY, j = (i - 4) - e * RD_ENTRY;
        if (e >= ne)
            state[i] = 0;
        else if (j < RD_META)
            state[i] = s_m[j][e];
    }
}

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_track_reid_version(void) { return FRCNN_TRACK_REID_VERSION; }

extern "C" size_t frcnn_track_reid_state_bytes(int capacity) {
    return capacity >= 1 && capacity <= FRCNN_TRACK_REID_MAX ? sizeof(int32_t) * (4 + (size_t)capacity * RD_ENTRY) : 0;
}

extern "C" size_t frcnn_track_reid_workspace_bytes(int frames, int max_rows) {
    if (frames < 1 || frames > FRCNN_TRACK_MAX_FRAMES || max_rows < 1 || max_rows > FRCNN_REDACT_MAX_ROWS) return 0;
    return sizeof(int32_t) * RD_WS * (size_t)frames * max_rows;
}

extern "C" int frcnn_track_reid_update(int32_t* state, int capacity, const uint8_t* frames_u8, long long frame_stride, int h, int w, int rgb,
                                       const int32_t* tracked, long long tracked_stride, int max_rows, int frames, const int32_t* n_frames,
                                       const int32_t* cuts, const uint8_t* classes, int num_classes, int pct, int keep, int32_t* workspace,
                                       int32_t* out, long long out_stride, int32_t* lists, void* stream) {
    const char* who = "track_reid_update";
    if (!state || !frames_u8 || !tracked || !n_frames || !classes || !workspace || !out || !lists)
        return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (out == tracked) return fail(FRCNN_E_ARG, "%s: out must not be the tracked buffer", who);
    if (capacity < 1 || capacity > FRCNN_TRACK_REID_MAX)
        return fail(FRCNN_E_ARG, "%s: capacity=%d not in [1, %d]", who, capacity, FRCNN_TRACK_REID_MAX);
    if (frames < 1 || frames > FRCNN_TRACK_MAX_FRAMES)
        return fail(FRCNN_E_ARG, "%s: frames=%d not in [1, %d]", who, frames, FRCNN_TRACK_MAX_FRAMES);
    if (max_rows < 1 || max_rows > FRCNN_REDACT_MAX_ROWS)
        return fail(FRCNN_E_ARG, "%s: max_rows=%d not in [1, %d]", who, max_rows, FRCNN_REDACT_MAX_ROWS);
    if (h < 1 || h > FRCNN_REDACT_MAX_SIDE || w < 1 || w > FRCNN_REDACT_MAX_SIDE)
        return fail(FRCNN_E_ARG, "%s: frame %dx%d out of range (sides 1..%d)", who, h, w, FRCNN_REDACT_MAX_SIDE);
    if (frames > 1 && frame_stride < 3LL * h * w)
        return fail(FRCNN_E_ARG, "%s: frame_stride=%lld under the %lld bytes of a frame", who, frame_stride, 3LL * h * w);
    if (frames > 1 && (tracked_stride < 4 + 8LL * max_rows || out_stride < 4 + 8LL * max_rows))
        return fail(FRCNN_E_ARG, "%s: tracked_stride=%lld or out_stride=%lld under the %d words of a tracked buffer", who, tracked_stride,
                    out_stride, 4 + 8 * max_rows);
    if (num_classes < 1 || num_classes > 256) return fail(FRCNN_E_ARG, "%s: num_classes=%d not in [1, 256]", who, num_classes);
    if (pct < 1 || pct > 100) return fail(FRCNN_E_ARG, "%s: pct=%d not in [1, 100]", who, pct);
    if (keep < 1 || keep > FRCNN_TRACK_REID_MAX_KEEP)
        return fail(FRCNN_E_ARG, "%s: keep=%d not in [1, %d]", who, keep, FRCNN_TRACK_REID_MAX_KEEP);
    if (rgb != 0 && rgb != 1) return fail(FRCNN_E_ARG, "%s: rgb=%d is neither 0 nor 1", who, rgb);
    if (reinterpret_cast<uintptr_t>(workspace) & 3) return fail(FRCNN_E_ARG, "%s: workspace is not 4-byte aligned", who);
    hipStream_t st = as_stream(stream);
    k_reid_signatures<<<dim3(max_rows, frames), RD_THREADS, 0, st>>>(frames_u8, frame_stride, h, w, rgb, tracked, tracked_stride, max_rows,
                                                                     frames, n_frames, classes, num_classes, workspace);
    k_reid_step<<<1, RD_THREADS, 0, st>>>(state, capacity, tracked, tracked_stride, max_rows, frames, n_frames, cuts, classes, num_classes, pct,
                                          keep, workspace, out, out_stride, lists);
    return check_launch(who);
}
