// The path of every track, kept on the device and drawn into the frames (include/ext/frcnn_hip_track_trails.h states the rule, DESIGN §8
// "Trail rule").  gfx950 (CDNA4) only.
// k_trails_update: ONE workgroup walks the frames of a call in order -- frame f + 1 needs frame f's table.  The table lives in LDS for the
// whole call: an entry keeps its physical slot from birth to expiry (its points are a ring there, a point packed into one word: both
// coordinates lie inside a frame whose sides are at most 32768), and `s_order` lists the slots in ascending id order.  Inside a frame the
// parallelism is over rows and entries: the eligible rows are compacted in row order with wave64 ballots, each finds its entry by binary
// search, the new ids are ranked with ballots again and take the free slots, and then a thread per ENTRY walks the compacted rows and
// appends its own -- rows that share an id append in row order without any thread looking at another's entry.  Every word of the frame's
// point list, and at the end of the call of the state, is written by one thread with a plain store.  No atomics.
// k_trails_draw: a gather.  A workgroup owns a tile of 256 byte columns x 16 rows, as csrc/redact.hip's phase two does and for its reason
// (threads are bytes: 64 lanes on 64 consecutive bytes are one coalesced access wherever a row of 3-byte pixels starts).  It stages the
// segments whose grown bounding box meets the tile in LDS, 256 candidates at a time, and tests its pixels whenever the staging area could
// not take another 256 and behind the last candidate; a tile that no segment meets stores nothing.
#include "common.h"
#include "../../include/ext/frcnn_hip_redact.h"
#include "../../include/ext/frcnn_hip_track.h"
#include "../../include/ext/frcnn_hip_track_trails.h"

namespace frcnn {

constexpr int TT_THREADS = 256, TT_WAVES = TT_THREADS / 64;
constexpr int TT_CAP = FRCNN_TRACK_MAX, TT_LEN = FRCNN_TRACK_TRAILS_MAX_LENGTH, TT_ROWS = FRCNN_REDACT_MAX_ROWS;
constexpr int TT_TILE_ROWS = 16;
constexpr int TT_SEGS = 1024;                                               // segments staged in LDS at a time
static_assert(TT_CAP <= TT_THREADS && TT_SEGS >= 2 * TT_THREADS, "a thread per entry; the staging area takes a chunk of candidates");

__constant__ uint8_t TT_PALETTE[8][3] = {{255, 64, 64}, {64, 160, 255}, {255, 208, 0}, {255, 0, 255},
                                         {0, 224, 224}, {255, 128, 0}, {160, 96, 255}, {255, 255, 255}};

// The number of threads in front of this one, in thread order, whose ``flag`` is set, and ``total``, the workgroup's count.  Every thread
// of the workgroup calls it; ``s_cnt`` is free again when it returns.
__device__ inline int tt_rank(bool flag, int* s_cnt, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(flag);
    if (lane == 0) s_cnt[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < TT_WAVES; ++k) {
        const int c = s_cnt[k];
        before += k < wave ? c : 0;
        all += c;
    }
    __syncthreads();
    total = all;
    return before + __popcll(mask & ((1ull << lane) - 1ull));
}

// Word ``i`` of a state or point list of ``count`` entries: entry t is slot order[t]; ``third`` is the slots' third word (last_seen in a
// state, n in a list) and ``fourth`` their fourth (n in a state; nullptr: 0).
__device__ inline int tt_word(int i, int count, const int* order, const int* s_id, const int* s_cls, const int* third, const int* fourth,
                              const int* s_n, const int* s_start, const uint32_t (*s_pts)[TT_LEN], int N) {
    const int ew = 4 + 2 * N, t = (i - 4) / ew, j = (i - 4) - t * ew;
    if (t >= count) return 0;
    const int e = order[t];
    if (j == 0) return s_id[e];
    if (j == 1) return s_cls[e];
    if (j == 2) return third[e];
    if (j == 3) return fourth ? fourth[e] : 0;
    const int q = (j - 4) >> 1;
    if (q >= s_n[e]) return 0;
    const uint32_t pt = s_pts[e][(s_start[e] + q) % N];
    return (j & 1) ? (int)(pt >> 16) : (int)(pt & 0xffffu);
}

__global__ void __launch_bounds__(TT_THREADS) k_trails_update(int32_t* state, int cap, const int32_t* tracked, long long stride, int R, int frames,
                                                                const int32_t* n_frames, const int32_t* gate, int N, int E, int h, int w,
                                                                int32_t* lists) {
    __shared__ uint32_t s_pts[TT_CAP][TT_LEN];                              // x | y << 16, a ring per slot
    __shared__ int s_id[TT_CAP], s_cls[TT_CAP], s_seen[TT_CAP], s_n[TT_CAP], s_start[TT_CAP], s_used[TT_CAP];
    __shared__ int s_order[TT_CAP], s_snap[TT_CAP], s_free[TT_CAP];       // slots by id: all live ones, this frame's; the free slots
    __shared__ int s_rid[TT_ROWS], s_rcls[TT_ROWS], s_rent[TT_ROWS], s_rfirst[TT_ROWS];    // the frame's eligible rows, in row order
    __shared__ uint32_t s_rpt[TT_ROWS];
    __shared__ int s_cnt[TT_WAVES];
    const int tid = threadIdx.x;
    const int nf = gate && *gate == 0 ? 0 : min(max(*n_frames, 0), frames);
    const int ew = 4 + 2 * N, words = 4 + cap * ew;
    for (long long i = (long long)nf * words + tid; i < (long long)frames * words; i += TT_THREADS) lists[i] = 0;      // padding frames
    if (nf <= 0) return;
    int ne = min(max(state[0], 0), cap), fr = state[1], dropped = state[2];
    if (tid < TT_CAP) {
        const bool live = tid < ne;
        const int32_t* e = state + 4 + (size_t)(live ? tid : 0) * ew;
        s_used[tid] = live;
        s_id[tid] = live ? e[0] : 0;
        s_cls[tid] = live ? e[1] : 0;
        s_seen[tid] = live ? e[2] : 0;
        s_n[tid] = live ? min(max(e[3], 0), N) : 0;
        s_start[tid] = 0;
        s_order[tid] = tid;
    }
    for (int i = tid; i < ne * N; i += TT_THREADS) {
        const int k = i / N, q = i - k * N;
        const int32_t* p = state + 4 + (size_t)k * ew + 4 + 2 * q;
        s_pts[k][q] = ((uint32_t)p[0] & 0xffffu) | ((uint32_t)p[1] << 16);
    }
    __syncthreads();
    for (int f = 0; f < nf; ++f) {
        fr += 1;
        const int32_t* buf = tracked + (long long)f * stride;
        const int nl = min(max(buf[1], 0), R);
        const int32_t *bbox = buf + 4, *cls = buf + 4 + 4 * R, *ids = buf + 4 + 6 * R;
        int total, nfree;
        {
            const bool is_free = tid < cap && !s_used[tid];
            const int k = tt_rank(is_free, s_cnt, nfree);
            if (is_free) s_free[k] = tid;
        }
        // the eligible rows, compacted in row order
        int m = 0;
        for (int base = 0; base < nl; base += TT_THREADS) {
            const int r = base + tid;
            bool ok = false;
            int rid = 0;
            uint32_t pt = 0;
            if (r < nl && (rid = ids[r]) >= 1) {
                const int x1 = bbox[4 * r], y1 = bbox[4 * r + 1], x2 = bbox[4 * r + 2], y2 = bbox[4 * r + 3];
                const int xa = max(min(x1, x2), 0), xb = min(max(x1, x2), w - 1), ya = max(min(y1, y2), 0), yb = min(max(y1, y2), h - 1);
                ok = xa <= xb && ya <= yb;
                pt = (uint32_t)((xa + xb) >> 1) | ((uint32_t)((ya + yb) >> 1) << 16);
            }
            const int k = m + tt_rank(ok, s_cnt, total);
            if (ok) {
                s_rid[k] = rid;
                s_rcls[k] = cls[r];
                s_rpt[k] = pt;
            }
            m += total;
        }
        __syncthreads();
        // each row's entry (a slot, or -1), and for a row without one the first row of the frame that has its id
        for (int k = tid; k < m; k += TT_THREADS) {
            const int rid = s_rid[k];
            int lo = 0, hi = ne, found = -1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1, e = s_order[mid], v = s_id[e];
                if (v == rid) { found = e; break; }
                if (v < rid) lo = mid + 1; else hi = mid;
            }
            int first = k;
            if (found < 0)
                for (int j = 0; j < k; ++j)
                    if (s_rid[j] == rid) { first = j; break; }
            s_rent[k] = found;
            s_rfirst[k] = first;
        }
        __syncthreads();
        // the new ids in row order take the free slots while there are any
        int births = 0;
        for (int base = 0; base < m; base += TT_THREADS) {
            const int k = base + tid;
            const bool is_new = k < m && s_rent[k] < 0 && s_rfirst[k] == k;
            const int rank = births + tt_rank(is_new, s_cnt, total);
            if (is_new && rank < nfree) {
                const int e = s_free[rank];
                s_rent[k] = e;
                s_used[e] = 1;
                s_id[e] = s_rid[k];
                s_cls[e] = s_rcls[k];
                s_seen[e] = fr;
                s_n[e] = 0;
                s_start[e] = 0;
            }
            births += total;
        }
        __syncthreads();
        // later rows of a new id follow its first row; the rows left without an entry are counted
        for (int base = 0; base < m; base += TT_THREADS) {
            const int k = base + tid;
            bool lost = false;
            if (k < m) {
                int e = s_rent[k];
                if (e < 0 && s_rfirst[k] != k) s_rent[k] = e = s_rent[s_rfirst[k]];     // (a first row's word: nobody writes it here)
                lost = e < 0;
            }
            tt_rank(lost, s_cnt, total);
            dropped += total;
        }
        __syncthreads();
        // APPEND: a thread per entry takes its rows in row order
        if (tid < cap && s_used[tid]) {
            int n = s_n[tid], st = s_start[tid];
            bool seen = false;
            for (int k = 0; k < m; ++k) {
                if (s_rent[k] != tid) continue;
                if (n < N) {
                    s_pts[tid][(st + n) % N] = s_rpt[k];
                    n += 1;
                } else {
                    s_pts[tid][st] = s_rpt[k];
                    st = (st + 1) % N;
                }
                seen = true;
            }
            if (seen) {
                s_n[tid] = n;
                s_start[tid] = st;
                s_seen[tid] = fr;
            }
            if (fr - s_seen[tid] > E) s_used[tid] = 0;                      // EXPIRE
        }
        __syncthreads();
        // the slots in id order: all of them, and those of this frame
        const bool used = tid < cap && s_used[tid], shown = used && s_seen[tid] == fr;
        if (used) {
            const int my = s_id[tid];
            int pos = 0, snap = 0;
            for (int e = 0; e < cap; ++e) {
                const bool lower = s_used[e] && s_id[e] < my;
                pos += lower;
                snap += lower && s_seen[e] == fr;
            }
            s_order[pos] = tid;
            if (shown) s_snap[snap] = tid;
        }
        int nsnap;
        tt_rank(used, s_cnt, ne);
        tt_rank(shown, s_cnt, nsnap);                                       // (its barriers also publish s_order and s_snap)
        int32_t* L = lists + (long long)f * words;
        for (int i = tid; i < words; i += TT_THREADS)
            L[i] = i < 4 ? (i == 0 ? nsnap : 0) : tt_word(i, nsnap, s_snap, s_id, s_cls, s_n, nullptr, s_n, s_start, s_pts, N);
        __syncthreads();
    }
    for (int i = tid; i < words; i += TT_THREADS)
        state[i] = i < 4 ? (i == 0 ? ne : i == 1 ? fr : i == 2 ? dropped : 0)
                         : tt_word(i, ne, s_order, s_id, s_cls, s_seen, s_n, s_n, s_start, s_pts, N);
}

__global__ void __launch_bounds__(TT_THREADS) k_trails_draw(uint8_t* frame, int h, int w, const int32_t* list, int N, int W, int rgb) {
    __shared__ int4 s_seg[TT_SEGS];                                         // (ax, ay, bx, by)
    __shared__ int s_sid[TT_SEGS];
    __shared__ int s_cnt[TT_WAVES];
    const int nt = min(max(list[0], 0), TT_CAP);
    if (nt == 0) return;
    const int tid = threadIdx.x;
    const int rowbytes = 3 * w, j0 = blockIdx.x * TT_THREADS, y0 = blockIdx.y * TT_TILE_ROWS;
    const int y1 = min(y0 + TT_TILE_ROWS, h) - 1;
    const int tx0 = j0 / 3, tx1 = min(j0 + TT_THREADS - 1, rowbytes - 1) / 3;
    const int g = (W + 1) >> 1, ew = 4 + 2 * N, per = N - 1, cands = nt * per;
    const long long r2 = (long long)(W * W) >> 2;
    const int j = j0 + tid, x = j / 3, c = j - 3 * x;
    const bool active = j < rowbytes;
    int best[TT_TILE_ROWS];
#pragma unroll
    for (int r = 0; r < TT_TILE_ROWS; ++r) best[r] = 0;
    int n = 0, total;
    for (int base = 0; base < cands; base += TT_THREADS) {
        const int slot = base + tid;
        bool hit = false;
        int4 sg = make_int4(0, 0, 0, 0);
        int sid = 0;
        if (slot < cands) {
            const int t = slot / per, i = slot - t * per;
            const int32_t* tr = list + 4 + (size_t)t * ew;
            if (i + 1 < min(tr[2], N)) {
                sid = tr[0];
                sg = make_int4(tr[4 + 2 * i], tr[5 + 2 * i], tr[6 + 2 * i], tr[7 + 2 * i]);
                hit = sid >= 1 && (long long)max(sg.x, sg.z) + g >= tx0 && (long long)min(sg.x, sg.z) - g <= tx1 &&
                      (long long)max(sg.y, sg.w) + g >= y0 && (long long)min(sg.y, sg.w) - g <= y1;
            }
        }
        const int k = n + tt_rank(hit, s_cnt, total);
        if (hit) {
            s_seg[k] = sg;
            s_sid[k] = sid;
        }
        n += total;
        if (n + TT_THREADS <= TT_SEGS && base + TT_THREADS < cands) continue;     // room for another chunk, and there is one
        __syncthreads();
        if (active)
            for (int s = 0; s < n; ++s) {
                const int4 q = s_seg[s];
                const int id = s_sid[s];
                if (x < min(q.x, q.z) - g || x > max(q.x, q.z) + g) continue;
                const long long dx = (long long)q.z - q.x, dy = (long long)q.w - q.y, dd = dx * dx + dy * dy;
                const long long px = (long long)x - q.x, bx = (long long)x - q.z;
#pragma unroll
                for (int r = 0; r < TT_TILE_ROWS; ++r) {
                    if (id <= best[r]) continue;
                    const long long py = (long long)(y0 + r) - q.y, u = px * dx + py * dy;
                    bool cov;
                    if (dd == 0 || u <= 0) {
                        cov = px * px + py * py <= r2;
                    } else if (u >= dd) {
                        const long long by = (long long)(y0 + r) - q.w;
                        cov = bx * bx + by * by <= r2;
                    } else {
                        const long long cr = px * dy - py * dx;
                        cov = cr * cr <= ((long long)(W * W) * dd) >> 2;
                    }
                    if (cov) best[r] = id;
                }
            }
        __syncthreads();
        n = 0;
    }
    if (!active) return;
#pragma unroll
    for (int r = 0; r < TT_TILE_ROWS; ++r)
        if (y0 + r <= y1 && best[r] > 0) frame[(size_t)(y0 + r) * rowbytes + j] = TT_PALETTE[best[r] & 7][rgb ? c : 2 - c];
}

static bool trails_shape_ok(int capacity, int length) {
    return capacity >= 1 && capacity <= FRCNN_TRACK_MAX && length >= FRCNN_TRACK_TRAILS_MIN_LENGTH && length <= FRCNN_TRACK_TRAILS_MAX_LENGTH;
}

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_track_trails_version(void) { return FRCNN_TRACK_TRAILS_VERSION; }

extern "C" size_t frcnn_track_trails_list_words(int capacity, int length) {
    return trails_shape_ok(capacity, length) ? 4 + (size_t)capacity * (4 + 2 * (size_t)length) : 0;
}

extern "C" size_t frcnn_track_trails_state_bytes(int capacity, int length) {
    return sizeof(int32_t) * frcnn_track_trails_list_words(capacity, length);
}

extern "C" int frcnn_track_trails_update(int32_t* state, int capacity, const int32_t* tracked, long long tracked_stride, int rows, int frames,
                                         const int32_t* n_frames, const int32_t* gate, int length, int expire, int h, int w, int32_t* lists,
                                         void* stream) {
    const char* who = "track_trails_update";
    if (!state || !tracked || !n_frames || !lists) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (capacity < 1 || capacity > FRCNN_TRACK_MAX) return fail(FRCNN_E_ARG, "%s: capacity=%d not in [1, %d]", who, capacity, FRCNN_TRACK_MAX);
    if (rows < 1 || rows > FRCNN_REDACT_MAX_ROWS) return fail(FRCNN_E_ARG, "%s: rows=%d not in [1, %d]", who, rows, FRCNN_REDACT_MAX_ROWS);
    if (frames < 1 || frames > FRCNN_TRACK_MAX_FRAMES)
        return fail(FRCNN_E_ARG, "%s: frames=%d not in [1, %d]", who, frames, FRCNN_TRACK_MAX_FRAMES);
    if (frames > 1 && tracked_stride < 4 + 8LL * rows)
        return fail(FRCNN_E_ARG, "%s: tracked_stride=%lld under the %d words of a tracked buffer", who, tracked_stride, 4 + 8 * rows);
    if (length < FRCNN_TRACK_TRAILS_MIN_LENGTH || length > FRCNN_TRACK_TRAILS_MAX_LENGTH)
        return fail(FRCNN_E_ARG, "%s: length=%d not in [%d, %d]", who, length, FRCNN_TRACK_TRAILS_MIN_LENGTH, FRCNN_TRACK_TRAILS_MAX_LENGTH);
    if (expire < 0 || expire > FRCNN_TRACK_TRAILS_MAX_EXPIRE)
        return fail(FRCNN_E_ARG, "%s: expire=%d not in [0, %d]", who, expire, FRCNN_TRACK_TRAILS_MAX_EXPIRE);
    if (h < 1 || h > FRCNN_REDACT_MAX_SIDE || w < 1 || w > FRCNN_REDACT_MAX_SIDE)
        return fail(FRCNN_E_ARG, "%s: frame %dx%d out of range (sides 1..%d)", who, h, w, FRCNN_REDACT_MAX_SIDE);
    k_trails_update<<<1, TT_THREADS, 0, as_stream(stream)>>>(state, capacity, tracked, tracked_stride, rows, frames, n_frames, gate, length, expire,
                                                             h, w, lists);
    return check_launch(who);
}

extern "C" int frcnn_track_trails_draw_u8(uint8_t* frame, int h, int w, const int32_t* list, int length, int width, int rgb, void* stream) {
    const char* who = "track_trails_draw_u8";
    if (!frame || !list) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (h < 1 || h > FRCNN_REDACT_MAX_SIDE || w < 1 || w > FRCNN_REDACT_MAX_SIDE)
        return fail(FRCNN_E_ARG, "%s: frame %dx%d out of range (sides 1..%d)", who, h, w, FRCNN_REDACT_MAX_SIDE);
    if (length < FRCNN_TRACK_TRAILS_MIN_LENGTH || length > FRCNN_TRACK_TRAILS_MAX_LENGTH)
        return fail(FRCNN_E_ARG, "%s: length=%d not in [%d, %d]", who, length, FRCNN_TRACK_TRAILS_MIN_LENGTH, FRCNN_TRACK_TRAILS_MAX_LENGTH);
    if (width < 1 || width > FRCNN_TRACK_TRAILS_MAX_WIDTH)
        return fail(FRCNN_E_ARG, "%s: width=%d not in [1, %d]", who, width, FRCNN_TRACK_TRAILS_MAX_WIDTH);
    k_trails_draw<<<dim3((3 * w + TT_THREADS - 1) / TT_THREADS, (h + TT_TILE_ROWS - 1) / TT_TILE_ROWS), TT_THREADS, 0, as_stream(stream)>>>(
        frame, h, w, list, length, width, rgb ? 1 : 0);
    return check_launch(who);
}
