// The path of every track, kept on the device and drawn into the frames (include/ext/frcnn_hip_track_trails.h states the rule, DESIGN §8
// "Trail rule").  gfx950 (CDNA4) only.
// k_trails_update: the id-table walk of csrc/id_table.h -- ONE workgroup walks the frames of a call in order, frame f + 1 needs frame f's
// table -- over a table of its own: an entry keeps its physical slot from birth to expiry (its points are a ring there, a point packed
// into one word: both coordinates lie inside a frame whose sides are at most 32768), and `s_order` lists the slots in ascending id order,
// so the binary search goes through it and the births take the free slots.  A thread per ENTRY walks the compacted rows and appends its
// own -- rows that share an id append in row order without any thread looking at another's entry.  Every word of the frame's point list,
// and at the end of the call of the state, is written by one thread with a plain store.  No atomics.
// k_trails_draw: a gather over the tiles of csrc/overlay.h.  It stages the segments whose grown bounding box meets the tile in LDS, 256
// candidates at a time, and tests its pixels whenever the staging area could not take another 256 and behind the last candidate; a tile
// that no segment meets stores nothing.
#include "id_table.h"
#include "overlay.h"
#include "../../include/ext/frcnn_hip_track_trails.h"

namespace frcnn {

constexpr int TT_LEN = FRCNN_TRACK_TRAILS_MAX_LENGTH;
constexpr int TT_SEGS = 1024;                                               // segments staged in LDS at a time
static_assert(TT_SEGS >= 2 * OV_THREADS && OV_THREADS == IDT_THREADS, "the staging area takes a chunk of candidates; wg_append ranks a drawing workgroup");

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

__global__ void __launch_bounds__(IDT_THREADS) k_trails_update(int32_t* state, int cap, const int32_t* tracked, long long stride, int R, int frames,
                                                                 const int32_t* n_frames, const int32_t* gate, int N, int E, int h, int w,
                                                                 int32_t* lists) {
    __shared__ uint32_t s_pts[IDT_CAP][TT_LEN];                             // x | y << 16, a ring per slot
    __shared__ int s_id[IDT_CAP], s_cls[IDT_CAP], s_seen[IDT_CAP], s_n[IDT_CAP], s_start[IDT_CAP], s_used[IDT_CAP];
    __shared__ int s_order[IDT_CAP], s_snap[IDT_CAP], s_free[IDT_CAP];    // slots by id: all live ones, this frame's; the free slots
    __shared__ int s_rid[IDT_ROWS], s_rcls[IDT_ROWS], s_rent[IDT_ROWS], s_rfirst[IDT_ROWS];    // the frame's eligible rows, in row order
    __shared__ uint32_t s_rpt[IDT_ROWS];
    __shared__ int s_cnt[IDT_WAVES];
    const int tid = threadIdx.x;
    const int ew = 4 + 2 * N, words = 4 + cap * ew;
    const int nf = idt_begin(gate, n_frames, frames, lists, words);
    if (nf <= 0) return;
    int ne = min(max(state[0], 0), cap), fr = state[1], dropped = state[2];
    if (tid < IDT_CAP) {
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
    for (int i = tid; i < ne * N; i += IDT_THREADS) {
        const int k = i / N, q = i - k * N;
        const int32_t* p = state + 4 + (size_t)k * ew + 4 + 2 * q;
        s_pts[k][q] = ((uint32_t)p[0] & 0xffffu) | ((uint32_t)p[1] << 16);
    }
    __syncthreads();
    for (int f = 0; f < nf; ++f) {
        fr += 1;
        const IdRows rows = idt_rows(tracked, stride, f, R);
        int nfree;
        {
            const bool is_free = tid < cap && !s_used[tid];
            const int k = wg_rank(is_free, s_cnt, nfree);
            if (is_free) s_free[k] = tid;
        }
        // the eligible rows, compacted in row order: the live ones, their point the centre
        int m = 0;
        for (int base = 0; base < rows.n; base += IDT_THREADS) {
            const int r = base + tid;
            int rid = 0, xa = 0, xb = 0, ya = 0, yb = 0;
            const bool ok = idt_live(rows, r, h, w, rid, xa, xb, ya, yb);
            const int k = wg_append(ok, s_cnt, m);
            if (ok) {
                s_rid[k] = rid;
                s_rcls[k] = rows.cls[r];
                s_rpt[k] = (uint32_t)((xa + xb) >> 1) | ((uint32_t)((ya + yb) >> 1) << 16);
            }
        }
        __syncthreads();
        for (int k = tid; k < m; k += IDT_THREADS) idt_lookup(k, s_rid, s_id, s_order, ne, s_rent, s_rfirst);
        __syncthreads();
        // the new ids in row order take the free slots while there are any
        int births = 0;
        for (int base = 0; base < m; base += IDT_THREADS) {
            const int k = base + tid;
            const bool is_new = idt_birth(k, m, s_rent, s_rfirst);
            const int rank = wg_append(is_new, s_cnt, births);
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
        }
        __syncthreads();
        dropped += idt_follow(m, s_rent, s_rfirst, s_cnt);
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
        wg_rank(used, s_cnt, ne);
        wg_rank(shown, s_cnt, nsnap);                                       // (its barriers also publish s_order and s_snap)
        int32_t* L = lists + (long long)f * words;
        for (int i = tid; i < words; i += IDT_THREADS)
            L[i] = i < 4 ? (i == 0 ? nsnap : 0) : tt_word(i, nsnap, s_snap, s_id, s_cls, s_n, nullptr, s_n, s_start, s_pts, N);
        __syncthreads();
    }
    for (int i = tid; i < words; i += IDT_THREADS)
        state[i] = i < 4 ? (i == 0 ? ne : i == 1 ? fr : i == 2 ? dropped : 0)
                         : tt_word(i, ne, s_order, s_id, s_cls, s_seen, s_n, s_n, s_start, s_pts, N);
}

__global__ void __launch_bounds__(OV_THREADS) k_trails_draw(uint8_t* frame, int h, int w, const int32_t* list, int N, int W, int rgb) {
    __shared__ int4 s_seg[TT_SEGS];                                         // (ax, ay, bx, by)
    __shared__ int s_sid[TT_SEGS];
    __shared__ int s_cnt[IDT_WAVES];
    const int nt = min(max(list[0], 0), IDT_CAP);
    if (nt == 0) return;
    const int tid = threadIdx.x;
    const OvTile t = ov_tile(h, w);
    const int g = ov_grow(W), ew = 4 + 2 * N, per = N - 1, cands = nt * per;
    const bool active = t.j < t.rowbytes;
    int best[OV_TILE_ROWS];
#pragma unroll
    for (int r = 0; r < OV_TILE_ROWS; ++r) best[r] = 0;
    int n = 0;
    for (int base = 0; base < cands; base += OV_THREADS) {
        const int slot = base + tid;
        bool hit = false;
        int4 sg = make_int4(0, 0, 0, 0);
        int sid = 0;
        if (slot < cands) {
            const int tr_i = slot / per, i = slot - tr_i * per;
            const int32_t* tr = list + 4 + (size_t)tr_i * ew;
            if (i + 1 < min(tr[2], N)) {
                sid = tr[0];
                sg = make_int4(tr[4 + 2 * i], tr[5 + 2 * i], tr[6 + 2 * i], tr[7 + 2 * i]);
                // (ov_meets in 64 bits: the words of a list are whatever the caller's memory holds)
                hit = sid >= 1 && (long long)max(sg.x, sg.z) + g >= t.tx0 && (long long)min(sg.x, sg.z) - g <= t.tx1 &&
                      (long long)max(sg.y, sg.w) + g >= t.ty0 && (long long)min(sg.y, sg.w) - g <= t.ty1;
            }
        }
        const int k = wg_append(hit, s_cnt, n);
        if (hit) {
            s_seg[k] = sg;
            s_sid[k] = sid;
        }
        if (n + OV_THREADS <= TT_SEGS && base + OV_THREADS < cands) continue;     // room for another chunk, and there is one
        __syncthreads();
        if (active)
            for (int s = 0; s < n; ++s) {
                const int4 q = s_seg[s];
                const int id = s_sid[s];
                if (!ov_column_near(q.x, q.z, g, t.x)) continue;
                const OvCapsule cap = ov_capsule(q.x, q.y, q.z, q.w, t.x, W);
#pragma unroll
                for (int r = 0; r < OV_TILE_ROWS; ++r)
                    if (id > best[r]) capsule_paint<false>(cap, t.ty0 + r, best[r], id);
            }
        __syncthreads();
        n = 0;
    }
    if (!active) return;
#pragma unroll
    for (int r = 0; r < OV_TILE_ROWS; ++r)
        if (t.ty0 + r <= t.ty1 && best[r] > 0) frame[(size_t)(t.ty0 + r) * t.rowbytes + t.j] = ov_colour(best[r] & 7, t.c, rgb);
}

static bool trails_shape_ok(int capacity, int length) {
    return capacity >= 1 && capacity <= FRCNN_TRACK_MAX && length >= FRCNN_TRACK_TRAILS_MIN_LENGTH && length <= FRCNN_TRACK_TRAILS_MAX_LENGTH;
}

static int trails_length_ok(const char* who, int length) {
    if (length < FRCNN_TRACK_TRAILS_MIN_LENGTH || length > FRCNN_TRACK_TRAILS_MAX_LENGTH)
        return fail(FRCNN_E_ARG, "%s: length=%d not in [%d, %d]", who, length, FRCNN_TRACK_TRAILS_MIN_LENGTH, FRCNN_TRACK_TRAILS_MAX_LENGTH);
    return FRCNN_OK;
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
    if (int rc = idt_call_ok(who, capacity, rows, frames, tracked_stride)) return rc;
    if (int rc = trails_length_ok(who, length)) return rc;
    if (int rc = idt_expire_ok(who, expire, FRCNN_TRACK_TRAILS_MAX_EXPIRE)) return rc;
    if (int rc = ov_frame_ok(who, h, w)) return rc;
    k_trails_update<<<1, IDT_THREADS, 0, as_stream(stream)>>>(state, capacity, tracked, tracked_stride, rows, frames, n_frames, gate, length, expire,
                                                              h, w, lists);
    return check_launch(who);
}

extern "C" int frcnn_track_trails_draw_u8(uint8_t* frame, int h, int w, const int32_t* list, int length, int width, int rgb, void* stream) {
    const char* who = "track_trails_draw_u8";
    if (!frame || !list) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (int rc = ov_frame_ok(who, h, w)) return rc;
    if (int rc = trails_length_ok(who, length)) return rc;
    if (int rc = ov_width_ok(who, width, FRCNN_TRACK_TRAILS_MAX_WIDTH)) return rc;
    k_trails_draw<<<ov_grid(h, w), OV_THREADS, 0, as_stream(stream)>>>(frame, h, w, list, length, width, rgb ? 1 : 0);
    return check_launch(who);
}
