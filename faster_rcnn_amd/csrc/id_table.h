// What the kernels that follow the tracker's ids from frame to frame share (k_trails_update, k_count_update, k_zone_update; DESIGN §8 "The
// id-table walk"): ONE workgroup of 256 threads walks the frames of a call in order with its table in LDS.  A frame's phases are the same
// for every rule -- the live rows compacted in row order, each row's entry found by binary search, the new ids ranked and given the free
// places, later rows of a new id sent after its first row, the rows without a place counted, a thread per entry stepping through its rows
// -- and the functions here are those phases, on the kernel's own LDS arrays.  What a rule keeps per entry, its STEP and its events stay
// in its file.  Behind them: the two-copy compacted table of count and zone, and the refusals the update entries share.  gfx950 only.
#pragma once
#include "common.h"
#include "../../include/ext/frcnn_hip_redact.h"
#include "../../include/ext/frcnn_hip_track.h"

namespace frcnn {

constexpr int IDT_THREADS = 256, IDT_WAVES = IDT_THREADS / 64;
constexpr int IDT_CAP = FRCNN_TRACK_MAX, IDT_ROWS = FRCNN_REDACT_MAX_ROWS;
static_assert(IDT_CAP <= IDT_THREADS, "a thread per entry");

// The number of threads in front of this one, in thread order, whose ``flag`` is set, and ``total``, the workgroup's count.  Every thread
// of the workgroup calls it; ``s_cnt`` (a word per wave) is free again when it returns.
__device__ inline int wg_rank(bool flag, int* s_cnt, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(flag);
    if (lane == 0) s_cnt[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < IDT_WAVES; ++k) {
        const int c = s_cnt[k];
        before += k < wave ? c : 0;
        all += c;
    }
    __syncthreads();
    total = all;
    return before + __popcll(mask & ((1ull << lane) - 1ull));
}

// The sum of ``v`` over the threads in front of this one, in thread order, and ``total``, the workgroup's sum.  As wg_rank.
__device__ inline int wg_prefix(int v, int* s_cnt, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    if (lane == 63) s_cnt[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < IDT_WAVES; ++k) {
        const int c = s_cnt[k];
        before += k < wave ? c : 0;
        all += c;
    }
    __syncthreads();
    total = all;
    return before + inc - v;
}

// The place of a flagged thread's item behind the ``n`` items a compacted list has, in thread order; ``n`` grows by the workgroup's count.
__device__ inline int wg_append(bool flag, int* s_cnt, int& n) {
    int total;
    const int k = n + wg_rank(flag, s_cnt, total);
    n += total;
    return k;
}

// The head of a call -> the frames that are real; the lists of the others (``words`` each) are zeroed.
__device__ inline int idt_begin(const int32_t* gate, const int32_t* n_frames, int frames, int32_t* lists, int words) {
    const int nf = gate && *gate == 0 ? 0 : min(max(*n_frames, 0), frames);
    for (long long i = (long long)nf * words + threadIdx.x; i < (long long)frames * words; i += IDT_THREADS) lists[i] = 0;
    return nf;
}

struct IdRows {                                                             // frame f's tracked buffer: its rows, clamped to R, and their arrays
    int n;
    const int32_t *bbox, *cls, *ids;
};

__device__ inline IdRows idt_rows(const int32_t* tracked, long long stride, int f, int R) {
    const int32_t* buf = tracked + (long long)f * stride;
    return {min(max(buf[1], 0), R), buf + 4, buf + 4 + 4 * R, buf + 4 + 6 * R};
}

// LIVE: row r is one, carries an id and its box clipped to the frame is not empty -> ``rid`` and the clipped box.
__device__ inline bool idt_live(const IdRows& rows, int r, int h, int w, int& rid, int& xa, int& xb, int& ya, int& yb) {
    if (!(r < rows.n && (rid = rows.ids[r]) >= 1)) return false;
    const int x1 = rows.bbox[4 * r], y1 = rows.bbox[4 * r + 1], x2 = rows.bbox[4 * r + 2], y2 = rows.bbox[4 * r + 3];
    xa = max(min(x1, x2), 0), xb = min(max(x1, x2), w - 1), ya = max(min(y1, y2), 0), yb = min(max(y1, y2), h - 1);
    return xa <= xb && ya <= yb;
}

// class ``rc`` is one of the ``nc`` of the table and set in it
__device__ inline bool idt_class_set(const uint8_t* classes, int nc, int rc) { return rc >= 0 && rc < nc && classes[rc] != 0; }

// Compacted row k's entry-- the place of its id among the ``ne`` ascending ids id[order[0]], id[order[1]], ... (``order`` nullptr: id[0],
// id[1], ...), or -1 -- and for a row without one the first row of the frame that has its id.
__device__ inline void idt_lookup(int k, const int* s_rid, const int* id, const int* order, int ne, int* s_rent, int* s_rfirst) {
    const int rid = s_rid[k];
    int lo = 0, hi = ne, found = -1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1, e = order ? order[mid] : mid, v = id[e];
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

// A BIRTH: the first of the ``m`` compacted rows with an id that has no entry.  Ranked with wg_append, the births take the free places.
__device__ inline bool idt_birth(int k, int m, const int* s_rent, const int* s_rfirst) { return k < m && s_rent[k] < 0 && s_rfirst[k] == k; }

// Later rows of a new id follow its first row -> the rows left without an entry.  Every thread calls it, behind a barrier after the
// births; the caller's barrier follows.
__device__ inline int idt_follow(int m, int* s_rent, const int* s_rfirst, int* s_cnt) {
    int dropped = 0;
    for (int base = 0; base < m; base += IDT_THREADS) {
        const int k = base + threadIdx.x;
        bool lost = false;
        if (k < m) {
            int e = s_rent[k];
            if (e < 0 && s_rfirst[k] != k) s_rent[k] = e = s_rent[s_rfirst[k]];     // (a first row's word: nobody writes it here)
            lost = e < 0;
        }
        wg_append(lost, s_cnt, dropped);
    }
    return dropped;
}

// ---- the two-copy table of count and zone: ENTRY words an entry (word 0 its id), word j of entry t at T[j][t], compacted in ascending id
// order; a state is [n_entries, frames, dropped, events_dropped | HEAD - 4 totals | the entries].

// The call's table from ``state`` (``ne`` entries) and its totals.
template <int ENTRY, int HEAD>
__device__ inline void idt_load(const int32_t* state, int ne, int (*T)[IDT_CAP], int* s_tot) {
    const int tid = threadIdx.x;
    if (tid < HEAD - 4) s_tot[tid] = state[4 + tid];
    if (tid < IDT_CAP) {
        const bool live = tid < ne;
        const int32_t* e = state + HEAD + (size_t)(live ? tid : 0) * ENTRY;
#pragma unroll
        for (int j = 0; j < ENTRY; ++j) T[j][tid] = live ? e[j] : 0;
    }
}

// The survivors among T's ``nt`` entries (s_live) into the other copy ``U``, in id order -> how many.  Its barriers also publish what the
// threads wrote to LDS before it.
template <int ENTRY>
__device__ inline int idt_compact(int nt, const int* s_live, const int (*T)[IDT_CAP], int (*U)[IDT_CAP], int* s_cnt) {
    const int tid = threadIdx.x;
    const bool live = tid < nt && s_live[tid];
    if (live) {
        const int my = T[0][tid];
        int pos = 0;
        for (int e = 0; e < nt; ++e) pos += s_live[e] && T[0][e] < my;
#pragma unroll
        for (int j = 0; j < ENTRY; ++j) U[j][pos] = T[j][tid];
    }
    int ne;
    wg_rank(live, s_cnt, ne);
    return ne;
}

// The state at the end of the call: every word, by one thread each.
template <int ENTRY, int HEAD>
__device__ inline void idt_store(int32_t* state, int cap, int ne, int fr, int dropped, int evdrop, const int* s_tot, const int (*T)[IDT_CAP]) {
    const int words = HEAD + cap * ENTRY;
    for (int i = threadIdx.x; i < words; i += IDT_THREADS) {
        int v;
        if (i < 4) {
            v = i == 0 ? ne : i == 1 ? fr : i == 2 ? dropped : evdrop;
        } else if (i < HEAD) {
            v = s_tot[i - 4];
        } else {
            const int t = (i - HEAD) / ENTRY, j = (i - HEAD) - t * ENTRY;
            v = t < ne ? T[j][t] : 0;
        }
        state[i] = v;
    }
}

// ---- the refusals of the update entries, in the order every one of them keeps

inline int idt_call_ok(const char* who, int capacity, int rows, int frames, long long tracked_stride) {
    if (capacity < 1 || capacity > FRCNN_TRACK_MAX) return fail(FRCNN_E_ARG, "%s: capacity=%d not in [1, %d]", who, capacity, FRCNN_TRACK_MAX);
    if (rows < 1 || rows > FRCNN_REDACT_MAX_ROWS) return fail(FRCNN_E_ARG, "%s: rows=%d not in [1, %d]", who, rows, FRCNN_REDACT_MAX_ROWS);
    if (frames < 1 || frames > FRCNN_TRACK_MAX_FRAMES)
        return fail(FRCNN_E_ARG, "%s: frames=%d not in [1, %d]", who, frames, FRCNN_TRACK_MAX_FRAMES);
    if (frames > 1 && tracked_stride < 4 + 8LL * rows)
        return fail(FRCNN_E_ARG, "%s: tracked_stride=%lld under the %d words of a tracked buffer", who, tracked_stride, 4 + 8 * rows);
    return FRCNN_OK;
}

inline int idt_expire_ok(const char* who, int expire, int most) {
    if (expire < 0 || expire > most) return fail(FRCNN_E_ARG, "%s: expire=%d not in [0, %d]", who, expire, most);
    return FRCNN_OK;
}

}  // namespace frcnn
