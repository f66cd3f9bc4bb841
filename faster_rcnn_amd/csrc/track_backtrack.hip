// Tracks hidden on the frames between two detections, from both sides (include/ext/frcnn_hip_track_backtrack.h states the rule, DESIGN §8
// "Back-track rule"): the look-back's window over the tracked buffers of the interval rule, and from every tracked live row of a KEY frame
// a block match BACKWARDS through it -- a new track over the whole look-back, a continued one through the between frames in front of it.
// gfx950 (CDNA4) only.  Five launches per call, all guarded by device words (*n_frames, the window's count), so a captured call replays:
//   join, emit, close   csrc/track_lookback.hip's kernels, launched through csrc/track_lookback.h;
//   k_bt_chain   grid (capacity, frames); a between frame's workgroups return at once, a key frame has one workgroup per SOURCE.  Its waves
//                first take one frame each -- wave 0 the key frame itself, wave d the frame d in front -- and a wave finds a key frame's
//                sources by a flag prefix over the live rows (a ballot a 64 rows): wave 0 leaves the workgroup's source row, whether it is
//                a birth, and its rank among the births; the others the source and birth counts of the call's key frames in between.  The
//                workgroup then walks its steps itself, each a search of csrc/track_motion_search.h, and writes one row a step.  A row's
//                place is the frame's n_rows as it was + the births of the call's key frames in between + the corrections of the first
//                key frame behind the frame when the frame lies in that one's between-run + the source's rank (among all sources inside
//                its own between-run, among the births beyond it): nothing is handed from one workgroup to another;
//   k_bt_counts  one workgroup: per frame of the sequence the rows that reach it, n_rows moved behind them, the dropped rows summed into
//                back_overflow.
// One writer per word; no atomics.  The chain writes rows at and behind a frame's n_rows only and reads rows in front of n_live only.
#include "track_lookback.h"
#include "../../include/ext/frcnn_hip_track_backtrack.h"
#include "../../include/ext/frcnn_hip_track_interval.h"
#include "track_motion_search.h"

namespace frcnn {

constexpr int BT_MAX_L = FRCNN_TRACK_LOOKBACK_MAX;
static_assert(BT_MAX_L <= TM_WAVES, "a wave of the chain's workgroup takes one frame of the look-back");
static_assert(2 * FRCNN_TRACK_MAX_FRAMES <= TM_THREADS, "a thread of k_bt_counts takes one frame of the sequence");

// is frame ``s`` of the sequence a key frame: the window's frames and the call's both start on one
__device__ __forceinline__ bool bt_is_key(int c, int K, int s) { return (s < c ? s : s - c) % K == 0; }

// ONE WAVE: the sources of key frame ``t`` >= 1 of the sequence -- live rows with id >= 1, the first ``cap`` in row order -- by a flag prefix
// over the live rows.  -> in every lane: ``ns`` sources, ``nb`` of them births; with ``want`` >= 0 and a source of that rank: its ``row``
// (else -1), whether it is a ``birth`` and its rank ``brank`` among the births.
__device__ __forceinline__ void bt_scan(uint8_t* window, const LbGeom& g, int c, int half, int t, int lane, int want, int& ns, int& nb, int& row,
                                        int& birth, int& brank) {
    const int32_t* bt = reinterpret_cast<const int32_t*>(lb_cell(window, g, c, half, t));
    const int32_t* bp = reinterpret_cast<const int32_t*>(lb_cell(window, g, c, half, t - 1));
    const int live = clampi(bt[1], 0, g.R2), first = bp[2];
    const unsigned long long below = (1ull << lane) - 1;
    ns = nb = 0, row = -1, birth = brank = 0;
    for (int base = 0; base < live && ns < g.cap; base += 64) {            // (wave-uniform: the ballots below see all 64 lanes)
        const int r = base + lane;
        const int id = r < live ? bt[4 + 6 * g.R2 + r] : 0;
        const unsigned long long m_src = __ballot(r < live && id >= 1);
        const bool take = r < live && id >= 1 && ns + __popcll(m_src & below) < g.cap;
        const unsigned long long m_take = __ballot(take), m_birth = __ballot(take && id >= first);
        const unsigned long long m_hit = __ballot(take && ns + __popcll(m_src & below) == want);
        if (m_hit) {
            const int l = __ffsll((long long)m_hit) - 1;
            row = base + l;
            birth = (int)((m_birth >> l) & 1);
            brank = nb + __popcll(m_birth & ((1ull << l) - 1));
        }
        ns += __popcll(m_take);
        nb += __popcll(m_birth);
    }
}

// grid (capacity, frames): source blockIdx.x of the call's KEY frame blockIdx.y, chained back over at most ``L`` frames
__global__ void __launch_bounds__(TM_THREADS) k_bt_chain(uint8_t* window, LbGeom g, const int32_t* n_frames, int L, int radius, int grow, int K) {
    __shared__ TmShared sh;
    __shared__ int s_ns[BT_MAX_L], s_nb[BT_MAX_L];                          // [d]: key frame t - d of the call; [0] is the source's own
    __shared__ int s_pick[3], s_mv[2];
    const int j = blockIdx.x, f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (f % K != 0) return;                                                 // a between frame has no sources
    if (f >= clampi(*n_frames, 0, g.frames)) return;
    const int32_t* hd = reinterpret_cast<const int32_t*>(window);
    const int c = clampi(hd[0], 0, g.frames), half = hd[1] & 1, t = c + f, R2 = g.R2;
    if (t == 0) return;                                                     // no frame in front of it: nothing to fill into
    if (wave < BT_MAX_L) {                                                  // wave d: frame t - d
        int ns = 0, nb = 0, row = -1, birth = 0, brank = 0;
        if (wave < L && f - wave >= 0 && (f - wave) % K == 0 && t - wave >= 1)
            bt_scan(window, g, c, half, t - wave, lane, wave == 0 ? j : -1, ns, nb, row, birth, brank);
        if (lane == 0) {
            s_ns[wave] = ns, s_nb[wave] = nb;
            if (wave == 0) s_pick[0] = row, s_pick[1] = birth, s_pick[2] = brank;
        }
    }
    __syncthreads();
    const int row = s_pick[0], birth = s_pick[1], brank = s_pick[2];
    if (j >= s_ns[0] || row < 0) return;                                    // (the whole workgroup)
    const int32_t* bt = reinterpret_cast<const int32_t*>(lb_cell(window, g, c, half, t));
    int x1 = bt[4 + 4 * row], y1 = bt[4 + 4 * row + 1], x2 = bt[4 + 4 * row + 2], y2 = bt[4 + 4 * row + 3];
    const int cls = bt[4 + 4 * R2 + row], prob = bt[4 + 5 * R2 + row], id = bt[4 + 6 * R2 + row];
    int between = 0;              // births of the call's key frames between g and t: their rows lie in front
    int near_corr = 0;            // corrections of the first key frame behind g: in front too while g lies in that one's between-run
    bool run = true;              // g lies in t's own between-run: no key frame at or behind g so far
    for (int k = 1; k <= L; ++k) {
        const int gi = t - k;
        if (gi < 0) break;
        if (k >= 2 && bt_is_key(c, K, gi + 1)) {                            // (a window frame has no sources of this call)
            between += gi + 1 >= c ? s_nb[k - 1] : 0;
            near_corr = gi + 1 >= c ? s_ns[k - 1] - s_nb[k - 1] : 0;
        }
        const bool gkey = bt_is_key(c, K, gi);
        if (gkey) {
            run = false;
            if (!birth) break;                                              // a correction stops in front of the previous key frame
        }
        uint8_t* cell = lb_cell(window, g, c, half, gi);
        int dx = 0, dy = 0;
        const bool took = radius > 0 && tm_search(lb_cell(window, g, c, half, gi + 1) + g.tracked_bytes, cell + g.tracked_bytes, x1, y1, x2, y2,
                                                  radius, g.h, g.w, sh, dx, dy);
        if (tid == 0) {                                                     // (wave 0 holds the result)
            s_mv[0] = took ? dx : 0;
            s_mv[1] = took ? dy : 0;
        }
        __syncthreads();
        x1 += s_mv[0], x2 += s_mv[0], y1 += s_mv[1], y2 += s_mv[1];
        int32_t* bg = reinterpret_cast<int32_t*>(cell);
        const int place = clampi(bg[0], 0, R2) + between + (!run && !gkey ? near_corr : 0) + (run ? j : brank);
        if (place < R2 && tid < 8) {
            const int xa = max(min(x1, x2), 0), xb = min(max(x1, x2), g.w - 1), ya = max(min(y1, y2), 0), yb = min(max(y1, y2), g.h - 1);
            const bool none = xa > xb || ya > yb;
            const int e = grow * k;
            if (tid < 4) bg[4 + 4 * place + tid] = none ? -1 : tid == 0 ? xa - e : tid == 1 ? ya - e : tid == 2 ? xb + e : yb + e;
            else bg[4 + tid * R2 + place] = tid == 4 ? cls : tid == 5 ? prob : tid == 6 ? id : -k;
        }
        __syncthreads();                                                    // s_mv and sh are written again
    }
}

// one workgroup: n_rows of every frame of the sequence behind its new rows; what did not fit is counted
__global__ void __launch_bounds__(TM_THREADS) k_bt_counts(uint8_t* window, LbGeom g, const int32_t* n_frames, int L, int K) {
    __shared__ int s_ns[FRCNN_TRACK_MAX_FRAMES], s_nb[FRCNN_TRACK_MAX_FRAMES], s_drop[2 * FRCNN_TRACK_MAX_FRAMES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nf = clampi(*n_frames, 0, g.frames);
    if (nf <= 0) return;
    int32_t* hd = reinterpret_cast<int32_t*>(window);
    const int c = clampi(hd[0], 0, g.frames), half = hd[1] & 1, total = c + nf;
    for (int f = wave; f < nf; f += TM_WAVES) {
        int ns = 0, nb = 0, row, birth, brank;
        if (f % K == 0 && c + f >= 1) bt_scan(window, g, c, half, c + f, lane, -1, ns, nb, row, birth, brank);
        if (lane == 0) s_ns[f] = ns, s_nb[f] = nb;
    }
    __syncthreads();
    if (tid < 2 * FRCNN_TRACK_MAX_FRAMES) {
        int drop = 0;
        if (tid < total) {
            int added = 0;
            bool nearest = !bt_is_key(c, K, tid);                           // the next key frame's corrections reach a between frame
            for (int t = tid + 1; t <= min(tid + L, total - 1); ++t) {
                if (!bt_is_key(c, K, t)) continue;
                if (t >= c) added += s_nb[t - c] + (nearest ? s_ns[t - c] - s_nb[t - c] : 0);
                nearest = false;
            }
            int32_t* b = reinterpret_cast<int32_t*>(lb_cell(window, g, c, half, tid));
            const int rows = clampi(b[0], 0, g.R2) + added;
            drop = max(rows - g.R2, 0);
            if (added) b[0] = rows - drop;
        }
        s_drop[tid] = drop;
    }
    __syncthreads();
    if (tid == 0) {
        int sum = 0;
        for (int s = 0; s < total; ++s) sum += s_drop[s];
        if (sum) hd[2] += sum;
    }
}

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_track_backtrack_version(void) { return FRCNN_TRACK_BACKTRACK_VERSION; }

extern "C" int frcnn_track_backtrack(uint8_t* window, const uint8_t* frames_u8, long long frame_stride, const int32_t* tracked,
                                     long long tracked_stride, int frames, const int32_t* n_frames, int max_rows, int capacity, int back,
                                     int lookback, int radius, int grow, int interval, int h, int w, uint8_t* out_frames,
                                     long long out_frame_stride, int32_t* out_tracked, long long out_tracked_stride, int32_t* out_count,
                                     void* stream) {
    const char* who = "track_backtrack";
    LbGeom g;
    const int bad = lookback_check(who, window, frames_u8, frame_stride, tracked, tracked_stride, frames, n_frames, max_rows, capacity, back, lookback,
                                   radius, grow, h, w, out_frames, out_frame_stride, out_tracked, out_tracked_stride, out_count, g);
    if (bad != FRCNN_OK) return bad;
    if (interval < FRCNN_TRACK_INTERVAL_MIN || interval > FRCNN_TRACK_INTERVAL_MAX)
        return fail(FRCNN_E_ARG, "%s: interval=%d not in [%d, %d]", who, interval, FRCNN_TRACK_INTERVAL_MIN, FRCNN_TRACK_INTERVAL_MAX);
    hipStream_t st = as_stream(stream);
    lookback_join_launch(window, g, frames_u8, frame_stride, tracked, tracked_stride, n_frames, st);
    k_bt_chain<<<dim3(capacity, frames), TM_THREADS, 0, st>>>(window, g, n_frames, lookback, radius, grow, interval);
    k_bt_counts<<<1, TM_THREADS, 0, st>>>(window, g, n_frames, lookback, interval);
    lookback_emit_launch(window, g, out_frames, out_frame_stride, out_tracked, out_tracked_stride, out_count, st);
    lookback_close_launch(window, g, n_frames, st);
    return check_launch(who);
}
