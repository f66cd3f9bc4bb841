// Detections of consecutive frames joined into tracks (include/ext/frcnn_hip_track.h states the rule, DESIGN §8 "Tracking rule"): a greedy
// IoU match of the live slots against a frame's rows, in integers.  gfx950 (CDNA4) only.  ONE workgroup walks the frames of a pass in
// order -- frame i + 1 needs frame i's state -- with the state in LDS from the first frame to the last; the parallelism is inside a frame.
// A thread owns two consecutive rows (at most 512 of them) and keeps their clipped boxes in registers.  The slots take their rows one after
// another (a slot's choice removes a row from the next slot's): per slot every thread scores its rows, a shuffle reduction finds the wave's
// best, four LDS records (double-buffered: one barrier per slot) the workgroup's, and the thread that owns the winning row updates the
// slot.  Ageing with compaction, births and the held rows' places in the output are exclusive prefix sums over the workgroup, so ids and
// places do not depend on which thread runs when.  Every output word has one writer; no atomics.
// The host half is the whole family's (csrc/track_call.h): the one check of a call's arguments and the one walk over its frames, which the
// motion, interval and cut entries (csrc/track_motion.hip, track_interval.hip, track_cut.hip) go through as frcnn_track_update does.
#include "common.h"
#include "../../include/ext/frcnn_hip_redact.h"
#include "../../include/ext/frcnn_hip_track.h"
#include "../../include/ext/frcnn_hip_track_cut.h"
#include "../../include/ext/frcnn_hip_track_interval.h"
#include "../../include/ext/frcnn_hip_track_motion.h"
#include "../../include/ext/frcnn_hip_track_weak.h"
#include "track_call.h"

namespace frcnn {

constexpr int TR_THREADS = 256;
constexpr int TR_WAVES = TR_THREADS / 64;
static_assert(2 * TR_THREADS >= FRCNN_REDACT_MAX_ROWS, "a thread owns two rows");
static_assert(FRCNN_TRACK_MAX <= TR_THREADS, "a thread owns one slot");

struct Cand { long long inter, uni; int row; };                             // inter 0: none

// "a better than b", ties to the lower row; products of a 2^30 and a 2^31 value: int64
__device__ __forceinline__ bool better(const Cand& a, const Cand& b) {
    if (a.inter <= 0) return false;
    if (b.inter <= 0) return true;
    const long long l = a.inter * b.uni, r = b.inter * a.uni;
    return l != r ? l > r : a.row < b.row;
}

struct Box { int xa, xb, ya, yb; };

__device__ __forceinline__ Box clipped(int x1, int y1, int x2, int y2, int h, int w) {
    return Box{max(min(x1, x2), 0), min(max(x1, x2), w - 1), max(min(y1, y2), 0), min(max(y1, y2), h - 1)};
}

// exclusive prefix sum of ``v`` over the workgroup's threads, and the total; s_w: TR_WAVES ints
__device__ int block_scan(int v, int* s_w, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    __syncthreads();                                                        // (the readers of the last scan are done with s_w)
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int base = 0, sum = 0;
    for (int k = 0; k < TR_WAVES; ++k) {
        const int t = s_w[k];
        base += k < wave ? t : 0;
        sum += t;
    }
    *total = sum;
    return base + inc - v;
}

// The workgroup's best open row of class ``scls`` for the slot box ``sb`` (inter 0: none), the same value in every thread: each thread
// scores its two rows, a shuffle reduction finds the wave's best and the waves' records in LDS set ``buf`` (0 / 1, alternating from one
// call to the next: one barrier per call) the workgroup's.  The match stages of both rules go through here.
__device__ __forceinline__ Cand slot_best(const Box& sb, int scls, int thr, const bool (&open)[2], const int (&rcls)[2], const Box (&rb)[2],
                                          const long long (&rarea)[2], int buf, long long (*s_ri)[TR_WAVES], long long (*s_ru)[TR_WAVES],
                                          int (*s_rr)[TR_WAVES]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long sarea = (long long)(sb.xb - sb.xa + 1) * (sb.yb - sb.ya + 1);
    Cand best{0, 0, 0x7fffffff};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (!open[k] || rcls[k] != scls) continue;
        const int iw = min(sb.xb, rb[k].xb) - max(sb.xa, rb[k].xa) + 1, ih = min(sb.yb, rb[k].yb) - max(sb.ya, rb[k].ya) + 1;
        if (iw <= 0 || ih <= 0) continue;                                   // (an empty slot box never gets here)
        const long long inter = (long long)iw * ih, uni = rarea[k] + sarea - inter;
        if (inter * 100 < (long long)thr * uni) continue;
        const Cand c{inter, uni, 2 * tid + k};
        if (better(c, best)) best = c;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const Cand c{__shfl_xor(best.inter, off), __shfl_xor(best.uni, off), __shfl_xor(best.row, off)};
        if (better(c, best)) best = c;
    }
    if (lane == 0) { s_ri[buf][wave] = best.inter; s_ru[buf][wave] = best.uni; s_rr[buf][wave] = best.row; }
    __syncthreads();
    best = Cand{s_ri[buf][0], s_ru[buf][0], s_rr[buf][0]};
    for (int k = 1; k < TR_WAVES; ++k) {
        const Cand c{s_ri[buf][k], s_ru[buf][k], s_rr[buf][k]};
        if (better(c, best)) best = c;
    }
    return best;
}

// ``det`` and ``out`` are those of frame ``first`` of a call of ``total`` frames, and the launch walks ``frames`` of them: a frame whose index
// in the CALL is at or behind *n_frames is padding (frcnn_track_update walks a whole call, first = 0 and frames = total; the motion
// extension one frame per launch, with the block match in between).
// WEAK (include/ext/frcnn_hip_track_weak.h, DESIGN §8 "Weak rule"): a row whose score is not >= ``strong`` is weak; the match has a stage B
// in which the slots stage A left alone take weak rows, births are the strong rows' alone, and the live part of the output is the strong
// rows and the matched weak ones, moved up in row order by one more prefix sum.  Without WEAK ``strong`` is not read.
template <bool WEAK>
__global__ void __launch_bounds__(TR_THREADS) k_track_update(int32_t* state, int cap, const int32_t* det, long long det_stride, int first,
                                                               int frames, int total, const int32_t* n_frames, int max_rows,
                                                               const uint8_t* tracked, int num_classes, int thr, int hold, int grow, int h,
                                                               int w, float strong, int32_t* out, long long out_stride) {
    __shared__ int s_id[FRCNN_TRACK_MAX], s_cls[FRCNN_TRACK_MAX], s_prob[FRCNN_TRACK_MAX], s_age[FRCNN_TRACK_MAX], s_hit[FRCNN_TRACK_MAX];
    __shared__ int s_box[FRCNN_TRACK_MAX][4];
    __shared__ long long s_ri[2][TR_WAVES], s_ru[2][TR_WAVES];
    __shared__ int s_rr[2][TR_WAVES];
    __shared__ int s_w[TR_WAVES];
    const int tid = threadIdx.x;
    const int nf = min(max(*n_frames, 0), total) - first;                   // real frames from this launch's first one on
    const int R = max_rows + cap;
    int n_slots = min(max(state[0], 0), cap), issued = state[1], overflow = state[2], seen = state[3];
    if (tid < cap) {
        const bool live = tid < n_slots;
        s_id[tid] = live ? state[4 + tid] : 0;
        s_cls[tid] = live ? state[4 + cap + tid] : 0;
        for (int c = 0; c < 4; ++c) s_box[tid][c] = live ? state[4 + 2 * cap + 4 * tid + c] : 0;
        s_prob[tid] = live ? state[4 + 6 * cap + tid] : 0;
        s_age[tid] = live ? state[4 + 7 * cap + tid] : 0;
    }
    for (int f = 0; f < frames; ++f) {
        int32_t* o = out + (long long)f * out_stride;
        int32_t *o_box = o + 4, *o_cls = o + 4 + 4 * R, *o_prob = o + 4 + 5 * R, *o_id = o + 4 + 6 * R, *o_age = o + 4 + 7 * R;
        if (f >= nf) {                                                      // a short pass's padding: no frame at all
            if (tid == 0) { o[0] = 0; o[1] = 0; o[2] = issued + 1; o[3] = overflow; }
            for (int r = tid; r < R; r += TR_THREADS) {
                for (int c = 0; c < 4; ++c) o_box[4 * r + c] = -1;
                o_cls[r] = -1; o_prob[r] = 0; o_id[r] = 0; o_age[r] = 0;
            }
            continue;
        }
        const int32_t* d = det + (long long)f * det_stride;
        const int n = min(max(d[0], 0), max_rows);
        const int32_t *d_box = d + 4, *d_cls = d + 4 + 4 * max_rows, *d_prob = d + 4 + 5 * max_rows;
        // ---- this thread's rows 2 tid and 2 tid + 1
        int raw[2][4], rcls[2], rprob[2], rid[2];
        Box rb[2];
        long long rarea[2];
        bool open[2];                                                       // eligible and not yet matched (WEAK: and strong)
        bool wopen[2] = {false, false}, kept_row[2] = {false, false};       // WEAK: the same of the weak rows; a row of the live part
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int r = 2 * tid + k;
            open[k] = false; rid[k] = 0; rcls[k] = -1; rprob[k] = 0; rarea[k] = 0;
            rb[k] = Box{0, -1, 0, -1};
            for (int c = 0; c < 4; ++c) raw[k][c] = -1;
            if (r < n) {
                for (int c = 0; c < 4; ++c) raw[k][c] = d_box[4 * r + c];
                rcls[k] = d_cls[r];
                rprob[k] = d_prob[r];
                rb[k] = clipped(raw[k][0], raw[k][1], raw[k][2], raw[k][3], h, w);
                const bool some = rb[k].xa <= rb[k].xb && rb[k].ya <= rb[k].yb;
                open[k] = some && rcls[k] >= 0 && rcls[k] < num_classes && tracked[rcls[k]] != 0;
                rarea[k] = some ? (long long)(rb[k].xb - rb[k].xa + 1) * (rb[k].yb - rb[k].ya + 1) : 0;
                if constexpr (WEAK) {
                    kept_row[k] = __int_as_float(rprob[k]) >= strong;       // (false for a NaN score)
                    wopen[k] = open[k] && !kept_row[k];
                    open[k] = open[k] && kept_row[k];
                }
            }
        }
        if (tid < cap) s_hit[tid] = 0;
        __syncthreads();
        // ---- 1 match: the slots in id order, each against the rows still open
        if (n > 0) {
            for (int s = 0; s < n_slots; ++s) {
                const Box sb = clipped(s_box[s][0], s_box[s][1], s_box[s][2], s_box[s][3], h, w);
                const Cand best = slot_best(sb, s_cls[s], thr, open, rcls, rb, rarea, s & 1, s_ri, s_ru, s_rr);   // (two sets of records)
                if (best.inter <= 0) continue;                              // (the whole workgroup)
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    if (2 * tid + k != best.row) continue;                  // the row's owner moves the slot onto it
                    open[k] = false;
                    rid[k] = s_id[s];
                    for (int c = 0; c < 4; ++c) s_box[s][c] = raw[k][c];
                    s_prob[s] = rprob[k];
                    s_hit[s] = 1;
                }
            }
            if constexpr (WEAK) {
                // ---- 1B: the slots stage A left alone, in id order, each against the weak rows still open; a round is a slot that goes
                // again, and the records' sets alternate by rounds (behind the barrier, so stage A's last reads are done)
                if (__syncthreads_or(wopen[0] || wopen[1])) {
                    int round = 0;
                    for (int s = 0; s < n_slots; ++s) {
                        if (s_hit[s]) continue;                             // (the whole workgroup: written behind slot s's barrier alone)
                        const Box sb = clipped(s_box[s][0], s_box[s][1], s_box[s][2], s_box[s][3], h, w);
                        const Cand best = slot_best(sb, s_cls[s], thr, wopen, rcls, rb, rarea, round++ & 1, s_ri, s_ru, s_rr);
                        if (best.inter <= 0) continue;
#pragma unroll
                        for (int k = 0; k < 2; ++k) {
                            if (2 * tid + k != best.row) continue;
                            wopen[k] = false; kept_row[k] = true;
                            rid[k] = s_id[s];
                            for (int c = 0; c < 4; ++c) s_box[s][c] = raw[k][c];
                            s_prob[s] = rprob[k];
                            s_hit[s] = 1;
                        }
                    }
                }
            }
        }
        __syncthreads();
        // ---- 2 age: thread i holds slot i; the slots that stay move up, order kept
        int keep = 0, a_id = 0, a_cls = 0, a_prob = 0, a_age = 0, a_box[4] = {0, 0, 0, 0};
        if (tid < n_slots) {
            a_id = s_id[tid]; a_cls = s_cls[tid]; a_prob = s_prob[tid];
            for (int c = 0; c < 4; ++c) a_box[c] = s_box[tid][c];
            a_age = s_hit[tid] ? 0 : s_age[tid] + 1;
            keep = a_age <= hold;
        }
        int kept = 0;
        const int pos = block_scan(keep, s_w, &kept);                      // (its barriers: every slot is read before one is written)
        if (keep) {
            s_id[pos] = a_id; s_cls[pos] = a_cls; s_prob[pos] = a_prob; s_age[pos] = a_age;
            for (int c = 0; c < 4; ++c) s_box[pos][c] = a_box[c];
        }
        n_slots = kept;
        // ---- 3 birth: the open rows in row order take the free slots, the rest overflow
        int wanted = 0;
        int rank = block_scan((int)open[0] + (int)open[1], s_w, &wanted);
        const int room = cap - n_slots;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (!open[k]) continue;
            if (rank < room) {
                const int at = n_slots + rank;
                rid[k] = issued + 1 + rank;
                s_id[at] = rid[k]; s_cls[at] = rcls[k]; s_prob[at] = rprob[k]; s_age[at] = 0;
                for (int c = 0; c < 4; ++c) s_box[at][c] = raw[k][c];
            }
            ++rank;
        }
        const int born = min(wanted, room);
        issued += born; overflow += wanted - born; n_slots += born; seen += 1;
        __syncthreads();
        // ---- 4 output: the frame's rows with their ids, the held slots behind them, dead rows behind those
        int live = n;                                                       // rows of the live part
        if constexpr (WEAK) {                                               // the strong rows and the matched weak ones move up, order kept
            int at = block_scan((int)kept_row[0] + (int)kept_row[1], s_w, &live);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (!kept_row[k]) continue;                                 // (never set for a row at or behind n)
                for (int c = 0; c < 4; ++c) o_box[4 * at + c] = raw[k][c];
                o_cls[at] = rcls[k]; o_prob[at] = rprob[k]; o_id[at] = rid[k]; o_age[at] = 0;
                ++at;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int r = 2 * tid + k;
                if (r >= n) continue;
                for (int c = 0; c < 4; ++c) o_box[4 * r + c] = raw[k][c];
                o_cls[r] = rcls[k]; o_prob[r] = rprob[k]; o_id[r] = rid[k]; o_age[r] = 0;
            }
        }
        const int age = tid < n_slots ? s_age[tid] : 0;
        int held = 0;
        const int hp = block_scan(age >= 1, s_w, &held);
        if (age >= 1) {
            const int r = live + hp, g = grow * age;
            const Box sb = clipped(s_box[tid][0], s_box[tid][1], s_box[tid][2], s_box[tid][3], h, w);
            o_box[4 * r] = sb.xa - g; o_box[4 * r + 1] = sb.ya - g; o_box[4 * r + 2] = sb.xb + g; o_box[4 * r + 3] = sb.yb + g;
            o_cls[r] = s_cls[tid]; o_prob[r] = s_prob[tid]; o_id[r] = s_id[tid]; o_age[r] = age;
        }
        for (int r = live + held + tid; r < R; r += TR_THREADS) {
            for (int c = 0; c < 4; ++c) o_box[4 * r + c] = -1;
            o_cls[r] = -1; o_prob[r] = 0; o_id[r] = 0; o_age[r] = 0;
        }
        if (tid == 0) { o[0] = live + held; o[1] = live; o[2] = issued + 1; o[3] = overflow; }
    }
    if (nf <= 0) return;                                                    // no frame: the state keeps every word
    __syncthreads();
    if (tid == 0) { state[0] = n_slots; state[1] = issued; state[2] = overflow; state[3] = seen; }
    if (tid < cap) {
        const bool live = tid < n_slots;
        state[4 + tid] = live ? s_id[tid] : 0;
        state[4 + cap + tid] = live ? s_cls[tid] : 0;
        for (int c = 0; c < 4; ++c) state[4 + 2 * cap + 4 * tid + c] = live ? s_box[tid][c] : 0;
        state[4 + 6 * cap + tid] = live ? s_prob[tid] : 0;
        state[4 + 7 * cap + tid] = live ? s_age[tid] : 0;
    }
}

int track_call_check(const char* who, const TrackCall& c) {
    if (c.interval < FRCNN_TRACK_INTERVAL_MIN || c.interval > FRCNN_TRACK_INTERVAL_MAX)
        return fail(FRCNN_E_ARG, "%s: interval=%d not in [%d, %d]", who, c.interval, FRCNN_TRACK_INTERVAL_MIN, FRCNN_TRACK_INTERVAL_MAX);
    if (!c.state || !c.det_packed || !c.n_frames || !c.tracked || !c.out) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (c.capacity < 1 || c.capacity > FRCNN_TRACK_MAX)
        return fail(FRCNN_E_ARG, "%s: capacity=%d not in [1, %d]", who, c.capacity, FRCNN_TRACK_MAX);
    if (c.frames < 1 || c.frames > FRCNN_TRACK_MAX_FRAMES)
        return fail(FRCNN_E_ARG, "%s: frames=%d not in [1, %d]", who, c.frames, FRCNN_TRACK_MAX_FRAMES);
    if (c.max_rows <= 0 || c.max_rows > FRCNN_REDACT_MAX_ROWS - c.capacity)
        return fail(FRCNN_E_ARG, "%s: max_rows=%d: max_rows + capacity (%d) not in [2, %d]", who, c.max_rows, c.capacity, FRCNN_REDACT_MAX_ROWS);
    // the packed buffers are one per KEY frame: their distance is read only when the call has more than one of them
    const long long det_words = 4 + 7LL * c.max_rows, out_words = 4 + 8LL * (c.max_rows + c.capacity);
    if ((c.frames + c.interval - 1) / c.interval > 1 && c.det_stride < det_words)
        return fail(FRCNN_E_ARG, "%s: det_stride=%lld words, a packed buffer of %d rows has %lld", who, c.det_stride, c.max_rows, det_words);
    if (c.frames > 1 && c.out_stride < out_words)
        return fail(FRCNN_E_ARG, "%s: out_stride=%lld words, a tracked buffer has %lld", who, c.out_stride, out_words);
    if (c.num_classes <= 0 || c.num_classes > 256) return fail(FRCNN_E_ARG, "%s: num_classes=%d not in [1, 256]", who, c.num_classes);
    if (c.thr < 1 || c.thr > 100) return fail(FRCNN_E_ARG, "%s: thr=%d not in [1, 100] (percent)", who, c.thr);
    if (c.hold < 0 || c.hold > FRCNN_TRACK_MAX_HOLD) return fail(FRCNN_E_ARG, "%s: hold=%d not in [0, %d]", who, c.hold, FRCNN_TRACK_MAX_HOLD);
    if (c.grow < 0 || c.grow > FRCNN_TRACK_MAX_GROW) return fail(FRCNN_E_ARG, "%s: grow=%d not in [0, %d]", who, c.grow, FRCNN_TRACK_MAX_GROW);
    if (c.h < 1 || c.h > FRCNN_REDACT_MAX_SIDE || c.w < 1 || c.w > FRCNN_REDACT_MAX_SIDE)
        return fail(FRCNN_E_ARG, "%s: frame %dx%d out of range (sides 1..%d)", who, c.h, c.w, FRCNN_REDACT_MAX_SIDE);
    if (c.form != TRACK_PLAIN) {
        if (!c.motion_state || !c.frames_u8) return fail(FRCNN_E_ARG, "%s: null pointer", who);
        if (reinterpret_cast<uintptr_t>(c.motion_state) & 3) return fail(FRCNN_E_ARG, "%s: motion_state is not 4-byte aligned", who);
        if (c.radius < FRCNN_TRACK_MOTION_MIN_RADIUS || c.radius > FRCNN_TRACK_MOTION_MAX_RADIUS)
            return fail(FRCNN_E_ARG, "%s: radius=%d not in [%d, %d]", who, c.radius, FRCNN_TRACK_MOTION_MIN_RADIUS, FRCNN_TRACK_MOTION_MAX_RADIUS);
        const long long frame_bytes = 3LL * c.h * c.w;
        if (c.frames > 1 && c.frame_stride < frame_bytes)
            return fail(FRCNN_E_ARG, "%s: frame_stride=%lld bytes, a %dx%d frame has %lld", who, c.frame_stride, c.h, c.w, frame_bytes);
    }
    if (c.form == TRACK_CUT) {
        if (c.pct < FRCNN_TRACK_CUT_MIN_PCT || c.pct > FRCNN_TRACK_CUT_MAX_PCT)
            return fail(FRCNN_E_ARG, "%s: pct=%d not in [%d, %d]", who, c.pct, FRCNN_TRACK_CUT_MIN_PCT, FRCNN_TRACK_CUT_MAX_PCT);
        if (!c.workspace || !c.cuts) return fail(FRCNN_E_ARG, "%s: null pointer", who);
        if (reinterpret_cast<uintptr_t>(c.workspace) & 3) return fail(FRCNN_E_ARG, "%s: workspace is not 4-byte aligned", who);
    }
    if (c.strong && *c.strong != *c.strong) return fail(FRCNN_E_ARG, "%s: strong is NaN", who);
    return FRCNN_OK;
}

void track_launch(const TrackCall& c, int first, int frames, const int32_t* det, int32_t* out, hipStream_t stream) {
    if (c.strong)
        k_track_update<true><<<1, TR_THREADS, 0, stream>>>(c.state, c.capacity, det, c.det_stride, first, frames, c.frames, c.n_frames, c.max_rows,
                                                           c.tracked, c.num_classes, c.thr, c.hold, c.grow, c.h, c.w, *c.strong, out, c.out_stride);
    else
        k_track_update<false><<<1, TR_THREADS, 0, stream>>>(c.state, c.capacity, det, c.det_stride, first, frames, c.frames, c.n_frames, c.max_rows,
                                                            c.tracked, c.num_classes, c.thr, c.hold, c.grow, c.h, c.w, 0.0f, out, c.out_stride);
}

int track_walk(const char* who, const TrackCall& c, hipStream_t stream) {
    if (c.form == TRACK_PLAIN) {
        track_launch(c, 0, c.frames, c.det_packed, c.out, stream);
        return check_launch(who);
    }
    for (int f = 0; f < c.frames; ++f) {                                    // (the search of frame f + 1 needs the boxes after frame f)
        if (c.form == TRACK_CUT) cut_apply_launch(c, f, stream);
        motion_search_launch(c, f, stream);
        int32_t* o = c.out + (long long)f * c.out_stride;
        if (f % c.interval == 0)
            track_launch(c, f, 1, c.det_packed + (long long)(f / c.interval) * c.det_stride, o, stream);
        else
            interval_between_launch(c, f, o, stream);
    }
    motion_keep_launch(c, stream);
    return check_launch(who);
}

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_track_version(void) { return FRCNN_TRACK_VERSION; }

extern "C" size_t frcnn_track_state_bytes(int capacity) {
    if (capacity < 1 || capacity > FRCNN_TRACK_MAX) return 0;
    return 4 * (4 + 8 * (size_t)capacity);
}

extern "C" int frcnn_track_update(int32_t* state, int capacity, const int32_t* det_packed, long long det_stride, int frames,
                                  const int32_t* n_frames, int max_rows, const uint8_t* tracked, int num_classes, int thr, int hold, int grow,
                                  int h, int w, int32_t* out, long long out_stride, void* stream) {
    TrackCall c{};
    c.form = TRACK_PLAIN; c.state = state; c.capacity = capacity; c.det_packed = det_packed; c.det_stride = det_stride; c.frames = frames;
    c.n_frames = n_frames; c.max_rows = max_rows; c.tracked = tracked; c.num_classes = num_classes; c.thr = thr; c.hold = hold; c.grow = grow;
    c.interval = 1; c.h = h; c.w = w; c.out = out; c.out_stride = out_stride;
    const int bad = track_call_check("track_update", c);
    return bad ? bad : track_walk("track_update", c, as_stream(stream));
}

extern "C" int frcnn_track_weak_version(void) { return FRCNN_TRACK_WEAK_VERSION; }

extern "C" int frcnn_track_update_weak(int32_t* state, int capacity, const int32_t* det_packed, long long det_stride, int frames,
                                       const int32_t* n_frames, int max_rows, const uint8_t* tracked, int num_classes, int thr, int hold,
                                       int grow, int h, int w, float strong, int32_t* out, long long out_stride, void* stream) {
    TrackCall c{};
    c.form = TRACK_PLAIN; c.state = state; c.capacity = capacity; c.det_packed = det_packed; c.det_stride = det_stride; c.frames = frames;
    c.n_frames = n_frames; c.max_rows = max_rows; c.tracked = tracked; c.num_classes = num_classes; c.thr = thr; c.hold = hold; c.grow = grow;
    c.interval = 1; c.h = h; c.w = w; c.strong = &strong; c.out = out; c.out_stride = out_stride;
    const int bad = track_call_check("track_update_weak", c);
    return bad ? bad : track_walk("track_update_weak", c, as_stream(stream));
}
