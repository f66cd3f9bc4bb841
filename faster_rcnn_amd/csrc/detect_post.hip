// Detection post-process with soft-NMS and box voting (include/ext/frcnn_hip_detect_post.h states the rule), gfx950.
//
// One workgroup per image, like k_detections (detect.hip), whose phases 1 and 2 -- arg-max, threshold, f64 decode, ranking -- are
// restated here expression for expression.  Behind them the ranked rows are grouped by class (classes in emission order, ranked order
// inside a class) and whole classes are handed to waves: a wave keeps its class's scores, exponents and boxes in registers, U = 1, 2
// or 4 consecutive rows per lane, finds each pick with a DPP maximum over an order-preserving 64-bit key plus one ballot (lowest
// lane = lowest rank among equals) and decays its rows; no workgroup barrier stands inside that loop.  A class of more than
// DP_WG_ROWS rows is worked on by the whole workgroup instead, a barrier per pick (dp_pick_class_wg).  Voting: one thread per
// emitted row walks its class's rows in ranked order.
// Compiled with -ffp-contract=off: the linear mode and the voting sums are exact IEEE sequences.
#include "common.h"
#include "../../include/ext/frcnn_hip_detect_post.h"
#include <math.h>
#include <stdlib.h>

namespace frcnn {

typedef unsigned long long u64;
constexpr int DP_MAX = 512;
constexpr int DP_WAVES = DP_MAX / 64;
constexpr int DP_MAX_CLASSES = 128;

__device__ __forceinline__ double dp_iou(const double4 a, const double4 b) {          // det_suppresses' expression (detect.hip)
    const double area_a = (a.z - a.x + 1.0) * (a.w - a.y + 1.0);
    const double area_b = (b.z - b.x + 1.0) * (b.w - b.y + 1.0);
    const double w = fmax(0.0, fmin(a.z, b.z) - fmax(a.x, b.x) + 1.0);
    const double h = fmax(0.0, fmin(a.w, b.w) - fmax(a.y, b.y) + 1.0);
    const double inter = w * h;
    return inter / (area_a + area_b - inter);
}

// a 64-bit key that orders like the double (-0.0 counted as +0.0); 0 is below every key of a number
__device__ __forceinline__ u64 dp_key(double s) {
    const u64 b = (u64)__double_as_longlong(s + 0.0);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ u64 dp_max_step(u64 v) {
    // lanes the control leaves without a source, and rows outside ROW_MASK, read 0: the identity of the maximum
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, ROW_MASK, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, ROW_MASK, 0xf, false);
    const u64 o = ((u64)hi << 32) | lo;
    return o > v ? o : v;
}

// maximum over the 64 lanes (all active), uniform
__device__ __forceinline__ u64 dp_wave_max(u64 v) {
    v = dp_max_step<0x111, 0xf>(v);          // row_shr:1
    v = dp_max_step<0x112, 0xf>(v);          // row_shr:2
    v = dp_max_step<0x114, 0xf>(v);          // row_shr:4
    v = dp_max_step<0x118, 0xf>(v);          // row_shr:8   -> lane 15 of every row holds its row's maximum
    v = dp_max_step<0x142, 0xa>(v);          // row_bcast:15 into rows 1 and 3
    v = dp_max_step<0x143, 0xc>(v);          // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave's
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
    return ((u64)hi << 32) | lo;
}

// One class (grouped rows start .. start + n - 1) by one wave: lane l holds rows l * U + u.  Writes the pick list of the class.
template <int U>
__device__ __forceinline__ void dp_pick_class(const double4* g_box, const float* g_prob, int start, int n, int mode, double nt,
                                              double sigma, double min_score, int* s_pick, float* s_pprob) {
    const int lane = threadIdx.x & 63;
    double4 b[U];
    double s[U], s0[U], E[U];
    unsigned alive = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int k = lane * U + u;
        const bool in = k < n;
        b[u] = in ? g_box[start + k] : make_double4(0, 0, 0, 0);
        s0[u] = in ? (double)g_prob[start + k] : 0.0;
        s[u] = s0[u];
        E[u] = 0.0;
        alive |= in ? 1u << u : 0u;
    }
    for (int picked = 0; picked < n; ++picked) {
        u64 bk = 0; int bu = 0; double bs = 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u64 key = ((alive >> u) & 1) ? dp_key(s[u]) : 0ull;
            if (key > bk) { bk = key; bu = u; bs = s[u]; }          // strict: the lower row among a lane's equals
        }
        const u64 m = dp_wave_max(bk);
        if (m == 0) break;                                          // no row left
        const u64 who = __ballot(bk == m);
        const int L = __builtin_ctzll(who) & 63;                    // lowest lane = lowest rank among equals
        const int ku = __builtin_amdgcn_readlane(bu, L);
        const u64 sb = (u64)__double_as_longlong(bs);
        const unsigned sl = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)sb, L);
        const unsigned sh = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(sb >> 32), L);
        const double sp = __longlong_as_double((long long)(((u64)sh << 32) | sl));
        if (mode != FRCNN_NMS_HARD && sp < min_score) break;
        const int k = L * U + ku;
        if (lane == 0) { s_pick[start + picked] = start + k; s_pprob[start + picked] = (float)sp; }
        if (lane == L) alive &= ~(1u << ku);
        const double4 pb = g_box[start + k];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if ((alive >> u) & 1) {
                const double o = dp_iou(pb, b[u]);
                if (mode == FRCNN_NMS_HARD) {
                    if (!(o <= nt)) alive &= ~(1u << u);
                } else if (mode == FRCNN_NMS_SOFT_LINEAR) {
                    if (!(o <= nt)) s[u] = s[u] * (1.0 - o);
                } else {
                    E[u] = E[u] + o * o;
                    s[u] = s0[u] * exp(-(E[u] / sigma));
                }
            }
        }
    }
}

// A class of more than DP_WG_ROWS rows is worked on by ALL eight waves instead, one row per thread, ONE workgroup barrier per pick: each
// wave's best goes through a parity-double-buffered LDS record and every thread folds the eight records.  Same picks, same scores.
// Measured (scripts/profile_detect_post.py, DESIGN §8 "Post-process rule"): a pick costs ~1.2 us this way whatever the class's size,
// ~2.5 us on one wave at 8 rows per lane, and well under 1 us on one wave at 1 row per lane, where the classes also run side by side.
// -DDP_WG_ROWS=0 / =512 build the two pure forms for that comparison.
#ifndef DP_WG_ROWS
#define DP_WG_ROWS 256
#endif
struct DpWaveBest { u64 key[2][DP_WAVES]; int k[2][DP_WAVES]; };

__device__ __forceinline__ void dp_pick_class_wg(const double4* g_box, const float* g_prob, int start, int n, int mode, double nt,
                                                 double sigma, double min_score, int* s_pick, float* s_pprob, DpWaveBest* wb) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    bool alive = t < n;
    const double4 b = alive ? g_box[start + t] : make_double4(0, 0, 0, 0);
    const double s0 = alive ? (double)g_prob[start + t] : 0.0;
    double s = s0, E = 0.0;
    for (int picked = 0; picked < n; ++picked) {
        const int par = picked & 1;
        const u64 bk = alive ? dp_key(s) : 0ull;
        const u64 m = dp_wave_max(bk);
        const u64 who = __ballot(bk == m);
        if (lane == 0) { wb->key[par][wave] = m; wb->k[par][wave] = m ? wave * 64 + (__builtin_ctzll(who) & 63) : 0; }
        __syncthreads();
        u64 best = 0; int k = 0;
#pragma unroll
        for (int w = 0; w < DP_WAVES; ++w) { const u64 kw = wb->key[par][w]; if (kw > best) { best = kw; k = wb->k[par][w]; } }
        if (best == 0) break;
        const double sp = __longlong_as_double((long long)((best >> 63) ? (best & 0x7fffffffffffffffull) : ~best));
        if (mode != FRCNN_NMS_HARD && sp < min_score) break;
        if (t == 0) { s_pick[start + picked] = start + k; s_pprob[start + picked] = (float)sp; }
        if (t == k) alive = false;
        const double4 pb = g_box[start + k];
        if (alive) {
            const double o = dp_iou(pb, b);
            if (mode == FRCNN_NMS_HARD) {
                if (!(o <= nt)) alive = false;
            } else if (mode == FRCNN_NMS_SOFT_LINEAR) {
                if (!(o <= nt)) s = s * (1.0 - o);
            } else {
                E = E + o * o;
                s = s0 * exp(-(E / sigma));
            }
        }
    }
    __syncthreads();          // the records of the last round are read before the next class writes them
}

__global__ void __launch_bounds__(DP_MAX) k_detections_post(
        const float4* rois, const int32_t* n_rois_ptr, int max_rows, const float* out_cls, const float* out_reg, int C,
        int bg_idx, double det_threshold, double stride, double resize_ratio, double nms_thresh,
        int32_t* det_cls, float* det_prob, int32_t* det_bbox, int32_t* det_roi, int32_t* n_dets,
        const double* dyn, int roi_batch, int mode, double sigma, double min_score, double vote_iou) {
    __shared__ float u_prob[DP_MAX];        // unsorted staging (the box stays in its thread's registers)
    __shared__ int u_cls[DP_MAX];
    __shared__ double4 s_box[DP_MAX];       // ranked
    __shared__ float s_prob[DP_MAX];
    __shared__ int s_cls[DP_MAX];
    __shared__ int s_roi[DP_MAX];
    __shared__ int s_fj[DP_MAX];
    __shared__ double4 g_box[DP_MAX];       // grouped: classes in emission order, ranked order inside a class
    __shared__ float g_prob[DP_MAX];
    __shared__ int g_cls[DP_MAX];
    __shared__ int g_roi[DP_MAX];
    __shared__ int s_pick[DP_MAX];          // per class, from its start: the grouped rows it emits in pick order, -1 behind them
    __shared__ float s_pprob[DP_MAX];
    __shared__ int s_first[DP_MAX_CLASSES];
    __shared__ int s_cstart[DP_MAX_CLASSES];
    __shared__ int s_ccount[DP_MAX_CLASSES];
    __shared__ int s_wcnt[DP_WAVES];
    __shared__ int s_nvalid;

    const int r = threadIdx.x;
    if (dyn) { resize_ratio = dyn[0]; det_threshold = dyn[1]; }
    if (min_score < 0.0) min_score = det_threshold;
    const int n_live = *n_rois_ptr;
    const int n_scored = (roi_batch > 0 && n_live > 0) ? (n_live + roi_batch - 1) / roi_batch * roi_batch : n_live;
    const int n = min(min(n_scored, max_rows), DP_MAX);
    if (r < DP_MAX_CLASSES) { s_first[r] = 0x7fffffff; s_cstart[r] = 0x7fffffff; s_ccount[r] = 0; }
    if (r == 0) s_nvalid = 0;
    s_pick[r] = -1;
    __syncthreads();

    // ---- 1. per-RoI class / confidence / decoded box (k_detections phase 1)
    int cls = -1; float conf = 0.0f; double4 box = make_double4(0, 0, 0, 0);
    if (r < n) {
        const float* pc = out_cls + (size_t)r * C;
        int best = 0; float bv = pc[0];
#pragma unroll 8
        for (int c = 1; c < C; ++c) { const float v = pc[c]; if (v > bv) { bv = v; best = c; } }   // np.argmax: first max
        if (best != bg_idx && !((double)bv < det_threshold)) {
            cls = best; conf = bv;
            const float4 roi = rois[r];
            const float* pr = out_reg + (size_t)r * 4 * (C - 1) + 4 * best;
            const float tx = pr[0] / 10.0f, ty = pr[1] / 10.0f, tw = pr[2] / 5.0f, th = pr[3] / 5.0f;   // / BBREG_MULTIPLIERS (f32)
            const double cxa = (double)(roi.x + roi.z) / 2.0, cya = (double)(roi.y + roi.w) / 2.0;
            const float wa = roi.z - roi.x, ha = roi.w - roi.y;
            const double cx = (double)(tx * wa) + cxa, cy = (double)(ty * ha) + cya;
            const double w = exp((double)tw) * (double)wa, h = exp((double)th) * (double)ha;
            const double x = cx - w / 2.0, y = cy - h / 2.0;
            box = make_double4(stride * x, stride * y, stride * (x + w), stride * (y + h));
            atomicMin(&s_first[best], r);
        }
    }
    u_prob[r] = conf; u_cls[r] = cls;
    const u64 vb = __ballot(cls >= 0);
    if ((r & 63) == 0 && vb) atomicAdd(&s_nvalid, __popcll(vb));
    __syncthreads();
    const int nv = s_nvalid;

    // ---- 2. rank by (score desc, roi index asc) among valid rows (k_detections phase 2)
    int rank = -1;
    if (cls >= 0) {
        rank = 0;
#pragma unroll 8
        for (int j = 0; j < n; ++j) {
            const float pj = u_prob[j];
            rank += (u_cls[j] >= 0) && (pj > conf || (pj == conf && j < r));
        }
        s_box[rank] = box; s_prob[rank] = conf; s_cls[rank] = cls; s_roi[rank] = r; s_fj[rank] = s_first[cls];
    }
    __syncthreads();

    // ---- 3. group by class: key (first valid row of the class, rank)
    if (r < nv) {
        const int mc = s_cls[r], mf = s_fj[r];
        int pos = 0;
#pragma unroll 8
        for (int j = 0; j < nv; ++j) {
            const int fj = s_fj[j];
            pos += (fj < mf) || (fj == mf && j < r);
        }
        g_box[pos] = s_box[r]; g_prob[pos] = s_prob[r]; g_cls[pos] = mc; g_roi[pos] = s_roi[r];
        atomicMin(&s_cstart[mc], pos);
        atomicAdd(&s_ccount[mc], 1);
    }
    __syncthreads();

    // ---- 4. pick loops: the (at most one, with the default DP_WG_ROWS) large class by the whole workgroup, then whole classes to waves,
    //         nothing shared between them
    {
        __shared__ DpWaveBest s_wb;
        for (int c = 0; c < C; ++c) {
            const int cn = s_ccount[c];                                  // (uniform: every thread takes the same branch)
            if (cn > DP_WG_ROWS) dp_pick_class_wg(g_box, g_prob, s_cstart[c], cn, mode, nms_thresh, sigma, min_score, s_pick, s_pprob, &s_wb);
        }
    }
    {
        const int wave = r >> 6;
        for (int c = wave; c < C; c += DP_WAVES) {
            const int cn = s_ccount[c];
            if (cn == 0 || cn > DP_WG_ROWS) continue;
            const int cs = s_cstart[c];
            if (cn <= 64) dp_pick_class<1>(g_box, g_prob, cs, cn, mode, nms_thresh, sigma, min_score, s_pick, s_pprob);
            else if (cn <= 128) dp_pick_class<2>(g_box, g_prob, cs, cn, mode, nms_thresh, sigma, min_score, s_pick, s_pprob);
            else if (cn <= 256) dp_pick_class<4>(g_box, g_prob, cs, cn, mode, nms_thresh, sigma, min_score, s_pick, s_pprob);
            else dp_pick_class<8>(g_box, g_prob, cs, cn, mode, nms_thresh, sigma, min_score, s_pick, s_pprob);
        }
    }
    __syncthreads();

    // ---- 5. emission: slot r of the pick lists -> its place among all picks; the box, voted or not
    const int g = r < nv ? s_pick[r] : -1;
    const bool emit = g >= 0;
    const u64 eb = __ballot(emit);
    if ((r & 63) == 0) s_wcnt[r >> 6] = __popcll(eb);
    __syncthreads();
    int total = 0, before = 0;
#pragma unroll
    for (int w = 0; w < DP_WAVES; ++w) { const int cw = s_wcnt[w]; total += cw; before += w < (r >> 6) ? cw : 0; }
    if (emit) {
        const int pos = before + __popcll(eb & ((1ull << (r & 63)) - 1));
        const int mc = g_cls[g];
        double4 b = g_box[g];
        if (vote_iou > 0.0) {
            const int cs = s_cstart[mc], cn = s_ccount[mc];
            double ax = 0.0, ay = 0.0, az = 0.0, aw = 0.0, ws = 0.0;
            for (int j = cs; j < cs + cn; ++j) {
                const double4 bj = g_box[j];
                if (dp_iou(b, bj) >= vote_iou) {
                    const double wj = (double)g_prob[j];
                    ax = ax + wj * bj.x; ay = ay + wj * bj.y; az = az + wj * bj.z; aw = aw + wj * bj.w;
                    ws = ws + wj;
                }
            }
            if (ws > 0.0) b = make_double4(ax / ws, ay / ws, az / ws, aw / ws);
        }
        det_cls[pos] = mc;
        det_prob[pos] = s_pprob[r];
        det_roi[pos] = g_roi[g];
        det_bbox[4 * pos + 0] = (int)rint(b.x / resize_ratio);
        det_bbox[4 * pos + 1] = (int)rint(b.y / resize_ratio);
        det_bbox[4 * pos + 2] = (int)rint(b.z / resize_ratio);
        det_bbox[4 * pos + 3] = (int)rint(b.w / resize_ratio);
    }
    for (int i = total + r; i < max_rows; i += DP_MAX) {      // rows past the last detection: the same "empty" values every call
        det_cls[i] = -1; det_prob[i] = 0.0f; det_roi[i] = -1;
        det_bbox[4 * i + 0] = det_bbox[4 * i + 1] = det_bbox[4 * i + 2] = det_bbox[4 * i + 3] = 0;
    }
    if (r == 0) {
        n_dets[0] = total;
        if (dyn) n_dets[1] = n_live;
    }
}

static int dp_check(const char* what, int max_rows, int num_classes, double nms_thresh, int nms_mode, double sigma, double min_score,
                    double vote_iou) {
    if (max_rows <= 0 || max_rows > DP_MAX) return fail(FRCNN_E_ARG, "%s: max_rows=%d exceeds %d", what, max_rows, DP_MAX);
    if (num_classes < 2 || num_classes > DP_MAX_CLASSES) return fail(FRCNN_E_ARG, "%s: num_classes=%d out of range", what, num_classes);
    if (nms_mode < FRCNN_NMS_HARD || nms_mode > FRCNN_NMS_SOFT_GAUSSIAN) return fail(FRCNN_E_ARG, "%s: nms_mode=%d (0..2)", what, nms_mode);
    if (!(nms_thresh >= 0.0 && nms_thresh <= 1.0)) return fail(FRCNN_E_ARG, "%s: nms_thresh=%g outside [0, 1]", what, nms_thresh);
    if (!(sigma > 0.0) || !isfinite(sigma)) return fail(FRCNN_E_ARG, "%s: sigma=%g must be finite and > 0", what, sigma);
    if (!(min_score <= 1.0)) return fail(FRCNN_E_ARG, "%s: min_score=%g (negative: the threshold; else at most 1)", what, min_score);
    if (!(vote_iou >= 0.0 && vote_iou <= 1.0)) return fail(FRCNN_E_ARG, "%s: vote_iou=%g (0: off; else in (0, 1])", what, vote_iou);
    return FRCNN_OK;
}

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_detect_post_version(void) { return FRCNN_DETECT_POST_VERSION; }

extern "C" int frcnn_detections_post(const float* rois, const int32_t* n_rois, int max_rows, const float* out_cls, const float* out_reg,
                                     int num_classes, int bg_idx, double det_threshold, double stride, double resize_ratio,
                                     double nms_thresh, int32_t* det_cls, float* det_prob, int32_t* det_bbox, int32_t* det_roi,
                                     int32_t* n_dets, int nms_mode, double sigma, double min_score, double vote_iou, void* stream) {
    if (!rois || !n_rois || !out_cls || !out_reg || !det_cls || !det_prob || !det_bbox || !det_roi || !n_dets)
        return fail(FRCNN_E_ARG, "detections_post: null pointer");
    if (int e = dp_check("detections_post", max_rows, num_classes, nms_thresh, nms_mode, sigma, min_score, vote_iou)) return e;
    k_detections_post<<<1, DP_MAX, 0, as_stream(stream)>>>((const float4*)rois, n_rois, max_rows, out_cls, out_reg, num_classes, bg_idx,
                                                           det_threshold, stride, resize_ratio, nms_thresh, det_cls, det_prob, det_bbox,
                                                           det_roi, n_dets, nullptr, 0, nms_mode, sigma, min_score, vote_iou);
    return check_launch("detections_post");
}

extern "C" int frcnn_detections_post_dyn(const float* rois, const int32_t* n_rois, int roi_batch, int max_rows, const float* out_cls,
                                         const float* out_reg, int num_classes, int bg_idx, double stride, double nms_thresh,
                                         const double* dyn, int32_t* det_cls, float* det_prob, int32_t* det_bbox, int32_t* det_roi,
                                         int32_t* counts, int nms_mode, double sigma, double min_score, double vote_iou, void* stream) {
    if (!rois || !n_rois || !out_cls || !out_reg || !dyn || !det_cls || !det_prob || !det_bbox || !det_roi || !counts)
        return fail(FRCNN_E_ARG, "detections_post_dyn: null pointer");
    if (int e = dp_check("detections_post_dyn", max_rows, num_classes, nms_thresh, nms_mode, sigma, min_score, vote_iou)) return e;
    if (roi_batch < 0) return fail(FRCNN_E_ARG, "detections_post_dyn: roi_batch=%d", roi_batch);
    if (((uintptr_t)dyn & 7) != 0) return fail(FRCNN_E_ARG, "detections_post_dyn: dyn must be 8-byte aligned");
    k_detections_post<<<1, DP_MAX, 0, as_stream(stream)>>>((const float4*)rois, n_rois, max_rows, out_cls, out_reg, num_classes, bg_idx,
                                                           0.0, stride, 1.0, nms_thresh, det_cls, det_prob, det_bbox, det_roi, counts,
                                                           dyn, roi_batch, nms_mode, sigma, min_score, vote_iou);
    return check_launch("detections_post_dyn");
}
