// Tracks counted as they cross lines, and the lines and their totals drawn into the frames (include/ext/frcnn_hip_count.h states the rule,
// DESIGN §8 "Count rule").  gfx950 (CDNA4) only.
// k_count_update: ONE workgroup walks the frames of a call in order -- frame f + 1 needs frame f's table.  The table lives in LDS for the
// whole call, six words an entry, compacted in ascending id order, in two copies that take turns.  Inside a frame the parallelism is over
// rows and entries: the eligible rows are compacted in row order with wave64 ballots, each finds its entry by binary search, the new ids
// are ranked with ballots again and take the places behind the table, and then a thread per ENTRY walks the compacted rows and steps
// through its own -- rows that share an id step in row order without any thread looking at another's entry -- and leaves each row the
// mask of the bits it set.  A prefix over the rows' bit counts gives every event its place in (row, line) order, sixteen ballots a round
// give the totals, and a count per entry puts the survivors into the other copy in id order.  Every word of a frame's count list, and at
// the end of the call of the state, is written by one thread with a plain store.  No atomics.
// k_count_draw: a gather.  A workgroup owns a tile of 256 byte columns x 16 rows, as k_trails_draw does and for its reason (threads are
// bytes).  Its first threads stage one line each: the segment, whether its grown bounding box meets the tile, the label's text formatted
// in decimal, its box and whether that meets the tile; a tile that nothing meets stores nothing.
#include "common.h"
#include "../../include/ext/frcnn_hip_redact.h"
#include "../../include/ext/frcnn_hip_track.h"
#include "../../include/ext/frcnn_hip_count.h"

namespace frcnn {

constexpr int CT_THREADS = 256, CT_WAVES = CT_THREADS / 64;
constexpr int CT_CAP = FRCNN_TRACK_MAX, CT_ROWS = FRCNN_REDACT_MAX_ROWS, CT_LINES = FRCNN_COUNT_MAX_LINES, CT_EVENTS = FRCNN_COUNT_MAX_EVENTS;
constexpr int CT_BITS = 2 * CT_LINES, CT_HEAD = 4 + CT_BITS, CT_ENTRY = 6, CT_LIST = FRCNN_COUNT_LIST_WORDS;
constexpr int CT_TILE_ROWS = 16;
constexpr int CT_TEXT = 28;                                                 // "L7 +2147483647 -2147483647" is 26 characters
enum { CT_ID, CT_CLS, CT_SEEN, CT_COUNTED, CT_PX, CT_PY };
static_assert(CT_CAP <= CT_THREADS && 4 * CT_EVENTS == CT_THREADS && CT_BITS <= 16, "a thread per entry and per word of a list's events");

struct CountLines {                                                         // passed by value as a kernel argument
    int n;
    int v[CT_LINES][4];                                                     // (ax, ay, bx, by)
};

__constant__ uint8_t CT_PALETTE[8][3] = {{255, 64, 64}, {64, 160, 255}, {255, 208, 0}, {255, 0, 255},
                                         {0, 224, 224}, {255, 128, 0}, {160, 96, 255}, {255, 255, 255}};
// the glyphs a label needs, rows as frcnn_annotate_u8's table has them (bit 4 = the leftmost column): ' ', '+', '-', '0'..'9', 'L'
enum { CT_G_SPACE = 0, CT_G_PLUS = 1, CT_G_MINUS = 2, CT_G_0 = 3, CT_G_L = 13 };
__constant__ uint8_t CT_GLYPHS[14][7] = {
    {0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00}, {0x00, 0x04, 0x04, 0x1F, 0x04, 0x04, 0x00}, {0x00, 0x00, 0x00, 0x1F, 0x00, 0x00, 0x00},
    {0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E}, {0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E}, {0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F},
    {0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E}, {0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02}, {0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E},
    {0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E}, {0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08}, {0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E},
    {0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C}, {0x10, 0x10, 0x10, 0x10, 0x10, 0x10, 0x1F}};

// The number of threads in front of this one, in thread order, whose ``flag`` is set, and ``total``, the workgroup's count.  Every thread
// of the workgroup calls it; ``s_cnt`` is free again when it returns.
__device__ inline int ct_rank(bool flag, int* s_cnt, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(flag);
    if (lane == 0) s_cnt[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < CT_WAVES; ++k) {
        const int c = s_cnt[k];
        before += k < wave ? c : 0;
        all += c;
    }
    __syncthreads();
    total = all;
    return before + __popcll(mask & ((1ull << lane) - 1ull));
}

// The sum of ``v`` over the threads in front of this one, in thread order, and ``total``, the workgroup's sum.  As ct_rank.
__device__ inline int ct_prefix(int v, int* s_cnt, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    if (lane == 63) s_cnt[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < CT_WAVES; ++k) {
        const int c = s_cnt[k];
        before += k < wave ? c : 0;
        all += c;
    }
    __syncthreads();
    total = all;
    return before + inc - v;
}

// CROSSING of line L = (ax, ay, bx, by) by the step P -> Q: -1, or the direction.
__device__ inline int ct_cross(const int* L, int px, int py, int qx, int qy) {
    const long long ax = L[0], ay = L[1], bx = L[2], by = L[3], dx = bx - ax, dy = by - ay;
    const bool sp = dx * (py - ay) - dy * (px - ax) >= 0, sq = dx * (qy - ay) - dy * (qx - ax) >= 0;
    if (sp == sq) return -1;
    const long long ex = (long long)qx - px, ey = (long long)qy - py;
    const bool ta = ex * (ay - py) - ey * (ax - px) >= 0, tb = ex * (by - py) - ey * (bx - px) >= 0;
    if (ta == tb) return -1;
    return sq ? 1 : 0;
}

__device__ inline void ct_stage_lines(const CountLines& lines, int (*s_line)[4]) {
#pragma unroll
    for (int l = 0; l < CT_LINES; ++l)                                      // (unrolled: the argument is read with constant indices)
        if ((int)threadIdx.x == l) {
            s_line[l][0] = lines.v[l][0];
            s_line[l][1] = lines.v[l][1];
            s_line[l][2] = lines.v[l][2];
            s_line[l][3] = lines.v[l][3];
        }
}

__global__ void __launch_bounds__(CT_THREADS) k_count_update(int32_t* state, int cap, const int32_t* tracked, long long stride, int R, int frames,
                                                               const int32_t* n_frames, const int32_t* gate, CountLines lines,
                                                               const uint8_t* classes, int nc, int E, int h, int w, int32_t* lists) {
    __shared__ int s_tab[2][CT_ENTRY][CT_CAP];                              // the table, twice: a frame's survivors move to the other copy
    __shared__ int s_live[CT_CAP];
    __shared__ int s_rid[CT_ROWS], s_rcls[CT_ROWS], s_rpx[CT_ROWS], s_rpy[CT_ROWS];      // the frame's eligible rows, in row order
    __shared__ int s_rent[CT_ROWS], s_rfirst[CT_ROWS], s_rev[CT_ROWS];    // their entry, the first row of their id, the bits they set
    __shared__ int s_ev[4 * CT_EVENTS], s_tot[CT_BITS], s_wtot[CT_WAVES][CT_BITS];
    __shared__ int s_line[CT_LINES][4];
    __shared__ int s_cnt[CT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nf = gate && *gate == 0 ? 0 : min(max(*n_frames, 0), frames);
    for (long long i = (long long)nf * CT_LIST + tid; i < (long long)frames * CT_LIST; i += CT_THREADS) lists[i] = 0;       // padding frames
    if (nf <= 0) return;
    const int nlines = lines.n;
    int ne = min(max(state[0], 0), cap), fr = state[1], dropped = state[2], evdrop = state[3], cur = 0;
    if (tid < CT_BITS) s_tot[tid] = state[4 + tid];
    if (tid < CT_CAP) {
        const bool live = tid < ne;
        const int32_t* e = state + CT_HEAD + (size_t)(live ? tid : 0) * CT_ENTRY;
#pragma unroll
        for (int j = 0; j < CT_ENTRY; ++j) s_tab[0][j][tid] = live ? e[j] : 0;
    }
    ct_stage_lines(lines, s_line);
    __syncthreads();
    for (int f = 0; f < nf; ++f) {
        fr += 1;
        int (*T)[CT_CAP] = s_tab[cur];
        const int32_t* buf = tracked + (long long)f * stride;
        const int nl = min(max(buf[1], 0), R);
        const int32_t *bbox = buf + 4, *cls = buf + 4 + 4 * R, *ids = buf + 4 + 6 * R;
        int total;
        s_ev[tid] = 0;
        // the eligible rows, compacted in row order
        int m = 0;
        for (int base = 0; base < nl; base += CT_THREADS) {
            const int r = base + tid;
            bool ok = false;
            int rid = 0, rc = 0, cx = 0, cy = 0;
            if (r < nl && (rid = ids[r]) >= 1) {
                const int x1 = bbox[4 * r], y1 = bbox[4 * r + 1], x2 = bbox[4 * r + 2], y2 = bbox[4 * r + 3];
                const int xa = max(min(x1, x2), 0), xb = min(max(x1, x2), w - 1), ya = max(min(y1, y2), 0), yb = min(max(y1, y2), h - 1);
                if (xa <= xb && ya <= yb) {
                    rc = cls[r];
                    ok = rc >= 0 && rc < nc && classes[rc] != 0;
                    cx = (xa + xb) >> 1;
                    cy = (ya + yb) >> 1;
                }
            }
            const int k = m + ct_rank(ok, s_cnt, total);
            if (ok) {
                s_rid[k] = rid;
                s_rcls[k] = rc;
                s_rpx[k] = cx;
                s_rpy[k] = cy;
            }
            m += total;
        }
        __syncthreads();
        // each row's entry (its place in the table, or -1), and for a row without one the first row of the frame that has its id
        for (int k = tid; k < m; k += CT_THREADS) {
            const int rid = s_rid[k];
            int lo = 0, hi = ne, found = -1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1, v = T[CT_ID][mid];
                if (v == rid) { found = mid; break; }
                if (v < rid) lo = mid + 1; else hi = mid;
            }
            int first = k;
            if (found < 0)
                for (int j = 0; j < k; ++j)
                    if (s_rid[j] == rid) { first = j; break; }
            s_rent[k] = found;
            s_rfirst[k] = first;
            s_rev[k] = 0;
        }
        __syncthreads();
        // the new ids in row order take the places behind the table while there are any
        const int nfree = cap - ne;
        int births = 0;
        for (int base = 0; base < m; base += CT_THREADS) {
            const int k = base + tid;
            const bool is_new = k < m && s_rent[k] < 0 && s_rfirst[k] == k;
            const int rank = births + ct_rank(is_new, s_cnt, total);
            if (is_new && rank < nfree) {
                const int e = ne + rank;
                s_rent[k] = e;
                T[CT_ID][e] = s_rid[k];
                T[CT_CLS][e] = s_rcls[k];
                T[CT_SEEN][e] = fr;
                T[CT_COUNTED][e] = 0;
                T[CT_PX][e] = s_rpx[k];
                T[CT_PY][e] = s_rpy[k];
            }
            births += total;
        }
        __syncthreads();
        const int nt = ne + min(births, nfree);
        // later rows of a new id follow its first row; the rows left without an entry are counted
        for (int base = 0; base < m; base += CT_THREADS) {
            const int k = base + tid;
            bool lost = false;
            if (k < m) {
                int e = s_rent[k];
                if (e < 0 && s_rfirst[k] != k) s_rent[k] = e = s_rent[s_rfirst[k]];     // (a first row's word: nobody writes it here)
                lost = e < 0;
            }
            ct_rank(lost, s_cnt, total);
            dropped += total;
        }
        __syncthreads();
        // STEP: a thread per entry takes its rows in row order; a new entry's first row is the one that made it
        if (tid < nt) {
            int px = T[CT_PX][tid], py = T[CT_PY][tid], counted = T[CT_COUNTED][tid], seen = T[CT_SEEN][tid];
            bool birth = tid >= ne;
            for (int k = 0; k < m; ++k) {
                if (s_rent[k] != tid) continue;
                if (birth) { birth = false; continue; }
                const int qx = s_rpx[k], qy = s_rpy[k];
                int mask = 0;
                for (int l = 0; l < nlines; ++l) {
                    const int dir = ct_cross(s_line[l], px, py, qx, qy);
                    const int bit = 1 << (2 * l + max(dir, 0));
                    if (dir >= 0 && !(counted & bit)) {                     // ONCE
                        counted |= bit;
                        mask |= bit;
                    }
                }
                s_rev[k] = mask;
                px = qx;
                py = qy;
                seen = fr;
            }
            T[CT_PX][tid] = px;
            T[CT_PY][tid] = py;
            T[CT_COUNTED][tid] = counted;
            T[CT_SEEN][tid] = seen;
            s_live[tid] = fr - seen <= E;                                   // EXPIRE
        }
        __syncthreads();
        // the events in (row, line) order, and the totals
        int nev = 0;
        for (int base = 0; base < m; base += CT_THREADS) {
            const int k = base + tid;
            const int mask = k < m ? s_rev[k] : 0;
            int at = nev + ct_prefix(__popc(mask), s_cnt, total);
            if (total > 0) {                                                // (the same for every thread)
                for (int b = 0; b < CT_BITS; ++b) {
                    const int c = __popcll(__ballot((mask >> b) & 1));
                    if (lane == 0) s_wtot[wave][b] = c;
                }
                __syncthreads();
                if (tid < CT_BITS) {
                    int c = 0;
                    for (int k2 = 0; k2 < CT_WAVES; ++k2) c += s_wtot[k2][tid];
                    s_tot[tid] += c;
                }
                if (mask) {
                    const int rid = s_rid[k], ec = T[CT_CLS][s_rent[k]];
                    for (int b = 0; b < CT_BITS; ++b) {
                        if (!((mask >> b) & 1)) continue;
                        if (at < CT_EVENTS) {
                            s_ev[4 * at] = b >> 1;
                            s_ev[4 * at + 1] = b & 1;
                            s_ev[4 * at + 2] = rid;
                            s_ev[4 * at + 3] = ec;
                        }
                        at += 1;
                    }
                }
                __syncthreads();
            }
            nev += total;
        }
        evdrop += max(nev - CT_EVENTS, 0);
        // the survivors, in id order, into the other copy
        const bool live = tid < nt && s_live[tid];
        if (live) {
            const int my = T[CT_ID][tid];
            int pos = 0;
            for (int e = 0; e < nt; ++e) pos += s_live[e] && T[CT_ID][e] < my;
#pragma unroll
            for (int j = 0; j < CT_ENTRY; ++j) s_tab[cur ^ 1][j][pos] = T[j][tid];
        }
        ct_rank(live, s_cnt, ne);                                           // (its barriers also publish the copy, s_ev and s_tot)
        cur ^= 1;
        int32_t* L = lists + (long long)f * CT_LIST;
        for (int i = tid; i < CT_LIST; i += CT_THREADS)
            L[i] = i == 0 ? min(nev, CT_EVENTS) : i == 1 ? fr : i < 4 ? 0 : i < CT_HEAD ? s_tot[i - 4] : s_ev[i - CT_HEAD];
        __syncthreads();
    }
    const int words = CT_HEAD + cap * CT_ENTRY;
    for (int i = tid; i < words; i += CT_THREADS) {
        int v;
        if (i < 4) {
            v = i == 0 ? ne : i == 1 ? fr : i == 2 ? dropped : evdrop;
        } else if (i < CT_HEAD) {
            v = s_tot[i - 4];
        } else {
            const int t = (i - CT_HEAD) / CT_ENTRY, j = (i - CT_HEAD) - t * CT_ENTRY;
            v = t < ne ? s_tab[cur][j][t] : 0;
        }
        state[i] = v;
    }
}

__global__ void __launch_bounds__(CT_THREADS) k_count_draw(uint8_t* frame, int h, int w, const int32_t* list, CountLines lines, int W, int rgb) {
    __shared__ int s_line[CT_LINES][4];
    __shared__ int s_hit[CT_LINES], s_x0[CT_LINES], s_y0[CT_LINES], s_len[CT_LINES];      // 1: the segment meets the tile, 2: the label box
    __shared__ uint8_t s_txt[CT_LINES][CT_TEXT];                           // the label's glyphs (CT_GLYPHS rows)
    if (list[1] <= 0) return;                                               // the list of a frame that is not real
    const int tid = threadIdx.x, nlines = lines.n;
    const int rowbytes = 3 * w, j0 = blockIdx.x * CT_THREADS, ty0 = blockIdx.y * CT_TILE_ROWS;
    const int ty1 = min(ty0 + CT_TILE_ROWS, h) - 1;
    const int tx0 = j0 / 3, tx1 = min(j0 + CT_THREADS - 1, rowbytes - 1) / 3;
    const int g = (W + 1) >> 1;
    ct_stage_lines(lines, s_line);
    __syncthreads();
    if (tid < nlines) {
        const int l = tid, ax = s_line[l][0], ay = s_line[l][1], bx = s_line[l][2], by = s_line[l][3];
        int hit = max(ax, bx) + g >= tx0 && min(ax, bx) - g <= tx1 && max(ay, by) + g >= ty0 && min(ay, by) - g <= ty1;
        uint8_t* t = s_txt[l];
        int n = 0;
        t[n++] = CT_G_L;
        t[n++] = CT_G_0 + l;
        for (int d = 1; d >= 0; --d) {                                      // pos, then neg
            t[n++] = CT_G_SPACE;
            t[n++] = d ? CT_G_PLUS : CT_G_MINUS;
            unsigned v = (unsigned)max(list[4 + 2 * l + d], 0);
            int nd = 1;
            for (unsigned p = v; p >= 10u; p /= 10u) nd += 1;
            for (int i = nd - 1; i >= 0; --i) {
                t[n + i] = (uint8_t)(CT_G_0 + v % 10u);
                v /= 10u;
            }
            n += nd;
        }
        const int bw = 12 * n, bh = 16, mx = (ax + bx) >> 1, my = (ay + by) >> 1;
        const int x0 = bw <= w ? min(max(mx, 0), w - bw) : mx, y0 = bh <= h ? min(max(my, 0), h - bh) : my;
        if (x0 <= tx1 && x0 + bw - 1 >= tx0 && y0 <= ty1 && y0 + bh - 1 >= ty0) hit |= 2;
        s_hit[l] = hit;
        s_x0[l] = x0;
        s_y0[l] = y0;
        s_len[l] = n;
    }
    __syncthreads();
    int any = 0;
    for (int l = 0; l < nlines; ++l) any |= s_hit[l];
    const int j = j0 + tid, x = j / 3, c = j - 3 * x;
    if (!any || j >= rowbytes) return;
    int col[CT_TILE_ROWS];                                                  // -1: untouched; 0..7: the palette; 8: black
#pragma unroll
    for (int r = 0; r < CT_TILE_ROWS; ++r) col[r] = -1;
    const long long r2 = (long long)(W * W) >> 2;
    for (int l = 0; l < nlines; ++l) {                                      // ascending: the highest line that covers a pixel stays
        if (!(s_hit[l] & 1)) continue;
        const int ax = s_line[l][0], ay = s_line[l][1], bx = s_line[l][2], by = s_line[l][3];
        if (x < min(ax, bx) - g || x > max(ax, bx) + g) continue;
        const long long dx = (long long)bx - ax, dy = (long long)by - ay, dd = dx * dx + dy * dy;
        const long long px = (long long)x - ax, qx = (long long)x - bx, bound = ((long long)(W * W) * dd) >> 2;
#pragma unroll
        for (int r = 0; r < CT_TILE_ROWS; ++r) {
            const long long py = (long long)(ty0 + r) - ay, u = px * dx + py * dy;
            bool cov;
            if (dd == 0 || u <= 0) {
                cov = px * px + py * py <= r2;
            } else if (u >= dd) {
                const long long qy = (long long)(ty0 + r) - by;
                cov = qx * qx + qy * qy <= r2;
            } else {
                long long cr = px * dy - py * dx;
                cr = cr < 0 ? -cr : cr;
                cov = cr < (1LL << 31) && cr * cr <= bound;                 // (bound < 2^40: beyond 2^31 nothing covers, and below it the square fits)
            }
            if (cov) col[r] = l & 7;
        }
    }
    for (int l = 0; l < nlines; ++l) {                                      // the labels, above every line, the highest box on top
        if (!(s_hit[l] & 2)) continue;
        const int rel = x - s_x0[l], y0 = s_y0[l];
        if (rel < 0 || rel >= 12 * s_len[l]) continue;
        const int k = (rel - 1) / 12, gx = (rel - 1) - 12 * k;
        const uint8_t* gl = CT_GLYPHS[s_txt[l][rel >= 1 ? k : 0]];
#pragma unroll
        for (int r = 0; r < CT_TILE_ROWS; ++r) {
            const int ry = ty0 + r - y0;
            if (ry < 0 || ry >= 16) continue;
            const bool ink = rel >= 1 && gx < 10 && ry >= 1 && ry <= 14 && ((gl[(ry - 1) >> 1] >> (4 - (gx >> 1))) & 1);
            col[r] = ink ? (l & 7) : 8;
        }
    }
#pragma unroll
    for (int r = 0; r < CT_TILE_ROWS; ++r)
        if (ty0 + r <= ty1 && col[r] >= 0)
            frame[(size_t)(ty0 + r) * rowbytes + j] = col[r] == 8 ? (uint8_t)0 : CT_PALETTE[col[r]][rgb ? c : 2 - c];
}

static int count_lines_ok(const char* who, const int32_t* lines, int n_lines, CountLines* out) {
    if (n_lines < 1 || n_lines > FRCNN_COUNT_MAX_LINES)
        return fail(FRCNN_E_ARG, "%s: n_lines=%d not in [1, %d]", who, n_lines, FRCNN_COUNT_MAX_LINES);
    *out = CountLines{};
    out->n = n_lines;
    for (int l = 0; l < n_lines; ++l) {
        for (int i = 0; i < 4; ++i) {
            const int v = lines[4 * l + i];
            if (v < FRCNN_COUNT_MIN_COORD || v > FRCNN_COUNT_MAX_COORD)
                return fail(FRCNN_E_ARG, "%s: line %d has the coordinate %d outside [%d, %d]", who, l, v, FRCNN_COUNT_MIN_COORD,
                            FRCNN_COUNT_MAX_COORD);
            out->v[l][i] = v;
        }
        if (lines[4 * l] == lines[4 * l + 2] && lines[4 * l + 1] == lines[4 * l + 3])
            return fail(FRCNN_E_ARG, "%s: line %d has A = B = (%d, %d)", who, l, lines[4 * l], lines[4 * l + 1]);
    }
    return FRCNN_OK;
}

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_count_version(void) { return FRCNN_COUNT_VERSION; }

extern "C" size_t frcnn_count_list_words(void) { return FRCNN_COUNT_LIST_WORDS; }

extern "C" size_t frcnn_count_state_bytes(int capacity) {
    return capacity >= 1 && capacity <= FRCNN_TRACK_MAX ? sizeof(int32_t) * (CT_HEAD + (size_t)capacity * CT_ENTRY) : 0;
}

extern "C" int frcnn_count_update(int32_t* state, int capacity, const int32_t* tracked, long long tracked_stride, int rows, int frames,
                                  const int32_t* n_frames, const int32_t* gate, const int32_t* lines, int n_lines, const uint8_t* classes,
                                  int num_classes, int expire, int h, int w, int32_t* lists, void* stream) {
    const char* who = "count_update";
    if (!state || !tracked || !n_frames || !lines || !classes || !lists) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (capacity < 1 || capacity > FRCNN_TRACK_MAX) return fail(FRCNN_E_ARG, "%s: capacity=%d not in [1, %d]", who, capacity, FRCNN_TRACK_MAX);
    if (rows < 1 || rows > FRCNN_REDACT_MAX_ROWS) return fail(FRCNN_E_ARG, "%s: rows=%d not in [1, %d]", who, rows, FRCNN_REDACT_MAX_ROWS);
    if (frames < 1 || frames > FRCNN_TRACK_MAX_FRAMES)
        return fail(FRCNN_E_ARG, "%s: frames=%d not in [1, %d]", who, frames, FRCNN_TRACK_MAX_FRAMES);
    if (frames > 1 && tracked_stride < 4 + 8LL * rows)
        return fail(FRCNN_E_ARG, "%s: tracked_stride=%lld under the %d words of a tracked buffer", who, tracked_stride, 4 + 8 * rows);
    CountLines cl;
    if (int rc = count_lines_ok(who, lines, n_lines, &cl)) return rc;
    if (num_classes < 1 || num_classes > FRCNN_COUNT_MAX_CLASSES)
        return fail(FRCNN_E_ARG, "%s: num_classes=%d not in [1, %d]", who, num_classes, FRCNN_COUNT_MAX_CLASSES);
    if (expire < 0 || expire > FRCNN_COUNT_MAX_EXPIRE)
        return fail(FRCNN_E_ARG, "%s: expire=%d not in [0, %d]", who, expire, FRCNN_COUNT_MAX_EXPIRE);
    if (h < 1 || h > FRCNN_REDACT_MAX_SIDE || w < 1 || w > FRCNN_REDACT_MAX_SIDE)
        return fail(FRCNN_E_ARG, "%s: frame %dx%d out of range (sides 1..%d)", who, h, w, FRCNN_REDACT_MAX_SIDE);
    k_count_update<<<1, CT_THREADS, 0, as_stream(stream)>>>(state, capacity, tracked, tracked_stride, rows, frames, n_frames, gate, cl, classes,
                                                            num_classes, expire, h, w, lists);
    return check_launch(who);
}

extern "C" int frcnn_count_draw_u8(uint8_t* frame, int h, int w, const int32_t* list, const int32_t* lines, int n_lines, int width, int rgb,
                                   void* stream) {
    const char* who = "count_draw_u8";
    if (!frame || !list || !lines) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (h < 1 || h > FRCNN_REDACT_MAX_SIDE || w < 1 || w > FRCNN_REDACT_MAX_SIDE)
        return fail(FRCNN_E_ARG, "%s: frame %dx%d out of range (sides 1..%d)", who, h, w, FRCNN_REDACT_MAX_SIDE);
    CountLines cl;
    if (int rc = count_lines_ok(who, lines, n_lines, &cl)) return rc;
    if (width < 1 || width > FRCNN_COUNT_MAX_WIDTH) return fail(FRCNN_E_ARG, "%s: width=%d not in [1, %d]", who, width, FRCNN_COUNT_MAX_WIDTH);
    k_count_draw<<<dim3((3 * w + CT_THREADS - 1) / CT_THREADS, (h + CT_TILE_ROWS - 1) / CT_TILE_ROWS), CT_THREADS, 0, as_stream(stream)>>>(
        frame, h, w, list, cl, width, rgb ? 1 : 0);
    return check_launch(who);
}
