// Tracks counted as they cross lines, and the lines and their totals drawn into the frames (include/ext/frcnn_hip_count.h states the rule,
// DESIGN §8 "Count rule").  gfx950 (CDNA4) only.
// k_count_update: the id-table walk of csrc/id_table.h -- ONE workgroup walks the frames of a call in order, frame f + 1 needs frame f's
// table -- over the two-copy table, six words an entry.  What is the count rule's own: a row's point is the centre of its clipped box and
// its class must be set; a thread per ENTRY walks the compacted rows and steps through its own -- rows that share an id step in row order
// without any thread looking at another's entry -- and leaves each row the mask of the bits it set.  A prefix over the rows' bit counts
// gives every event its place in (row, line) order, sixteen ballots a round give the totals.  Every word of a frame's count list, and at
// the end of the call of the state, is written by one thread with a plain store.  No atomics.
// k_count_draw: a gather over the tiles of csrc/overlay.h.  Its first threads stage one line each: the segment, whether its grown bounding
// box meets the tile, the label's text formatted in decimal, its box and whether that meets the tile; a tile that nothing meets stores
// nothing.  Then the capsules, the labels above them, and the store.
#include "id_table.h"
#include "overlay.h"
#include "../../include/ext/frcnn_hip_count.h"

namespace frcnn {

constexpr int CT_LINES = FRCNN_COUNT_MAX_LINES, CT_EVENTS = FRCNN_COUNT_MAX_EVENTS;
constexpr int CT_BITS = 2 * CT_LINES, CT_HEAD = 4 + CT_BITS, CT_ENTRY = 6, CT_LIST = FRCNN_COUNT_LIST_WORDS;
constexpr int CT_TEXT = 28;                                                 // "L7 +2147483647 -2147483647" is 26 characters
enum { CT_ID, CT_CLS, CT_SEEN, CT_COUNTED, CT_PX, CT_PY };
static_assert(4 * CT_EVENTS == IDT_THREADS && CT_BITS <= 16, "a thread per word of a list's events");

struct CountLines {                                                         // passed by value as a kernel argument
    int n;
    int v[CT_LINES][4];                                                     // (ax, ay, bx, by)
};

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

__global__ void __launch_bounds__(IDT_THREADS) k_count_update(int32_t* state, int cap, const int32_t* tracked, long long stride, int R, int frames,
                                                                const int32_t* n_frames, const int32_t* gate, CountLines lines,
                                                                const uint8_t* classes, int nc, int E, int h, int w, int32_t* lists) {
    __shared__ int s_tab[2][CT_ENTRY][IDT_CAP];                             // the table, twice: a frame's survivors move to the other copy
    __shared__ int s_live[IDT_CAP];
    __shared__ int s_rid[IDT_ROWS], s_rcls[IDT_ROWS], s_rpx[IDT_ROWS], s_rpy[IDT_ROWS];  // the frame's eligible rows, in row order
    __shared__ int s_rent[IDT_ROWS], s_rfirst[IDT_ROWS], s_rev[IDT_ROWS]; // their entry, the first row of their id, the bits they set
    __shared__ int s_ev[4 * CT_EVENTS], s_tot[CT_BITS], s_wtot[IDT_WAVES][CT_BITS];
    __shared__ int s_line[CT_LINES][4];
    __shared__ int s_cnt[IDT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nf = idt_begin(gate, n_frames, frames, lists, CT_LIST);
    if (nf <= 0) return;
    const int nlines = lines.n;
    int ne = min(max(state[0], 0), cap), fr = state[1], dropped = state[2], evdrop = state[3], cur = 0;
    idt_load<CT_ENTRY, CT_HEAD>(state, ne, s_tab[0], s_tot);
    ct_stage_lines(lines, s_line);
    __syncthreads();
    for (int f = 0; f < nf; ++f) {
        fr += 1;
        int (*T)[IDT_CAP] = s_tab[cur];
        const IdRows rows = idt_rows(tracked, stride, f, R);
        int total;
        s_ev[tid] = 0;
        // the eligible rows, compacted in row order: the live ones of a class that is set, their point the centre
        int m = 0;
        for (int base = 0; base < rows.n; base += IDT_THREADS) {
            const int r = base + tid;
            int rid = 0, rc = 0, xa = 0, xb = 0, ya = 0, yb = 0;
            bool ok = idt_live(rows, r, h, w, rid, xa, xb, ya, yb);
            if (ok) {
                rc = rows.cls[r];
                ok = idt_class_set(classes, nc, rc);
            }
            const int k = wg_append(ok, s_cnt, m);
            if (ok) {
                s_rid[k] = rid;
                s_rcls[k] = rc;
                s_rpx[k] = (xa + xb) >> 1;
                s_rpy[k] = (ya + yb) >> 1;
            }
        }
        __syncthreads();
        for (int k = tid; k < m; k += IDT_THREADS) {
            idt_lookup(k, s_rid, T[CT_ID], nullptr, ne, s_rent, s_rfirst);
            s_rev[k] = 0;
        }
        __syncthreads();
        // the new ids in row order take the places behind the table while there are any
        const int nfree = cap - ne;
        int births = 0;
        for (int base = 0; base < m; base += IDT_THREADS) {
            const int k = base + tid;
            const bool is_new = idt_birth(k, m, s_rent, s_rfirst);
            const int rank = wg_append(is_new, s_cnt, births);
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
        }
        __syncthreads();
        const int nt = ne + min(births, nfree);
        dropped += idt_follow(m, s_rent, s_rfirst, s_cnt);
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
        for (int base = 0; base < m; base += IDT_THREADS) {
            const int k = base + tid;
            const int mask = k < m ? s_rev[k] : 0;
            int at = nev + wg_prefix(__popc(mask), s_cnt, total);
            if (total > 0) {                                                // (the same for every thread)
                for (int b = 0; b < CT_BITS; ++b) {
                    const int c = __popcll(__ballot((mask >> b) & 1));
                    if (lane == 0) s_wtot[wave][b] = c;
                }
                __syncthreads();
                if (tid < CT_BITS) {
                    int c = 0;
                    for (int k2 = 0; k2 < IDT_WAVES; ++k2) c += s_wtot[k2][tid];
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
        ne = idt_compact<CT_ENTRY>(nt, s_live, T, s_tab[cur ^ 1], s_cnt);  // (its barriers also publish s_ev and s_tot)
        cur ^= 1;
        int32_t* L = lists + (long long)f * CT_LIST;
        for (int i = tid; i < CT_LIST; i += IDT_THREADS)
            L[i] = i == 0 ? min(nev, CT_EVENTS) : i == 1 ? fr : i < 4 ? 0 : i < CT_HEAD ? s_tot[i - 4] : s_ev[i - CT_HEAD];
        __syncthreads();
    }
    idt_store<CT_ENTRY, CT_HEAD>(state, cap, ne, fr, dropped, evdrop, s_tot, s_tab[cur]);
}

__global__ void __launch_bounds__(OV_THREADS) k_count_draw(uint8_t* frame, int h, int w, const int32_t* list, CountLines lines, int W, int rgb) {
    __shared__ int s_line[CT_LINES][4];
    __shared__ int s_hit[CT_LINES], s_x0[CT_LINES], s_y0[CT_LINES], s_len[CT_LINES];      // 1: the segment meets the tile, 2: the label box
    __shared__ uint8_t s_txt[CT_LINES][CT_TEXT];                           // the label's glyphs (OV_GLYPHS rows)
    if (list[1] <= 0) return;                                               // the list of a frame that is not real
    const int tid = threadIdx.x, nlines = lines.n, g = ov_grow(W);
    const OvTile t = ov_tile(h, w);
    ct_stage_lines(lines, s_line);
    __syncthreads();
    if (tid < nlines) {
        const int l = tid, ax = s_line[l][0], ay = s_line[l][1], bx = s_line[l][2], by = s_line[l][3];
        int hit = ov_meets(min(ax, bx), max(ax, bx), min(ay, by), max(ay, by), g, t);
        uint8_t* txt = s_txt[l];
        int n = 0;
        txt[n++] = OV_G_L;
        txt[n++] = OV_G_0 + l;
        for (int d = 1; d >= 0; --d) {                                      // pos, then neg
            txt[n++] = OV_G_SPACE;
            txt[n++] = d ? OV_G_PLUS : OV_G_MINUS;
            n = ov_decimal(txt, n, list[4 + 2 * l + d]);
        }
        int x0, y0;
        if (ov_label_place(n, (ax + bx) >> 1, (ay + by) >> 1, h, w, t, x0, y0)) hit |= 2;
        s_hit[l] = hit;
        s_x0[l] = x0;
        s_y0[l] = y0;
        s_len[l] = n;
    }
    __syncthreads();
    int any = 0;
    for (int l = 0; l < nlines; ++l) any |= s_hit[l];
    if (!any || t.j >= t.rowbytes) return;
    int col[OV_TILE_ROWS];                                                  // -1: untouched; 0..7: the palette; 8: black
#pragma unroll
    for (int r = 0; r < OV_TILE_ROWS; ++r) col[r] = -1;
    for (int l = 0; l < nlines; ++l) {                                      // ascending: the highest line that covers a pixel stays
        if (!(s_hit[l] & 1)) continue;
        const int ax = s_line[l][0], ay = s_line[l][1], bx = s_line[l][2], by = s_line[l][3];
        if (!ov_column_near(ax, bx, g, t.x)) continue;
        const OvCapsule s = ov_capsule(ax, ay, bx, by, t.x, W);
#pragma unroll
        for (int r = 0; r < OV_TILE_ROWS; ++r) capsule_paint<true>(s, t.ty0 + r, col[r], l & 7);
    }
    for (int l = 0; l < nlines; ++l)                                        // the labels, above every line, the highest box on top
        if (s_hit[l] & 2) ov_label_blit(s_txt[l], s_len[l], s_x0[l], s_y0[l], l & 7, t, col);
#pragma unroll
    for (int r = 0; r < OV_TILE_ROWS; ++r)
        if (t.ty0 + r <= t.ty1 && col[r] >= 0)
            frame[(size_t)(t.ty0 + r) * t.rowbytes + t.j] = col[r] == OV_COL_BLACK ? (uint8_t)0 : ov_colour(col[r], t.c, rgb);
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
    if (int rc = idt_call_ok(who, capacity, rows, frames, tracked_stride)) return rc;
    CountLines cl;
    if (int rc = count_lines_ok(who, lines, n_lines, &cl)) return rc;
    if (num_classes < 1 || num_classes > FRCNN_COUNT_MAX_CLASSES)
        return fail(FRCNN_E_ARG, "%s: num_classes=%d not in [1, %d]", who, num_classes, FRCNN_COUNT_MAX_CLASSES);
    if (int rc = idt_expire_ok(who, expire, FRCNN_COUNT_MAX_EXPIRE)) return rc;
    if (int rc = ov_frame_ok(who, h, w)) return rc;
    k_count_update<<<1, IDT_THREADS, 0, as_stream(stream)>>>(state, capacity, tracked, tracked_stride, rows, frames, n_frames, gate, cl, classes,
                                                             num_classes, expire, h, w, lists);
    return check_launch(who);
}

extern "C" int frcnn_count_draw_u8(uint8_t* frame, int h, int w, const int32_t* list, const int32_t* lines, int n_lines, int width, int rgb,
                                   void* stream) {
    const char* who = "count_draw_u8";
    if (!frame || !list || !lines) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (int rc = ov_frame_ok(who, h, w)) return rc;
    CountLines cl;
    if (int rc = count_lines_ok(who, lines, n_lines, &cl)) return rc;
    if (int rc = ov_width_ok(who, width, FRCNN_COUNT_MAX_WIDTH)) return rc;
    k_count_draw<<<ov_grid(h, w), OV_THREADS, 0, as_stream(stream)>>>(frame, h, w, list, cl, width, rgb ? 1 : 0);
    return check_launch(who);
}
