// Polygon zones over the tracker's ids -- who is inside, who has been, how long they stayed -- and the zones and their figures drawn into
// the frames (include/ext/frcnn_hip_zone.h states the rule, DESIGN §8 "Zone rule").  gfx950 (CDNA4) only.
// k_zone_update: the id-table walk of csrc/id_table.h over the two-copy table, thirteen words an entry.  What is the zone rule's own: the
// row's thread tests its point against every zone -- the mask of zones is a function of the row alone, so the 64-bit edge tests run over
// the rows in parallel; a thread per ENTRY walks the compacted rows and steps through its own, leaving each row the bits that entered and
// left and the dwell of those that left.  A shuffle prefix over the rows' bit counts places the events in (row, zone) order, a second one
// over the expiring entries the LOST events behind them; the totals are per-zone wave reductions of what each entry's thread summed, the
// occupancy eight ballots.  Every word of a list, and at the end of the call of the state, is written by one thread with a plain store.
// No atomics.
// k_zone_draw: a gather over the tiles of csrc/overlay.h.  The first threads stage a zone each: its edges, whether its bounding box
// (occupied zones only: the fill) and its grown box (the outline) meet the tile, the label formatted in decimal and its box; a tile that
// nothing meets stores nothing.  A thread keeps a row-parity mask per zone: for an edge, (px - xi) dy is one 64-bit product and the
// sixteen rows of the tile step the other product down by dx, exactly.  Then the capsules of the outlines, the labels, and the store.
#include "id_table.h"
#include "overlay.h"
#include "../../include/ext/frcnn_hip_zone.h"

namespace frcnn {

constexpr int ZN_ZONES = FRCNN_ZONE_MAX_ZONES, ZN_VERTS = FRCNN_ZONE_MAX_VERTS;
constexpr int ZN_EVENTS = FRCNN_ZONE_MAX_EVENTS, ZN_HEAD = FRCNN_ZONE_HEAD_WORDS, ZN_ENTRY = FRCNN_ZONE_ENTRY_WORDS, ZN_LIST = FRCNN_ZONE_LIST_WORDS;
constexpr int ZN_LHEAD = 4 + 5 * ZN_ZONES;                                  // a list's words in front of its events
constexpr int ZN_TEXT = 24;                                                 // "Z7 2147483647/2147483647" is 24 characters
constexpr unsigned ZN_SAT = FRCNN_ZONE_MAX_DWELL;
enum { ZN_ID, ZN_CLS, ZN_SEEN, ZN_INSIDE, ZN_VISITED, ZN_SINCE };           // since[z] is word ZN_SINCE + z
static_assert(ZN_ZONES == 8 && ZN_ENTRY == 13 && ZN_HEAD == 36, "masks of eight bits");

struct ZoneSet {                                                            // passed by value as a kernel argument
    int n;
    int nv[ZN_ZONES];
    int v[ZN_ZONES * ZN_VERTS * 2];                                         // zone z's vertex i at v[2 (16 z + i)], (x, y)
};

// a + b for a, b in 0..2^30, stopping at 2^30: associative and commutative, so a sum of dwells can be taken in any grouping
__device__ inline unsigned zn_sat(unsigned a, unsigned b) { return min(a + b, ZN_SAT); }

// The vertices into LDS: s_v as ZoneSet::v, s_nv the counts (0 for the zones a call does not have).
__device__ inline void zn_stage(const ZoneSet& zs, int* s_v, int* s_nv) {
    for (int i = threadIdx.x; i < ZN_ZONES * ZN_VERTS * 2; i += IDT_THREADS) s_v[i] = zs.v[i];
    if (threadIdx.x < ZN_ZONES) s_nv[threadIdx.x] = (int)threadIdx.x < zs.n ? zs.nv[threadIdx.x] : 0;
}

// INSIDE of the polygon of ``nv`` vertices at ``v`` (x, y pairs in LDS; every thread of a wave reads the same word: a broadcast)
__device__ inline bool zn_inside(const int* v, int nv, int px, int py) {
    bool in = false;
    int xi = v[2 * nv - 2], yi = v[2 * nv - 1];                             // the edge (V_{nv-1}, V_0) first: the parity does not mind
    for (int j = 0; j < nv; ++j) {
        const int xj = v[2 * j], yj = v[2 * j + 1];
        if ((yi > py) != (yj > py)) {
            const long long dy = (long long)yj - yi;
            const long long t = ((long long)px - xi) * dy - ((long long)py - yi) * ((long long)xj - xi);
            in ^= dy > 0 ? t < 0 : t > 0;
        }
        xi = xj;
        yi = yj;
    }
    return in;
}

__global__ void __launch_bounds__(IDT_THREADS) k_zone_update(int32_t* state, int cap, const int32_t* tracked, long long stride, int R, int frames,
                                                               const int32_t* n_frames, const int32_t* gate, ZoneSet zs, const uint8_t* classes,
                                                               int nc, int anchor, int E, int h, int w, int32_t* lists) {
    __shared__ int s_tab[2][ZN_ENTRY][IDT_CAP];                             // the table, twice: a frame's survivors move to the other copy
    __shared__ int s_live[IDT_CAP];
    __shared__ int s_rid[IDT_ROWS], s_rcls[IDT_ROWS], s_rm[IDT_ROWS];       // the frame's eligible rows, in row order; their mask of zones
    __shared__ int s_rent[IDT_ROWS], s_rfirst[IDT_ROWS], s_rev[IDT_ROWS];   // their entry, the first row of their id, entered | left << 8
    __shared__ int s_rd[ZN_ZONES][IDT_ROWS];                                // the dwell of the zones a row left
    __shared__ int s_ev[5 * ZN_EVENTS], s_tot[4 * ZN_ZONES], s_occ[ZN_ZONES];
    __shared__ unsigned s_wacc[IDT_WAVES][2 * ZN_ZONES];
    __shared__ int s_wocc[IDT_WAVES][ZN_ZONES];
    __shared__ int s_v[ZN_ZONES * ZN_VERTS * 2], s_nv[ZN_ZONES];
    __shared__ int s_cnt[IDT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nf = idt_begin(gate, n_frames, frames, lists, ZN_LIST);
    if (nf <= 0) return;
    const int nz = zs.n;
    int ne = min(max(state[0], 0), cap), fr = state[1], dropped = state[2], evdrop = state[3], cur = 0;
    idt_load<ZN_ENTRY, ZN_HEAD>(state, ne, s_tab[0], s_tot);
    zn_stage(zs, s_v, s_nv);
    __syncthreads();
    for (int f = 0; f < nf; ++f) {
        fr += 1;
        int (*T)[IDT_CAP] = s_tab[cur];
        const IdRows rows = idt_rows(tracked, stride, f, R);
        int total;
        for (int i = tid; i < 5 * ZN_EVENTS; i += IDT_THREADS) s_ev[i] = 0;
        // the eligible rows, compacted in row order: the live ones of a class that is set, each with the mask of the zones its point is inside
        int m = 0;
        for (int base = 0; base < rows.n; base += IDT_THREADS) {
            const int r = base + tid;
            int rid = 0, rc = 0, rm = 0, xa = 0, xb = 0, ya = 0, yb = 0;
            bool ok = idt_live(rows, r, h, w, rid, xa, xb, ya, yb);
            if (ok) {
                rc = rows.cls[r];
                ok = idt_class_set(classes, nc, rc);
            }
            if (ok) {
                const int px = (xa + xb) >> 1, py = anchor ? yb : (ya + yb) >> 1;
                for (int z = 0; z < nz; ++z) rm |= (int)zn_inside(s_v + 2 * ZN_VERTS * z, s_nv[z], px, py) << z;
            }
            const int k = wg_append(ok, s_cnt, m);
            if (ok) {
                s_rid[k] = rid;
                s_rcls[k] = rc;
                s_rm[k] = rm;
            }
        }
        __syncthreads();
        for (int k = tid; k < m; k += IDT_THREADS) {
            idt_lookup(k, s_rid, T[ZN_ID], nullptr, ne, s_rent, s_rfirst);
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
                T[ZN_ID][e] = s_rid[k];
                T[ZN_CLS][e] = s_rcls[k];
                T[ZN_SEEN][e] = fr;
#pragma unroll
                for (int j = ZN_INSIDE; j < ZN_ENTRY; ++j) T[j][e] = 0;
            }
        }
        __syncthreads();
        const int nt = ne + min(births, nfree);
        dropped += idt_follow(m, s_rent, s_rfirst, s_cnt);
        __syncthreads();
        // STEP: a thread per entry takes its rows in row order, a new entry's first row included: it enters where it is first seen
        unsigned acc_n[ZN_ZONES], acc_d[ZN_ZONES];                          // new visitors | stays << 16, and the dwell, of this entry's events
#pragma unroll
        for (int z = 0; z < ZN_ZONES; ++z) acc_n[z] = acc_d[z] = 0;
        int ins = 0, gone = 0, my_id = 0, my_cls = 0, my_seen = 0;
        int since[ZN_ZONES];
#pragma unroll
        for (int z = 0; z < ZN_ZONES; ++z) since[z] = 0;
        if (tid < nt) {
            int vis = T[ZN_VISITED][tid];
            ins = T[ZN_INSIDE][tid];
            my_id = T[ZN_ID][tid];
            my_cls = T[ZN_CLS][tid];
            my_seen = T[ZN_SEEN][tid];
#pragma unroll
            for (int z = 0; z < ZN_ZONES; ++z) since[z] = T[ZN_SINCE + z][tid];
            for (int k = 0; k < m; ++k) {
                if (s_rent[k] != tid) continue;
                const int mk = s_rm[k], ent = mk & ~ins, ex = ins & ~mk;
#pragma unroll
                for (int z = 0; z < ZN_ZONES; ++z) {
                    if ((ent >> z) & 1) {                                   // ENTER
                        since[z] = fr;
                        if (!((vis >> z) & 1)) {                            // a visitor ONCE
                            vis |= 1 << z;
                            acc_n[z] += 1u;
                        }
                    } else if ((ex >> z) & 1) {                             // EXIT
                        const int d = fr - since[z];
                        s_rd[z][k] = d;
                        acc_n[z] += 1u << 16;
                        acc_d[z] = zn_sat(acc_d[z], min((unsigned)d, ZN_SAT));
                        since[z] = 0;
                    }
                }
                s_rev[k] = ent | (ex << 8);
                ins = mk;
                my_seen = fr;
            }
            const bool live = fr - my_seen <= E;                            // EXPIRE
            if (!live) {
                gone = ins;
#pragma unroll
                for (int z = 0; z < ZN_ZONES; ++z)
                    if ((gone >> z) & 1) {                                  // LOST: the stay ends with the frame it was last seen in
                        acc_n[z] += 1u << 16;
                        acc_d[z] = zn_sat(acc_d[z], min((unsigned)(my_seen - since[z] + 1), ZN_SAT));
                    }
            }
            T[ZN_SEEN][tid] = my_seen;
            T[ZN_INSIDE][tid] = ins;
            T[ZN_VISITED][tid] = vis;
#pragma unroll
            for (int z = 0; z < ZN_ZONES; ++z) T[ZN_SINCE + z][tid] = since[z];
            s_live[tid] = live;
        }
        __syncthreads();
        // the rows' events in (row, zone) order
        int nev = 0;
        for (int base = 0; base < m; base += IDT_THREADS) {
            const int k = base + tid;
            const int mask = k < m ? s_rev[k] : 0;
            int at = nev + wg_prefix(__popc(mask), s_cnt, total);
            if (mask && at < ZN_EVENTS) {
                const int rid = s_rid[k], ec = T[ZN_CLS][s_rent[k]];
                for (int z = 0; z < ZN_ZONES; ++z) {
                    const int enter = (mask >> z) & 1, leave = (mask >> (8 + z)) & 1;
                    if (!(enter | leave)) continue;
                    if (at < ZN_EVENTS) {
                        s_ev[5 * at] = z;
                        s_ev[5 * at + 1] = enter;
                        s_ev[5 * at + 2] = rid;
                        s_ev[5 * at + 3] = ec;
                        s_ev[5 * at + 4] = enter ? 0 : s_rd[z][k];
                    }
                    at += 1;
                }
            }
            nev += total;
        }
        // behind them the LOST events, in (id, zone) order: the entries that expire were in the table before this frame, in id order
        {
            int at = nev + wg_prefix(__popc(gone), s_cnt, total);
            if (gone && at < ZN_EVENTS)
                for (int z = 0; z < ZN_ZONES; ++z) {
                    if (!((gone >> z) & 1)) continue;
                    if (at < ZN_EVENTS) {
                        s_ev[5 * at] = z;
                        s_ev[5 * at + 1] = 2;
                        s_ev[5 * at + 2] = my_id;
                        s_ev[5 * at + 3] = my_cls;
                        s_ev[5 * at + 4] = my_seen - since[z] + 1;
                    }
                    at += 1;
                }
            nev += total;
        }
        evdrop += max(nev - ZN_EVENTS, 0);
        // the totals: a reduction per zone over the entries' sums (nev is the same for every thread), and the occupancy
        const bool live = tid < nt && s_live[tid];
        if (nev > 0) {
#pragma unroll
            for (int z = 0; z < ZN_ZONES; ++z) {
                unsigned a = acc_n[z], d = acc_d[z];
                for (int s = 32; s >= 1; s >>= 1) {
                    a += __shfl_xor(a, s);
                    d = zn_sat(d, __shfl_xor(d, s));
                }
                if (lane == 0) {
                    s_wacc[wave][z] = a;
                    s_wacc[wave][ZN_ZONES + z] = d;
                }
            }
        }
#pragma unroll
        for (int z = 0; z < ZN_ZONES; ++z) {
            const int c = __popcll(__ballot(live && ((ins >> z) & 1)));
            if (lane == 0) s_wocc[wave][z] = c;
        }
        __syncthreads();
        if (tid < ZN_ZONES) {
            int occ = 0;
            for (int k = 0; k < IDT_WAVES; ++k) occ += s_wocc[k][tid];
            if (nev > 0) {
                unsigned a = 0, d = (unsigned)min(max(s_tot[2 * ZN_ZONES + tid], 0), (int)ZN_SAT);
                for (int k = 0; k < IDT_WAVES; ++k) {
                    a += s_wacc[k][tid];
                    d = zn_sat(d, s_wacc[k][ZN_ZONES + tid]);
                }
                s_tot[tid] += (int)(a & 0xffffu);                           // visitors
                s_tot[ZN_ZONES + tid] += (int)(a >> 16);                    // stays
                s_tot[2 * ZN_ZONES + tid] = (int)d;                         // dwell
            }
            s_tot[3 * ZN_ZONES + tid] = max(s_tot[3 * ZN_ZONES + tid], occ);    // peak
            s_occ[tid] = occ;
        }
        ne = idt_compact<ZN_ENTRY>(nt, s_live, T, s_tab[cur ^ 1], s_cnt);  // (its barriers also publish s_ev, s_tot and s_occ)
        cur ^= 1;
        int32_t* L = lists + (long long)f * ZN_LIST;
        for (int i = tid; i < ZN_LIST; i += IDT_THREADS)
            L[i] = i == 0 ? min(nev, ZN_EVENTS) : i == 1 ? fr : i < 4 ? 0 : i < 4 + ZN_ZONES ? s_occ[i - 4] : i < ZN_LHEAD ? s_tot[i - 4 - ZN_ZONES]
                                                                                                                          : s_ev[i - ZN_LHEAD];
        __syncthreads();
    }
    idt_store<ZN_ENTRY, ZN_HEAD>(state, cap, ne, fr, dropped, evdrop, s_tot, s_tab[cur]);
}

__global__ void __launch_bounds__(OV_THREADS) k_zone_draw(uint8_t* frame, int h, int w, const int32_t* list, ZoneSet zs, int W, int rgb) {
    __shared__ int s_v[ZN_ZONES * ZN_VERTS * 2], s_nv[ZN_ZONES];
    __shared__ int s_hit[ZN_ZONES], s_x0[ZN_ZONES], s_y0[ZN_ZONES], s_len[ZN_ZONES];      // 1: the outline meets the tile, 2: the label box, 4: the fill
    __shared__ uint8_t s_txt[ZN_ZONES][ZN_TEXT];                            // the label's glyphs (OV_GLYPHS rows)
    if (list[1] <= 0) return;                                               // the list of a frame that is not real
    const int tid = threadIdx.x, nz = zs.n, g = ov_grow(W);
    const OvTile t = ov_tile(h, w);
    const int x = t.x, ty0 = t.ty0, ty1 = t.ty1;
    zn_stage(zs, s_v, s_nv);
    __syncthreads();
    if (tid < nz) {
        const int z = tid, nv = s_nv[z];
        const int* v = s_v + 2 * ZN_VERTS * z;
        int minx = v[0], maxx = v[0], miny = v[1], maxy = v[1];
        for (int i = 1; i < nv; ++i) {
            minx = min(minx, v[2 * i]);
            maxx = max(maxx, v[2 * i]);
            miny = min(miny, v[2 * i + 1]);
            maxy = max(maxy, v[2 * i + 1]);
        }
        int hit = ov_meets(minx, maxx, miny, maxy, g, t);
        const int occ = list[4 + z], visitors = list[4 + ZN_ZONES + z];
        if (occ > 0 && maxx >= t.tx0 && minx <= t.tx1 && maxy > ty0 && miny <= ty1) hit |= 4;   // (inside needs miny <= py < maxy)
        uint8_t* txt = s_txt[z];
        int n = 0;
        txt[n++] = OV_G_Z;
        txt[n++] = OV_G_0 + z;
        txt[n++] = OV_G_SPACE;
        n = ov_decimal(txt, n, occ);
        txt[n++] = OV_G_SLASH;
        n = ov_decimal(txt, n, visitors);
        int x0, y0;
        if (ov_label_place(n, (minx + maxx) >> 1, (miny + maxy) >> 1, h, w, t, x0, y0)) hit |= 2;
        s_hit[z] = hit;
        s_x0[z] = x0;
        s_y0[z] = y0;
        s_len[z] = n;
    }
    __syncthreads();
    int any = 0;
    for (int z = 0; z < nz; ++z) any |= s_hit[z];
    if (!any || t.j >= t.rowbytes) return;
    int col[OV_TILE_ROWS];                                                  // -1: untouched; 0..7: the palette; 8: black
    int fill[OV_TILE_ROWS];                                                 // -1, or the zone whose colour is blended in
#pragma unroll
    for (int r = 0; r < OV_TILE_ROWS; ++r) col[r] = fill[r] = -1;
    // FILL: the parity of the edges that count, a bit per row of the tile
    for (int z = 0; z < nz; ++z) {                                          // ascending: the highest occupied zone a pixel is inside stays
        if (!(s_hit[z] & 4)) continue;
        const int nv = s_nv[z];
        const int* v = s_v + 2 * ZN_VERTS * z;
        unsigned par = 0;
        int xi = v[2 * nv - 2], yi = v[2 * nv - 1];
        for (int e = 0; e < nv; ++e) {
            const int xj = v[2 * e], yj = v[2 * e + 1];
            if (max(yi, yj) > ty0 && min(yi, yj) <= ty1) {                  // (the same for every thread: some row of the tile may lie between)
                const long long dy = (long long)yj - yi, dx = (long long)xj - xi;
                long long q = ((long long)x - xi) * dy - ((long long)ty0 - yi) * dx;
                const bool up = dy > 0;
#pragma unroll
                for (int r = 0; r < OV_TILE_ROWS; ++r) {
                    const int py = ty0 + r;
                    const bool counts = ((yi > py) != (yj > py)) && (up ? q < 0 : q > 0);
                    par ^= (unsigned)counts << r;
                    q -= dx;
                }
            }
            xi = xj;
            yi = yj;
        }
#pragma unroll
        for (int r = 0; r < OV_TILE_ROWS; ++r)
            if ((par >> r) & 1) fill[r] = z;
    }
    // OUTLINE: a capsule around every edge
    for (int z = 0; z < nz; ++z) {                                          // ascending: the highest zone that covers a pixel stays
        if (!(s_hit[z] & 1)) continue;
        const int nv = s_nv[z];
        const int* v = s_v + 2 * ZN_VERTS * z;
        int ax = v[2 * nv - 2], ay = v[2 * nv - 1];
        for (int e = 0; e < nv; ++e) {
            const int bx = v[2 * e], by = v[2 * e + 1];
            if (ov_meets(min(ax, bx), max(ax, bx), min(ay, by), max(ay, by), g, t) && ov_column_near(ax, bx, g, x)) {
                const OvCapsule s = ov_capsule(ax, ay, bx, by, x, W);
#pragma unroll
                for (int r = 0; r < OV_TILE_ROWS; ++r) capsule_paint<true>(s, ty0 + r, col[r], z & 7);
            }
            ax = bx;
            ay = by;
        }
    }
    for (int z = 0; z < nz; ++z)                                            // the labels, above every outline, the highest box on top
        if (s_hit[z] & 2) ov_label_blit(s_txt[z], s_len[z], s_x0[z], s_y0[z], z & 7, t, col);
#pragma unroll
    for (int r = 0; r < OV_TILE_ROWS; ++r) {
        if (ty0 + r > ty1) continue;
        uint8_t* p = frame + (size_t)(ty0 + r) * t.rowbytes + t.j;
        if (col[r] >= 0)
            *p = col[r] == OV_COL_BLACK ? (uint8_t)0 : ov_colour(col[r], t.c, rgb);
        else if (fill[r] >= 0)
            *p = (uint8_t)((3 * (int)*p + (int)ov_colour(fill[r] & 7, t.c, rgb) + 2) >> 2);
    }
}

static int zone_set_ok(const char* who, const int32_t* verts, const int32_t* nv, int n_zones, ZoneSet* out) {
    if (n_zones < 1 || n_zones > FRCNN_ZONE_MAX_ZONES)
        return fail(FRCNN_E_ARG, "%s: n_zones=%d not in [1, %d]", who, n_zones, FRCNN_ZONE_MAX_ZONES);
    *out = ZoneSet{};
    out->n = n_zones;
    for (int z = 0; z < n_zones; ++z)                                       // (every count first: no vertex is read past a bad one)
        if (nv[z] < FRCNN_ZONE_MIN_VERTS || nv[z] > FRCNN_ZONE_MAX_VERTS)
            return fail(FRCNN_E_ARG, "%s: zone %d has %d vertices, not %d..%d", who, z, nv[z], FRCNN_ZONE_MIN_VERTS, FRCNN_ZONE_MAX_VERTS);
    const int32_t* p = verts;
    for (int z = 0; z < n_zones; ++z) {
        const int n = nv[z];
        out->nv[z] = n;
        for (int i = 0; i < 2 * n; ++i) {
            if (p[i] < FRCNN_ZONE_MIN_COORD || p[i] > FRCNN_ZONE_MAX_COORD)
                return fail(FRCNN_E_ARG, "%s: zone %d has the coordinate %d outside [%d, %d]", who, z, p[i], FRCNN_ZONE_MIN_COORD,
                            FRCNN_ZONE_MAX_COORD);
            out->v[2 * ZN_VERTS * z + i] = p[i];
        }
        for (int i = 0; i < n; ++i) {
            const int j = i + 1 == n ? 0 : i + 1;
            if (p[2 * i] == p[2 * j] && p[2 * i + 1] == p[2 * j + 1])
                return fail(FRCNN_E_ARG, "%s: zone %d has the vertices %d and %d both at (%d, %d)", who, z, i, j, p[2 * i], p[2 * i + 1]);
        }
        p += 2 * n;
    }
    return FRCNN_OK;
}

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_zone_version(void) { return FRCNN_ZONE_VERSION; }

extern "C" size_t frcnn_zone_list_words(void) { return FRCNN_ZONE_LIST_WORDS; }

extern "C" size_t frcnn_zone_state_bytes(int capacity) {
    return capacity >= 1 && capacity <= FRCNN_TRACK_MAX ? sizeof(int32_t) * (ZN_HEAD + (size_t)capacity * ZN_ENTRY) : 0;
}

extern "C" int frcnn_zone_update(int32_t* state, int capacity, const int32_t* tracked, long long tracked_stride, int rows, int frames,
                                 const int32_t* n_frames, const int32_t* gate, const int32_t* verts, const int32_t* nv, int n_zones,
                                 const uint8_t* classes, int num_classes, int anchor, int expire, int h, int w, int32_t* lists, void* stream) {
    const char* who = "zone_update";
    if (!state || !tracked || !n_frames || !verts || !nv || !classes || !lists) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (int rc = idt_call_ok(who, capacity, rows, frames, tracked_stride)) return rc;
    ZoneSet zs;
    if (int rc = zone_set_ok(who, verts, nv, n_zones, &zs)) return rc;
    if (num_classes < 1 || num_classes > FRCNN_ZONE_MAX_CLASSES)
        return fail(FRCNN_E_ARG, "%s: num_classes=%d not in [1, %d]", who, num_classes, FRCNN_ZONE_MAX_CLASSES);
    if (anchor != 0 && anchor != 1) return fail(FRCNN_E_ARG, "%s: anchor=%d is neither 0 (centre) nor 1 (bottom)", who, anchor);
    if (int rc = idt_expire_ok(who, expire, FRCNN_ZONE_MAX_EXPIRE)) return rc;
    if (int rc = ov_frame_ok(who, h, w)) return rc;
    k_zone_update<<<1, IDT_THREADS, 0, as_stream(stream)>>>(state, capacity, tracked, tracked_stride, rows, frames, n_frames, gate, zs, classes,
                                                            num_classes, anchor, expire, h, w, lists);
    return check_launch(who);
}

extern "C" int frcnn_zone_draw_u8(uint8_t* frame, int h, int w, const int32_t* list, const int32_t* verts, const int32_t* nv, int n_zones,
                                  int width, int rgb, void* stream) {
    const char* who = "zone_draw_u8";
    if (!frame || !list || !verts || !nv) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (int rc = ov_frame_ok(who, h, w)) return rc;
    ZoneSet zs;
    if (int rc = zone_set_ok(who, verts, nv, n_zones, &zs)) return rc;
    if (int rc = ov_width_ok(who, width, FRCNN_ZONE_MAX_WIDTH)) return rc;
    k_zone_draw<<<ov_grid(h, w), OV_THREADS, 0, as_stream(stream)>>>(frame, h, w, list, zs, width, rgb ? 1 : 0);
    return check_launch(who);
}
