// Polygon zones over the tracker's ids -- who is inside, who has been, how long they stayed -- and the zones and their figures drawn into
// the frames (include/ext/frcnn_hip_zone.h states the rule, DESIGN §8 "Zone rule").  gfx950 (CDNA4) only.
// k_zone_update: count.hip's skeleton.  ONE workgroup walks the frames of a call in order with the table in LDS, thirteen words an entry,
// compacted in ascending id order, in two copies that take turns.  Inside a frame: the eligible rows are compacted in row order with
// wave64 ballots, and the row's thread tests its point against every zone -- the mask of zones is a function of the row alone, so the
// 64-bit edge tests run over the rows in parallel; each row finds its entry by binary search, the new ids are ranked with ballots and
// take the places behind the table; then a thread per ENTRY walks the compacted rows and steps through its own, leaving each row the
// bits that entered and left and the dwell of those that left.  A shuffle prefix over the rows' bit counts places the events in (row,
// zone) order, a second one over the expiring entries the LOST events behind them; the totals are per-zone wave reductions of what each
// entry's thread summed, the occupancy eight ballots.  Every word of a list, and at the end of the call of the state, is written by one
// thread with a plain store.  No atomics.
// k_zone_draw: a gather over tiles of 256 byte columns x 16 rows (threads are bytes).  The first threads stage a zone each: its edges,
// whether its bounding box (occupied zones only: the fill) and its grown box (the outline) meet the tile, the label formatted in
// decimal and its box; a tile that nothing meets stores nothing.  A thread keeps a row-parity mask per zone: for an edge, (px - xi) dy is
// one 64-bit product and the sixteen rows of the tile step the other product down by dx, exactly.
#include "common.h"
#include "../../include/ext/frcnn_hip_redact.h"
#include "../../include/ext/frcnn_hip_track.h"
#include "../../include/ext/frcnn_hip_zone.h"

namespace frcnn {

constexpr int ZN_THREADS = 256, ZN_WAVES = ZN_THREADS / 64;
constexpr int ZN_CAP = FRCNN_TRACK_MAX, ZN_ROWS = FRCNN_REDACT_MAX_ROWS, ZN_ZONES = FRCNN_ZONE_MAX_ZONES, ZN_VERTS = FRCNN_ZONE_MAX_VERTS;
constexpr int ZN_EVENTS = FRCNN_ZONE_MAX_EVENTS, ZN_HEAD = FRCNN_ZONE_HEAD_WORDS, ZN_ENTRY = FRCNN_ZONE_ENTRY_WORDS, ZN_LIST = FRCNN_ZONE_LIST_WORDS;
constexpr int ZN_LHEAD = 4 + 5 * ZN_ZONES;                                  // a list's words in front of its events
constexpr int ZN_TILE_ROWS = 16;
constexpr int ZN_TEXT = 24;                                                 // "Z7 2147483647/2147483647" is 24 characters
constexpr unsigned ZN_SAT = FRCNN_ZONE_MAX_DWELL;
enum { ZN_ID, ZN_CLS, ZN_SEEN, ZN_INSIDE, ZN_VISITED, ZN_SINCE };           // since[z] is word ZN_SINCE + z
static_assert(ZN_CAP <= ZN_THREADS && ZN_ZONES == 8 && ZN_ENTRY == 13 && ZN_HEAD == 36, "a thread per entry; masks of eight bits");

struct ZoneSet {                                                            // passed by value as a kernel argument
    int n;
    int nv[ZN_ZONES];
    int v[ZN_ZONES * ZN_VERTS * 2];                                         // zone z's vertex i at v[2 (16 z + i)], (x, y)
};

__constant__ uint8_t ZN_PALETTE[8][3] = {{255, 64, 64}, {64, 160, 255}, {255, 208, 0}, {255, 0, 255},
                                         {0, 224, 224}, {255, 128, 0}, {160, 96, 255}, {255, 255, 255}};
// the glyphs a label needs, rows as frcnn_annotate_u8's table has them (bit 4 = the leftmost column): ' ', '/', '0'..'9', 'Z'
enum { ZN_G_SPACE = 0, ZN_G_SLASH = 1, ZN_G_0 = 2, ZN_G_Z = 12 };
__constant__ uint8_t ZN_GLYPHS[13][7] = {
    {0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00}, {0x00, 0x01, 0x02, 0x04, 0x08, 0x10, 0x00},
    {0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E}, {0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E}, {0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F},
    {0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E}, {0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02}, {0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E},
    {0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E}, {0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08}, {0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E},
    {0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C}, {0x1F, 0x01, 0x02, 0x04, 0x08, 0x10, 0x1F}};

// The number of threads in front of this one, in thread order, whose ``flag`` is set, and ``total``, the workgroup's count.  Every thread
// of the workgroup calls it; ``s_cnt`` is free again when it returns.
__device__ inline int zn_rank(bool flag, int* s_cnt, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(flag);
    if (lane == 0) s_cnt[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < ZN_WAVES; ++k) {
        const int c = s_cnt[k];
        before += k < wave ? c : 0;
        all += c;
    }
    __syncthreads();
    total = all;
    return before + __popcll(mask & ((1ull << lane) - 1ull));
}

// The sum of ``v`` over the threads in front of this one, in thread order, and ``total``, the workgroup's sum.  As zn_rank.
__device__ inline int zn_prefix(int v, int* s_cnt, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    if (lane == 63) s_cnt[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < ZN_WAVES; ++k) {
        const int c = s_cnt[k];
        before += k < wave ? c : 0;
        all += c;
    }
    __syncthreads();
    total = all;
    return before + inc - v;
}

// a + b for a, b in 0..2^30, stopping at 2^30: associative and commutative, so a sum of dwells can be taken in any grouping
__device__ inline unsigned zn_sat(unsigned a, unsigned b) { return min(a + b, ZN_SAT); }

// The vertices into LDS: s_v as ZoneSet::v, s_nv the counts (0 for the zones a call does not have).
__device__ inline void zn_stage(const ZoneSet& zs, int* s_v, int* s_nv) {
    for (int i = threadIdx.x; i < ZN_ZONES * ZN_VERTS * 2; i += ZN_THREADS) s_v[i] = zs.v[i];
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

__global__ void __launch_bounds__(ZN_THREADS) k_zone_update(int32_t* state, int cap, const int32_t* tracked, long long stride, int R, int frames,
                                                              const int32_t* n_frames, const int32_t* gate, ZoneSet zs, const uint8_t* classes,
                                                              int nc, int anchor, int E, int h, int w, int32_t* lists) {
    __shared__ int s_tab[2][ZN_ENTRY][ZN_CAP];                              // the table, twice: a frame's survivors move to the other copy
    __shared__ int s_live[ZN_CAP];
    __shared__ int s_rid[ZN_ROWS], s_rcls[ZN_ROWS], s_rm[ZN_ROWS];          // the frame's eligible rows, in row order; their mask of zones
    __shared__ int s_rent[ZN_ROWS], s_rfirst[ZN_ROWS], s_rev[ZN_ROWS];      // their entry, the first row of their id, entered | left << 8
    __shared__ int s_rd[ZN_ZONES][ZN_ROWS];                                 // the dwell of the zones a row left
    __shared__ int s_ev[5 * ZN_EVENTS], s_tot[4 * ZN_ZONES], s_occ[ZN_ZONES];
    __shared__ unsigned s_wacc[ZN_WAVES][2 * ZN_ZONES];
    __shared__ int s_wocc[ZN_WAVES][ZN_ZONES];
    __shared__ int s_v[ZN_ZONES * ZN_VERTS * 2], s_nv[ZN_ZONES];
    __shared__ int s_cnt[ZN_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nf = gate && *gate == 0 ? 0 : min(max(*n_frames, 0), frames);
    for (long long i = (long long)nf * ZN_LIST + tid; i < (long long)frames * ZN_LIST; i += ZN_THREADS) lists[i] = 0;       // padding frames
    if (nf <= 0) return;
    const int nz = zs.n;
    int ne = min(max(state[0], 0), cap), fr = state[1], dropped = state[2], evdrop = state[3], cur = 0;
    if (tid < 4 * ZN_ZONES) s_tot[tid] = state[4 + tid];
    if (tid < ZN_CAP) {
        const bool live = tid < ne;
        const int32_t* e = state + ZN_HEAD + (size_t)(live ? tid : 0) * ZN_ENTRY;
#pragma unroll
        for (int j = 0; j < ZN_ENTRY; ++j) s_tab[0][j][tid] = live ? e[j] : 0;
    }
    zn_stage(zs, s_v, s_nv);
    __syncthreads();
    for (int f = 0; f < nf; ++f) {
        fr += 1;
        int (*T)[ZN_CAP] = s_tab[cur];
        const int32_t* buf = tracked + (long long)f * stride;
        const int nl = min(max(buf[1], 0), R);
        const int32_t *bbox = buf + 4, *cls = buf + 4 + 4 * R, *ids = buf + 4 + 6 * R;
        int total;
        for (int i = tid; i < 5 * ZN_EVENTS; i += ZN_THREADS) s_ev[i] = 0;
        // the eligible rows, compacted in row order, each with the mask of the zones its point is inside
        int m = 0;
        for (int base = 0; base < nl; base += ZN_THREADS) {
            const int r = base + tid;
            bool ok = false;
            int rid = 0, rc = 0, rm = 0;
            if (r < nl && (rid = ids[r]) >= 1) {
                const int x1 = bbox[4 * r], y1 = bbox[4 * r + 1], x2 = bbox[4 * r + 2], y2 = bbox[4 * r + 3];
                const int xa = max(min(x1, x2), 0), xb = min(max(x1, x2), w - 1), ya = max(min(y1, y2), 0), yb = min(max(y1, y2), h - 1);
                if (xa <= xb && ya <= yb) {
                    rc = cls[r];
                    ok = rc >= 0 && rc < nc && classes[rc] != 0;
                    if (ok) {
                        const int px = (xa + xb) >> 1, py = anchor ? yb : (ya + yb) >> 1;
                        for (int z = 0; z < nz; ++z) rm |= (int)zn_inside(s_v + 2 * ZN_VERTS * z, s_nv[z], px, py) << z;
                    }
                }
            }
            const int k = m + zn_rank(ok, s_cnt, total);
            if (ok) {
                s_rid[k] = rid;
                s_rcls[k] = rc;
                s_rm[k] = rm;
            }
            m += total;
        }
        __syncthreads();
        // each row's entry (its place in the table, or -1), and for a row without one the first row of the frame that has its id
        for (int k = tid; k < m; k += ZN_THREADS) {
            const int rid = s_rid[k];
            int lo = 0, hi = ne, found = -1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1, v = T[ZN_ID][mid];
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
        for (int base = 0; base < m; base += ZN_THREADS) {
            const int k = base + tid;
            const bool is_new = k < m && s_rent[k] < 0 && s_rfirst[k] == k;
            const int rank = births + zn_rank(is_new, s_cnt, total);
            if (is_new && rank < nfree) {
                const int e = ne + rank;
                s_rent[k] = e;
                T[ZN_ID][e] = s_rid[k];
                T[ZN_CLS][e] = s_rcls[k];
                T[ZN_SEEN][e] = fr;
#pragma unroll
                for (int j = ZN_INSIDE; j < ZN_ENTRY; ++j) T[j][e] = 0;
            }
            births += total;
        }
        __syncthreads();
        const int nt = ne + min(births, nfree);
        // later rows of a new id follow its first row; the rows left without an entry are counted
        for (int base = 0; base < m; base += ZN_THREADS) {
            const int k = base + tid;
            bool lost = false;
            if (k < m) {
                int e = s_rent[k];
                if (e < 0 && s_rfirst[k] != k) s_rent[k] = e = s_rent[s_rfirst[k]];     // (a first row's word: nobody writes it here)
                lost = e < 0;
            }
            zn_rank(lost, s_cnt, total);
            dropped += total;
        }
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
        for (int base = 0; base < m; base += ZN_THREADS) {
            const int k = base + tid;
            const int mask = k < m ? s_rev[k] : 0;
            int at = nev + zn_prefix(__popc(mask), s_cnt, total);
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
            int at = nev + zn_prefix(__popc(gone), s_cnt, total);
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
            for (int k = 0; k < ZN_WAVES; ++k) occ += s_wocc[k][tid];
            if (nev > 0) {
                unsigned a = 0, d = (unsigned)min(max(s_tot[2 * ZN_ZONES + tid], 0), (int)ZN_SAT);
                for (int k = 0; k < ZN_WAVES; ++k) {
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
        // the survivors, in id order, into the other copy
        if (live) {
            int pos = 0;
            for (int e = 0; e < nt; ++e) pos += s_live[e] && T[ZN_ID][e] < my_id;
#pragma unroll
            for (int j = 0; j < ZN_ENTRY; ++j) s_tab[cur ^ 1][j][pos] = T[j][tid];
        }
        zn_rank(live, s_cnt, ne);                                           // (its barriers also publish the copy, s_ev, s_tot and s_occ)
        cur ^= 1;
        int32_t* L = lists + (long long)f * ZN_LIST;
        for (int i = tid; i < ZN_LIST; i += ZN_THREADS)
            L[i] = i == 0 ? min(nev, ZN_EVENTS) : i == 1 ? fr : i < 4 ? 0 : i < 4 + ZN_ZONES ? s_occ[i - 4] : i < ZN_LHEAD ? s_tot[i - 4 - ZN_ZONES]
                                                                                                                          : s_ev[i - ZN_LHEAD];
        __syncthreads();
    }
    const int words = ZN_HEAD + cap * ZN_ENTRY;
    for (int i = tid; i < words; i += ZN_THREADS) {
        int v;
        if (i < 4) {
            v = i == 0 ? ne : i == 1 ? fr : i == 2 ? dropped : evdrop;
        } else if (i < ZN_HEAD) {
            v = s_tot[i - 4];
        } else {
            const int t = (i - ZN_HEAD) / ZN_ENTRY, j = (i - ZN_HEAD) - t * ZN_ENTRY;
            v = t < ne ? s_tab[cur][j][t] : 0;
        }
        state[i] = v;
    }
}

__global__ void __launch_bounds__(ZN_THREADS) k_zone_draw(uint8_t* frame, int h, int w, const int32_t* list, ZoneSet zs, int W, int rgb) {
    __shared__ int s_v[ZN_ZONES * ZN_VERTS * 2], s_nv[ZN_ZONES];
    __shared__ int s_hit[ZN_ZONES], s_x0[ZN_ZONES], s_y0[ZN_ZONES], s_len[ZN_ZONES];      // 1: the outline meets the tile, 2: the label box, 4: the fill
    __shared__ uint8_t s_txt[ZN_ZONES][ZN_TEXT];                            // the label's glyphs (ZN_GLYPHS rows)
    if (list[1] <= 0) return;                                               // the list of a frame that is not real
    const int tid = threadIdx.x, nz = zs.n;
    const int rowbytes = 3 * w, j0 = blockIdx.x * ZN_THREADS, ty0 = blockIdx.y * ZN_TILE_ROWS;
    const int ty1 = min(ty0 + ZN_TILE_ROWS, h) - 1;
    const int tx0 = j0 / 3, tx1 = min(j0 + ZN_THREADS - 1, rowbytes - 1) / 3;
    const int g = (W + 1) >> 1;
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
        int hit = maxx + g >= tx0 && minx - g <= tx1 && maxy + g >= ty0 && miny - g <= ty1;
        const int occ = list[4 + z], visitors = list[4 + ZN_ZONES + z];
        if (occ > 0 && maxx >= tx0 && minx <= tx1 && maxy > ty0 && miny <= ty1) hit |= 4;   // (inside needs miny <= py < maxy)
        uint8_t* t = s_txt[z];
        int n = 0;
        t[n++] = ZN_G_Z;
        t[n++] = ZN_G_0 + z;
        for (int d = 0; d < 2; ++d) {                                       // the occupancy, then the visitors
            t[n++] = d ? ZN_G_SLASH : ZN_G_SPACE;
            unsigned val = (unsigned)max(d ? visitors : occ, 0);
            int nd = 1;
            for (unsigned p = val; p >= 10u; p /= 10u) nd += 1;
            for (int i = nd - 1; i >= 0; --i) {
                t[n + i] = (uint8_t)(ZN_G_0 + val % 10u);
                val /= 10u;
            }
            n += nd;
        }
        const int bw = 12 * n, bh = 16, mx = (minx + maxx) >> 1, my = (miny + maxy) >> 1;
        const int x0 = bw <= w ? min(max(mx, 0), w - bw) : mx, y0 = bh <= h ? min(max(my, 0), h - bh) : my;
        if (x0 <= tx1 && x0 + bw - 1 >= tx0 && y0 <= ty1 && y0 + bh - 1 >= ty0) hit |= 2;
        s_hit[z] = hit;
        s_x0[z] = x0;
        s_y0[z] = y0;
        s_len[z] = n;
    }
    __syncthreads();
    int any = 0;
    for (int z = 0; z < nz; ++z) any |= s_hit[z];
    const int j = j0 + tid, x = j / 3, c = j - 3 * x;
    if (!any || j >= rowbytes) return;
    int col[ZN_TILE_ROWS];                                                  // -1: untouched; 0..7: the palette; 8: black
    int fill[ZN_TILE_ROWS];                                                 // -1, or the zone whose colour is blended in
#pragma unroll
    for (int r = 0; r < ZN_TILE_ROWS; ++r) col[r] = fill[r] = -1;
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
                long long t = ((long long)x - xi) * dy - ((long long)ty0 - yi) * dx;
                const bool up = dy > 0;
#pragma unroll
                for (int r = 0; r < ZN_TILE_ROWS; ++r) {
                    const int py = ty0 + r;
                    const bool counts = ((yi > py) != (yj > py)) && (up ? t < 0 : t > 0);
                    par ^= (unsigned)counts << r;
                    t -= dx;
                }
            }
            xi = xj;
            yi = yj;
        }
#pragma unroll
        for (int r = 0; r < ZN_TILE_ROWS; ++r)
            if ((par >> r) & 1) fill[r] = z;
    }
    // OUTLINE: the count rule's capsule around every edge
    const long long r2 = (long long)(W * W) >> 2;
    for (int z = 0; z < nz; ++z) {                                          // ascending: the highest zone that covers a pixel stays
        if (!(s_hit[z] & 1)) continue;
        const int nv = s_nv[z];
        const int* v = s_v + 2 * ZN_VERTS * z;
        int ax = v[2 * nv - 2], ay = v[2 * nv - 1];
        for (int e = 0; e < nv; ++e) {
            const int bx = v[2 * e], by = v[2 * e + 1];
            const bool near = max(ay, by) + g >= ty0 && min(ay, by) - g <= ty1 && max(ax, bx) + g >= tx0 && min(ax, bx) - g <= tx1;
            if (near && x >= min(ax, bx) - g && x <= max(ax, bx) + g) {
                const long long dx = (long long)bx - ax, dy = (long long)by - ay, dd = dx * dx + dy * dy;
                const long long px = (long long)x - ax, qx = (long long)x - bx, bound = ((long long)(W * W) * dd) >> 2;
#pragma unroll
                for (int r = 0; r < ZN_TILE_ROWS; ++r) {
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
                        cov = cr < (1LL << 31) && cr * cr <= bound;         // (bound <= 81 dd / 4 < 2^39: no cr >= 2^31 covers, and below it cr^2 < 2^62 fits)
                    }
                    if (cov) col[r] = z & 7;
                }
            }
            ax = bx;
            ay = by;
        }
    }
    for (int z = 0; z < nz; ++z) {                                          // the labels, above every outline, the highest box on top
        if (!(s_hit[z] & 2)) continue;
        const int rel = x - s_x0[z], y0 = s_y0[z];
        if (rel < 0 || rel >= 12 * s_len[z]) continue;
        const int k = (rel - 1) / 12, gx = (rel - 1) - 12 * k;
        const uint8_t* gl = ZN_GLYPHS[s_txt[z][rel >= 1 ? k : 0]];
#pragma unroll
        for (int r = 0; r < ZN_TILE_ROWS; ++r) {
            const int ry = ty0 + r - y0;
            if (ry < 0 || ry >= 16) continue;
            const bool ink = rel >= 1 && gx < 10 && ry >= 1 && ry <= 14 && ((gl[(ry - 1) >> 1] >> (4 - (gx >> 1))) & 1);
            col[r] = ink ? (z & 7) : 8;
        }
    }
#pragma unroll
    for (int r = 0; r < ZN_TILE_ROWS; ++r) {
        if (ty0 + r > ty1) continue;
        uint8_t* p = frame + (size_t)(ty0 + r) * rowbytes + j;
        if (col[r] >= 0)
            *p = col[r] == 8 ? (uint8_t)0 : ZN_PALETTE[col[r]][rgb ? c : 2 - c];
        else if (fill[r] >= 0)
            *p = (uint8_t)((3 * (int)*p + (int)ZN_PALETTE[fill[r] & 7][rgb ? c : 2 - c] + 2) >> 2);
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
    if (capacity < 1 || capacity > FRCNN_TRACK_MAX) return fail(FRCNN_E_ARG, "%s: capacity=%d not in [1, %d]", who, capacity, FRCNN_TRACK_MAX);
    if (rows < 1 || rows > FRCNN_REDACT_MAX_ROWS) return fail(FRCNN_E_ARG, "%s: rows=%d not in [1, %d]", who, rows, FRCNN_REDACT_MAX_ROWS);
    if (frames < 1 || frames > FRCNN_TRACK_MAX_FRAMES)
        return fail(FRCNN_E_ARG, "%s: frames=%d not in [1, %d]", who, frames, FRCNN_TRACK_MAX_FRAMES);
    if (frames > 1 && tracked_stride < 4 + 8LL * rows)
        return fail(FRCNN_E_ARG, "%s: tracked_stride=%lld under the %d words of a tracked buffer", who, tracked_stride, 4 + 8 * rows);
    ZoneSet zs;
    if (int rc = zone_set_ok(who, verts, nv, n_zones, &zs)) return rc;
    if (num_classes < 1 || num_classes > FRCNN_ZONE_MAX_CLASSES)
        return fail(FRCNN_E_ARG, "%s: num_classes=%d not in [1, %d]", who, num_classes, FRCNN_ZONE_MAX_CLASSES);
    if (anchor != 0 && anchor != 1) return fail(FRCNN_E_ARG, "%s: anchor=%d is neither 0 (centre) nor 1 (bottom)", who, anchor);
    if (expire < 0 || expire > FRCNN_ZONE_MAX_EXPIRE)
        return fail(FRCNN_E_ARG, "%s: expire=%d not in [0, %d]", who, expire, FRCNN_ZONE_MAX_EXPIRE);
    if (h < 1 || h > FRCNN_REDACT_MAX_SIDE || w < 1 || w > FRCNN_REDACT_MAX_SIDE)
        return fail(FRCNN_E_ARG, "%s: frame %dx%d out of range (sides 1..%d)", who, h, w, FRCNN_REDACT_MAX_SIDE);
    k_zone_update<<<1, ZN_THREADS, 0, as_stream(stream)>>>(state, capacity, tracked, tracked_stride, rows, frames, n_frames, gate, zs, classes,
                                                           num_classes, anchor, expire, h, w, lists);
    return check_launch(who);
}

extern "C" int frcnn_zone_draw_u8(uint8_t* frame, int h, int w, const int32_t* list, const int32_t* verts, const int32_t* nv, int n_zones,
                                  int width, int rgb, void* stream) {
    const char* who = "zone_draw_u8";
    if (!frame || !list || !verts || !nv) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (h < 1 || h > FRCNN_REDACT_MAX_SIDE || w < 1 || w > FRCNN_REDACT_MAX_SIDE)
        return fail(FRCNN_E_ARG, "%s: frame %dx%d out of range (sides 1..%d)", who, h, w, FRCNN_REDACT_MAX_SIDE);
    ZoneSet zs;
    if (int rc = zone_set_ok(who, verts, nv, n_zones, &zs)) return rc;
    if (width < 1 || width > FRCNN_ZONE_MAX_WIDTH) return fail(FRCNN_E_ARG, "%s: width=%d not in [1, %d]", who, width, FRCNN_ZONE_MAX_WIDTH);
    k_zone_draw<<<dim3((3 * w + ZN_THREADS - 1) / ZN_THREADS, (h + ZN_TILE_ROWS - 1) / ZN_TILE_ROWS), ZN_THREADS, 0, as_stream(stream)>>>(
        frame, h, w, list, zs, width, rgb ? 1 : 0);
    return check_launch(who);
}
