// Static areas hidden in a frame (include/ext/frcnn_hip_redact_region.h states the rule, DESIGN §8 "Region rule"): polygons and a painted
// mask become a plane of weights ONCE per frame size, and every frame is blended under that plane with no detection row anywhere.
// gfx950 (CDNA4) only.
//   build, three launches:
//     1. k_region_raster: a thread per point of the domain padded by F on every side; the vertices are staged in LDS and every thread
//        of a wave reads the same word (a broadcast); the inside test is csrc/zone.hip's, in int64.  One byte per point: hard or not.
//     2. k_region_hdist: d1 of every (padded row, frame column), by a walk outwards over the hard bytes of the row, F + 1 for none.
//     3. k_region_weights: in the tiles of the apply kernel -- 256 byte columns x 16 rows, threads as bytes -- e from 2F + 1 bytes of d1,
//        W, the tile's flag (a workgroup OR: one writer) and the two counts (a wave sum, then one integer atomic per wave and count).
//   prepare: csrc/redact.hip's phase one through redact.h, with the plane's word 5, which is always 1, as its count word.
//   apply, one launch per frame: a workgroup whose flag is 0 returns; else every thread walks its byte column down the tile, loads W of
//     its pixel and blends; the vertical blur sum slides while consecutive rows have W > 0.  No LDS, one writer per byte, plain byte
//     stores, no atomics, no floats.
// The kernels of prepare and apply compare the plane's header with (h, w) and return without writing when it is another size's.
#include "redact_region.h"                                                  // (the plane: its header words and its layout)
#include "../../include/ext/frcnn_hip_zone.h"

namespace frcnn {

constexpr int RR_REGIONS = FRCNN_REDACT_REGION_MAX, RR_VERTS = FRCNN_ZONE_MAX_VERTS;

struct RegionSet {                                                          // passed by value as a kernel argument
    int n;
    int nv[RR_REGIONS];
    int v[RR_REGIONS * RR_VERTS * 2];                                       // region z's vertex i at v[2 (16 z + i)], (x, y)
};

// INSIDE of the polygon of ``nv`` vertices at ``v`` (x, y pairs in LDS): csrc/zone.hip's test, word for word
__device__ inline bool rr_inside(const int* v, int nv, int px, int py) {
    bool in = false;
    int xi = v[2 * nv - 2], yi = v[2 * nv - 1];
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

// build 1: hard[(y + F)][(x + F)] for the padded domain, and the header (its counts zeroed: build 3 sums into them)
__global__ void __launch_bounds__(RD_THREADS) k_region_raster(uint8_t* plane, int h, int w, int F, RegionSet rs, const uint8_t* mask) {
    __shared__ int s_v[RR_REGIONS * RR_VERTS * 2];
    __shared__ int s_nv[RR_REGIONS];
    for (int i = threadIdx.x; i < RR_REGIONS * RR_VERTS * 2; i += RD_THREADS) s_v[i] = rs.v[i];
    if (threadIdx.x < RR_REGIONS) s_nv[threadIdx.x] = (int)threadIdx.x < rs.n ? rs.nv[threadIdx.x] : 0;
    __syncthreads();
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < RR_HEAD) {
        const int t = threadIdx.x;
        ((int32_t*)plane)[t] = t == RR_H ? h : t == RR_W ? w : t == RR_F ? F : t == RR_ONE ? 1 : 0;
    }
    const int pw = w + 2 * F, col = blockIdx.x * RD_THREADS + threadIdx.x, row = blockIdx.y;
    if (col >= pw) return;
    const int px = col - F, py = row - F;
    bool hard = false;
    for (int z = 0; z < rs.n; ++z) hard |= rr_inside(s_v + 2 * RR_VERTS * z, s_nv[z], px, py);
    if (mask && px >= 0 && px < w && py >= 0 && py < h) hard |= mask[(size_t)py * w + px] >= 128;
    plane[region_layout(h, w).hard_at + (size_t)row * pw + col] = hard ? 1 : 0;
}

// build 2: d1[(y' + F)][x] for the padded rows and the frame's columns
__global__ void __launch_bounds__(RD_THREADS) k_region_hdist(uint8_t* plane, int h, int w, int F) {
    const int x = blockIdx.x * RD_THREADS + threadIdx.x, row = blockIdx.y;
    if (x >= w) return;
    const RegionLayout L = region_layout(h, w);
    const uint8_t* hard = plane + L.hard_at + (size_t)row * (w + 2 * F) + (x + F);      // columns x - F .. x + F of the frame lie inside the row
    int d = F + 1;
    for (int dx = 0; dx <= F; ++dx)
        if (hard[-dx] | hard[dx]) { d = dx; break; }
    plane[L.d1_at + (size_t)row * w + x] = (uint8_t)d;
}

// build 3: W, the tile flags and the counts, in the tiles of k_region_apply
__global__ void __launch_bounds__(RD_THREADS) k_region_weights(uint8_t* plane, int h, int w, int F) {
    const RegionLayout L = region_layout(h, w);
    const int rowbytes = 3 * w, j = blockIdx.x * RD_THREADS + threadIdx.x, y0 = blockIdx.y * RD_TILE_ROWS;
    const int y1 = min(y0 + RD_TILE_ROWS, h) - 1;
    const bool active = j < rowbytes;
    const int x = active ? j / 3 : 0, c = j - 3 * (j / 3);
    const uint8_t* d1 = plane + L.d1_at;
    uint16_t* Wp = (uint16_t*)(plane + L.w_at);
    int covered = 0, full = 0, any = 0;
    if (active) {
        for (int y = y0; y <= y1; ++y) {
            int e = F + 1;
            for (int dy = -F; dy <= F; ++dy)                                // padded rows y + dy + F, all inside [0, h + 2F)
                e = min(e, max((int)d1[(size_t)(y + dy + F) * w + x], abs(dy)));
            const int W = e == 0 ? 256 : e > F ? 0 : (256 * (F + 1 - e)) / (F + 1);
            any |= W;
            if (c == 0) {                                                   // a pixel's first byte owns its word and its count
                Wp[(size_t)y * w + x] = (uint16_t)W;
                covered += W > 0;
                full += W == 256;
            }
        }
    }
    const int flag = __syncthreads_or(any);
    if (threadIdx.x == 0) plane[L.flags_at + (size_t)blockIdx.y * gridDim.x + blockIdx.x] = flag ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) { covered += __shfl_xor(covered, o); full += __shfl_xor(full, o); }
    if ((threadIdx.x & 63) == 0) {
        if (covered) atomicAdd((int*)plane + RR_COVERED, covered);
        if (full) atomicAdd((int*)plane + RR_FULL, full);
    }
}

// the hot path: the bytes of a tile with W > 0 blended from the workspace and themselves
__global__ void __launch_bounds__(RD_THREADS) k_region_apply(uint8_t* frame, int h, int w, const uint8_t* plane, int mode, int size,
                                                               const uint8_t* ws) {
    const int32_t* head = (const int32_t*)plane;
    if (head[RR_H] != h || head[RR_W] != w) return;                         // (another size's plane: its layout is not this one)
    const RegionLayout L = region_layout(h, w);
    if (!plane[L.flags_at + (size_t)blockIdx.y * gridDim.x + blockIdx.x]) return;      // (the whole workgroup: one word, a broadcast)
    const int rowbytes = 3 * w, j = blockIdx.x * RD_THREADS + threadIdx.x, y0 = blockIdx.y * RD_TILE_ROWS;
    const int y1 = min(y0 + RD_TILE_ROWS, h) - 1;
    if (j >= rowbytes) return;
    const int x = j / 3, c = j - 3 * x;
    const uint16_t* Wp = (const uint16_t*)(plane + L.w_at);
    const int cw = mode == FRCNN_REDACT_PIXELATE ? (w + size - 1) / size : 0;
    const int k = 2 * size + 1;
    int sum = 0;
    bool running = false;                                                   // BLUR: ``sum`` is the window of the row above
    for (int y = y0; y <= y1; ++y) {
        const int W = Wp[(size_t)y * w + x];
        if (W == 0) { running = false; continue; }
        int R = 0;
        if (mode == FRCNN_REDACT_PIXELATE) {
            R = ws[((size_t)(y / size) * cw + x / size) * 3 + c];
        } else if (mode == FRCNN_REDACT_BLUR) {
            if (running) {                                                  // one row down: row y + r enters, row y - 1 - r leaves
                sum += (int)ws[(size_t)min(y + size, h - 1) * rowbytes + j] - (int)ws[(size_t)max(y - 1 - size, 0) * rowbytes + j];
            } else {
                sum = 0;
                for (int d = -size; d <= size; ++d) sum += ws[(size_t)min(max(y + d, 0), h - 1) * rowbytes + j];
                running = true;
            }
            R = (sum + k / 2) / k;
        }
        uint8_t* at = frame + (size_t)y * rowbytes + j;
        *at = (uint8_t)(W == 256 ? R : (W * R + (256 - W) * (int)*at + 128) >> 8);
    }
}

static int region_set_ok(const char* who, const int32_t* verts, const int32_t* nv, int n_regions, RegionSet* out) {
    *out = RegionSet{};
    out->n = n_regions;
    for (int z = 0; z < n_regions; ++z)                                     // (every count first: no vertex is read past a bad one)
        if (nv[z] < FRCNN_ZONE_MIN_VERTS || nv[z] > FRCNN_ZONE_MAX_VERTS)
            return fail(FRCNN_E_ARG, "%s: region %d has %d vertices, not %d..%d", who, z, nv[z], FRCNN_ZONE_MIN_VERTS, FRCNN_ZONE_MAX_VERTS);
    const int32_t* p = verts;
    for (int z = 0; z < n_regions; ++z) {
        const int n = nv[z];
        out->nv[z] = n;
        for (int i = 0; i < 2 * n; ++i) {
            if (p[i] < FRCNN_ZONE_MIN_COORD || p[i] > FRCNN_ZONE_MAX_COORD)
                return fail(FRCNN_E_ARG, "%s: region %d has the coordinate %d outside [%d, %d]", who, z, p[i], FRCNN_ZONE_MIN_COORD,
                            FRCNN_ZONE_MAX_COORD);
            out->v[2 * RR_VERTS * z + i] = p[i];
        }
        for (int i = 0; i < n; ++i) {
            const int j = i + 1 == n ? 0 : i + 1;
            if (p[2 * i] == p[2 * j] && p[2 * i + 1] == p[2 * j + 1])
                return fail(FRCNN_E_ARG, "%s: region %d has the vertices %d and %d both at (%d, %d)", who, z, i, j, p[2 * i], p[2 * i + 1]);
        }
        p += 2 * n;
    }
    return FRCNN_OK;
}

static bool side_ok(int h, int w) { return h >= 1 && h <= FRCNN_REDACT_MAX_SIDE && w >= 1 && w <= FRCNN_REDACT_MAX_SIDE; }

// what prepare and apply refuse
static int region_call_ok(const char* who, const void* frame, int h, int w, const void* plane, int mode, int size, const void* workspace,
                          size_t ws_bytes) {
    if (!frame || !plane) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (!side_ok(h, w)) return fail(FRCNN_E_ARG, "%s: frame %dx%d out of range (sides 1..%d)", who, h, w, FRCNN_REDACT_MAX_SIDE);
    if (mode != FRCNN_REDACT_FILL && mode != FRCNN_REDACT_PIXELATE && mode != FRCNN_REDACT_BLUR)
        return fail(FRCNN_E_ARG, "%s: mode=%d (0 fill, 1 pixelate, 2 blur)", who, mode);
    const bool ok = mode == FRCNN_REDACT_FILL       ? size == 0
                    : mode == FRCNN_REDACT_PIXELATE ? size >= FRCNN_REDACT_PIXELATE_MIN && size <= FRCNN_REDACT_PIXELATE_MAX
                                                    : size >= FRCNN_REDACT_BLUR_MIN && size <= FRCNN_REDACT_BLUR_MAX;
    if (!ok)
        return fail(FRCNN_E_ARG, "%s: size=%d out of range for mode %d (fill: 0, pixelate: %d..%d, blur: %d..%d)", who, size, mode,
                    FRCNN_REDACT_PIXELATE_MIN, FRCNN_REDACT_PIXELATE_MAX, FRCNN_REDACT_BLUR_MIN, FRCNN_REDACT_BLUR_MAX);
    const size_t need = frcnn_redact_ws_bytes(h, w, mode, size);
    if (need && !workspace) return fail(FRCNN_E_ARG, "%s: null workspace", who);
    if (ws_bytes < need) return fail(FRCNN_E_ARG, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
    return FRCNN_OK;
}

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_redact_region_version(void) { return FRCNN_REDACT_REGION_VERSION; }

extern "C" size_t frcnn_redact_region_plane_bytes(int h, int w) { return side_ok(h, w) ? region_layout(h, w).total : 0; }

extern "C" int frcnn_redact_region_build(void* plane, int h, int w, const int32_t* verts, const int32_t* nv, int n_regions,
                                         const uint8_t* mask, int feather, void* stream) {
    const char* who = "redact_region_build";
    if (!plane) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (!side_ok(h, w)) return fail(FRCNN_E_ARG, "%s: frame %dx%d out of range (sides 1..%d)", who, h, w, FRCNN_REDACT_MAX_SIDE);
    if (feather < 0 || feather > RR_FMAX) return fail(FRCNN_E_ARG, "%s: feather=%d not in [0, %d]", who, feather, RR_FMAX);
    if (n_regions < 0 || n_regions > RR_REGIONS) return fail(FRCNN_E_ARG, "%s: n_regions=%d not in [0, %d]", who, n_regions, RR_REGIONS);
    if (n_regions == 0 && !mask) return fail(FRCNN_E_ARG, "%s: neither a polygon nor a mask", who);
    if (n_regions > 0 && (!verts || !nv)) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    RegionSet rs;
    if (int rc = region_set_ok(who, verts, nv, n_regions, &rs)) return rc;
    hipStream_t st = as_stream(stream);
    uint8_t* p = (uint8_t*)plane;
    const int F = feather, ph = h + 2 * F, pw = w + 2 * F;
    k_region_raster<<<dim3((pw + RD_THREADS - 1) / RD_THREADS, ph), RD_THREADS, 0, st>>>(p, h, w, F, rs, mask);
    if (int rc = check_launch("redact_region_build (raster)")) return rc;
    k_region_hdist<<<dim3((w + RD_THREADS - 1) / RD_THREADS, ph), RD_THREADS, 0, st>>>(p, h, w, F);
    if (int rc = check_launch("redact_region_build (rows)")) return rc;
    k_region_weights<<<dim3((3 * w + RD_THREADS - 1) / RD_THREADS, (h + RD_TILE_ROWS - 1) / RD_TILE_ROWS), RD_THREADS, 0, st>>>(p, h, w, F);
    return check_launch("redact_region_build (weights)");
}

extern "C" int frcnn_redact_region_prepare(const uint8_t* frame, int h, int w, const void* plane, int mode, int size, void* workspace,
                                           size_t ws_bytes, void* stream) {
    if (int rc = region_call_ok("redact_region_prepare", frame, h, w, plane, mode, size, workspace, ws_bytes)) return rc;
    // the count word phase one wants: the plane's word 5, always 1
    return redact_phase_one("redact_region_prepare", frame, h, w, (const int32_t*)plane + RR_ONE, mode, size, workspace, as_stream(stream));
}

extern "C" int frcnn_redact_region_apply_u8(uint8_t* frame, int h, int w, const void* plane, int mode, int size, const void* workspace,
                                            size_t ws_bytes, void* stream) {
    if (int rc = region_call_ok("redact_region_apply_u8", frame, h, w, plane, mode, size, workspace, ws_bytes)) return rc;
    k_region_apply<<<dim3((3 * w + RD_THREADS - 1) / RD_THREADS, (h + RD_TILE_ROWS - 1) / RD_TILE_ROWS), RD_THREADS, 0, as_stream(stream)>>>(
        frame, h, w, (const uint8_t*)plane, mode, size, (const uint8_t*)workspace);
    return check_launch("redact_region_apply_u8");
}
