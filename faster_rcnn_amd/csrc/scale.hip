// Frames scaled down by an exact area mean, the last step of the editing chain (include/ext/frcnn_hip_scale.h states the rule, DESIGN §8
// "Scale rule").  gfx950 (CDNA4) only.  Integers throughout, no atomics.
// k_downscale: tiles of 256 output byte columns x 4 output rows with threads as output bytes, as k_plate_fill and k_heat_draw and for
// their reason: a row of output bytes is one run of consecutive addresses.  The workgroup walks the source rows of its band from the top,
// a stage of them at a time: the bytes of the source pixels its columns read are copied into LDS by ALIGNED 16-byte loads -- a 3-byte
// pixel row starts at any byte, so a wave reads the aligned chunks that hold it, each fetched once, and a chunk that reaches over an end
// of the frame is put together from its bytes inside --, a thread forms the 32-bit horizontal sum of its column once per source row (first
// tap, a run of taps of weight W, last tap: at most 17) and adds it, times the row's weight, to the 64-bit sum of the output row the walk
// is at.  A source row is no longer than an output row, so it ends at most one output row and begins at most one: two sums are enough
// whatever the ratio, and the walk is uniform over the workgroup.  One 64-bit division per output byte.
// The 16x limit bounds the footprint: 256 byte columns meet at most 87 output pixels, those at most 87 * 16 + 1 source pixels, so a staged
// row is at most SC_MAX_PITCH bytes and the LDS tile has a static size (32 KiB: four workgroups a CU).
#include "common.h"
#include "../../include/ext/frcnn_hip_redact.h"
#include "../../include/ext/frcnn_hip_track.h"
#include "../../include/ext/frcnn_hip_scale.h"

namespace frcnn {

constexpr int SC_THREADS = 256, SC_WAVES = SC_THREADS / 64;
constexpr int SC_ROWS = 4;                                                  // output rows of a tile
constexpr int SC_LDS = 32768;
constexpr int SC_MAX_PIXELS = ((SC_THREADS + 1) / 3 + 2) * FRCNN_SCALE_MAX_RATIO + 1;   // source pixels under 256 byte columns, at most
constexpr int SC_MAX_PITCH = (3 * SC_MAX_PIXELS + 15 + 15) / 16 * 16;       // (the row's bytes behind up to 15 bytes of its first chunk)
static_assert(SC_MAX_PITCH <= SC_LDS, "a stage holds at least one source row");

// The aligned 16 bytes at q, of which only the bytes inside [lo, hi) exist.
__device__ inline uint4 scale_chunk(const uint8_t* q, const uint8_t* lo, const uint8_t* hi) {
    if (q >= lo && q + 16 <= hi) return *reinterpret_cast<const uint4*>(q);
    uint32_t v[4] = {0, 0, 0, 0};
    for (int i = 0; i < 16; ++i)
        if (q + i >= lo && q + i < hi) v[i >> 2] |= (uint32_t)q[i] << (8 * (i & 3));
    return make_uint4(v[0], v[1], v[2], v[3]);
}

__global__ void __launch_bounds__(SC_THREADS) k_downscale(const uint8_t* src, long long src_stride, int frames, const int32_t* n_frames, int h,
                                                            int w, uint8_t* dst, long long dst_stride, int H, int W) {
    __shared__ __align__(16) uint8_t s_tile[SC_LDS];
    const int f = blockIdx.z;
    if (n_frames && f >= min(max(*n_frames, 0), frames)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int outbytes = 3 * W, j0 = blockIdx.x * SC_THREADS, j = j0 + tid;
    const int Y0 = blockIdx.y * SC_ROWS, Y1 = min(Y0 + SC_ROWS, H) - 1;
    // the source pixels under the tile's columns: xs0 .. xs1
    const int tX0 = j0 / 3, tX1 = min(j0 + SC_THREADS - 1, outbytes - 1) / 3;
    const int xs0 = (int)(((long long)tX0 * w) / W), xs1 = (int)((((long long)tX1 + 1) * w + W - 1) / W) - 1;
    const int segbytes = 3 * (xs1 - xs0 + 1), pitch = (segbytes + 15 + 15) / 16 * 16;
    const int stage_rows = SC_LDS / pitch;                                  // (>= 1: pitch <= SC_MAX_PITCH)
    // this thread's column: taps xa .. xa + n - 1 with weights wf, W, ..., W, wl (n == 1: wf alone, and it is w)
    const bool mine = j < outbytes;
    const int X = min(j, outbytes - 1) / 3, c = min(j, outbytes - 1) - 3 * X;
    const long long Xw = (long long)X * w;
    const int xa = (int)(Xw / W), xb = (int)((Xw + w + W - 1) / W) - 1, n = xb - xa + 1;
    const int wf = (int)(min(Xw + w, ((long long)xa + 1) * W) - Xw), wl = (int)(Xw + w - (long long)xb * W);
    const int col = 3 * (xa - xs0) + c;
    const uint8_t* lo = src + (long long)f * src_stride;
    const uint8_t* hi = lo + 3 * (size_t)h * (size_t)w;
    const size_t rowbytes = 3 * (size_t)w;
    uint8_t* out = dst + (long long)f * dst_stride + j;
    const long long hw = (long long)h * w;
    // the source rows under the band: ys0 .. ys1
    const int ys0 = (int)(((long long)Y0 * h) / H), ys1 = (int)((((long long)Y1 + 1) * h + H - 1) / H) - 1;
    int Y = Y0;
    unsigned long long cur = 0;
    for (int base = ys0; base <= ys1 && Y <= Y1; base += stage_rows) {
        const int rows = min(stage_rows, ys1 - base + 1);
        for (int r = wave; r < rows; r += SC_WAVES) {                       // a wave copies a row's chunks
            const uint8_t* a = lo + (size_t)(base + r) * rowbytes + 3 * (size_t)xs0;
            const int sh = (int)(reinterpret_cast<uintptr_t>(a) & 15u), chunks = (sh + segbytes + 15) / 16;
            const uint8_t* q = a - sh;
            for (int k = lane; k < chunks; k += 64)
                *reinterpret_cast<uint4*>(s_tile + r * pitch + 16 * k) = scale_chunk(q + 16 * (size_t)k, lo, hi);
        }
        __syncthreads();
        for (int r = 0; r < rows && Y <= Y1; ++r) {
            const int y = base + r;
            const uint8_t* a = lo + (size_t)y * rowbytes + 3 * (size_t)xs0;
            const uint8_t* p = s_tile + r * pitch + (int)(reinterpret_cast<uintptr_t>(a) & 15u) + col;
            uint32_t hs = (uint32_t)wf * p[0];                              // below 255 w < 2^23
            if (n > 1) {
                uint32_t mid = 0;
                for (int t = 1; t < n - 1; ++t) mid += p[3 * t];
                hs += (uint32_t)W * mid + (uint32_t)wl * p[3 * (n - 1)];
            }
            const long long top = max((long long)Y * h, (long long)y * H), end = ((long long)y + 1) * H, Yend = ((long long)Y + 1) * h;
            cur += (unsigned long long)(min(Yend, end) - top) * hs;         // (y lies under Y: the weight is positive)
            if (end >= Yend) {                                              // y is the last source row of Y, and the first of Y + 1 when it reaches over
                if (mine) out[(size_t)Y * outbytes] = (uint8_t)((cur + (unsigned long long)(hw / 2)) / (unsigned long long)hw);
                cur = (unsigned long long)(end - Yend) * hs;
                ++Y;
            }
        }
        __syncthreads();                                                    // (the next stage overwrites the tile)
    }
}

static bool scale_side_ok(int v) { return v >= 1 && v <= FRCNN_REDACT_MAX_SIDE; }

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_scale_version(void) { return FRCNN_SCALE_VERSION; }

extern "C" int frcnn_downscale_u8(const uint8_t* src, long long src_stride, int frames, const int32_t* n_frames, int h, int w, uint8_t* dst,
                                  long long dst_stride, int H, int W, void* stream) {
    const char* who = "downscale_u8";
    if (!src || !dst) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (frames < 1 || frames > FRCNN_TRACK_MAX_FRAMES) return fail(FRCNN_E_ARG, "%s: frames=%d not in [1, %d]", who, frames, FRCNN_TRACK_MAX_FRAMES);
    if (!scale_side_ok(h) || !scale_side_ok(w))
        return fail(FRCNN_E_ARG, "%s: frame %dx%d out of range (sides 1..%d)", who, h, w, FRCNN_REDACT_MAX_SIDE);
    if (!scale_side_ok(H) || !scale_side_ok(W))
        return fail(FRCNN_E_ARG, "%s: output %dx%d out of range (sides 1..%d)", who, H, W, FRCNN_REDACT_MAX_SIDE);
    if (H > h || W > w) return fail(FRCNN_E_ARG, "%s: output %dx%d is larger than the frame %dx%d: this call only scales down", who, H, W, h, w);
    if ((long long)h > (long long)FRCNN_SCALE_MAX_RATIO * H || (long long)w > (long long)FRCNN_SCALE_MAX_RATIO * W)
        return fail(FRCNN_E_ARG, "%s: output %dx%d is less than 1/%d of the frame %dx%d along a side", who, H, W, FRCNN_SCALE_MAX_RATIO, h, w);
    if (frames > 1 && (src_stride < 3LL * h * w || dst_stride < 3LL * H * W))
        return fail(FRCNN_E_ARG, "%s: src_stride=%lld / dst_stride=%lld below a frame's bytes (%lld / %lld)", who, src_stride, dst_stride,
                    3LL * h * w, 3LL * H * W);
    if (frames == 1) src_stride = dst_stride = 0;
    k_downscale<<<dim3((3 * W + SC_THREADS - 1) / SC_THREADS, (H + SC_ROWS - 1) / SC_ROWS, frames), SC_THREADS, 0, as_stream(stream)>>>(
        src, src_stride, frames, n_frames, h, w, dst, dst_stride, H, W);
    return check_launch(who);
}
