// Detected objects hidden in a uint8 frame (include/ext/frcnn_hip_redact.h states the rule, DESIGN §8 "Redaction rule"): the union of
// the clipped boxes of the redacted classes is replaced by zeros, by the means of a pixel grid's cells or by a box blur.  gfx950 (CDNA4)
// only.  What replaces a pixel is a function of the SOURCE frame alone, so the call has two phases: phase one reads the frame and writes
// the workspace (the cell means, or the horizontal half H of the blur, for the whole frame), phase two is a pass over the frame that
// replaces the masked pixels from the workspace and never reads the frame.  Phase two works in tiles of 256 byte columns x 16 rows: a
// workgroup first collects the rows whose box meets its tile (from the device's *n_dets; usually none, and the workgroup is done), then
// each thread walks its byte column down the tile.  Threads are bytes, not pixels: a row is 3w bytes with no alignment to speak of, and
// 64 lanes on 64 consecutive bytes are one coalesced access wherever the row starts.  Every output byte has one writer.
#include "redact.h"

namespace frcnn {

constexpr int RD_HALO = 3 * FRCNN_REDACT_BLUR_MAX;                          // bytes of a row on either side of a blur window's centre

// phase one, PIXELATE: a wave per cell; cells[(i * cw + j) * 3 + c] = the rounded mean of channel c over cell (i, j)
__global__ void __launch_bounds__(RD_THREADS) k_redact_cells(const uint8_t* frame, int h, int w, const int32_t* n_dets, int P, int ch,
                                                               int cw, uint8_t* cells) {
    if (*n_dets <= 0) return;                                               // (phase two will read nothing)
    const long long cell = (long long)blockIdx.x * (RD_THREADS / 64) + (threadIdx.x >> 6);
    if (cell >= (long long)ch * cw) return;                                 // (the whole wave)
    const int lane = threadIdx.x & 63;
    const int y0 = (int)(cell / cw) * P, x0 = (int)(cell % cw) * P;
    const int rows = min(P, h - y0), cols = min(P, w - x0);
    const int rb = cols * 3, total = rows * rb;                             // <= 64 * 64 * 3 bytes
    const size_t stride = (size_t)w * 3;
    const uint8_t* base = frame + (size_t)y0 * stride + (size_t)x0 * 3;
    uint32_t s0 = 0, s1 = 0, s2 = 0;
    for (int i = lane; i < total; i += 64) {
        const int ry = i / rb, b = i - ry * rb;
        const uint32_t v = base[(size_t)ry * stride + b];
        const int c = b % 3;
        s0 += c == 0 ? v : 0u; s1 += c == 1 ? v : 0u; s2 += c == 2 ? v : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
    if (lane < 3) {
        const uint32_t n = (uint32_t)(rows * cols), s = lane == 0 ? s0 : (lane == 1 ? s1 : s2);
        cells[(size_t)cell * 3 + lane] = (uint8_t)((s + n / 2) / n);
    }
}

// phase one, BLUR: H, the horizontal box sums of a row segment of 256 bytes, from the segment and its halo staged in LDS (x clamped)
__global__ void __launch_bounds__(RD_THREADS) k_redact_hblur(const uint8_t* frame, int h, int w, const int32_t* n_dets, int r, uint8_t* H) {
    __shared__ uint8_t s_row[RD_THREADS + 2 * RD_HALO];
    if (*n_dets <= 0) return;
    const int rowbytes = 3 * w, j0 = blockIdx.x * RD_THREADS;
    const size_t at = (size_t)blockIdx.y * (size_t)rowbytes;
    const uint8_t* row = frame + at;
    for (int i = threadIdx.x; i < RD_THREADS + 6 * r; i += RD_THREADS) {
        const int p = j0 - 3 * r + i + 3 * 64;                              // byte position in the row + 3 * 64: never negative (3r <= 96)
        const int x = min(max(p / 3 - 64, 0), w - 1);
        s_row[i] = row[3 * x + p % 3];
    }
    __syncthreads();
    const int j = j0 + threadIdx.x;
    if (j >= rowbytes) return;
    uint32_t sum = 0;
    for (int d = 0; d <= 2 * r; ++d) sum += s_row[threadIdx.x + 3 * d];    // the taps x - r .. x + r of this byte's channel
    const uint32_t k = 2u * r + 1u;
    H[at + j] = (uint8_t)((sum + k / 2) / k);
}

// phase two: the masked bytes of a tile replaced from the workspace
__global__ void __launch_bounds__(RD_THREADS) k_redact_apply(uint8_t* frame, int h, int w, const int32_t* det_bbox, const int32_t* det_cls,
                                                               const int32_t* n_dets, int max_rows, const uint8_t* redact, int num_classes,
                                                               int mode, int size, int margin, const uint8_t* ws) {
    __shared__ int4 s_box[FRCNN_REDACT_MAX_ROWS];                           // (xa, xb, ya, yb) of the boxes that meet this tile
    __shared__ int s_n;
    const int nd = min(*n_dets, max_rows);
    if (nd <= 0) return;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const int rowbytes = 3 * w, j0 = blockIdx.x * RD_THREADS, y0 = blockIdx.y * RD_TILE_ROWS;
    const int y1 = min(y0 + RD_TILE_ROWS, h) - 1;
    const int tx0 = j0 / 3, tx1 = min(j0 + RD_THREADS - 1, rowbytes - 1) / 3;
    for (int row = threadIdx.x; row < nd; row += RD_THREADS) {
        const int cls = det_cls[row];
        if (cls < 0 || cls >= num_classes || !redact[cls]) continue;
        const long long x1 = det_bbox[4 * row], ya1 = det_bbox[4 * row + 1], x2 = det_bbox[4 * row + 2], ya2 = det_bbox[4 * row + 3];
        const long long xa = max(min(x1, x2) - margin, 0LL), xb = min(max(x1, x2) + margin, (long long)w - 1);
        const long long ya = max(min(ya1, ya2) - margin, 0LL), yb = min(max(ya1, ya2) + margin, (long long)h - 1);
        if (xa > xb || ya > yb) continue;                                   // nothing of it inside the frame
        if (xb < tx0 || xa > tx1 || yb < y0 || ya > y1) continue;
        s_box[atomicAdd(&s_n, 1)] = make_int4((int)xa, (int)xb, (int)ya, (int)yb);     // (an LDS counter; the list's order does not matter)
    }
    __syncthreads();
    const int nb = s_n, j = j0 + threadIdx.x;
    if (nb == 0 || j >= rowbytes) return;
    const int x = j / 3, c = j - 3 * x;
    const int cw = mode == FRCNN_REDACT_PIXELATE ? (w + size - 1) / size : 0;
    const int k = 2 * size + 1;
    int sum = 0;
    bool running = false;                                                   // BLUR: ``sum`` is the window of the row above
    for (int y = y0; y <= y1; ++y) {
        bool masked = false;
        for (int b = 0; b < nb; ++b) {
            const int4 q = s_box[b];
            masked |= x >= q.x && x <= q.y && y >= q.z && y <= q.w;
        }
        if (!masked) { running = false; continue; }
        uint8_t v = 0;
        if (mode == FRCNN_REDACT_PIXELATE) {
            v = ws[((size_t)(y / size) * cw + x / size) * 3 + c];
        } else if (mode == FRCNN_REDACT_BLUR) {
            if (running) {                                                  // one row down: row y + r enters, row y - 1 - r leaves
                sum += (int)ws[(size_t)min(y + size, h - 1) * rowbytes + j] - (int)ws[(size_t)max(y - 1 - size, 0) * rowbytes + j];
            } else {
                sum = 0;
                for (int d = -size; d <= size; ++d) sum += ws[(size_t)min(max(y + d, 0), h - 1) * rowbytes + j];
                running = true;
            }
            v = (uint8_t)((sum + k / 2) / k);
        }
        frame[(size_t)y * rowbytes + j] = v;
    }
}

static bool size_ok(int mode, int size) {
    if (mode == FRCNN_REDACT_FILL) return size == 0;
    if (mode == FRCNN_REDACT_PIXELATE) return size >= FRCNN_REDACT_PIXELATE_MIN && size <= FRCNN_REDACT_PIXELATE_MAX;
    if (mode == FRCNN_REDACT_BLUR) return size >= FRCNN_REDACT_BLUR_MIN && size <= FRCNN_REDACT_BLUR_MAX;
    return false;
}

int redact_check(const char* who, const uint8_t* frame, int h, int w, const int32_t* det_bbox, const int32_t* det_cls, const int32_t* n_dets,
                 int max_rows, const uint8_t* redact, int num_classes, int mode, int size, int margin, const void* workspace,
                 size_t ws_bytes) {
    if (!frame || !det_bbox || !det_cls || !n_dets || !redact) return fail(FRCNN_E_ARG, "%s: null pointer", who);
    if (h < 1 || h > FRCNN_REDACT_MAX_SIDE || w < 1 || w > FRCNN_REDACT_MAX_SIDE)
        return fail(FRCNN_E_ARG, "%s: frame %dx%d out of range (sides 1..%d)", who, h, w, FRCNN_REDACT_MAX_SIDE);
    if (max_rows <= 0 || max_rows > FRCNN_REDACT_MAX_ROWS)
        return fail(FRCNN_E_ARG, "%s: max_rows=%d not in [1, %d]", who, max_rows, FRCNN_REDACT_MAX_ROWS);
    if (num_classes <= 0 || num_classes > 256) return fail(FRCNN_E_ARG, "%s: num_classes=%d not in [1, 256]", who, num_classes);
    if (mode != FRCNN_REDACT_FILL && mode != FRCNN_REDACT_PIXELATE && mode != FRCNN_REDACT_BLUR)
        return fail(FRCNN_E_ARG, "%s: mode=%d (0 fill, 1 pixelate, 2 blur)", who, mode);
    if (!size_ok(mode, size))
        return fail(FRCNN_E_ARG, "%s: size=%d out of range for mode %d (fill: 0, pixelate: %d..%d, blur: %d..%d)", who, size, mode,
                    FRCNN_REDACT_PIXELATE_MIN, FRCNN_REDACT_PIXELATE_MAX, FRCNN_REDACT_BLUR_MIN, FRCNN_REDACT_BLUR_MAX);
    if (margin < 0) return fail(FRCNN_E_ARG, "%s: margin=%d is negative", who, margin);
    const size_t need = frcnn_redact_ws_bytes(h, w, mode, size);
    if (need && !workspace) return fail(FRCNN_E_ARG, "%s: null workspace", who);
    if (ws_bytes < need) return fail(FRCNN_E_ARG, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
    return FRCNN_OK;
}

int redact_phase_one(const char* who, const uint8_t* frame, int h, int w, const int32_t* n_dets, int mode, int size, void* workspace,
                     hipStream_t st) {
    char what[64];
    if (mode == FRCNN_REDACT_PIXELATE) {
        const int ch = (h + size - 1) / size, cw = (w + size - 1) / size;
        const long long cells = (long long)ch * cw;
        const unsigned blocks = (unsigned)((cells + RD_THREADS / 64 - 1) / (RD_THREADS / 64));
        k_redact_cells<<<blocks, RD_THREADS, 0, st>>>(frame, h, w, n_dets, size, ch, cw, (uint8_t*)workspace);
        snprintf(what, sizeof what, "%s (cells)", who);
        return check_launch(what);
    }
    if (mode == FRCNN_REDACT_BLUR) {
        k_redact_hblur<<<dim3((3 * w + RD_THREADS - 1) / RD_THREADS, h), RD_THREADS, 0, st>>>(frame, h, w, n_dets, size, (uint8_t*)workspace);
        snprintf(what, sizeof what, "%s (rows)", who);
        return check_launch(what);
    }
    return FRCNN_OK;
}

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_redact_version(void) { return FRCNN_REDACT_VERSION; }

extern "C" size_t frcnn_redact_ws_bytes(int h, int w, int mode, int size) {
    if (h < 1 || h > FRCNN_REDACT_MAX_SIDE || w < 1 || w > FRCNN_REDACT_MAX_SIDE || !size_ok(mode, size)) return 0;
    if (mode == FRCNN_REDACT_PIXELATE) return (size_t)((h + size - 1) / size) * (size_t)((w + size - 1) / size) * 3;
    if (mode == FRCNN_REDACT_BLUR) return (size_t)h * (size_t)w * 3;
    return 0;
}

extern "C" int frcnn_redact_u8(uint8_t* frame, int h, int w, const int32_t* det_bbox, const int32_t* det_cls, const int32_t* n_dets,
                               int max_rows, const uint8_t* redact, int num_classes, int mode, int size, int margin, void* workspace,
                               size_t ws_bytes, void* stream) {
    if (int rc = redact_check("redact_u8", frame, h, w, det_bbox, det_cls, n_dets, max_rows, redact, num_classes, mode, size, margin, workspace,
                              ws_bytes))
        return rc;
    hipStream_t st = as_stream(stream);
    if (int rc = redact_phase_one("redact_u8", frame, h, w, n_dets, mode, size, workspace, st)) return rc;
    const int col_blocks = (3 * w + RD_THREADS - 1) / RD_THREADS;
    k_redact_apply<<<dim3(col_blocks, (h + RD_TILE_ROWS - 1) / RD_TILE_ROWS), RD_THREADS, 0, st>>>(
        frame, h, w, det_bbox, det_cls, n_dets, max_rows, redact, num_classes, mode, size, margin, (const uint8_t*)workspace);
    return check_launch("redact_u8");
}
