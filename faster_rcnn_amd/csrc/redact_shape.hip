// Shaped redaction (include/ext/frcnn_hip_redact_shape.h states the rule, DESIGN §8 "Shape rule"): frcnn_redact_u8 with an elliptical
// mask and a soft edge that ramps OUTWARDS over F pixels.  gfx950 (CDNA4) only.  Phase one is csrc/redact.hip's (redact.h): the cell
// means or the horizontal blur stage H of the whole frame in the workspace.  Phase two is this unit's, in the same tiles of 256 byte
// columns x 16 rows with threads as bytes:
//   1. the workgroup collects the eligible rows whose grown box PLUS F meets its tile, 256 rows a round by wave64 ballots (the list keeps
//      the order of the rows; usually it is empty, and the workgroup is done);
//   2. for an ELLIPSE row the 128-bit test is not made per byte: for each of the tile's 16 rows y and each e in 0..F the REACH -- the
//      largest |u| inside the ellipse grown by e at that y, -1 for none -- is found once per tile by bisection and kept in LDS.  The
//      reaches of a row at one y do not fall with e, so a byte finds its e by bisection over F + 1 ints; it starts at the byte's BOX
//      distance, which the ellipse's never undercuts (the ellipse grown by e lies inside the box grown by e).  The table holds 4096 ints,
//      that is 4096 / (16 (F + 1)) rows (7 at F = 32): a longer list goes through it in rounds, the smallest e of every byte staying in
//      registers;
//   3. every thread walks its byte column down the tile and blends out = (W R + (256 - W) S + 128) >> 8 where W > 0.
// LDS: 8 KiB list + 512 B kinds + 16 KiB reaches = 25 120 B, six workgroups to a CU's 160 KiB.  One writer per byte, plain byte stores, no
// atomics, no floats, nothing read on the host; with *n_dets <= 0 the kernel returns at once.
#include "redact.h"
#include "../../include/ext/frcnn_hip_redact_shape.h"

namespace frcnn {

constexpr int RS_TABLE = 4096;                                              // ints of the reach table
constexpr int RS_FAR = 1 << 30;                                             // list coordinates are clamped to +-RS_FAR (see below)

// The largest u >= 0 with u^2 Be^2 + v^2 Ae^2 <= Ae^2 Be^2, -1 when there is none (v^2 > Be^2).  1 <= Ae, Be <= 131 136: the products
// pass 2^64 for large boxes, so they are compared in 128 bits there, and in 64 where Ae Be < 2^32.
__device__ inline int ellipse_reach(long long Ae, long long Be, long long v) {
    const unsigned long long A2 = (unsigned long long)(Ae * Ae), B2 = (unsigned long long)(Be * Be), v2 = (unsigned long long)(v * v);
    if (v2 > B2) return -1;
    long long lo = 0, hi = Ae;                                              // (u = 0 is inside; u = Ae + 1 never is)
    if (Ae * Be <= 0xFFFFFFFFLL) {
        const unsigned long long rhs = A2 * (B2 - v2);
        while (lo < hi) {
            const long long mid = (lo + hi + 1) >> 1;
            if ((unsigned long long)(mid * mid) * B2 <= rhs) lo = mid; else hi = mid - 1;
        }
    } else {
        const unsigned __int128 rhs = (unsigned __int128)A2 * (B2 - v2);
        while (lo < hi) {
            const long long mid = (lo + hi + 1) >> 1;
            if ((unsigned __int128)(unsigned long long)(mid * mid) * B2 <= rhs) lo = mid; else hi = mid - 1;
        }
    }
    return (int)lo;
}

// phase two: the bytes of a tile with W > 0 blended from the workspace and themselves
__global__ void __launch_bounds__(RD_THREADS) k_redact_shape_apply(uint8_t* frame, int h, int w, const int32_t* det_bbox, const int32_t* det_cls,
                                                                     const int32_t* n_dets, int max_rows, const uint8_t* redact,
                                                                     int num_classes, int mode, int size, int margin, int shape, int F,
                                                                     const uint8_t* ws) {
    __shared__ int4 s_box[FRCNN_REDACT_MAX_ROWS];                           // (X0, X1, Y0, Y1) of the grown boxes whose ring meets this tile
    __shared__ uint8_t s_ell[FRCNN_REDACT_MAX_ROWS];                        // 1: an ELLIPSE row
    __shared__ int s_reach[RS_TABLE];                                       // [row of the round][tile row][e]
    __shared__ int s_cnt[2][RD_THREADS / 64];
    const int nd = min(*n_dets, max_rows);
    if (nd <= 0) return;
    const int rowbytes = 3 * w, j0 = blockIdx.x * RD_THREADS, y0 = blockIdx.y * RD_TILE_ROWS;
    const int y1 = min(y0 + RD_TILE_ROWS, h) - 1;
    const int tx0 = j0 / 3, tx1 = min(j0 + RD_THREADS - 1, rowbytes - 1) / 3;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int nb = 0;
    for (int first = 0, round = 0; first < nd; first += RD_THREADS, ++round) {          // (nd is the workgroup's: every thread takes every round)
        const int row = first + threadIdx.x;
        bool hit = false, ell = false;
        int4 q = make_int4(0, 0, 0, 0);
        if (row < nd) {
            const int cls = det_cls[row];
            if (cls >= 0 && cls < num_classes && redact[cls]) {
                const long long x1 = det_bbox[4 * row], ya1 = det_bbox[4 * row + 1], x2 = det_bbox[4 * row + 2], ya2 = det_bbox[4 * row + 3];
                const long long X0 = min(x1, x2) - margin, X1 = max(x1, x2) + margin, Y0 = min(ya1, ya2) - margin, Y1 = max(ya1, ya2) + margin;
                hit = X0 - F <= tx1 && X1 + F >= tx0 && Y0 - F <= y1 && Y1 + F >= y0;
                ell = shape == FRCNN_REDACT_SHAPE_ELLIPSE && X1 - X0 + 1 <= FRCNN_REDACT_SHAPE_MAX_SIDE && Y1 - Y0 + 1 <= FRCNN_REDACT_SHAPE_MAX_SIDE;
                // a row that hits has X0 <= tx1 + F and X1 >= tx0 - F: the far side, clamped, is as far from every pixel of the frame as
                // the BOX distance can tell, and an ELLIPSE row, whose sides are bounded, is never clamped
                q = make_int4((int)max(X0, -(long long)RS_FAR), (int)min(X1, (long long)RS_FAR), (int)max(Y0, -(long long)RS_FAR),
                              (int)min(Y1, (long long)RS_FAR));
            }
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) s_cnt[round & 1][wave] = __popcll(m);
        __syncthreads();                                                    // (the round after the next writes these counts again, behind the next one's barrier)
        int at = nb;
        for (int k = 0; k < RD_THREADS / 64; ++k) {
            const int c = s_cnt[round & 1][k];
            at += k < wave ? c : 0;
            nb += c;
        }
        if (hit) {
            const int p = at + __popcll(m & ((1ull << lane) - 1ull));       // p < nb <= nd <= FRCNN_REDACT_MAX_ROWS
            s_box[p] = q;
            s_ell[p] = ell ? 1 : 0;
        }
    }
    if (nb == 0) return;                                                    // (the whole workgroup)
    __syncthreads();
    const int j = j0 + threadIdx.x;
    const bool active = j < rowbytes;                                       // (an idle thread still builds the table and meets the barriers)
    const int x = j / 3, c = j - 3 * x;
    const int per = RD_TILE_ROWS * (F + 1);                                 // ints of the table per row
    const int chunk = shape == FRCNN_REDACT_SHAPE_ELLIPSE ? RS_TABLE / per : nb;
    int emin[RD_TILE_ROWS];                                                 // the smallest e of this byte in each row of the tile; F + 1: none
#pragma unroll
    for (int yi = 0; yi < RD_TILE_ROWS; ++yi) emin[yi] = F + 1;
    for (int c0 = 0; c0 < nb; c0 += chunk) {
        const int cn = min(chunk, nb - c0);
        if (shape == FRCNN_REDACT_SHAPE_ELLIPSE) {
            if (c0) __syncthreads();                                        // the table of the round before is read no more
            for (int i = threadIdx.x; i < cn * per; i += RD_THREADS) {
                const int b = i / per, rem = i - b * per, yi = rem / (F + 1), e = rem - yi * (F + 1);
                if (!s_ell[c0 + b]) continue;
                const int4 q = s_box[c0 + b];
                s_reach[i] = ellipse_reach((long long)q.y - q.x + 1 + 2 * e, (long long)q.w - q.z + 1 + 2 * e,
                                           2LL * (y0 + yi) - ((long long)q.z + q.w));
            }
            __syncthreads();
        }
        if (!active) continue;
        for (int b = 0; b < cn; ++b) {
            const int4 q = s_box[c0 + b];
            const int ex = max(max(q.x - x, x - q.y), 0);
            if (ex > F) continue;
            const bool ell = s_ell[c0 + b];
            const int au = abs(2 * x - (q.x + q.y));                        // (read for ELLIPSE rows only, whose coordinates are small)
            const int* reach = s_reach + b * per;
#pragma unroll
            for (int yi = 0; yi < RD_TILE_ROWS; ++yi) {
                const int y = y0 + yi;
                int lo = max(ex, max(q.z - y, y - q.w)), hi = emin[yi];
                if (lo >= hi) continue;                                     // (the ELLIPSE distance is at least the BOX distance)
                if (ell) {
                    const int* t = reach + yi * (F + 1);
                    while (lo < hi) {                                       // the first e in [lo, hi) with au <= t[e], hi for none
                        const int mid = (lo + hi) >> 1;
                        if (au <= t[mid]) hi = mid; else lo = mid + 1;
                    }
                }
                emin[yi] = lo;
            }
        }
    }
    if (!active) return;
    const int cw = mode == FRCNN_REDACT_PIXELATE ? (w + size - 1) / size : 0;
    const int k = 2 * size + 1;
    int sum = 0;
    bool running = false;                                                   // BLUR: ``sum`` is the window of the row above
#pragma unroll
    for (int yi = 0; yi < RD_TILE_ROWS; ++yi) {
        const int y = y0 + yi, e = emin[yi];
        if (y > y1 || e > F) { running = false; continue; }
        const int W = e == 0 ? 256 : (256 * (F + 1 - e)) / (F + 1);       // > 0 up to e = F
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

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_redact_shape_version(void) { return FRCNN_REDACT_SHAPE_VERSION; }

extern "C" int frcnn_redact_shaped_u8(uint8_t* frame, int h, int w, const int32_t* det_bbox, const int32_t* det_cls, const int32_t* n_dets,
                                      int max_rows, const uint8_t* redact, int num_classes, int mode, int size, int margin, int shape,
                                      int feather, void* workspace, size_t ws_bytes, void* stream) {
    if (int rc = redact_check("redact_shaped_u8", frame, h, w, det_bbox, det_cls, n_dets, max_rows, redact, num_classes, mode, size, margin,
                              workspace, ws_bytes))
        return rc;
    if (shape != FRCNN_REDACT_SHAPE_BOX && shape != FRCNN_REDACT_SHAPE_ELLIPSE)
        return fail(FRCNN_E_ARG, "redact_shaped_u8: shape=%d (0 box, 1 ellipse)", shape);
    if (feather < 0 || feather > FRCNN_REDACT_FEATHER_MAX)
        return fail(FRCNN_E_ARG, "redact_shaped_u8: feather=%d not in [0, %d]", feather, FRCNN_REDACT_FEATHER_MAX);
    hipStream_t st = as_stream(stream);
    if (int rc = redact_phase_one("redact_shaped_u8", frame, h, w, n_dets, mode, size, workspace, st)) return rc;
    const int col_blocks = (3 * w + RD_THREADS - 1) / RD_THREADS;
    k_redact_shape_apply<<<dim3(col_blocks, (h + RD_TILE_ROWS - 1) / RD_TILE_ROWS), RD_THREADS, 0, st>>>(
        frame, h, w, det_bbox, det_cls, n_dets, max_rows, redact, num_classes, mode, size, margin, shape, feather, (const uint8_t*)workspace);
    return check_launch("redact_shaped_u8");
}
