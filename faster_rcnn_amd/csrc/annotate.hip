// Detections drawn into a uint8 frame (annotate_video.py:32-41 of the reference: cv2.rectangle + cv2.putText in (0,255,0)).
// gfx950 (CDNA4) only.  One workgroup per detection row; every primitive has the one colour and nothing is blended, so the
// result is the source frame with the union of the painted pixels set to (0,255,0) whatever order the workgroups run in:
// overlapping writes store the same bytes.  The drawing rule (square corners, a 5x7 bitmap font at scale 2) is this
// project's and is stated in DESIGN §8; faster_rcnn_amd/annotate_video.py documents the same rule for callers.
#include "common.h"
#include "../../include/ext/frcnn_hip_track.h"
#include <math.h>

namespace frcnn {

constexpr int ANN_THREADS = 256;
constexpr int ANN_MAX_ROWS = 512;
constexpr int ANN_MAX_LABEL_STRIDE = 64;
// name (<= 63) + ' ' + the number: sign, up to 39 integer digits of a float32, '.', 2 decimals
constexpr int ANN_LABEL_MAX = 128;
constexpr int ANN_ID_MAX = 11;                                              // '#' + the ten digits of an int32 track id
static_assert(ANN_MAX_LABEL_STRIDE - 1 + ANN_ID_MAX + 1 + 44 <= ANN_LABEL_MAX, "the label buffer holds the longest label with an id");

__device__ __forceinline__ void paint(uint8_t* frame, int width, int x, int y) {
    uint8_t* p = frame + ((size_t)y * (size_t)width + (size_t)x) * 3;
    p[0] = 0; p[1] = 255; p[2] = 0;
}

// all pixels of the rectangle [x0, x1] x [y0, y1] inside the frame, strided over the workgroup
__device__ void paint_rect(uint8_t* frame, int height, int width, long long x0, long long x1, long long y0, long long y1) {
    x0 = x0 < 0 ? 0 : x0; y0 = y0 < 0 ? 0 : y0;
    x1 = x1 > width - 1 ? width - 1 : x1; y1 = y1 > height - 1 ? height - 1 : y1;
    if (x0 > x1 || y0 > y1) return;
    const int cols = (int)(x1 - x0 + 1), n = cols * (int)(y1 - y0 + 1);     // a strip: at most 3 x (frame side) pixels
    for (int i = threadIdx.x; i < n; i += blockDim.x) paint(frame, width, (int)x0 + i % cols, (int)y0 + i / cols);
}

// "{:6.2f}".format(p) for a float32 p: v = rint((double)p * 100) is exact (24 + 7 significant bits) and rounds half to even,
// as Python's correctly rounded .2f does; printed as v / 100 "." v % 100, right-aligned in 6 columns.  The integer can reach
// 3.4e40 (> 2^64): it is spelled out from 32-bit limbs.  One thread; ``out``, ``digits`` (48) and ``limb`` (6) are LDS
// (dynamically indexed arrays in registers would go to scratch).  Returns the length written (<= 44).
__device__ int format_prob(float p, char* out, char* digits, uint32_t* limb) {
    int nd = 0;                                                             // digits[] least significant first
    bool neg = false;
    if (isnan(p)) {
        digits[nd++] = 'n'; digits[nd++] = 'a'; digits[nd++] = 'n';       // (reversed below: "nan")
    } else if (isinf(p)) {
        digits[nd++] = 'f'; digits[nd++] = 'n'; digits[nd++] = 'i';
        neg = p < 0;
    } else {
        const double v = fabs(rint((double)p * 100.0));
        int e = 0;
        const double f = frexp(v, &e);                                      // v = f * 2^e, f in [0.5, 1) (0 for v = 0)
        const unsigned long long m = (unsigned long long)ldexp(f, 53);      // v = m * 2^(e - 53), m < 2^53
        const int shift = e - 53;
        for (int i = 0; i < 6; ++i) limb[i] = 0;                            // little-endian; v < 2^136
        if (shift <= 0) {
            const unsigned long long iv = m >> (-shift);                   // (exact: v is an integer)
            limb[0] = (uint32_t)iv; limb[1] = (uint32_t)(iv >> 32);
        } else {
            for (int b = 0; b < 53; ++b)
                if ((m >> b) & 1ull) { const int k = b + shift; if (k < 192) limb[k >> 5] |= 1u << (k & 31); }
        }
        bool nonzero = true;
        while ((nonzero || nd < 4) && nd < 46) {                            // at least "0.00"
            unsigned long long rem = 0;
            nonzero = false;
            for (int i = 5; i >= 0; --i) {
                const unsigned long long cur = (rem << 32) | limb[i];
                limb[i] = (uint32_t)(cur / 10u);
                rem = cur % 10u;
                nonzero |= limb[i] != 0;
            }
            digits[nd++] = (char)('0' + rem);
            if (nd == 2) digits[nd++] = '.';
        }
        neg = signbit(p);
    }
    const int n = nd + (neg ? 1 : 0);
    const int pad = n < 6 ? 6 - n : 0;
    int o = 0;
    for (int i = 0; i < pad; ++i) out[o++] = ' ';
    if (neg) out[o++] = '-';
    for (int i = nd - 1; i >= 0; --i) out[o++] = digits[i];
    return o;
}

__global__ void __launch_bounds__(ANN_THREADS) k_annotate_u8(uint8_t* frame, int height, int width, const int32_t* det_bbox,
                                                              const int32_t* det_cls, const float* det_prob, const int32_t* n_dets,
                                                              const uint8_t* drawable, const char* labels,
                                                              int label_stride, int num_classes, const uint8_t* glyphs,
                                                              const int32_t* det_id) {
    // det_id: the rows' track ids (frcnn_annotate_ids_u8), or null: no row has one
    // glyphs: printable ASCII 0x20..0x7E, 7 row bytes each, bit 4 = the leftmost column
    __shared__ char s_label[ANN_LABEL_MAX];
    __shared__ char s_digits[48];
    __shared__ uint32_t s_limb[6];
    __shared__ int s_len;
    const int row = blockIdx.x;
    const int nd = *n_dets;
    if (row >= nd) return;
    const int cls = det_cls[row];
    if (cls < 0 || cls >= num_classes || !drawable[cls]) return;           // 'DontCare' / 'Misc' (annotate_video.py:33-34)
    const int4 b = make_int4(det_bbox[4 * row], det_bbox[4 * row + 1], det_bbox[4 * row + 2], det_bbox[4 * row + 3]);
    // annotate_video.py:36-38, against the frame's own size
    if (b.x < 0 || b.z > width || b.y < 0 || b.w > height) return;

    // ---- the box: thickness 3 (h = 1) around the normalised corners, square ends
    const long long xa = min(b.x, b.z), xb = max(b.x, b.z), ya = min(b.y, b.w), yb = max(b.y, b.w);
    paint_rect(frame, height, width, xa - 1, xb + 1, ya - 1, ya + 1);
    paint_rect(frame, height, width, xa - 1, xb + 1, yb - 1, yb + 1);
    paint_rect(frame, height, width, xa - 1, xa + 1, ya - 1, yb + 1);
    paint_rect(frame, height, width, xb - 1, xb + 1, ya - 1, yb + 1);

    // ---- the label "{} {:6.2f}".format(cls_name, prob) at (x1, y2 + 16), formatted once per workgroup; "{}#{} {:6.2f}" with a track id
    if (threadIdx.x == 0) {
        const char* name = labels + (size_t)cls * label_stride;
        int n = 0;
        while (n < label_stride - 1 && name[n] != 0) { s_label[n] = name[n]; ++n; }
        const int id = det_id ? det_id[row] : 0;
        if (id > 0) {
            s_label[n++] = '#';
            int nd = 0;
            for (int v = id; v > 0; v /= 10) s_digits[nd++] = (char)('0' + v % 10);
            while (nd > 0) s_label[n++] = s_digits[--nd];
        }
        s_label[n++] = ' ';
        n += format_prob(det_prob[row], s_label + n, s_digits, s_limb);
        s_len = n;
    }
    __syncthreads();
    const int len = s_len;
    const long long ox = b.x, oy = (long long)b.w + 16 - 13;               // top of the glyph cell: baseline - 13
    // per character 10 x 14 pixels (5 x 7 bits at scale 2), advance 12
    for (int i = threadIdx.x; i < len * 140; i += blockDim.x) {
        const int k = i / 140, px = i % 140 % 10, py = i % 140 / 10;
        const long long x = ox + 12LL * k + px, y = oy + py;
        if (x < 0 || x >= width || y < 0 || y >= height) continue;
        int ch = (unsigned char)s_label[k];
        if (ch < 0x20 || ch > 0x7E) ch = '?';
        if ((glyphs[(ch - 0x20) * 7 + (py >> 1)] >> (4 - (px >> 1))) & 1) paint(frame, width, (int)x, (int)y);
    }
}

}  // namespace frcnn

using namespace frcnn;

extern "C" int frcnn_annotate_u8(uint8_t* frame, int height, int width, const int32_t* det_bbox, const int32_t* det_cls,
                                 const float* det_prob, const int32_t* n_dets, int max_rows, const uint8_t* drawable,
                                 const char* labels, int label_stride, int num_classes, const uint8_t* glyphs, void* stream) {
    if (!frame || !det_bbox || !det_cls || !det_prob || !n_dets || !drawable || !labels || !glyphs)
        return fail(FRCNN_E_ARG, "annotate_u8: null pointer");
    if (height <= 0 || width <= 0)
        return fail(FRCNN_E_ARG, "annotate_u8: frame %dx%d out of range", height, width);
    if (max_rows <= 0 || max_rows > ANN_MAX_ROWS) return fail(FRCNN_E_ARG, "annotate_u8: max_rows=%d not in [1, %d]", max_rows, ANN_MAX_ROWS);
    if (label_stride < 1 || label_stride > ANN_MAX_LABEL_STRIDE)
        return fail(FRCNN_E_ARG, "annotate_u8: label_stride=%d not in [1, %d]", label_stride, ANN_MAX_LABEL_STRIDE);
    if (num_classes <= 0 || num_classes > 256) return fail(FRCNN_E_ARG, "annotate_u8: num_classes=%d not in [1, 256]", num_classes);
    k_annotate_u8<<<max_rows, ANN_THREADS, 0, as_stream(stream)>>>(frame, height, width, det_bbox, det_cls, det_prob, n_dets,
                                                                     drawable, labels, label_stride, num_classes, glyphs, nullptr);
    return check_launch("annotate_u8");
}

extern "C" int frcnn_annotate_ids_u8(uint8_t* frame, int height, int width, const int32_t* det_bbox, const int32_t* det_cls,
                                     const float* det_prob, const int32_t* det_id, const int32_t* n_dets, int max_rows,
                                     const uint8_t* drawable, const char* labels, int label_stride, int num_classes, const uint8_t* glyphs,
                                     void* stream) {
    if (!det_id) return frcnn_annotate_u8(frame, height, width, det_bbox, det_cls, det_prob, n_dets, max_rows, drawable, labels, label_stride,
                                          num_classes, glyphs, stream);
    if (!frame || !det_bbox || !det_cls || !det_prob || !n_dets || !drawable || !labels || !glyphs)
        return fail(FRCNN_E_ARG, "annotate_ids_u8: null pointer");
    if (height <= 0 || width <= 0)
        return fail(FRCNN_E_ARG, "annotate_ids_u8: frame %dx%d out of range", height, width);
    if (max_rows <= 0 || max_rows > ANN_MAX_ROWS) return fail(FRCNN_E_ARG, "annotate_ids_u8: max_rows=%d not in [1, %d]", max_rows, ANN_MAX_ROWS);
    if (label_stride < 1 || label_stride > ANN_MAX_LABEL_STRIDE)
        return fail(FRCNN_E_ARG, "annotate_ids_u8: label_stride=%d not in [1, %d]", label_stride, ANN_MAX_LABEL_STRIDE);
    if (num_classes <= 0 || num_classes > 256) return fail(FRCNN_E_ARG, "annotate_ids_u8: num_classes=%d not in [1, 256]", num_classes);
    k_annotate_u8<<<max_rows, ANN_THREADS, 0, as_stream(stream)>>>(frame, height, width, det_bbox, det_cls, det_prob, n_dets,
                                                                     drawable, labels, label_stride, num_classes, glyphs, det_id);
    return check_launch("annotate_ids_u8");
}
