/* Soft-NMS and box voting in the detection post-process, opt-in: an EXTENSION of the C ABI of libfrcnn_hip.so (include/frcnn_hip.h and
 * the other extension headers stay as they are, and so do frcnn_detections and frcnn_detections_dyn).  Same library, same conventions
 * (int status, message via the library's last-error call, `stream` = hipStream_t or NULL), a revision of its own: a host that uses these
 * entry points checks frcnn_detect_post_version() == FRCNN_DETECT_POST_VERSION.
 *   1 = frcnn_detections_post, frcnn_detections_post_dyn.
 *
 * The rule (DESIGN §8 "Post-process rule"; docs/DETECTIONS_PARITY.md; tests/detections_post_ref.py restates it in numpy).
 *   ROWS    exactly frcnn_detections': the rows scored, the arg-max (first maximum), the background class and the f64 threshold
 *           comparison, the f64 decode with exp, the ranking by score descending and row ascending, the class order by first valid row.
 *           Each class is then worked on alone, over its valid rows in ranked order with their ORIGINAL decoded f64 boxes.
 *   IOU     of two boxes a, b: area = (x2 - x1 + 1) * (y2 - y1 + 1); w = max(0, min(a.x2, b.x2) - max(a.x1, b.x1) + 1), h likewise;
 *           inter = w * h; IoU = inter / (area_a + area_b - inter), every step in f64, no contraction.
 *   NMS     nms_mode FRCNN_NMS_HARD: the greedy rule of frcnn_detections (a row is dropped when !(IoU(pick, row) <= nms_thresh)),
 *           det_prob the row's own score; sigma is checked and min_score is not used.
 *           FRCNN_NMS_SOFT_LINEAR / FRCNN_NMS_SOFT_GAUSSIAN: s0_k = (double)score_k, s_k = s0_k, E_k = 0.0; repeat: among the class's rows
 *           not yet picked take the one with the largest s, the lower rank among equals; if s < min_score the class is finished;
 *           else emit it with det_prob = (float)s; then for every row k not yet picked, o = IoU(pick, k) and
 *             linear:   if !(o <= nms_thresh) s_k = s_k * (1.0 - o)
 *             gaussian: E_k = E_k + o * o;  s_k = s0_k * exp(-(E_k / sigma))       (ONE exp of a summed exponent, never a product)
 *           min_score < 0 stands for the image's det_threshold (the dyn entry: dyn[1]).
 *   VOTE    vote_iou v, 0 = off.  The box of an emitted row k becomes the mean of the ORIGINAL boxes b_j of all valid rows j of its class
 *           with IoU(b_k, b_j) >= v -- dropped and never-picked rows too, k itself always --, taken in ranked order with weight
 *           w_j = (double)score_j: acc[c] += w_j * b_j[c], ws += w_j, sequentially from 0.0; the box is (int)rint((acc[c] / ws) /
 *           resize_ratio).  With !(ws > 0) the row keeps its own box.  Scores, suppression and the pick order never see a voted box.
 *   DEGENERATE  a pair of boxes whose IoU is 0 / 0 (two boxes of area 0 at a distance: x2 = x1 - 1) has no defined decay; proposals have
 *           x2 >= x1 and y2 >= y1 and a decoded box keeps a positive width, so no such pair arises; what a NaN score does is NOT part of
 *           the rule, and the reference does not define it either.
 *   OUTPUT  frcnn_detections': classes by first valid row, pick order inside a class, rows past the last detection "empty".
 * The defaults a caller may want -- sigma 0.5, vote_iou 0.5, min_score = det_threshold -- are PROVISIONAL: their effect on mAP has not
 * been measured on a dataset. */
#ifndef FRCNN_HIP_DETECT_POST_H
#define FRCNN_HIP_DETECT_POST_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_DETECT_POST_VERSION 1
#define FRCNN_NMS_HARD 0
#define FRCNN_NMS_SOFT_LINEAR 1
#define FRCNN_NMS_SOFT_GAUSSIAN 2
int frcnn_detect_post_version(void);

/* frcnn_detections with the rule above: its arguments in its order, then nms_mode, sigma, min_score, vote_iou in front of `stream`.  ONE
 * launch of one workgroup (max_rows <= 512, num_classes <= 128), static LDS, no allocation, nothing read on the host: capturable.
 * FRCNN_E_ARG, with nothing launched: everything frcnn_detections refuses; nms_mode outside 0..2; nms_thresh outside [0, 1]; sigma not
 * > 0 or not finite; min_score > 1 or NaN; vote_iou < 0, > 1 or NaN. */
int frcnn_detections_post(const float* rois, const int32_t* n_rois, int max_rows, const float* out_cls, const float* out_reg,
                          int num_classes, int bg_idx, double det_threshold, double stride, double resize_ratio, double nms_thresh,
                          int32_t* det_cls, float* det_prob, int32_t* det_bbox, int32_t* det_roi, int32_t* n_dets,
                          int nms_mode, double sigma, double min_score, double vote_iou, void* stream);

/* frcnn_detections_dyn likewise: resize_ratio = dyn[0], det_threshold = dyn[1] (and min_score, when negative) read on the device. */
int frcnn_detections_post_dyn(const float* rois, const int32_t* n_rois, int roi_batch, int max_rows, const float* out_cls,
                              const float* out_reg, int num_classes, int bg_idx, double stride, double nms_thresh, const double* dyn,
                              int32_t* det_cls, float* det_prob, int32_t* det_bbox, int32_t* det_roi, int32_t* counts,
                              int nms_mode, double sigma, double min_score, double vote_iou, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_DETECT_POST_H */
