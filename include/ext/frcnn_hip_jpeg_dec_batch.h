/* The device JPEG decoder's batched form: an EXTENSION of the C ABI of libfrcnn_hip.so beside include/ext/frcnn_hip_jpeg_dec.h (the
 * single-file form, whose revision, symbols and files stay as they are; include/frcnn_hip.h likewise).  Same library, same conventions
 * (int status, message via frcnn_last_error, `stream` = hipStream_t or NULL), a revision of its own: a host that uses these entry points
 * checks frcnn_jpeg_dec_batch_version() == FRCNN_JPEG_DEC_BATCH_VERSION besides frcnn_jpeg_dec_version() and frcnn_version().
 *   1 = frcnn_jpeg_dec_batch_layout, frcnn_jpeg_decode_batch_u8. */
#ifndef FRCNN_HIP_JPEG_DEC_BATCH_H
#define FRCNN_HIP_JPEG_DEC_BATCH_H
#include "frcnn_hip_jpeg_dec.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_JPEG_DEC_BATCH_VERSION 1
#define FRCNN_JPEG_DEC_BATCH_MAX 64
int frcnn_jpeg_dec_batch_version(void);

/* One file of a batch: its plan (frcnn_jpeg_dec_plan) and where its bytes, its frame and its workspace region lie.  The files of a batch
 * may differ in size, components and sampling; two items may name the same file bytes, never the same output or workspace bytes. */
typedef struct frcnn_jpeg_dec_batch_item {
    frcnn_jpeg_dec_plan_t plan;
    uint64_t file_off;   /* bytes into files_dev; no alignment needed */
    uint64_t out_off;    /* bytes into out_dev; the item's [h][w][3] frame, contiguous */
    uint64_t ws_off;     /* bytes into workspace; 16-byte aligned */
} frcnn_jpeg_dec_batch_item_t;

/* ws_off[i] for n plans laid back to back (each region frcnn_jpeg_dec_workspace_bytes(&plans[i]), 16-byte aligned) -> the total bytes
 * of workspace; 0, with ws_off untouched, for a null pointer, n outside 1..FRCNN_JPEG_DEC_BATCH_MAX or a plan that
 * frcnn_jpeg_dec_workspace_bytes refuses.  A caller may also lay the regions out itself, further apart. */
size_t frcnn_jpeg_dec_batch_layout(const frcnn_jpeg_dec_plan_t* plans, int n, uint64_t* ws_off /* n, out */);

/* frcnn_jpeg_decode_u8 for n files in ONE set of four launches: item i's file at files_dev + file_off -> its frame at out_dev + out_off
 * (R,G,B per pixel, bgr != 0: B,G,R), its status bits ORed into status_dev[i] (FRCNN_JPEG_DEC_*: sticky, the caller clears the words),
 * its intermediates in workspace + ws_off.  items_host (HOST memory) is validated and sizes the grids; the kernels read items_dev
 * (DEVICE memory, 8-byte aligned): the caller uploads THE SAME n * sizeof(item) BYTES on `stream` in front of the call and keeps
 * them unchanged until the launches have run.  What the kernels' bounds rest on is checked on items_host, so a device table that
 * differs from it voids them.
 *
 * Per item everything the single-file form promises holds: whatever the bytes of its scan are, nothing is read outside its file or
 * written outside its workspace region and its output range, a damaged item yields a non-zero status word (its frame is then
 * UNDEFINED) and leaves the other items' frames exact.  Four launches on `stream`: no allocation, no synchronisation, nothing read on
 * the host, whatever n is.
 *
 * Cost in the worst case: the single-file bound (frcnn_hip_jpeg_dec.h: up to `subsequences` rounds of `subsequence_bytes` on a lane,
 * at most 16 MiB of serial symbol decoding), reached CONCURRENTLY per item: the entropy kernel runs one workgroup per item, each on a
 * CU of its own while there are CUs, so a batch costs what its slowest item costs, not the sum.  The grids of the other three kernels
 * are sized by the batch's largest item; workgroups past a smaller item's extent return at once.
 *
 * FRCNN_E_ARG, with nothing launched and no device call made: a null pointer; n outside 1..FRCNN_JPEG_DEC_BATCH_MAX; a plan whose
 * fields contradict each other; file_off + file_len > files_capacity, out_off + h * w * 3 > out_capacity or ws_off +
 * frcnn_jpeg_dec_workspace_bytes(plan) > workspace_capacity; a ws_off or workspace that is not 16-byte aligned, a status_dev that is not
 * 4-byte aligned, an items_dev that is not 8-byte aligned; two items whose output ranges or workspace regions overlap. */
int frcnn_jpeg_decode_batch_u8(const frcnn_jpeg_dec_batch_item_t* items_host, const frcnn_jpeg_dec_batch_item_t* items_dev, int n,
                               const uint8_t* files_dev, size_t files_capacity, int bgr, uint8_t* out_dev, size_t out_capacity,
                               int32_t* status_dev /* n words */, void* workspace, size_t workspace_capacity, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_JPEG_DEC_BATCH_H */
