/* YUV4MPEG2 (.y4m) frames on the device: an EXTENSION of the C ABI of libfrcnn_hip.so (include/frcnn_hip.h and the other extension
 * headers stay as they are).  Same library, same conventions (int status, message via frcnn_last_error, `stream` = hipStream_t or
 * NULL), a revision of its own: a host that uses these entry points checks frcnn_y4m_version() == FRCNN_Y4M_VERSION.
 *   1 = frcnn_y4m_frame_bytes, frcnn_y4m_decode_batch_u8, frcnn_y4m_decode_u8, frcnn_y4m_encode_u8.
 *
 * A y4m frame is raw planar Y'CbCr, 8 bits per sample, rows unpadded: [Y: h x w | Cb | Cr], the chroma planes ceil(w / 2) wide and /
 * or ceil(h / 2) high by the stream's chroma mode.  The header (text) is parsed on the host; what is left per frame is per-pixel work:
 * chroma upsampling and a colour matrix on the way in, the inverse matrix and chroma downsampling on the way out.  Integers only:
 *
 *   upsampling  a CENTRED axis takes libjpeg's triangle filter: (3 a + b + bias) >> 2 with a the nearer and b the farther sample, bias
 *               1 towards the lower index and 2 towards the higher, 9-3-3-1 over 16 with biases 8 / 7 where both axes are centred
 *               (h2v2); a CO-SITED axis takes the sample itself at even positions and (c[i] + c[i + 1] + 1) >> 1 at odd ones; edges
 *               replicate.  C420MPEG2 filters vertically first ((3 a + b + bias) >> 2 per chroma column), then horizontally.
 *   downsampling (420JPEG) the 2x2 box average of the per-pixel Cb / Cr, (sum + bias) >> 2, bias 1 at even and 2 at odd chroma columns;
 *               a frame's last column / row repeats into a group that reaches past it.
 *   colour, FULL range: the JFIF matrices with 16 fractional bits, as the library's JPEG encoder and decoder compute them.
 *   colour, LIMITED range (BT.601: Y 16..235, Cb Cr 16..240), coefficients rounded once from the reals to 16 fractional bits:
 *       R = clamp((76309 (Y - 16)                     + 104597 (Cr - 128) + 32768) >> 16)
 *       G = clamp((76309 (Y - 16) -  25675 (Cb - 128) -  53279 (Cr - 128) + 32768) >> 16)
 *       B = clamp((76309 (Y - 16) + 132201 (Cb - 128)                     + 32768) >> 16)
 *       Y  = clamp( 16 + (( 16829 R + 33039 G +  6416 B + 32768) >> 16))
 *       Cb = clamp(128 + (( -9714 R - 19071 G + 28784 B + 32768) >> 16))
 *       Cr = clamp(128 + (( 28784 R - 24103 G -  4681 B + 32768) >> 16))
 *   (>> of a negative sum rounds towards minus infinity; clamp to 0..255.)  CMONO decodes with Cb = Cr = 128. */
#ifndef FRCNN_HIP_Y4M_H
#define FRCNN_HIP_Y4M_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_Y4M_VERSION 1
#define FRCNN_Y4M_BATCH_MAX 64
#define FRCNN_Y4M_MAX_SIDE 32768
int frcnn_y4m_version(void);

/* chroma modes (input: all; output: FRCNN_Y4M_C420JPEG and FRCNN_Y4M_C444) */
#define FRCNN_Y4M_C420JPEG 0   /* C420jpeg and bare C420: chroma centred in both directions */
#define FRCNN_Y4M_C420MPEG2 1  /* horizontally co-sited, vertically centred */
#define FRCNN_Y4M_C422 2       /* horizontally co-sited */
#define FRCNN_Y4M_C444 3
#define FRCNN_Y4M_CMONO 4      /* luma only */
/* colour ranges */
#define FRCNN_Y4M_LIMITED 0    /* the y4m default */
#define FRCNN_Y4M_FULL 1       /* XCOLORRANGE=FULL */

/* One stream's frame format; frame_bytes = frcnn_y4m_frame_bytes(h, w, chroma). */
typedef struct frcnn_y4m_plan {
    int32_t h, w, chroma, range;
    uint32_t frame_bytes, reserved;
} frcnn_y4m_plan_t;

/* One frame of a batch: its plan, where its bytes lie and where its [h][w][3] frame goes.  ws_off is there for the item layout every
 * device decoder shares and is ignored: these kernels need no workspace. */
typedef struct frcnn_y4m_batch_item {
    frcnn_y4m_plan_t plan;
    uint64_t file_off;   /* bytes into files_dev; no alignment needed */
    uint64_t out_off;    /* bytes into out_dev; the item's [h][w][3] frame, contiguous */
    uint64_t ws_off;
} frcnn_y4m_batch_item_t;

/* Bytes of one frame (without its "FRAME\n" line); 0 for h or w outside 1..FRCNN_Y4M_MAX_SIDE or an unknown chroma mode. */
size_t frcnn_y4m_frame_bytes(int h, int w, int chroma);

/* n frames -> interleaved 8-bit RGB in ONE launch: item i's planes at files_dev + file_off -> its frame at out_dev + out_off, R,G,B per
 * pixel (bgr != 0: B,G,R).  items_host (HOST memory) is validated and sizes the grid; the kernel reads items_dev (DEVICE memory,
 * 8-byte aligned): the caller uploads THE SAME n * sizeof(item) BYTES on `stream` in front of the call.  Two items may name the same
 * file bytes, never overlapping output ranges.  The argument order is the other batched decoders'; status_dev and workspace are not
 * touched (nothing in a frame can be damaged: every byte value is a sample) and may be NULL.  One launch on `stream`: no allocation,
 * no synchronisation, nothing read on the host.
 * FRCNN_E_ARG, with nothing launched: a null pointer; n outside 1..FRCNN_Y4M_BATCH_MAX; a plan with a side outside
 * 1..FRCNN_Y4M_MAX_SIDE, an unknown chroma mode or range, or a frame_bytes that is not frcnn_y4m_frame_bytes of it; file_off +
 * frame_bytes > files_capacity; out_off + h * w * 3 > out_capacity; an items_dev that is not 8-byte aligned; overlapping outputs. */
int frcnn_y4m_decode_batch_u8(const frcnn_y4m_batch_item_t* items_host, const frcnn_y4m_batch_item_t* items_dev, int n,
                              const uint8_t* files_dev, size_t files_capacity, int bgr, uint8_t* out_dev, size_t out_capacity,
                              int32_t* status_dev, void* workspace, size_t workspace_capacity, void* stream);

/* The batch of one whose item travels as a kernel argument: frame_dev (plan->frame_bytes bytes) -> out_dev ([h][w][3]). */
int frcnn_y4m_decode_u8(const uint8_t* frame_dev, size_t frame_capacity, const frcnn_y4m_plan_t* plan, int bgr, uint8_t* out_dev,
                        size_t out_capacity, void* stream);

/* n interleaved 8-bit frames of ONE size (frame i at frames_dev + i * frame_stride; R,G,B per pixel, bgr != 0: B,G,R) -> n records
 * [Y | Cb | Cr] of frcnn_y4m_frame_bytes(h, w, chroma) bytes (record i at out_dev + i * out_stride) in ONE launch.  chroma:
 * FRCNN_Y4M_C420JPEG or FRCNN_Y4M_C444.  FRCNN_E_ARG, with nothing launched: a null pointer, n outside 1..FRCNN_Y4M_BATCH_MAX, a side
 * outside 1..FRCNN_Y4M_MAX_SIDE, another chroma mode, an unknown range, a stride smaller than its frame / record, or (n - 1) *
 * out_stride + the record's bytes > out_capacity. */
int frcnn_y4m_encode_u8(const uint8_t* frames_dev, size_t frame_stride, int n, int h, int w, int bgr, int chroma, int range,
                        uint8_t* out_dev, size_t out_stride, size_t out_capacity, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_Y4M_H */
