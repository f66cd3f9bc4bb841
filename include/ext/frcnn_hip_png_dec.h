/* The device PNG decoder: an EXTENSION of the C ABI of libfrcnn_hip.so beside the other codec headers (include/ext/frcnn_hip_png.h,
 * frcnn_hip_png_huff.h, frcnn_hip_jpeg.h, frcnn_hip_jpeg_opt.h, frcnn_hip_jpeg_dec.h, frcnn_hip_jpeg_dec_batch.h), whose revisions,
 * symbols and files stay as they are; include/frcnn_hip.h likewise.  Same library, same conventions (int status, message via
 * frcnn_last_error, `stream` = hipStream_t or NULL), a revision of its own: a host that uses these entry points checks
 * frcnn_png_dec_version() == FRCNN_PNG_DEC_VERSION besides frcnn_version().
 *   1 = frcnn_png_dec_plan, frcnn_png_dec_spans, frcnn_png_dec_workspace_bytes, frcnn_png_dec_batch_layout, frcnn_png_decode_batch_u8.
 * The batched form is the only device entry point: one workgroup per file makes a single file a batch of one. */
#ifndef FRCNN_HIP_PNG_DEC_H
#define FRCNN_HIP_PNG_DEC_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_PNG_DEC_VERSION 1
#define FRCNN_PNG_DEC_BATCH_MAX 64
int frcnn_png_dec_version(void);

/* The supported set, decided from the chunks alone: the signature; IHDR first, with bit depth 8, colour type 0 (grey), 2 (RGB) or 6
 * (RGBA), compression 0, filter method 0, interlace 0, sides in 1..65535; at least one IDAT, the IDATs consecutive; IEND; a zlib header
 * with CM = 8, a window of at most 32 KiB and no preset dictionary; the CRC-32 of IHDR and of every IDAT right.  Ancillary chunks (tRNS,
 * gAMA, iCCP, pHYs, tEXt, ...) and a PLTE in a truecolour file are skipped.  The pixels are numpy.asarray(PIL.Image.open(f).convert("RGB")),
 * byte for byte: grey replicated, alpha dropped.
 *
 * Two caps, both compile-time, both refusals of the planner:
 *   FRCNN_PNG_DEC_MAX_STREAM    the IDAT payloads together (the zlib stream) stay BELOW this many bytes.  It bounds the inflate kernel's
 *                               worst case (below) and keeps every bit position of the stream inside 32 bits.
 *   FRCNN_PNG_DEC_MAX_INFLATED  h * (1 + w * channels), the inflated bytes, stays BELOW this: output positions are 32-bit, and the
 *                               workspace is that many bytes per file.
 *
 * Cost in the worst case.  The inflate kernel is ONE workgroup of 512 lanes per file.  It takes the compressed stream in windows of
 * FRCNN_PNG_DEC_WINDOW_BYTES, a stretch of 128 bits per lane; the lanes guess their entry bit and decode again until no entry changes,
 * at most 512 rounds per window (round r fixes entry r), each round at most 128 one-bit tokens on a lane.  A stream below 16 MiB has at
 * most 2048 windows: 2048 x 512 rounds of a 16-byte stretch, the order of a second, for a stream nobody meets (a photograph settles in a
 * handful of rounds).  The matches of a window are copied in rounds: one that reads only bytes below the earliest unresolved match goes,
 * so a round frees at least one; a stream of nothing but chained matches (a flat frame under Z_RLE) takes one round per match, at most
 * 32768 two-bit matches per window, each a serial copy of up to 258 bytes on one lane.  The unfilter kernel is one wave per file that
 * walks strips of 64 rows along a diagonal: h / 64 strips of w + 63 steps. */
#define FRCNN_PNG_DEC_MAX_STREAM (1u << 24)
#define FRCNN_PNG_DEC_MAX_INFLATED (1u << 31)
#define FRCNN_PNG_DEC_WINDOW_BYTES 8192 /* of compressed stream per window of the inflate kernel: a block larger than this carries its tables over */

/* The plan: what the host-side chunk parse finds, a POD.  The device never sees the file, only its zlib stream: the payloads of the
 * IDAT chunks back to back, `stream_len` bytes, which the caller stages contiguously (frcnn_png_dec_spans says where they lie). */
typedef struct frcnn_png_dec_plan {
    int32_t h, w, channels;             /* channels: 1 (grey), 3 (RGB) or 4 (RGBA) */
    uint32_t file_len;
    uint32_t idat_off, idat_count;      /* the first IDAT chunk (its length field) and how many follow each other */
    uint32_t stream_len;                /* bytes of all IDAT payloads: zlib header, deflate blocks, Adler-32 */
    uint32_t inflated_len;              /* h * (1 + w * channels) */
} frcnn_png_dec_plan_t;

/* Parses the chunks of the `len` bytes at file_host (HOST memory), verifies the CRC-32 of IHDR and of every IDAT and fills *plan.
 * FRCNN_E_UNSUPPORTED with a message that names the reason for every file outside the supported set (palette, grey + alpha, 16-bit and
 * sub-byte depths, Adam7, APNG, an unknown critical chunk, a chunk cut short, a CRC that differs, a missing IEND, ...) and for an empty
 * file: the caller decodes those on the host.  FRCNN_E_ARG for a null pointer.  Never reads past file_host + len; touches no device. */
int frcnn_png_dec_plan(const uint8_t* file_host, size_t len, frcnn_png_dec_plan_t* plan);

/* The IDAT payloads of the file the plan was made of: spans[2 * k] = offset, spans[2 * k + 1] = length of payload k, plan->idat_count of
 * them, their lengths summing to plan->stream_len.  FRCNN_E_ARG for a null pointer, capacity (in spans) < idat_count, or a file that is
 * not the plan's.  Host only. */
int frcnn_png_dec_spans(const uint8_t* file_host, size_t len, const frcnn_png_dec_plan_t* plan, uint32_t* spans, size_t capacity);

/* Bytes of device workspace a file of this plan needs (16-byte aligned): the inflated bytes.  0 for a plan it refuses. */
size_t frcnn_png_dec_workspace_bytes(const frcnn_png_dec_plan_t* plan);

/* Status bits (status_dev[i], ORed in: the words are sticky, the caller clears them). */
#define FRCNN_PNG_DEC_CODE 1            /* a code that is not in its Huffman table, a symbol outside deflate, a malformed length list */
#define FRCNN_PNG_DEC_BLOCK 2           /* block type 3, or a stored block whose LEN and NLEN disagree */
#define FRCNN_PNG_DEC_OVERSUBSCRIBED 4  /* a set of code lengths that no prefix code has */
#define FRCNN_PNG_DEC_DISTANCE 8        /* a match that reaches in front of the first byte */
#define FRCNN_PNG_DEC_OVERRUN 16        /* more inflated bytes than h * (1 + w * channels) */
#define FRCNN_PNG_DEC_UNDERRUN 32       /* the stream ends inside a block or before the Adler-32, or inflates to fewer bytes */
#define FRCNN_PNG_DEC_ADLER 64          /* the Adler-32 of the inflated bytes differs from the stream's */
#define FRCNN_PNG_DEC_FILTER 128        /* a row whose filter type is not 0..4 */

/* One file of a batch: its plan and where its zlib stream, its frame and its workspace region lie.  Two items may name the same stream
 * bytes, never the same output or workspace bytes. */
typedef struct frcnn_png_dec_batch_item {
    frcnn_png_dec_plan_t plan;
    uint64_t file_off;   /* bytes into files_dev: the staged zlib stream, plan.stream_len bytes; no alignment needed */
    uint64_t out_off;    /* bytes into out_dev; the item's [h][w][3] frame, contiguous */
    uint64_t ws_off;     /* bytes into workspace; 16-byte aligned */
} frcnn_png_dec_batch_item_t;

/* ws_off[i] for n plans laid back to back (each region frcnn_png_dec_workspace_bytes(&plans[i])) -> the total bytes of workspace; 0,
 * with ws_off untouched, for a null pointer, n outside 1..FRCNN_PNG_DEC_BATCH_MAX or a plan that frcnn_png_dec_workspace_bytes refuses. */
size_t frcnn_png_dec_batch_layout(const frcnn_png_dec_plan_t* plans, int n, uint64_t* ws_off /* n, out */);

/* n files in TWO launches, whatever n is (inflate: a workgroup per file; unfilter + pack: a wave per file): item i's zlib stream at
 * files_dev + file_off -> its frame at out_dev + out_off (R,G,B per pixel, bgr != 0: B,G,R), its status bits ORed into status_dev[i],
 * its inflated bytes in workspace + ws_off.  items_host (HOST memory) is validated; the kernels read items_dev (DEVICE memory, 8-byte
 * aligned): the caller uploads THE SAME n * sizeof(item) BYTES on `stream` in front of the call and keeps them unchanged until the
 * launches have run.  What the kernels' bounds rest on is checked on items_host, so a device table that differs from it voids them.
 *
 * Per item: whatever the bytes of its stream are, nothing is read outside its stream or written outside its workspace region and its
 * output range; a damaged item yields a non-zero status word (its frame is then UNDEFINED) and leaves the other items' frames exact.
 * No allocation, no synchronisation, nothing read on the host.
 *
 * FRCNN_E_ARG, with nothing launched and no device call made: a null pointer; n outside 1..FRCNN_PNG_DEC_BATCH_MAX; a plan whose fields
 * contradict each other; file_off + stream_len > files_capacity, out_off + h * w * 3 > out_capacity or ws_off +
 * frcnn_png_dec_workspace_bytes(plan) > workspace_capacity; a ws_off or workspace that is not 16-byte aligned, a status_dev that is not
 * 4-byte aligned, an items_dev that is not 8-byte aligned; two items whose output ranges or workspace regions overlap. */
int frcnn_png_decode_batch_u8(const frcnn_png_dec_batch_item_t* items_host, const frcnn_png_dec_batch_item_t* items_dev, int n,
                              const uint8_t* files_dev, size_t files_capacity, int bgr, uint8_t* out_dev, size_t out_capacity,
                              int32_t* status_dev /* n words */, void* workspace, size_t workspace_capacity, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_PNG_DEC_H */
