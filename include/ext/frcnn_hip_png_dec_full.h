/* The device PNG decoder for the whole of the format's still images: an EXTENSION of the C ABI of libfrcnn_hip.so beside
 * include/ext/frcnn_hip_png_dec.h, whose revision, symbols and files stay as they are.  Same library, same conventions (int status,
 * message via frcnn_last_error, `stream` = hipStream_t or NULL; the caller stages the IDAT payloads back to back; a batch is at most
 * FRCNN_PNG_DEC_BATCH_MAX files; one sticky status word per item, the FRCNN_PNG_DEC_* bits of revision 1's header), a revision of its
 * own: a host that uses these entry points checks frcnn_png_dec_full_version() == FRCNN_PNG_DEC_FULL_VERSION besides frcnn_version().
 *   1 = frcnn_png_dec_full_plan, frcnn_png_dec_full_spans, frcnn_png_dec_full_workspace_bytes, frcnn_png_dec_full_batch_layout,
 *       frcnn_png_decode_full_batch_u8. */
#ifndef FRCNN_HIP_PNG_DEC_FULL_H
#define FRCNN_HIP_PNG_DEC_FULL_H
#include <stddef.h>
#include <stdint.h>
#include "frcnn_hip_png_dec.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_PNG_DEC_FULL_VERSION 1
#define FRCNN_PNG_DEC_FULL_PLTE_BYTES 768 /* what the caller stages for a palette file: its PLTE entries, zero-padded to 256 x 3 */
int frcnn_png_dec_full_version(void);

/* The supported set, decided from the chunks alone.  Everything frcnn_png_dec_plan supports, and:
 *   colour type 3 (palette) at depths 1, 2, 4, 8: PLTE in front of the first IDAT, 1..256 entries, its length a multiple of 3; an index
 *       at or beyond plte_entries decodes to (0, 0, 0); tRNS is skipped (convert("RGB") ignores it for every colour type);
 *   colour type 0 (grey) at depths 1, 2, 4: samples scale by 255, 85, 17;
 *   colour type 4 (grey + alpha) at depth 8: alpha dropped;
 *   depth 16 for colour types 2, 4 and 6: the high byte of every sample (12 34 ab cd ff 01 -> (18, 171, 255));
 *   interlace method 1 (Adam7) for every combination above.
 * Refused, each named in the message: colour type 0 at depth 16 (Pillow opens it as I;16 and its convert("RGB") saturates: a quirk of
 * the library, so that file keeps the library); a palette file without PLTE or with PLTE behind an IDAT; a PLTE of bad length; a depth /
 * colour-type pair the PNG specification does not list; and every structural refusal of frcnn_png_dec_plan (CRC, a cut chunk, a missing
 * IEND, the zlib header, the two caps FRCNN_PNG_DEC_MAX_STREAM and FRCNN_PNG_DEC_MAX_INFLATED, APNG, an unknown critical chunk).
 * The pixels are numpy.asarray(PIL.Image.open(f).convert("RGB")), byte for byte.
 *
 * inflated_len is the sum over the passes that exist of ph * (1 + ceil(pw * bits_per_pixel / 8)); without interlace the one pass is
 * the frame.  The Adam7 passes have origin and step (x0, y0; dx, dy) = (0,0; 8,8) (4,0; 8,8) (0,4; 4,8) (2,0; 4,4) (0,2; 2,4) (1,0; 2,2)
 * (0,1; 1,2); pw = ceil((w - x0) / dx), ph = ceil((h - y0) / dy); a pass with pw == 0 or ph == 0 is absent from the stream. */
typedef struct frcnn_png_dec_full_plan {
    int32_t h, w, colour_type, bit_depth, interlace;
    uint32_t file_len;
    uint32_t idat_off, idat_count;      /* the first IDAT chunk (its length field) and how many follow each other */
    uint32_t stream_len;                /* bytes of all IDAT payloads: zlib header, deflate blocks, Adler-32 */
    uint32_t inflated_len;
    uint32_t plte_off, plte_entries;    /* colour type 3: the PLTE chunk's data in the file and its entries (1..256); else 0, 0 */
} frcnn_png_dec_full_plan_t;

/* As frcnn_png_dec_plan: FRCNN_E_UNSUPPORTED with the reason for a file outside the supported set and for an empty file, FRCNN_E_ARG for
 * a null pointer.  Never reads past file_host + len; touches no device. */
int frcnn_png_dec_full_plan(const uint8_t* file_host, size_t len, frcnn_png_dec_full_plan_t* plan);

/* As frcnn_png_dec_spans, for a plan of frcnn_png_dec_full_plan.  Host only. */
int frcnn_png_dec_full_spans(const uint8_t* file_host, size_t len, const frcnn_png_dec_full_plan_t* plan, uint32_t* spans, size_t capacity);

/* Bytes of device workspace a file of this plan needs (16-byte aligned): the inflated bytes.  0 for a plan it refuses. */
size_t frcnn_png_dec_full_workspace_bytes(const frcnn_png_dec_full_plan_t* plan);

/* One file of a batch.  plte_off: bytes into files_dev of the item's palette, FRCNN_PNG_DEC_FULL_PLTE_BYTES bytes (R,G,B per entry,
 * zero behind plte_entries), read for colour type 3 only and ignored otherwise. */
typedef struct frcnn_png_dec_full_batch_item {
    frcnn_png_dec_full_plan_t plan;
    uint64_t file_off;   /* bytes into files_dev: the staged zlib stream, plan.stream_len bytes; no alignment needed */
    uint64_t out_off;    /* bytes into out_dev; the item's [h][w][3] frame, contiguous */
    uint64_t ws_off;     /* bytes into workspace; 16-byte aligned */
    uint64_t plte_off;   /* bytes into files_dev: the staged palette */
} frcnn_png_dec_full_batch_item_t;

/* As frcnn_png_dec_batch_layout. */
size_t frcnn_png_dec_full_batch_layout(const frcnn_png_dec_full_plan_t* plans, int n, uint64_t* ws_off /* n, out */);

/* n files in THREE launches, whatever n is (inflate: a workgroup per file, the code of revision 1; reconstruction: a wave per (pass,
 * file); expansion: a lane per output pixel): item i's zlib stream at files_dev + file_off -> its frame at out_dev + out_off (R,G,B per
 * pixel, bgr != 0: B,G,R), its status bits ORed into status_dev[i], its inflated bytes in workspace + ws_off.  items_host, items_dev and
 * the guarantees per item are those of frcnn_png_decode_batch_u8: whatever the bytes of a stream are, nothing is read outside the item's
 * stream and palette or written outside its workspace region and its output range; a damaged item yields a non-zero status word (its
 * frame is then UNDEFINED) and leaves the other items' frames exact.  No allocation, no synchronisation, nothing read on the host.
 *
 * FRCNN_E_ARG, with nothing launched and no device call made: every argument error of frcnn_png_decode_batch_u8 (a null pointer; n
 * outside 1..FRCNN_PNG_DEC_BATCH_MAX; a plan whose fields contradict each other, among them a palette plan with plte_entries outside
 * 1..256; file_off + stream_len > files_capacity, out_off + h * w * 3 > out_capacity or ws_off + workspace bytes > workspace_capacity;
 * the alignments; overlapping output ranges or workspace regions) and, for colour type 3, plte_off + 768 > files_capacity. */
int frcnn_png_decode_full_batch_u8(const frcnn_png_dec_full_batch_item_t* items_host, const frcnn_png_dec_full_batch_item_t* items_dev, int n,
                                   const uint8_t* files_dev, size_t files_capacity, int bgr, uint8_t* out_dev, size_t out_capacity,
                                   int32_t* status_dev /* n words */, void* workspace, size_t workspace_capacity, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_PNG_DEC_FULL_H */
