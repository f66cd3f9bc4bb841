/* The device JPEG encoder's two size options, 4:2:0 chroma and per-frame optimised Huffman tables: an EXTENSION of the C ABI of
 * libfrcnn_hip.so beside include/ext/frcnn_hip_jpeg.h, whose revision, symbols and files stay as they are (frcnn_jpeg_encode_u8 writes the
 * same bytes); include/frcnn_hip.h and every other extension header likewise.  Same library, same conventions (int status, message via
 * frcnn_last_error, `stream` = hipStream_t or NULL), a revision of its own: a host that uses these entry points checks
 * frcnn_jpeg_opt_version() == FRCNN_JPEG_OPT_VERSION besides frcnn_version().
 *   1 = frcnn_jpeg_opt_restart_mcus, frcnn_jpeg_opt_bound, frcnn_jpeg_opt_workspace_bytes, frcnn_jpeg_opt_encode_u8,
 *       frcnn_jpeg_opt_build_tables. */
#ifndef FRCNN_HIP_JPEG_OPT_H
#define FRCNN_HIP_JPEG_OPT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_JPEG_OPT_VERSION 1
int frcnn_jpeg_opt_version(void);

/* The two knobs.  subsampling: FRCNN_JPEG_OPT_444 is the stream of include/ext/frcnn_hip_jpeg.h; FRCNN_JPEG_OPT_420 is SOF0 with Y at 2x2
 * and Cb, Cr at 1x1: an MCU is 16x16 pixels in block order Y00 Y01 Y10 Y11 Cb Cr, the frame's last column / row repeated to multiples of
 * 16, Cb and Cr computed per pixel and each 2x2 group averaged as (a + b + c + d + bias) >> 2 with bias 1 at even and 2 at odd output
 * columns (libjpeg's h2v2_downsample).  huffman: FRCNN_JPEG_OPT_STANDARD writes the tables of Annex K.3; FRCNN_JPEG_OPT_OPTIMIZED builds
 * four tables per frame (DC / AC for luma and for chroma) from the frame's own symbol counts by libjpeg's jpeg_gen_optimal_table and
 * writes them into the four DHT segments.  No such table is longer than Annex K's, so SOI .. SOS never exceeds frcnn_jpeg_header_bytes().
 * tests/jpeg_opt_ref.py states the stream in Python; (444, standard) is frcnn_jpeg_encode_u8's file byte for byte. */
#define FRCNN_JPEG_OPT_444 444
#define FRCNN_JPEG_OPT_420 420
#define FRCNN_JPEG_OPT_STANDARD 0
#define FRCNN_JPEG_OPT_OPTIMIZED 1

/* frcnn_jpeg_opt_restart_mcus: MCUs per restart interval, 16 at 4:4:4 and 8 at 4:2:0 (48 blocks either way); 0 for an unknown mode.
 * frcnn_jpeg_opt_bound: the largest file an h x w frame can become in either huffman mode = frcnn_jpeg_header_bytes() + 2 (EOI) + per
 * restart interval 416 * its blocks (3 per 8x8 MCU, 6 per 16x16 MCU; a block is at most 23 + 63 * 26 bits -- an optimised DC code is at
 * most 12 bits (12 categories and the reserved all-ones leaf), an AC code at most 16, value bits 11 and 10 -- which is 208 bytes, as with
 * Annex K's 20 + 63 * 26; each byte may be stuffed) + 2 (the padding byte and its stuffing) + 2 (RSTm); 0 for a size or a mode that
 * frcnn_jpeg_opt_encode_u8 refuses.  frcnn_jpeg_opt_workspace_bytes: the device workspace it needs (16-byte aligned), 0 likewise. */
int frcnn_jpeg_opt_restart_mcus(int subsampling);
size_t frcnn_jpeg_opt_bound(int h, int w, int subsampling);
size_t frcnn_jpeg_opt_workspace_bytes(int h, int w, int subsampling, int huffman);

/* As frcnn_jpeg_encode_u8 (same arguments, conventions and error rules; out_capacity >= frcnn_jpeg_opt_bound(h, w, subsampling)) with
 * the two modes; FRCNN_E_ARG for an unknown one.  Launches on `stream`: three with standard tables; six with optimised ones (the
 * histograms cleared, a statistics pass, the table kernel, then the three).  No allocation, no synchronisation, nothing read on the host
 * per frame: the call can be captured in a hipGraph and replayed; the histograms are cleared inside the call.  The symbol counts are
 * integer sums, so the file is a function of (frame, quality, subsampling, huffman) alone.  Nothing is launched on an error. */
int frcnn_jpeg_opt_encode_u8(const uint8_t* frame, int h, int w, int bgr, int quality, int subsampling, int huffman, uint8_t* out,
                             size_t out_capacity, int32_t* out_len, void* workspace, void* stream);

/* A Huffman table as a DHT segment holds it: BITS (codes per length 1..16), HUFFVAL (the first `count` entries, the rest zero). */
typedef struct {
    uint8_t bits[16];
    uint8_t huffval[256];
    uint32_t count;
} frcnn_jpeg_opt_table_t;

/* The table kernel alone: hist = four histograms of 256 uint32 (DEVICE; in the encoder: DC luma, AC luma, DC chroma, AC chroma) ->
 * tables_out = four frcnn_jpeg_opt_table_t (DEVICE, 4-byte aligned), table k from histogram k by libjpeg's jpeg_gen_optimal_table (a
 * 257th pseudo-symbol of count 1, the largest index on a tie, lengths limited to 16, HUFFVAL by (tree depth, symbol)); any counts are
 * handled, an all-zero histogram gives an empty table.  One launch on `stream`.  FRCNN_E_ARG for a null or misaligned pointer. */
int frcnn_jpeg_opt_build_tables(const uint32_t* hist, void* tables_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_JPEG_OPT_H */
