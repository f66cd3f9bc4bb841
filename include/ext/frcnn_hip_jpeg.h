/* The device JPEG encoder: an EXTENSION of the C ABI of libfrcnn_hip.so beside the two PNG encoder headers (include/ext/frcnn_hip_png.h,
 * include/ext/frcnn_hip_png_huff.h), whose revisions, symbols and files stay as they are; include/frcnn_hip.h likewise: FRCNN_ABI_VERSION
 * 110.  Same library, same conventions (int status, message via frcnn_last_error, `stream` = hipStream_t or NULL), a revision of its own: a
 * host that uses these entry points checks frcnn_jpeg_version() == FRCNN_JPEG_VERSION besides frcnn_version().
 *   1 = frcnn_jpeg_restart_mcus, frcnn_jpeg_header_bytes, frcnn_jpeg_bound, frcnn_jpeg_workspace_bytes, frcnn_jpeg_encode_u8. */
#ifndef FRCNN_HIP_JPEG_H
#define FRCNN_HIP_JPEG_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_JPEG_VERSION 1
int frcnn_jpeg_version(void);

/* The encoder writes a JFIF baseline sequential (SOF0) file: 8 bits, Y Cb Cr, every component sampled 1x1 (4:4:4), the quantisation
 * tables of ITU-T T.81 Annex K.1 / K.2 scaled by the IJG quality rule, the Huffman tables of Annex K.3, a restart interval of
 * FRCNN_JPEG_RESTART_MCUS MCUs (RST0..RST7 between the intervals).  Colour transform, DCT and quantisation are integer arithmetic with
 * fixed rounding: the bytes are a function of (frame, quality) alone, and tests/jpeg_ref.py states them in Python.  Any JPEG reader
 * decodes the file.
 * frcnn_jpeg_header_bytes: SOI .. SOS, the same for every frame.  frcnn_jpeg_bound: the largest file an h x w frame can become = header
 * + 2 (EOI) + per restart interval 416 * 3 * its MCUs (a block is at most 208 bytes, each of which may be stuffed) + 2 (the padding byte
 * and its stuffing) + 2 (RSTm); 0 for a size frcnn_jpeg_encode_u8 refuses.  frcnn_jpeg_workspace_bytes: the device workspace it needs
 * (16-byte aligned), 0 likewise. */
#define FRCNN_JPEG_RESTART_MCUS 16
int frcnn_jpeg_restart_mcus(void);
size_t frcnn_jpeg_header_bytes(void);
size_t frcnn_jpeg_bound(int h, int w);
size_t frcnn_jpeg_workspace_bytes(int h, int w);

/* frame [h][w][3] uint8 DEVICE, contiguous, R,G,B per pixel (bgr != 0: B,G,R; the file is the same either way), quality 1..100 -> out:
 * the whole file, and *out_len (DEVICE int32, 4-byte aligned) its length in bytes (<= frcnn_jpeg_bound(h, w)); bytes of out beyond it
 * are left as they were.  out needs no alignment; out_capacity >= frcnn_jpeg_bound(h, w) (FRCNN_E_ARG otherwise, as for a null pointer
 * and for a quality outside 1..100).  Three launches on `stream`: no allocation, no synchronisation, nothing read on the host per frame
 * -- the call can be captured in a hipGraph and replayed (the quantisation tables travel as kernel arguments).  FRCNN_E_UNSUPPORTED: h or
 * w < 1, h or w > 65535, or a bound past 2^31 - 1.  Nothing is launched on an error. */
int frcnn_jpeg_encode_u8(const uint8_t* frame, int h, int w, int bgr, int quality, uint8_t* out, size_t out_capacity, int32_t* out_len,
                         void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_JPEG_H */
