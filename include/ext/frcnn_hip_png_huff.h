/* The device PNG encoder's `huffman` mode: an EXTENSION of the C ABI of libfrcnn_hip.so beside include/ext/frcnn_hip_png.h (the `runs`
 * mode, whose revision, symbols and files stay as they are; include/frcnn_hip.h likewise: FRCNN_ABI_VERSION 110).  Same library, same
 * conventions (int status, message via frcnn_last_error, `stream` = hipStream_t or NULL), a revision of its own: a host that uses these
 * entry points checks frcnn_png_huff_version() == FRCNN_PNG_HUFF_VERSION besides frcnn_version().
 *   1 = frcnn_png_huff_band_rows, frcnn_png_huff_bound, frcnn_png_huff_workspace_bytes, frcnn_png_huff_encode_u8. */
#ifndef FRCNN_HIP_PNG_HUFF_H
#define FRCNN_HIP_PNG_HUFF_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_PNG_HUFF_VERSION 1
int frcnn_png_huff_version(void);

/* The encoder writes an 8-bit RGB, non-interlaced PNG.  Every scanline takes the filter (None, Sub, Up, Average, Paeth) with the smallest
 * sum of |filtered byte as int8|, the lowest type on a tie; the filtered stream is cut into bands of frcnn_png_huff_band_rows() rows, each
 * band one IDAT chunk: one dynamic-Huffman deflate block (literals and run matches at distance 1, code lengths at most 15 bits, the
 * distance alphabet code 0 alone) closed by a sync flush, or stored blocks where the dynamic block is not strictly shorter; then a closing
 * IDAT with the final empty block and the Adler-32, and IEND.  Any PNG reader decodes it; the bytes are a function of the frame alone (no
 * float arithmetic, no dependence on scheduling).
 * frcnn_png_huff_bound: the largest file an h x w frame can become = 66 + 2 + sum over bands of (12 + n + 5 * ceil(n / 65535)), n = the
 * band's filtered bytes (rows * (1 + 3w)); 0 for a size frcnn_png_huff_encode_u8 refuses.  frcnn_png_huff_workspace_bytes: the device
 * workspace it needs (16-byte aligned), 0 likewise. */
int frcnn_png_huff_band_rows(void);
size_t frcnn_png_huff_bound(int h, int w);
size_t frcnn_png_huff_workspace_bytes(int h, int w);

/* The arguments of frcnn_png_encode_u8: frame [h][w][3] uint8 DEVICE, contiguous, R,G,B per pixel (bgr != 0: B,G,R; the file is RGB
 * either way) -> out: the whole file, and *out_len (DEVICE int32, 4-byte aligned) its length in bytes (<= frcnn_png_huff_bound(h, w));
 * bytes of out beyond it are left as they were.  out needs no alignment; out_capacity >= frcnn_png_huff_bound(h, w) (FRCNN_E_ARG
 * otherwise, as for a null pointer).  Three launches on `stream`: no allocation, no synchronisation, nothing read on the host per frame
 * -- the call can be captured in a hipGraph and replayed.  FRCNN_E_UNSUPPORTED: h or w < 1, or h * (1 + 3w) > 2^31 - 1.  Nothing is
 * launched on an error. */
int frcnn_png_huff_encode_u8(const uint8_t* frame, int h, int w, int bgr, uint8_t* out, size_t out_capacity, int32_t* out_len,
                             void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_PNG_HUFF_H */
