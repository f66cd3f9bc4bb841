/* The device JPEG decoder: an EXTENSION of the C ABI of libfrcnn_hip.so beside the encoders' headers (include/ext/frcnn_hip_jpeg.h,
 * include/ext/frcnn_hip_png.h, include/ext/frcnn_hip_png_huff.h), whose revisions, symbols and files stay as they are; include/frcnn_hip.h
 * likewise.  Same library, same conventions (int status, message via frcnn_last_error, `stream` = hipStream_t or NULL), a revision of its
 * own: a host that uses these entry points checks frcnn_jpeg_dec_version() == FRCNN_JPEG_DEC_VERSION besides frcnn_version().
 *   1 = frcnn_jpeg_dec_plan, frcnn_jpeg_dec_workspace_bytes, frcnn_jpeg_decode_u8. */
#ifndef FRCNN_HIP_JPEG_DEC_H
#define FRCNN_HIP_JPEG_DEC_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_JPEG_DEC_VERSION 1
int frcnn_jpeg_dec_version(void);

/* The supported set: baseline sequential (SOF0), 8 bits, ONE scan holding all components; 1 component, or 3 components Y Cb Cr (a JFIF
 * file; or an Adobe marker with transform 1; or neither marker and component ids other than 'R' 'G' 'B'); luma sampled 1x1, 2x1 or 2x2
 * with both chroma components 1x1; quantisation tables with 8-bit entries; any Huffman tables with ids 0..1; with or without a restart
 * interval; sides in 1..65535; an entropy-coded segment below FRCNN_JPEG_DEC_MAX_SCAN bytes.  The pixels are those of libjpeg's default decoder (the ISLOW
 * integer IDCT, "fancy" chroma upsampling, 16-bit fixed-point colour conversion): tests/jpeg_dec_ref.py states them in Python and the
 * kernels agree with it byte for byte.
 *
 * The plan: what the host-side marker parse finds, a POD that travels to the kernels by value.  Offsets are bytes from the start of the
 * file.  The entropy-coded segment [scan_off, scan_off + scan_len) runs to the first 0xFF followed by anything but 0x00 or RST0..RST7.
 * It is cut into `subsequences` stretches of `subsequence_bytes` raw bytes (>= 32, a multiple of 4, growing with the segment so that
 * there are at most 1024 of them), one lane of the entropy kernel each.
 *
 * Cost in the worst case.  The entropy kernel is ONE workgroup whose round loop is bounded by the number of subsequences: a stream that
 * re-synchronises as slowly as it can (noise at quality 100 does) makes every lane decode its stretch up to `subsequences` times, i.e.
 * up to 1024 x subsequence_bytes of serial decoding on a lane.  FRCNN_JPEG_DEC_MAX_SCAN = 16 MiB keeps a stretch at or below 16 KiB:
 * at most 16 MiB of serial symbol decoding, of the order of a second, for a file nobody meets (a VOC image has a scan of 85 KB and takes
 * 16 rounds of 84 bytes).  Longer scans are FRCNN_E_UNSUPPORTED: decode them on the host.  The DC kernel is one workgroup per
 * component, each lane walking blocks / 1024 of them serially: cheap at photograph sizes (3 per lane for 375x500), tens of thousands
 * per lane for frames near 65535 x 65535, whose workspace (193 bytes per block: tens of GB) is the practical limit long before. */
#define FRCNN_JPEG_DEC_MAX_SCAN (1u << 24)
typedef struct frcnn_jpeg_dec_plan {
    int32_t h, w, components;           /* components: 1 or 3 */
    int32_t hs, vs;                     /* luma sampling factors: 1x1, 2x1 or 2x2 (1x1 for a single component) */
    int32_t mcus_x, mcus_y, blocks_per_mcu;
    uint32_t expected_blocks;           /* mcus_x * mcus_y * blocks_per_mcu */
    uint32_t restart_interval;          /* MCUs, 0 = none (informative: the decoder follows the markers) */
    uint32_t file_len, scan_off, scan_len;
    uint32_t dqt_off[3];                /* per component: its 64 table entries, zigzag order */
    uint32_t dht_off[2][2];             /* [class: 0 DC, 1 AC][id]: BITS (16 bytes) with HUFFVAL behind them; 0 = not defined */
    uint32_t dht_count[2][2];           /* symbols in HUFFVAL (<= 256) */
    uint8_t comp_dc[4], comp_ac[4];     /* per component: the id of its DC and AC table */
    uint32_t subsequence_bytes, subsequences;
} frcnn_jpeg_dec_plan_t;

/* Parses the markers of the `len` bytes at file_host (HOST memory) and fills *plan.  FRCNN_E_UNSUPPORTED with a message that names
 * the reason for every file outside the supported set (progressive, arithmetic-coded, 12-bit, 16-bit DQT, CMYK / YCCK, Adobe transform 0,
 * several scans, other sampling factors, ...), for a header that is cut short and for an empty file; FRCNN_E_ARG for a null pointer.
 * Never reads past file_host + len; touches no device. */
int frcnn_jpeg_dec_plan(const uint8_t* file_host, size_t len, frcnn_jpeg_dec_plan_t* plan);

/* Bytes of device workspace frcnn_jpeg_decode_u8 needs for this plan (16-byte aligned): the coefficients (int16, 64 per block), a
 * restart flag per block and the component planes at padded size.  0 for a plan it refuses. */
size_t frcnn_jpeg_dec_workspace_bytes(const frcnn_jpeg_dec_plan_t* plan);

/* Status bits (*status_dev, ORed in: the word is sticky, the caller clears it). */
#define FRCNN_JPEG_DEC_BLOCKS 1         /* the scan holds another number of blocks than the frame header implies */
#define FRCNN_JPEG_DEC_ZIGZAG 2         /* a coefficient's zigzag index passed 63 */
#define FRCNN_JPEG_DEC_CODE 4           /* a code that is not in its Huffman table */
#define FRCNN_JPEG_DEC_TABLE 8          /* a symbol outside baseline (DC category above 11, AC size above 10) or outside its table */

/* file_dev: the file's plan->file_len bytes in DEVICE memory, no alignment needed -> out [h][w][3] uint8 DEVICE, contiguous, R,G,B per
 * pixel (bgr != 0: B,G,R); a single component is written to all three.  out_capacity >= h * w * 3.  *status_dev: DEVICE int32, 4-byte
 * aligned; 0 stays 0 for a sound file, see the bits above; with a non-zero status `out` is UNDEFINED (blocks the walk never reached keep
 * whatever the workspace held); whatever the bytes of the scan are, nothing is read or written outside the
 * file, the workspace and out, and the entropy kernel ends after at most `subsequences` rounds.  Four launches on `stream`: no allocation,
 * no synchronisation, nothing read on the host.  Not meant to be captured in a hipGraph (the plan, a kernel argument, differs per file):
 * it runs eagerly on the stream in front of a replay.  FRCNN_E_ARG: a null pointer, a misaligned workspace or status word, a capacity
 * that is too small, a plan whose fields contradict each other (one that frcnn_jpeg_dec_plan did not make).  Nothing is launched on an
 * error. */
int frcnn_jpeg_decode_u8(const uint8_t* file_dev, const frcnn_jpeg_dec_plan_t* plan, int bgr, uint8_t* out, size_t out_capacity,
                         int32_t* status_dev, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_JPEG_DEC_H */
