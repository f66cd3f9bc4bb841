/* The device JPEG decoder for PROGRESSIVE files: an EXTENSION of the C ABI of libfrcnn_hip.so beside include/ext/frcnn_hip_jpeg_dec.h and
 * include/ext/frcnn_hip_jpeg_dec_batch.h (the baseline decoder, whose revisions, symbols and files stay as they are; include/frcnn_hip.h
 * likewise).  Same library, same conventions (int status, message via frcnn_last_error, `stream` = hipStream_t or NULL), a revision of its
 * own: a host that uses these entry points checks frcnn_jpeg_dec_full_version() == FRCNN_JPEG_DEC_FULL_VERSION besides frcnn_version().
 *   1 = frcnn_jpeg_dec_full_plan, frcnn_jpeg_dec_full_workspace_bytes, frcnn_jpeg_dec_full_batch_layout, frcnn_jpeg_decode_full_batch_u8,
 *       frcnn_jpeg_decode_full_u8. */
#ifndef FRCNN_HIP_JPEG_DEC_FULL_H
#define FRCNN_HIP_JPEG_DEC_FULL_H
#include "frcnn_hip_jpeg_dec_batch.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_JPEG_DEC_FULL_VERSION 1
/* Scans per file.  libjpeg's default script has 10 scans for colour and 6 for grey; the finest legal script that moves every band of every
 * component one bit at a time has a few hundred, which nobody writes.  64 covers every script met in practice and keeps the plan, a
 * fixed-size POD, below 5 KB.  A file with more is FRCNN_E_UNSUPPORTED. */
#define FRCNN_JPEG_DEC_FULL_MAX_SCANS 64
int frcnn_jpeg_dec_full_version(void);

/* The supported set: progressive DCT (SOF2), Huffman-coded, 8 bits; 1 component, or 3 components Y Cb Cr (a JFIF file; or an Adobe marker
 * with transform 1; or neither marker and component ids other than 'R' 'G' 'B'); luma sampled 1x1, 2x1 or 2x2 with both chroma components
 * 1x1; quantisation tables with 8-bit entries; Huffman tables with ids 0..3; with or without restart intervals; DHT, DQT and DRI segments
 * between scans, valid from that point on (tables are a property of the SCAN; a component's quantisation table is the one that stands
 * when its first scan starts, as libjpeg latches it); sides in 1..65535; at most FRCNN_JPEG_DEC_FULL_MAX_SCANS scans whose entropy-coded
 * segments hold fewer than FRCNN_JPEG_DEC_MAX_SCAN bytes together; EOI behind the last scan; and a LEGAL, COMPLETE scan script:
 *   - a DC scan has Ss = Se = 0 and may interleave components (in frame order); an AC scan has 1 <= Ss <= Se <= 63 and ONE component;
 *   - for every coefficient of every component the first scan that touches it has Ah = 0, every later one Ah = the previous Al and
 *     Al = Ah - 1; Al <= 13;
 *   - no AC scan of a component comes before its first DC scan;
 *   - at the end every coefficient 0..63 of every component stands at Al = 0 (libjpeg smooths the blocks of a file whose low AC bits
 *     are not all known: an incomplete file has other pixels, so it is refused).
 * Baseline files (SOF0) are refused too: they belong to frcnn_jpeg_dec_plan.  The pixels are those of libjpeg's default decoder, as for
 * the baseline decoder; tests/jpeg_prog_ref.py states the planner and the four scan decoders in Python.
 *
 * One scan of the plan.  Offsets are bytes from the start of the file.  The entropy-coded segment [off, off + len) runs to the first
 * 0xFF followed by anything but 0x00 or RST0..RST7 and is cut into `subsequences` stretches of `subsequence_bytes` raw bytes by the
 * baseline's rule (>= 32, a multiple of 4, at most 1024 of them).  Tables are indexed by FRAME component; those the scan does not use
 * (a component outside `comps`; the AC tables of a DC scan, the DC tables of an AC scan, both for a DC refinement) are 0. */
typedef struct frcnn_jpeg_dec_full_scan {
    uint32_t off, len;
    uint32_t restart_interval;          /* as it stands at this scan, in MCUs OF THE SCAN (blocks for a single component); 0 = none */
    uint32_t subsequence_bytes, subsequences;
    uint32_t dc_off[3], dc_count[3];    /* per component: BITS (16 bytes) with HUFFVAL behind them, and the symbols in HUFFVAL */
    uint32_t ac_off[3], ac_count[3];
    uint8_t comps;                      /* bit c: component c is in the scan */
    uint8_t ss, se, ah, al;
    uint8_t reserved[3];
} frcnn_jpeg_dec_full_scan_t;

/* The plan.  `frame` holds the frame fields with the baseline's meaning (h .. expected_blocks, file_len, dqt_off); its scan_off is the
 * first scan's segment, scan_len the bytes of ALL segments together, restart_interval the first scan's, subsequence_bytes / subsequences
 * those of the longest segment; dht_off, dht_count, comp_dc and comp_ac are 0 (see the scans).  About 5 KB: it does not travel by value,
 * the batched form below is the primary one. */
typedef struct frcnn_jpeg_dec_full_plan {
    frcnn_jpeg_dec_plan_t frame;
    uint32_t scans, reserved;
    frcnn_jpeg_dec_full_scan_t scan[FRCNN_JPEG_DEC_FULL_MAX_SCANS];
} frcnn_jpeg_dec_full_plan_t;

/* Parses the markers of the `len` bytes at file_host (HOST memory) and fills *plan.  FRCNN_E_UNSUPPORTED with a message that names the
 * reason for every file outside the supported set: a baseline file, an illegal or incomplete script, too many scans, arithmetic coding,
 * 12 bits, SOF1, CMYK / YCCK, Adobe transform 0, other sampling factors, a header cut short, a scan that runs to the end of the file
 * (no EOI), too many entropy-coded bytes, an empty file; FRCNN_E_ARG for a null pointer.  Never reads past file_host + len; touches no
 * device. */
int frcnn_jpeg_dec_full_plan(const uint8_t* file_host, size_t len, frcnn_jpeg_dec_full_plan_t* plan);

/* Bytes of device workspace a file of this plan needs (16-byte aligned; the baseline's layout: int16 coefficients in natural order, 64
 * per block, blocks in MCU order padded to whole MCUs, a restart flag per block, the component planes at padded size).  0 for a plan it
 * refuses. */
size_t frcnn_jpeg_dec_full_workspace_bytes(const frcnn_jpeg_dec_full_plan_t* plan);

/* Status bits (ORed into the item's word: sticky, the caller clears it). */
#define FRCNN_JPEG_DEC_FULL_BLOCKS 1    /* a scan holds another number of blocks than the frame header implies */
#define FRCNN_JPEG_DEC_FULL_ZIGZAG 2    /* a coefficient's zigzag index passed the scan's Se */
#define FRCNN_JPEG_DEC_FULL_CODE 4      /* a code that is not in its Huffman table (or a restart marker missing where one is due) */
#define FRCNN_JPEG_DEC_FULL_TABLE 8     /* a symbol outside what the scan kind allows (DC category above 11, AC size above 10, a size
                                           other than 0 / 1 in a refinement scan) or outside its table */
#define FRCNN_JPEG_DEC_FULL_EOBRUN 16   /* an end-of-band run that reaches past the scan's last block */

typedef struct frcnn_jpeg_dec_full_batch_item {
    frcnn_jpeg_dec_full_plan_t plan;
    uint64_t file_off;   /* bytes into files_dev: the WHOLE file; no alignment needed */
    uint64_t out_off;    /* bytes into out_dev; the item's [h][w][3] frame, contiguous */
    uint64_t ws_off;     /* bytes into workspace; 16-byte aligned */
} frcnn_jpeg_dec_full_batch_item_t;

/* frcnn_jpeg_dec_batch_layout for these plans: ws_off[i] for n plans laid back to back -> the total; 0 for a null pointer, n outside
 * 1..FRCNN_JPEG_DEC_BATCH_MAX or a plan that frcnn_jpeg_dec_full_workspace_bytes refuses. */
size_t frcnn_jpeg_dec_full_batch_layout(const frcnn_jpeg_dec_full_plan_t* plans, int n, uint64_t* ws_off /* n, out */);

/* n progressive files in ONE set of FOUR launches, whatever the files and their scripts are: (1) the coefficients zeroed (an AC scan never
 * visits the padding blocks of partial MCUs), (2) the entropy stage: one workgroup of 1024 lanes per file walks the file's scans in
 * order, (3) the IDCT, (4) upsampling and colour.  Arguments, alignment rules, the items_host / items_dev contract and the FRCNN_E_ARG
 * cases are those of frcnn_jpeg_decode_batch_u8 (include/ext/frcnn_hip_jpeg_dec_batch.h); "a plan whose fields contradict each other"
 * includes every scan's fields.  Per item: whatever the bytes of its scans are, nothing is read outside its file or written outside its
 * workspace region and its output range; a damaged item yields a non-zero status word (FRCNN_JPEG_DEC_FULL_*; its frame is then
 * UNDEFINED) and leaves the other items' frames exact.  No allocation, no synchronisation, nothing read on the host.
 *
 * Cost in the worst case.  Per scan the workgroup runs the baseline's round loop over the scan's subsequences.  A DC-first or AC-first
 * scan re-synchronises as a baseline scan does and is bounded in the same way (up to `subsequences` rounds of `subsequence_bytes` on
 * a lane).  A REFINEMENT scan does not: which bits a block consumes depends on which of its coefficients are already non-zero, so the
 * state handed from lane to lane carries the absolute block index, a lane's guess of it is never right, and the loop fixes exactly one
 * lane per round: ALWAYS `subsequences` rounds, i.e. the scan's bytes decoded once serially, bit by bit (a 375 x 500 photograph from
 * libjpeg's default script: four refinement scans of a few KB each, a few hundred rounds of 32 bytes).  Together at most
 * FRCNN_JPEG_DEC_MAX_SCAN bytes of serial decoding per file, reached concurrently per item. */
int frcnn_jpeg_decode_full_batch_u8(const frcnn_jpeg_dec_full_batch_item_t* items_host, const frcnn_jpeg_dec_full_batch_item_t* items_dev, int n,
                                    const uint8_t* files_dev, size_t files_capacity, int bgr, uint8_t* out_dev, size_t out_capacity,
                                    int32_t* status_dev /* n words */, void* workspace, size_t workspace_capacity, void* stream);

/* A batch of one: file_dev holds the file's plan->frame.file_len bytes, item_dev (DEVICE memory, 8-byte aligned) a
 * frcnn_jpeg_dec_full_batch_item_t that the caller uploaded on `stream`: *plan with file_off = out_off = ws_off = 0. */
int frcnn_jpeg_decode_full_u8(const uint8_t* file_dev, const frcnn_jpeg_dec_full_plan_t* plan, const frcnn_jpeg_dec_full_batch_item_t* item_dev,
                              int bgr, uint8_t* out, size_t out_capacity, int32_t* status_dev, void* workspace, size_t workspace_capacity,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_JPEG_DEC_FULL_H */
