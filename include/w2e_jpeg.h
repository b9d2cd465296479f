/* w2e_jpeg.h -- C ABI of the baseline-JPEG encoder (csrc/jpeg.hip) and decoder (csrc/jpeg_decode.hip, further down) in libw2e.so
 * (gfx950).  The encoder: the file that torchvision 0.8.2's `save_image(x, "name.jpg", ...)` writes through Pillow's default JPEG (libjpeg: quality 75, 4:2:0, the Annex K Huffman tables, no
 * optimisation), for uint8 RGB images that live on the GPU.  Integer arithmetic from end to end, so the bytes are Pillow's own
 * (DESIGN.md "K17b": the rules).  Two stages, each reachable on its own:
 *   1. w2e_jpeg_coefficients: pixels -> quantised DCT coefficients (colour conversion, edge repetition, chroma down-sampling,
 *      libjpeg's accurate integer DCT, quantisation: one launch);
 *   2. w2e_jpeg_entropy: coefficients -> the Huffman-coded segment of each image, before byte stuffing (three launches: code every
 *      block into a fixed slot; exclusive prefix sum of the lengths; every output word gathers the blocks that cover it).
 * Header, byte stuffing (0xFF -> 0xFF 0x00) and the EOI marker stay with the host (where2edit_amd/image_io.py).
 * Same conventions as w2e_image.h: device pointers, caller-allocated outputs and workspace, asynchronous on `stream` (void*), no
 * allocation, copy, memset or global atomic inside, 0 = OK, otherwise w2e_last_error(); arguments are checked before any HIP call.
 * The same input gives the same bytes on every run.
 *
 * Geometry.  MCUs of 16 x 16 pixels in raster order, mx = ceil(w / 16) across and my = ceil(h / 16) down; six blocks per MCU in the
 * order Y(0,0) Y(0,1) Y(1,0) Y(1,1) Cb Cr; blocks = 6 mx my.  A Y block outside the ceil(h / 8) x ceil(w / 8) real ones is a dummy:
 * all AC coefficients zero, DC that of the previous Y block in scan order (it then codes as a zero difference and an end-of-block).
 */
#ifndef W2E_JPEG_H
#define W2E_JPEG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define W2E_JPEG_SLOT_WORDS 52     /* 32-bit words of a block's slot: the longest block is 20 + 63 * 26 = 1658 bits */
#define W2E_JPEG_SCAN_TILE 1024    /* blocks per step of the prefix sum (one workgroup per image walks its tiles in order) */
#define W2E_JPEG_STRIP_MCUS 8      /* MCUs of one MCU row that a workgroup of stage 1 stages and transforms */

/* w2e_jpeg_plan (pure host).  plan has 8 entries:
 *   plan[0]  blocks per image (6 mx my)
 *   plan[1], plan[2]  mx, my
 *   plan[3]  bytes of workspace w2e_jpeg_entropy needs for this batch: the slots, the lengths and the 64-bit offsets
 *   plan[4]  the largest possible segment of one image in bytes, before stuffing: blocks * 208 (a multiple of 4)
 *   plan[5]  int16 elements of the coefficient tensor of one image (64 * blocks)
 *   plan[6]  workgroups of stage 1 for this batch (batch * my * ceil(mx / W2E_JPEG_STRIP_MCUS))
 *   plan[7]  W2E_JPEG_SCAN_TILE
 * h and w are in 1..W2E_IMAGE_MAX_SIZE (w2e_image.h), batch >= 0. */
int w2e_jpeg_plan(int batch, int h, int w, int64_t* plan);

/* Stage 1.  src: contiguous uint8 [batch, h, w, 3], any alignment.  quality in 1..100: the Annex K tables scaled as libjpeg's
 * jpeg_set_quality does (baseline forced).  coef: int16 [batch, blocks, 64], 16-byte aligned, every block in zigzag order, dummies
 * included and filled.  An empty batch returns 0 without a launch. */
int w2e_jpeg_coefficients(const uint8_t* src, int batch, int h, int w, int quality, int16_t* coef, void* stream);

/* Stage 2.  coef: as stage 1 writes it.  huff: uint32 [4, 256] device table in the order DC0, AC0, DC1, AC1, entry [symbol] =
 * (code << 5) | length (length 1..16; 0 for a symbol the table does not have), made by the host from the Annex K lists.
 * out: image b's segment starts at out + b * out_stride (out and out_stride multiples of 4, out_stride >= plan[4]); the bytes after
 * the last coded bit are 1-bits up to the end of its 32-bit word.  lengths: int64 [batch], the bytes of each segment (the coded bits
 * rounded up to a byte).  workspace: plan[3] bytes, 8-byte aligned. */
int w2e_jpeg_entropy(const int16_t* coef, int batch, int h, int w, const uint32_t* huff, uint8_t* out, int64_t out_stride,
                     int64_t* lengths, void* workspace, void* stream);

/* ---- decoding (csrc/jpeg_decode.hip): the pixels of Pillow's Image.open(fp).convert("RGB") for a baseline file (DESIGN.md "K17c") ----
 * In scope: SOF0, 8 bits, Huffman coded, ONE scan, no restart interval; grey, YCbCr 4:4:4, YCbCr 4:2:0 (Y 2x2); any DQT / DHT tables.
 * The host (image_io.jpeg_parse) walks the markers, refuses everything else, removes the byte stuffing and builds the code tables.
 * Two stages, each reachable on its own:
 *   1. scan -> coefficients.  The scan is cut into subsequences of sub_bits bits, one thread each; a decoder state is (bit position
 *      of the next symbol, block position in the MCU, next zigzag index).  w2e_jpeg_decode_sync relaxes the entry states of all
 *      subsequences towards the sequential decoder's (a workgroup of W2E_JPEG_DECODE_GROUP subsequences to its fixed point per
 *      launch); the caller repeats it until the launch's "changed" word stays 0, at most plan[6] times.
 *      w2e_jpeg_decode_coefficients then counts, places and writes the blocks and sums the DC differences (four launches).
 *   2. w2e_jpeg_pixels: dequantisation, libjpeg's accurate integer IDCT, fancy 4:2:0 up-sampling, colour conversion (two launches
 *      through one byte per sample of workspace).
 * Same conventions as above.  The only atomic on global memory is the OR into the "changed" word.  A corrupt scan gives a nonzero
 * status and wrong coefficients, never an access outside a buffer: every read of the scan is clamped to scan_bytes, every loop is
 * bounded by sub_bits, every table index is masked.  libjpeg's warn-and-continue behaviour is NOT reproduced.
 *
 * Geometry.  sampling W2E_JPEG_420: MCUs of 16 x 16 pixels, six blocks Y00 Y01 Y10 Y11 Cb Cr; W2E_JPEG_444: MCUs of 8 x 8, three
 * blocks Y Cb Cr; W2E_JPEG_GREY: MCUs of 8 x 8, one block.  mx = ceil(w / mcu) across, my = ceil(h / mcu) down, in raster order; the
 * blocks outside the image are in the stream and are decoded like any other.  Coefficients: int16 [batch, blocks, 64], zigzag order,
 * scan order -- for a file w2e_jpeg_entropy coded, what w2e_jpeg_coefficients wrote.
 *
 * Inputs of stage 1 (device memory, made by the host):
 *   scan    the unstuffed scans of the batch, each padded with 0xFF to a multiple of 4 bytes; scan_bytes is the size of the whole
 *           buffer (a multiple of 4).  Bits past an image's end read as 1.
 *   meta    int64 [batch, 2]: the byte offset of image b's scan inside `scan` (a multiple of 4) and its length in BITS (8 * bytes,
 *           before the padding; at most scan_bits).
 *   tables  uint32 [batch, 6, W2E_JPEG_TABLE_WORDS]: for component c (0..2; a grey image uses only c = 0) the DC table at
 *           [2 c] and the AC table at [2 c + 1].  One table, in 32-bit words: [0, 256) 512 uint16, entry [next 9 bits] =
 *           (length << 8) | symbol of the code of at most 9 bits that begins them, 0 when there is none; [256, 274) int32
 *           maxcode[0..17] (the largest code of each length 1..16, -1 when the length has none, as libjpeg's jdhuff does;
 *           [0] and [17] unused); [274, 291) int32 valoffset[0..16] (index of the length's first symbol minus its first code);
 *           [320, 384) the symbols in code order, 256 bytes.
 * scan_bits: the largest of the batch's scan lengths in bits; sub_bits: a multiple of 32 in 32..4096. */
#define W2E_JPEG_420 0
#define W2E_JPEG_444 1
#define W2E_JPEG_GREY 2
#define W2E_JPEG_TABLE_WORDS 384
#define W2E_JPEG_DECODE_GROUP 256          /* subsequences that one workgroup of w2e_jpeg_decode_sync relaxes among themselves */
#define W2E_JPEG_MAX_SCAN_BITS 0x7fff0000  /* bit positions are 32-bit: an image whose scan is longer (256 MB) is refused */
#define W2E_JPEG_STATUS_COUNT 1            /* status bits: the blocks in the scan are not the image's count */
#define W2E_JPEG_STATUS_CATEGORY 2         /* a DC category above 11 or an AC size above 10 */
#define W2E_JPEG_STATUS_INSIDE 4           /* the scan ends inside a block */

/* w2e_jpeg_decode_plan (pure host).  plan has 8 entries:
 *   plan[0]  blocks per image
 *   plan[1], plan[2]  mx, my
 *   plan[3]  subsequences per image: n = max(1, ceil(scan_bits / sub_bits))
 *   plan[4]  bytes of workspace of stage 1 for this batch: batch * 16 * (n + ceil(n / W2E_JPEG_DECODE_GROUP)) -- the entry states
 *            int32 [batch, n, 2] = (bit position, slot << 8 | zigzag index) at its start, then the hand-over buffers, the block
 *            counts and the first block of each subsequence
 *   plan[5]  bytes of workspace of w2e_jpeg_pixels for this batch: batch * 64 * blocks (one byte per sample)
 *   plan[6]  the most launches of w2e_jpeg_decode_sync that the relaxation can take: ceil(n / W2E_JPEG_DECODE_GROUP) + 1
 *   plan[7]  int16 elements of the coefficient tensor of one image (64 * blocks)
 * h and w are in 1..W2E_IMAGE_MAX_SIZE, batch in 0..65535. */
int w2e_jpeg_decode_plan(int batch, int h, int w, int sampling, int64_t scan_bits, int sub_bits, int64_t* plan);

/* One launch of the relaxation.  launch: 0 for the first call on a batch (every subsequence starts from its guess), then 1, 2, ...
 * (the entry states of the launch before are in the workspace).  changed: one int32 that is 0 before the call; nonzero after it when
 * another launch is needed.  workspace: plan[4] bytes, 8-byte aligned, kept between the calls and handed to
 * w2e_jpeg_decode_coefficients. */
int w2e_jpeg_decode_sync(const uint8_t* scan, const int64_t* meta, const uint32_t* tables, int64_t scan_bytes, int batch, int h, int w,
                         int sampling, int64_t scan_bits, int sub_bits, int launch, void* workspace, int32_t* changed, void* stream);

/* After the relaxation: coef int16 [batch, blocks, 64], 16-byte aligned, every element written exactly once when status is 0;
 * status int32 [batch], an OR of the W2E_JPEG_STATUS_ bits. */
int w2e_jpeg_decode_coefficients(const uint8_t* scan, const int64_t* meta, const uint32_t* tables, int64_t scan_bytes, int batch, int h, int w,
                                 int sampling, int64_t scan_bits, int sub_bits, void* workspace, int16_t* coef, int32_t* status, void* stream);

/* Stage 2.  coef: as stage 1 writes it.  qtables: int32 [batch, 3, 64], natural (row-major) order, one table per component (a grey
 * image uses only the first).  out: uint8 [batch, h, w, 3], 4-byte aligned.  workspace: plan[5] bytes, 16-byte aligned. */
int w2e_jpeg_pixels(const int16_t* coef, const int32_t* qtables, int batch, int h, int w, int sampling, uint8_t* out, void* workspace,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif
