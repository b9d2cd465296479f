/* w2e_jpeg.h -- C ABI of the baseline-JPEG encoder (csrc/jpeg.hip) in libw2e.so (gfx950): the file that torchvision 0.8.2's
 * `save_image(x, "name.jpg", ...)` writes through Pillow's default JPEG (libjpeg: quality 75, 4:2:0, the Annex K Huffman tables, no
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

#ifdef __cplusplus
}
#endif
#endif
