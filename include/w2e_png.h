/* w2e_png.h -- C ABI of the PNG decoder (csrc/png.hip, csrc/png_core.h) in libw2e.so (gfx950): the pixels of Pillow's
 * Image.open(fp) and Image.open(fp).convert("RGB") for the files the reference reads -- the CelebAMask-HQ parsing labels and the
 * demo's portraits (DESIGN.md "K17d").  PNG is lossless, so the answer is exact.
 * In scope: non-interlaced; colour types 0 (grey), 2 (RGB), 4 (grey + alpha), 6 (RGBA) at 8 bits, colour type 3 (palette) at 1, 2, 4
 * and 8 bits; all five row filters; zlib streams with stored, fixed and dynamic blocks and any window size.  The host
 * (image_io.png_parse) walks the chunks, verifies their CRCs, refuses everything else, joins the IDAT payloads and checks the two zlib
 * header bytes; only the compressed stream and the palette cross to the device.  Two stages, each reachable on its own:
 *   1. w2e_png_inflate: a batch of zlib streams -> the filtered rows of each (one launch; one wave per stream, the 32 KiB window as a
 *      ring in LDS, the decode tables in LDS, matches copied by all lanes, the Adler-32 checked);
 *   2. w2e_png_pixels: filtered rows -> pixels (one launch; one wave per image takes bands of W2E_PNG_BAND rows, lane r on row y0 + r
 *      one pixel behind lane r - 1, so that the row above arrives by a lane shuffle).
 * Same conventions as w2e_jpeg.h: device pointers, caller-allocated outputs, asynchronous on `stream` (void*), no allocation, copy,
 * memset or global atomic inside, 0 = OK, otherwise w2e_last_error(); arguments are checked before any HIP call.  No workgroup waits
 * on another.  A corrupt stream gives a nonzero status and garbage pixels, never an access outside a buffer and never an unbounded
 * loop (csrc/png_core.h: the rules). */
#ifndef W2E_PNG_H
#define W2E_PNG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define W2E_PNG_BAND 64            /* rows that the wave of stage 2 takes at once (its lanes) */
#define W2E_PNG_MODE_RGB 0         /* out is uint8 [batch, h, w, 3]: grey replicated, alpha dropped, the palette looked up */
#define W2E_PNG_MODE_RAW 1         /* out is uint8 [batch, h, w, channels]: 1 for grey and palette (the index), 2 LA, 3 RGB, 4 RGBA */
#define W2E_PNG_INFLATE_LDS 40960  /* an upper bound of the LDS of one workgroup of stage 1, in bytes: four streams per CU */

/* status bits (int32 per image; stage 1 writes the word, stage 2 ORs into it) */
#define W2E_PNG_STATUS_TYPE 1        /* a block of type 3 */
#define W2E_PNG_STATUS_STORED 2      /* a stored block whose LEN and NLEN disagree */
#define W2E_PNG_STATUS_LENGTHS 4     /* a bad code-length set: over-subscribed, HLIT > 286, HDIST > 30, a repeat with nothing before it
                                        or past the end, a code-length code that matches no symbol, no end-of-block code */
#define W2E_PNG_STATUS_CODE 8        /* a code that matches no symbol, a length symbol 286 / 287, a distance symbol 30 / 31 */
#define W2E_PNG_STATUS_DISTANCE 16   /* a distance that reaches before the start of the output */
#define W2E_PNG_STATUS_INPUT 32      /* the input ends inside the stream (or the stream is not inside the buffer) */
#define W2E_PNG_STATUS_SHORT 64      /* the stream ends before the expected size */
#define W2E_PNG_STATUS_LONG 128      /* the stream goes on past the expected size */
#define W2E_PNG_STATUS_ADLER 256     /* the Adler-32 of the inflated bytes is not the stream's */
#define W2E_PNG_STATUS_FILTER 512    /* a filter byte above 4 */

/* w2e_png_plan (pure host).  colour: the PNG colour type 0, 2, 3, 4 or 6; depth: 8, or 1 / 2 / 4 / 8 for colour 3.  plan has 8 entries:
 *   plan[0]  bytes of one filtered row, its filter byte included: 1 + ceil(w * bits per pixel / 8)
 *   plan[1]  the inflated size of one image: h * plan[0]
 *   plan[2]  raw_pitch: plan[1] rounded up to a multiple of 4
 *   plan[3]  channels of `out` in this mode
 *   plan[4]  bytes of `out` for one image: h * w * plan[3]
 *   plan[5]  the filters' pixel distance in bytes (1, 2, 3 or 4)
 *   plan[6]  W2E_PNG_INFLATE_LDS
 *   plan[7]  W2E_PNG_BAND
 * h and w are in 1..W2E_IMAGE_MAX_SIZE (w2e_image.h), batch in 0..65535. */
int w2e_png_plan(int batch, int h, int w, int colour, int depth, int mode, int64_t* plan);

/* Stage 1.  streams: the zlib streams of the batch in one buffer (4-byte aligned, stream_bytes long, a multiple of 4), each from its
 * two header bytes to its Adler-32.  meta: int64 [batch, 2] = the byte offset of stream b (a multiple of 4) and its length in bytes.
 * sizes: int64 [batch], the exact number of bytes stream b inflates to (at most raw_pitch).  raw: uint8 [batch, raw_pitch] (4-byte
 * aligned, raw_pitch a multiple of 4): bytes [0, sizes[b]) of row b are written when status is 0, never any other.  status: int32
 * [batch], written for every stream. */
int w2e_png_inflate(const uint8_t* streams, const int64_t* meta, const int64_t* sizes, int64_t stream_bytes, int batch, uint8_t* raw,
                    int64_t raw_pitch, int32_t* status, void* stream);

/* Stage 2.  raw: uint8 [batch, raw_pitch], the h filtered rows of each image as stage 1 wrote them (raw_pitch >= plan[1]); the kernel
 * keeps the reconstructed last row of every band in it, so it is NOT preserved.  palette: uint32 [batch, 256], entry = R | G << 8 |
 * B << 16, 0 past the end of PLTE (read only for colour 3 in RGB mode; it may be null otherwise).  out: plan[4] bytes per image.
 * status: int32 [batch]; W2E_PNG_STATUS_FILTER is ORed into it (the row is then taken as unfiltered). */
int w2e_png_pixels(uint8_t* raw, int64_t raw_pitch, const uint32_t* palette, int batch, int h, int w, int colour, int depth, int mode,
                   uint8_t* out, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
