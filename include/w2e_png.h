/* w2e_png.h -- C ABI of the PNG decoder (csrc/png.hip, csrc/png_core.h) and, further down, of the PNG encoder in libw2e.so (gfx950).
 * Decoding: the pixels of Pillow's
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

/* ---- encoding (csrc/png_encode.hip, csrc/png_deflate_core.h; DESIGN.md "K17e") ----
 * The file of `Image.fromarray(x).save(fp, "PNG")` for Pillow's modes L, LA, RGB and RGBA up to the compressed bytes: the filtered rows
 * are Pillow's byte for byte (its adaptive filter choice), the deflate stream is this library's own.  Non-interlaced, 8 bits, colour types
 * 0 / 4 / 2 / 6 for 1 / 2 / 3 / 4 channels.  The host (image_io.to_png) adds the signature, IHDR, the framing of the one IDAT and IEND.
 * Out of scope: palette and sub-8-bit output, 16 bits, interlacing, ancillary chunks, matches across chunk boundaries, Pillow's
 * `optimize` and `compress_level`.  Two stages, each reachable on its own:
 *   1. w2e_png_filter: pixels -> filtered rows, filter byte included (one launch; one wave per row scores None, Sub, Up and Paeth by the
 *      sum of min(v, 256 - v) over the row's filtered bytes and takes the smallest; on a tie Up wins over Sub, otherwise the lower number);
 *   2. w2e_png_deflate: filtered bytes -> one zlib stream per image (two launches).  The input is cut into chunks of W2E_PNG_CHUNK bytes;
 *      no match reaches before its chunk, so one workgroup codes one chunk into a slot of the workspace: ONE deflate block, the cheapest
 *      of stored, fixed and dynamic by bit cost, then -- unless it is the image's last, which carries BFINAL -- an empty stored block
 *      (zlib's sync-flush marker) that ends the slot on a byte boundary.  The second launch sums the slot lengths of an image in order,
 *      gathers the slots behind the two header bytes and appends the Adler-32, combined from the chunks' (s1, s2, length).
 * The conventions above hold: nothing inside allocates, copies, memsets or uses a global atomic; no workgroup waits on another; the same
 * input gives the same bytes on every run, and the bytes of tests/png_deflate_host.cpp, which runs the same core with one lane. */
#define W2E_PNG_CHUNK 32768        /* bytes of input that one workgroup of stage 2 codes */
#define W2E_PNG_SLOT 32780         /* bytes of a chunk's slot: the stored form's W2E_PNG_CHUNK + 10, rounded up to a multiple of 4 */
#define W2E_PNG_DEFLATE_LDS 61440  /* an upper bound of the LDS of one workgroup of stage 2, in bytes: two chunks per CU */

/* w2e_png_deflate_plan (pure host): a batch of buffers of at most max_size bytes (0..2^31-1) each.  plan has 4 entries:
 *   plan[0]  chunks per image: max(1, ceil(max_size / W2E_PNG_CHUNK))
 *   plan[1]  W2E_PNG_SLOT
 *   plan[2]  workspace bytes: batch * plan[0] * (W2E_PNG_SLOT + 4 * W2E_PNG_CHUNK + 16) -- slots, token lists, (length, s1, s2, n)
 *   plan[3]  the largest possible stream, from the stored form: max_size + 10 * plan[0] + 6 */
int w2e_png_deflate_plan(int batch, int64_t max_size, int64_t* plan);

/* w2e_png_encode_plan (pure host).  channels: 1 (L), 2 (LA), 3 (RGB) or 4 (RGBA).  plan has 8 entries:
 *   plan[0]  bytes of one filtered row, its filter byte included: 1 + w * channels
 *   plan[1]  the filtered size of one image: h * plan[0]
 *   plan[2]  raw_pitch: plan[1] rounded up to a multiple of 4
 *   plan[3]  chunks per image          \
 *   plan[4]  slot bytes per chunk       | w2e_png_deflate_plan(batch, plan[1])
 *   plan[5]  workspace bytes            |
 *   plan[6]  the largest possible stream/
 *   plan[7]  out_pitch: plan[6] rounded up to a multiple of 4
 * h and w are in 1..W2E_IMAGE_MAX_SIZE (w2e_image.h), batch in 0..65535. */
int w2e_png_encode_plan(int batch, int h, int w, int channels, int64_t* plan);

/* Stage 1.  x: uint8 [batch, h, w, channels].  raw: uint8 [batch, raw_pitch], raw_pitch >= plan[1]: bytes [0, plan[1]) of every row are
 * written, never any other. */
int w2e_png_filter(const uint8_t* x, int batch, int h, int w, int channels, uint8_t* raw, int64_t raw_pitch, void* stream);

/* Stage 2.  raw: uint8 [batch, raw_pitch] (4-byte aligned, raw_pitch a multiple of 4 and >= max_size).  sizes: int64 [batch], the bytes of
 * buffer b (taken as 0 below 0 and as max_size above it).  out: uint8 [batch, out_pitch] (4-byte aligned, out_pitch a multiple of 4 and >=
 * plan[3] of w2e_png_deflate_plan(batch, max_size)); lengths: int64 [batch], the bytes of stream b.  work: plan[2] bytes, 8-byte aligned;
 * it needs no initialisation. */
int w2e_png_deflate(const uint8_t* raw, int64_t raw_pitch, const int64_t* sizes, int batch, int64_t max_size, uint8_t* out, int64_t out_pitch,
                    int64_t* lengths, uint8_t* work, int64_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
