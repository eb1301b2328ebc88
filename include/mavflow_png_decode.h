/* libmavflow -- PNG decode on the device: the zlib stream of a file's IDAT chunks goes up as it is, is inflated (RFC 1950 / 1951), checked
 * against its Adler-32, un-filtered (PNG filters 0 - 4) and converted, and the frames appear in device memory where the gray conversion
 * and Farneback read.  No pixel crosses PCIe.  Chunk parsing stays host code (mavflow/frame_source.py).
 *
 * The rules of mavflow_shapes.h hold: the entry points KEEP everything a context holds resident, run on the context's stream, write
 * only what the caller passes in and hold no device memory of the context's.  The `_dev` form takes device pointers, allocates nothing
 * and only enqueues; the host form takes staging blocks behind the last call's, runs, synchronises and gives the blocks back.
 * 0 = OK, < 0 = MAV_ERR_*, mav_last_error() has the message.  A refused call has enqueued and written nothing.
 *
 * IMAGES.  W and H are the CALL'S OWN, not the context's (segmentation and half-resolution prediction files have other sizes than the
 *   frames); `channels` = samples per pixel of the files, 1 gray / 2 gray + alpha / 3 RGB / 4 RGBA, 8 bits each, not interlaced.  `count`
 *   runs from 1 to MAV_PNG_DECODE_MAX_COUNT and is independent of the context's max_batch.  Every stream of a call inflates to exactly
 *   raw = H * (1 + W * channels) bytes: per row a filter-type byte and W * channels filtered bytes.
 *
 * STREAMS.  `streams` holds the zlib streams, `index` count x (offset, size) pairs of uint64 -- the layout the encoder's index has, so
 *   an encode call's outputs are a decode call's inputs as they are.  The streams may lie anywhere in `streams` and may overlap (the host
 *   form copies the bytes up to the largest offset + size); a size of 0 is a TRUNCATED stream.  Bytes behind the Adler-32 are ignored,
 *   as zlib.decompress ignores them, and show in `consumed` (which stops at the trailer's end).
 *
 * THE VERDICTS are zlib's own (inflate's, inftrees.c's): CM = 8, CINFO <= 7, FDICT clear, header a multiple of 31; an over-subscribed
 *   set of code lengths is an error; an incomplete set is an error unless no code of it is longer than one bit -- which leaves the
 *   distance set of one code of length 1 or of no code at all, and (as in zlib) the literal/length set whose only code is end-of-block;
 *   a missing end-of-block code is an error; HLIT above 29 or HDIST above 29 is an error; a decoded symbol without a code (the unused
 *   half of a one-code set, literal/length 286 / 287, distance 30 / 31) is an error; a distance further back than the bytes written
 *   is an error.  Other than zlib, the decoder knows the size it must produce: more is OVERFLOW, less is SHORT.  Which of two errors
 *   of one stream is reported is the order of the stream's bytes: the first that a reader of the stream meets.
 *
 * STATUS.  One mav_png_status per stream: `code` 0 or MAV_PNG_E_*; the Adler-32 the stream carries and the one computed from the bytes
 *   written (both 0 when the stream failed before its trailer); bytes consumed (header, blocks and trailer) and produced; the blocks met
 *   by type (stored, fixed, dynamic); the longest match and the farthest distance.  The same source computes them on host and device.
 *   AN IMAGE WHOSE CODE IS NOT 0 LEAVES ITS WHOLE OUTPUT AS ZERO BYTES, so that nothing downstream reads garbage; the call itself
 *   returns 0 -- the statuses are the caller's to read (the host form brings them back; the Python binding raises on them).
 *
 * OUTPUT.  out = count images of H x W x c bytes:
 *     MAV_PNG_OUT_SAMPLES  c = channels: the file's own samples.
 *     MAV_PNG_OUT_BGR      c = 3: what cv2.imread returns -- gray replicated, alpha dropped, RGB swapped.
 *     MAV_PNG_OUT_GRAY     c = 1: cv2.cvtColor(imread, COLOR_BGR2GRAY), through the one function the context's gray conversion uses
 *                          ((B * 1868 + G * 9617 + R * 4899 + 8192) >> 14), so the bits agree; gray files pass their sample through
 *                          (the formula maps (g, g, g) to g: the weights sum to 2^14).
 *
 * SCRATCH of the _dev form: mav_png_decode_scratch_bytes(W, H, channels, count) bytes aligned to 16 (0 for a bad argument); written in
 *   full before it is read.  mav_png_inflate_host: the same inflate source with a serial copy, no context, no GPU; returns MAV_OK when it
 *   ran (the verdict is status->code) and MAV_ERR_ARG for a NULL argument. */
#ifndef MAVFLOW_PNG_DECODE_H
#define MAVFLOW_PNG_DECODE_H
#include "mavflow.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MAV_PNG_DECODE_MAX_COUNT 1024

#define MAV_PNG_OUT_SAMPLES 0
#define MAV_PNG_OUT_BGR 1
#define MAV_PNG_OUT_GRAY 2

#define MAV_PNG_E_HEADER 1        /* zlib header: CM, CINFO, FDICT or FCHECK */
#define MAV_PNG_E_TRUNCATED 2     /* the stream ends inside a field */
#define MAV_PNG_E_BLOCK_TYPE 3    /* block type 3 */
#define MAV_PNG_E_STORED_LEN 4    /* a stored block's length and its complement disagree */
#define MAV_PNG_E_CODE_LENGTHS 5  /* a code-length set zlib refuses, a repeat with nothing before it or past the end */
#define MAV_PNG_E_SYMBOL 6        /* a symbol without a code: literal/length 286 / 287, distance 30 / 31, an unused code */
#define MAV_PNG_E_DISTANCE 7      /* a distance further back than the output written */
#define MAV_PNG_E_OVERFLOW 8      /* more bytes than the image holds */
#define MAV_PNG_E_SHORT 9         /* fewer */
#define MAV_PNG_E_ADLER 10        /* the Adler-32 of the bytes written is not the stream's */
#define MAV_PNG_E_FILTER 11       /* a filter-type byte above 4 (set by the un-filter pass) */

typedef struct mav_png_status {
    int32_t code;
    uint32_t adler_stream, adler_computed;
    uint32_t blocks[3];           /* stored, fixed, dynamic */
    uint64_t consumed, produced;
    uint32_t max_length, max_distance;
} mav_png_status;                 /* 48 bytes */

size_t mav_png_decode_scratch_bytes(int W, int H, int channels, int count);
int mav_png_decode_dev(mav_ctx*, const uint8_t* streams_dev, const uint64_t* index_dev /* count x (offset, size) */, int count, int W, int H,
                       int channels, int out_format, uint8_t* out_dev, mav_png_status* status_dev, void* scratch);   /* enqueue only */
int mav_png_decode(mav_ctx*, const uint8_t* streams_host, const uint64_t* index_host, int count, int W, int H, int channels,
                   int out_format, uint8_t* out_host, mav_png_status* status_host);                                  /* host in / out, synchronous */
int mav_png_inflate_host(const uint8_t* z, size_t n, uint8_t* raw, size_t raw_bytes, mav_png_status* status);

#ifdef __cplusplus
}
#endif
#endif
