/* libmavflow -- JPEG decode on the device: a baseline (SOF0, Huffman) file goes up as it is; the host reads its segments up to SOS and
 * never touches the entropy bytes.  Restart-interval search, Huffman decoding, dequantisation, the exact "islow" IDCT, "fancy" triangle
 * upsampling and the fixed-point YCbCr -> RGB conversion run on the device, and the frames appear in device memory where the gray
 * conversion and Farneback read.  No pixel crosses PCIe.  The arithmetic is libjpeg-turbo's (what Pillow and the cv2 wheels bundle):
 * integers from the bit stream to the BGR byte, so the gate is EQUAL BYTES.
 *
 * The rules of mavflow_png_decode.h hold: the entry points KEEP everything a context holds resident, run on the context's stream, write
 * only what the caller passes in and hold no device memory of the context's.  The `_dev` form takes device pointers, allocates nothing
 * and only enqueues; the host form takes staging blocks behind the last call's, runs, synchronises and gives the blocks back.
 * 0 = OK, < 0 = MAV_ERR_*, mav_last_error() has the message.  A refused call has enqueued and written nothing.
 *
 * FILES ACCEPTED.  SOF0, 8-bit samples, ONE interleaved scan; one component (gray) or three (YCbCr) with chroma 1 x 1 and luma 1 x 1
 *   (4:4:4), 2 x 1 (4:2:2) or 2 x 2 (4:2:0); up to four 8-bit quantisation tables; DC and AC Huffman tables 0 - 3; any DRI; any APPn / COM.
 *   NOT accepted: every other SOFn (SOF2, progressive, is the follow-up), arithmetic coding, 16-bit quantisation tables, four
 *   components, any other sampling, more than one scan, an Adobe APP14 segment with transform 0, component ids 'R', 'G', 'B'.
 *   mav_jpeg_parse refuses those with MAV_JPEG_E_UNSUPPORTED and mav_last_error() names the marker; a file that ends inside a segment
 *   or before SOS is MAV_JPEG_E_TRUNCATED.  (Both are > 0: verdicts on the file, not MAV_ERR_*.)
 *
 * mav_jpeg_parse is host code and needs no context.  It walks the segments up to SOS and no further and fills a fixed-size
 *   mav_jpeg_info: W, H, the components (h, v, quantisation table, DC table, AC table), the quantisation tables in NATURAL order, the
 *   Huffman tables as their 16 counts and up to 256 values, the restart interval, the byte offset of the entropy segment in the file
 *   and what remains of the file behind that offset.  It checks that segment lengths stay inside the file, that a table's counts sum
 *   to <= 256, that a code set is not over-subscribed, that the scan's table ids exist and that Ss, Se, Ah/Al = 0, 63, 0.
 *
 * IMAGES of a call share W, H and the component count (the CALL'S OWN sizes, not the context's); sampling, tables and restart interval
 *   are each image's own.  `count` runs from 1 to MAV_JPEG_MAX_COUNT and is independent of the context's max_batch.  `files` holds the
 *   files' bytes, `index` count x (offset, size) pairs of uint64 -- file i is files[offset .. offset + size) -- and info[i] is
 *   mav_jpeg_parse's answer for file i.  An info the parser would not have produced (other sizes than the call's, an undefined table,
 *   an entropy segment outside the file) is MAV_JPEG_E_UNSUPPORTED for that image.  The entry points take no component count: THE
 *   CALL'S COMPONENT COUNT IS IMAGE 0's (info[0].components; 3, or else 1), `out` and `scratch` are sized by it, and an image of
 *   another count is UNSUPPORTED.
 *
 * OUTPUT.  out = count images of H x W x c bytes:
 *     MAV_JPEG_OUT_SAMPLES  c = components: the upsampled Y, Cb, Cr before the colour conversion.
 *     MAV_JPEG_OUT_BGR      c = 3: what cv2.imread returns (gray replicated).
 *     MAV_JPEG_OUT_GRAY     c = 1: cv2.cvtColor(imread(...), COLOR_BGR2GRAY) through the one function the context's gray conversion uses,
 *                           (B * 1868 + G * 9617 + R * 4899 + 8192) >> 14; a gray file passes its sample through.  It is NOT
 *                           IMREAD_GRAYSCALE, which hands out libjpeg's Y plane.
 *
 * STATUS.  One mav_jpeg_status per image: `code` 0 or MAV_JPEG_E_*, and counters with which a test proves it reached its corner: the
 *   restart intervals the image has, the MCUs decoded, the nonzero AC and DC-difference coefficients, the ZRL symbols, the stuffed
 *   bytes (FF 00) fetched, the longest code a symbol used, and `consumed`: the entropy bytes up to the end of the last interval (of
 *   the failing interval, when there is one).  Every interval is decoded, whatever another one's verdict, and the counters sum over
 *   all of them.  WHICH ERROR an image reports is the one in its LOWEST restart interval, and within that interval the first a reader
 *   meets.  Host and device compute the status from the same source.
 *     TRUNCATED    the entropy bytes end (or a marker that is no RSTn stands) inside an MCU
 *     CODE         16 bits that are no code of the table
 *     COEF_INDEX   a run past coefficient 63
 *     RESTART      an RSTn missing where the interval ends, carrying the wrong number, or present where none is due
 *     UNSUPPORTED  an `info` the parser would not have produced
 *   AN IMAGE WHOSE CODE IS NOT 0 LEAVES ITS WHOLE OUTPUT AS ZERO BYTES and the call returns 0, as with the PNG decoder.  libjpeg itself
 *   warns and carries on with such files (it feeds zero bits, resynchronises at the next marker); this decoder does not follow it.
 *   Nor does it follow libjpeg's range table where IDCT output + 128 leaves [-256, 639]: that table wraps, this decoder clamps.
 *
 * SCRATCH of the _dev form: mav_jpeg_decode_scratch_bytes(W, H, components, count) bytes aligned to 16 (0 for a bad argument): per
 *   image, with bw = 2 ceil(W / 16) and bh = 2 ceil(H / 16) blocks (every component at full resolution on a grid of whole 16 x 16
 *   MCUs, the worst case of the samplings accepted), components x bw x bh x 64 int16 coefficients, components x 8 bw x 8 bh plane
 *   bytes, a header of 16 bytes and the interval table of bw x bh rows of 16 bytes.  Written in full before it is read.
 * mav_jpeg_decode_host: the same decoding source on the host, serially, no context, no GPU; MAV_OK when it ran (the verdict is
 *   status->code), MAV_ERR_ARG for a NULL argument. */
#ifndef MAVFLOW_JPEG_H
#define MAVFLOW_JPEG_H
#include "mavflow.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MAV_JPEG_MAX_COUNT 1024

#define MAV_JPEG_OUT_SAMPLES 0
#define MAV_JPEG_OUT_BGR 1
#define MAV_JPEG_OUT_GRAY 2

#define MAV_JPEG_E_TRUNCATED 1
#define MAV_JPEG_E_CODE 2
#define MAV_JPEG_E_COEF_INDEX 3
#define MAV_JPEG_E_RESTART 4
#define MAV_JPEG_E_UNSUPPORTED 5

typedef struct mav_jpeg_component {
    uint8_t id, h, v, tq, td, ta, pad[2];
} mav_jpeg_component;             /* 8 bytes */

typedef struct mav_jpeg_huffman {
    uint8_t counts[16];           /* codes of length 1 .. 16 */
    uint8_t values[256];          /* the symbols in code order */
} mav_jpeg_huffman;               /* 272 bytes */

typedef struct mav_jpeg_info {
    int32_t W, H, components, restart_interval;
    uint64_t entropy_offset, entropy_bytes;       /* the first byte behind SOS; what remains of the file from there */
    mav_jpeg_component comp[4];                   /* [components] used */
    uint8_t quant_defined[4], dc_defined[4], ac_defined[4], pad[4];
    uint8_t quant[4][64];                         /* natural order */
    mav_jpeg_huffman dc[4], ac[4];
} mav_jpeg_info;                  /* 2512 bytes */

typedef struct mav_jpeg_status {
    int32_t code;
    uint32_t intervals;
    uint64_t consumed;
    uint32_t mcus, nonzero, zrl, stuffed, max_code_len, pad;
} mav_jpeg_status;                /* 40 bytes */

int mav_jpeg_parse(const uint8_t* file, size_t n, mav_jpeg_info* info);
size_t mav_jpeg_decode_scratch_bytes(int W, int H, int components, int count);
int mav_jpeg_decode_dev(mav_ctx*, const uint8_t* files_dev, const uint64_t* index_dev /* count x (offset, size) */, const mav_jpeg_info* info_dev,
                        int count, int W, int H, int out_format, uint8_t* out_dev, mav_jpeg_status* status_dev, void* scratch);   /* enqueue only */
int mav_jpeg_decode(mav_ctx*, const uint8_t* files_host, const uint64_t* index_host, const mav_jpeg_info* info_host, int count, int W, int H,
                    int out_format, uint8_t* out_host, mav_jpeg_status* status_host);                               /* host in / out, synchronous */
int mav_jpeg_decode_host(const uint8_t* file, size_t n, const mav_jpeg_info* info, int out_format, uint8_t* out, mav_jpeg_status* status);

#ifdef __cplusplus
}
#endif
#endif
