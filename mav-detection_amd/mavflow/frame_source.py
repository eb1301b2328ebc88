"""Frame decode in front of the path: the reference reads its frames with cv2.VideoCapture over `{img_path}/image_%05d.png`
(/root/reference/src/datasets/dataset.py:26,38,57,223-230) and hands them to Farneback as BGR u8 arrays (src/farneback.py:17-21,73-74).
cv2 is not part of this build; this module is that capture for PNG sequences:

    decode_png(bytes) -> u8 array        chunk parsing + zlib inflate (Python stdlib), un-filtering in libmavflow (mav_png_unfilter:
                                         two of PNG's five filters are per-pixel recurrences).  Every colour type (gray, gray + alpha,
                                         RGB, RGBA, palette) at every legal bit depth (1 / 2 / 4 / 8 / 16), non-interlaced and Adam7
                                         interlaced; 16-bit samples are narrowed to their high byte, which is what cv2.imread's
                                         default flag does (libpng's png_set_strip_16).
    imread(path) -> BGR u8 (H, W, 3)     what cv2.imread(path) (IMREAD_COLOR) returns: gray replicated, alpha dropped, palette expanded.
    png_wrap(W, H, channels, zstream)    the PNG file around a zlib stream of scanline data that was deflated elsewhere (on the device:
                                         Context.png_encode / render_last_png / overlay_last_png).
    PngSequenceCapture(pattern)          cv2.VideoCapture(pattern)'s read() / get(3|4|7) / isOpened() / release() for an image sequence;
                                         decoder="device" decodes `ahead` files per device call.
    imread_many(files, ctx, out)         imread over a list: 8-bit non-interlaced gray / RGB (+ alpha) files are inflated, un-filtered and
                                         converted on the device (include/mavflow_png_decode.h), the rest by decode_png.  A file that
                                         starts with FF D8 is a JPEG: baseline files are decoded on the device (include/mavflow_jpeg.h),
                                         the rest are refused with the parser's reason.
    jpg_to_png(img_path, ctx)            the reference's Dataset.jpg_to_png (src/datasets/dataset.py:240-248): N.jpg -> image_%05d.png,
                                         decoded and encoded on the device.

The decoder is pinned by PIL-decoded fixtures generated in the build container (tools/gen_png_fixtures.py,
tests/golden/png_frames.npz), 16-bit and interlaced files included (round 6).
"""
from __future__ import annotations

import os
import struct
import zlib
from typing import Optional, Tuple

import numpy as np

from . import _lib

PNG_MAGIC = b"\x89PNG\r\n\x1a\n"
JPEG_MAGIC = b"\xff\xd8"
_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}          # colour type -> samples per pixel


def png_chunks(data: bytes, crc: str = "all"):
    """The chunk walk of a PNG file: (IHDR fields, PLTE (n, 3) u8 or None, tRNS u8 or None, [(offset, length) of every IDAT body in
    `data`]).  crc="all": every chunk's CRC is checked as it is met; crc="small": every chunk's but IDAT's (the device route, which
    checks the Adler-32 of the inflated bytes instead).  ValueError for a bad signature, a truncated chunk, a CRC mismatch, a file
    without IHDR or IDAT."""
    if data[:8] != PNG_MAGIC:
        raise ValueError("not a PNG file (bad signature)")
    pos = 8
    ihdr = None
    idat = []
    plte = trns = None
    while pos + 8 <= len(data):
        (length,), kind = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        if pos + 12 + length > len(data):
            raise ValueError("truncated PNG chunk")
        body = None if kind == b"IDAT" and crc == "small" else data[pos + 8:pos + 8 + length]
        if body is not None:
            (want,) = struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])
            if zlib.crc32(kind + body) & 0xFFFFFFFF != want:
                raise ValueError(f"PNG chunk {kind!r}: CRC mismatch")
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append((pos + 8, length))
        elif kind == b"PLTE":
            plte = np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif kind == b"tRNS":
            trns = np.frombuffer(body, np.uint8)
        pos += 12 + length
        if kind == b"IEND":
            break
    if ihdr is None or not idat:
        raise ValueError("PNG without IHDR / IDAT")
    return ihdr, plte, trns, idat


def device_eligible(ihdr) -> bool:
    """What the device decoder takes (include/mavflow_png_decode.h): 8-bit samples, gray / RGB / gray + alpha / RGBA, not interlaced.
    Everything else -- 16-bit samples, depths below 8, palette, Adam7 -- stays on decode_png."""
    W, H, depth, ctype, comp, filt, interlace = ihdr
    return depth == 8 and ctype in (0, 2, 4, 6) and comp == 0 and filt == 0 and interlace == 0 and W >= 1 and H >= 1


def decode_png(data: bytes) -> Tuple[np.ndarray, int]:
    """(pixels, colour type): pixels u8 (H, W) for gray / (H, W, 2) gray + alpha / (H, W, 3) RGB / (H, W, 4) RGBA; palette images
    come back expanded to RGB (or RGBA when the file has a tRNS chunk), colour type 2 / 6."""
    ihdr, plte, trns, spans = png_chunks(data)
    idat = [data[o:o + n] for o, n in spans]
    W, H, depth, ctype, comp, filt, interlace = ihdr
    if ctype not in _CHANNELS or comp != 0 or filt != 0:
        raise ValueError(f"unsupported PNG header (colour type {ctype}, compression {comp}, filter method {filt})")
    if interlace not in (0, 1):
        raise ValueError(f"unknown PNG interlace method {interlace}")
    if depth not in (1, 2, 4, 8, 16) or (depth < 8 and ctype not in (0, 3)) or (depth == 16 and ctype == 3):
        raise ValueError(f"invalid PNG bit depth {depth} for colour type {ctype}")
    ch = _CHANNELS[ctype]
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8)
    lib = _lib.load()

    def samples(off, pw, ph):
        """one (sub-)image of pw x ph pixels starting at byte `off` of the inflated stream -> ((ph, pw * ch) u8 sample values, next offset)"""
        stride = (pw * ch * depth + 7) // 8
        n = ph * (stride + 1)
        if off + n > len(raw):
            raise ValueError(f"PNG image data holds {len(raw)} bytes, more expected")
        rows = np.empty((ph, stride), np.uint8)
        _lib.check(lib.mav_png_unfilter(raw[off:off + n].ctypes.data, ph, stride, max(1, ch * depth // 8), rows.ctypes.data))
        if depth == 8:
            v = rows
        elif depth == 16:                            # big-endian 16-bit samples -> their high byte (png_set_strip_16)
            v = np.ascontiguousarray(rows.reshape(ph, pw * ch, 2)[..., 0])
        else:                                        # samples packed most significant bit first
            bits = np.unpackbits(rows, axis=1)[:, :pw * depth].reshape(ph, pw, depth)
            v = np.zeros((ph, pw), np.uint8)
            for b in range(depth):
                v = (v << 1) | bits[..., b]
        return v, off + n

    if interlace == 0:
        out, end = samples(0, W, H)
    else:                                            # Adam7: seven reduced images, each filtered on its own, scattered onto the 8 x 8 lattice
        out = np.empty((H, W * ch), np.uint8)
        grid = out.reshape(H, W, ch)
        end = 0
        for x0, y0, dx, dy in ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)):
            pw, ph = (W - x0 + dx - 1) // dx, (H - y0 + dy - 1) // dy
            if pw <= 0 or ph <= 0:
                continue                             # an empty pass has no bytes at all, not even filter bytes
            v, end = samples(end, pw, ph)
            grid[y0::dy, x0::dx] = v.reshape(ph, pw, ch)
    if end != len(raw):
        raise ValueError(f"PNG image data holds {len(raw)} bytes, {end} expected")
    if depth < 8 and ctype == 0:                     # gray levels scale to 0 .. 255
        out = (out * (255 // ((1 << depth) - 1))).astype(np.uint8)
    out = out.reshape(H, W) if ch == 1 else out.reshape(H, W, ch)
    if ctype == 3:
        if plte is None:
            raise ValueError("palette PNG without PLTE chunk")
        if int(out.max(initial=0)) >= len(plte):
            raise ValueError("palette index out of range")
        rgb = plte[out]
        if trns is not None:
            alpha = np.full(len(plte), 255, np.uint8)
            alpha[:len(trns)] = trns[:len(plte)]
            return np.dstack([rgb, alpha[out]]), 6
        return rgb, 2
    return out, ctype


def imread(path: str) -> Optional[np.ndarray]:
    """cv2.imread(path): BGR u8 (H, W, 3), None when the file does not exist or cannot be read as a PNG or a baseline JPEG.  (Gray
    replicated into three channels, alpha dropped -- IMREAD_COLOR, the flag the reference's calls default to.)  The file's first bytes
    decide: FF D8 goes to mav_jpeg_decode_host (None when the library is not loaded), anything else to decode_png."""
    try:
        with open(path, "rb") as f:
            data = f.read()
        if data[:2] == JPEG_MAGIC:                   # baseline JPEG: the decoding source of the device route, run on the host
            return _lib.jpeg_decode_host(data, "bgr") if _lib.loaded() else None
        px, ctype = decode_png(data)
    except (OSError, ValueError, zlib.error):
        return None
    if ctype in (0, 4):
        g = px if ctype == 0 else px[..., 0]
        return np.repeat(g[..., None], 3, axis=2)
    return np.ascontiguousarray(px[..., 2::-1])      # RGB(A) -> BGR


def _to_out(px: np.ndarray, ctype: int, out: str) -> np.ndarray:
    """decode_png's pixels in one of imread_many's forms, with the arithmetic of the device route"""
    if out == "samples":
        return px
    bgr = np.repeat((px if ctype == 0 else px[..., 0])[..., None], 3, axis=2) if ctype in (0, 4) else np.ascontiguousarray(px[..., 2::-1])
    if out == "bgr":
        return bgr
    b, g, r = (bgr[..., k].astype(np.uint32) for k in range(3))
    return ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(np.uint8)      # cv2.cvtColor(COLOR_BGR2GRAY), as Context.bgr2gray


class ImreadResult:
    """imread_many's answer: frames[k] = file k's array (None: unreadable, as cv2.imread; None as well for a device-route file when
    to_host=False), routes[k] = "device" / "host" (None: unreadable), device[k] = (DeviceBuffer, byte offset, shape) of a frame left
    on the device (to_host=False; free() gives the buffers back), refused[k] = why file k, a JPEG, was not taken: the parser's reason
    (a progressive file, say) or the decoder's verdict."""

    def __init__(self, n: int) -> None:
        self.frames = [None] * n
        self.routes = [None] * n
        self.device = {}
        self.refused = {}
        self._buffers = []

    def free(self) -> None:
        for b in self._buffers:
            b.free()
        self._buffers, self.device = [], {}


def imread_many(paths_or_bytes, ctx, out: str = "bgr", to_host: bool = True, verify_crc: bool = False) -> ImreadResult:
    """cv2.imread over a list of files (paths, or the files' bytes).  Files the device decodes (device_eligible) go up compressed, one
    call per (W, H, channels) group (Context.png_decode); the rest -- and nothing else -- are read by decode_png.  out: "bgr" (cv2.imread),
    "gray" (cvtColor(BGR2GRAY) of it) or "samples" (the file's own channels).  A file neither route can read is None, as cv2.imread's.
    The device route checks the small chunks' CRCs and the Adler-32 of the inflated bytes, and the IDAT CRC only with verify_crc=True:
    a file with a wrong IDAT CRC and intact data decodes there and is None on the host route.
    A file that starts with FF D8 is a JPEG and takes the JPEG route: baseline files go up as they are, one call per (W, H, components)
    group (Context.jpeg_decode; "samples" are then the upsampled Y, Cb, Cr); a file mav_jpeg_parse refuses (a progressive one, say) or
    the decoder refuses is None, and refused[k] holds the reason."""
    if out not in ("bgr", "gray", "samples"):
        raise ValueError(f"imread_many: out must be 'bgr', 'gray' or 'samples', got {out!r}")
    datas = []
    for f in paths_or_bytes:
        if isinstance(f, (bytes, bytearray, memoryview)):
            datas.append(bytes(f))
        else:
            try:
                with open(f, "rb") as fh:
                    datas.append(fh.read())
            except OSError:
                datas.append(None)
    res = ImreadResult(len(datas))
    groups, jpeg_groups = {}, {}
    for k, data in enumerate(datas):
        if data is None:
            continue
        if data[:2] == JPEG_MAGIC:
            info, why = _lib.jpeg_info(data)
            if info is None:
                res.refused[k] = why
            else:
                jpeg_groups.setdefault((int(info["W"][0]), int(info["H"][0]), int(info["components"][0])), []).append(k)
            continue
        try:
            ihdr, _, _, _ = png_chunks(data, "all" if verify_crc else "small")
        except (ValueError, struct.error):
            continue
        if device_eligible(ihdr):
            groups.setdefault((ihdr[0], ihdr[1], ihdr[3]), []).append(k)
        else:
            try:
                res.frames[k] = _to_out(*decode_png(data), out)
                res.routes[k] = "host"
            except (ValueError, zlib.error, struct.error):
                pass
    for members in groups.values():
        for lo in range(0, len(members), _lib.PNG_DECODE_MAX_COUNT):
            part = members[lo:lo + _lib.PNG_DECODE_MAX_COUNT]
            files = [datas[k] for k in part]
            W, H, ch, streams, index = ctx._png_streams(files, verify_crc)
            if to_host:
                imgs, status = ctx.png_decode_streams(streams, index, W, H, ch, out, return_status=True)
                for j, k in enumerate(part):
                    if status["code"][j] == 0:
                        res.frames[k], res.routes[k] = imgs[j], "device"
            else:
                oc = {"samples": ch, "bgr": 3, "gray": 1}[out]
                n = len(part)
                bufs = [ctx.alloc(streams.nbytes).upload(streams), ctx.alloc(index.nbytes).upload(index), ctx.alloc(n * _lib.PNG_STATUS_DTYPE.itemsize),
                        ctx.alloc(ctx.png_decode_scratch_bytes(W, H, ch, n))]
                d_out = ctx.alloc(n * H * W * oc)
                try:
                    ctx.png_decode_dev(bufs[0], bufs[1], n, W, H, ch, out, d_out, bufs[2], bufs[3])
                    status = bufs[2].download(_lib.PNG_STATUS_DTYPE, (n,))
                finally:
                    ctx.sync()
                    for b in bufs:
                        b.free()
                res._buffers.append(d_out)
                for j, k in enumerate(part):
                    if status["code"][j] == 0:
                        res.routes[k] = "device"
                        res.device[k] = (d_out, j * H * W * oc, (H, W) if oc == 1 else (H, W, oc))
    for (W, H, comps), members in jpeg_groups.items():
        for lo in range(0, len(members), _lib.JPEG_MAX_COUNT):
            part = members[lo:lo + _lib.JPEG_MAX_COUNT]
            files = [datas[k] for k in part]
            oc = {"samples": comps, "bgr": 3, "gray": 1}[out]
            if to_host:
                imgs, status = ctx.jpeg_decode(files, out, return_status=True)
            else:
                d_out, _, status = ctx.jpeg_decode_to_device(files, out, return_status=True)
                res._buffers.append(d_out)
            for j, k in enumerate(part):
                code = int(status["code"][j])
                if code:
                    res.refused[k] = f"MAV_JPEG_E_{_lib.JPEG_ERRORS[code]} ({code}) after {int(status['consumed'][j])} bytes of its entropy segment"
                    continue
                res.routes[k] = "device"
                if to_host:
                    res.frames[k] = imgs[j]
                else:
                    res.device[k] = (d_out, j * H * W * oc, (H, W) if oc == 1 else (H, W, oc))
    return res


def jpg_to_png(img_path: str, ctx, png_encoder: str = "device", remove: bool = True) -> dict:
    """The reference's Dataset.jpg_to_png (src/datasets/dataset.py:240-248): every `N.jpg` of the directory becomes `image_%05d.png` with
    N as its index, and the .jpg is removed (remove=False keeps it).  The JPEG files go up compressed and are decoded on the device
    (mav_jpeg_decode_dev); png_encoder="device": the BGR frames stay there as mav_png_encode_dev's input and the PNG files come back
    compressed, so no pixel crosses PCIe (the files must then have the context's size); png_encoder="host": the frames come back and
    are written by imwrite.  Returns {"written": [paths], "refused": {path: reason}}; a refused file is left where it is."""
    if png_encoder not in ("device", "host"):
        raise ValueError(f"png_encoder must be 'device' or 'host', got {png_encoder!r}")
    names = sorted(n for n in os.listdir(img_path) if os.path.splitext(n)[1] == ".jpg")
    for n in names:
        int(n.replace(".jpg", ""))                   # the reference's naming: a file that is no number is an error before anything is written
    groups, refused, written, datas = {}, {}, [], {}
    for n in names:
        with open(os.path.join(img_path, n), "rb") as f:
            datas[n] = f.read()
        info, why = _lib.jpeg_info(datas[n])
        if info is None:
            refused[os.path.join(img_path, n)] = why
        else:
            groups.setdefault((int(info["W"][0]), int(info["H"][0]), int(info["components"][0])), []).append(n)
    for (W, H, comps), members in groups.items():
        if png_encoder == "device" and (W, H) != (ctx.W, ctx.H):
            raise ValueError(f"jpg_to_png: {members[0]} is {W} x {H}, the context (whose PNG encoder is used) is {ctx.W} x {ctx.H}")
        for lo in range(0, len(members), _lib.JPEG_MAX_COUNT):
            part = members[lo:lo + _lib.JPEG_MAX_COUNT]
            files = [datas[n] for n in part]
            if png_encoder == "host":
                imgs, status = ctx.jpeg_decode(files, "bgr", return_status=True)
                pngs = [encode_png(imgs[j]) if status["code"][j] == 0 else None for j in range(len(part))]
            else:
                pngs = _jpeg_to_png_on_device(ctx, files, W, H)
            for n, png in zip(part, pngs):
                src = os.path.join(img_path, n)
                if png is None:
                    refused[src] = "the decoder refused the file"
                    continue
                dst = os.path.join(img_path, f"image_{int(n.replace('.jpg', '')):05d}.png")
                with open(dst, "wb") as f:
                    f.write(png)
                written.append(dst)
                if remove:
                    os.remove(src)
    return {"written": written, "refused": refused}


def _jpeg_to_png_on_device(ctx, files, W: int, H: int):
    """JPEG files -> PNG files (None for one the decoder refused): mav_jpeg_decode_dev's output is mav_png_encode_dev's input"""
    n = len(files)
    d_bgr, _, status = ctx.jpeg_decode_to_device(files, "bgr", return_status=True)
    bound = ctx.lib.mav_png_bound(W, H, 3)
    bufs = [d_bgr]
    try:
        bufs += [ctx.alloc(n * bound), ctx.alloc(16 * n)]
        _lib.check(ctx.lib.mav_png_encode_dev(ctx.h, d_bgr.ptr, n, 3, bufs[1].ptr, n * bound, bufs[2].ptr))
        index = bufs[2].download(np.uint64, (n, 2))
        streams = bufs[1].download(np.uint8, (int((index[:, 0] + index[:, 1]).max()),))
    finally:
        ctx.sync()
        for b in bufs:
            b.free()
    return [png_wrap(W, H, 3, streams[int(o):int(o) + int(z)].tobytes()) if status["code"][j] == 0 else None for j, (o, z) in enumerate(index)]


def _chunk(kind: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def encode_png(img: np.ndarray, level: int = 1) -> bytes:
    """PNG bytes of an 8-bit image as cv2.imencode('.png', img) lays it out: (H, W) or (H, W, 1) gray, (H, W, 3) BGR -> RGB file,
    (H, W, 4) BGRA -> RGBA file.  Filter type 0 on every row, zlib level `level` (OpenCV's default PNG compression is 1)."""
    a = np.asarray(img)
    if a.dtype != np.uint8:
        raise ValueError(f"imwrite: only 8-bit images are written here, got {a.dtype}")
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if a.ndim == 2:
        ctype, rows = 0, a
    elif a.ndim == 3 and a.shape[2] in (3, 4):
        ctype = 2 if a.shape[2] == 3 else 6
        rows = a[:, :, [2, 1, 0] if ctype == 2 else [2, 1, 0, 3]]
    else:
        raise ValueError(f"imwrite: expected (H, W), (H, W, 1), (H, W, 3) or (H, W, 4), got {a.shape}")
    H, W = rows.shape[:2]
    if H < 1 or W < 1:
        raise ValueError(f"imwrite: empty image {a.shape}")
    raw = np.empty((H, 1 + rows[0].size), np.uint8)
    raw[:, 0] = 0
    raw[:, 1:] = rows.reshape(H, -1)
    return (PNG_MAGIC + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, ctype, 0, 0, 0))
            + _chunk(b"IDAT", zlib.compress(raw.tobytes(), level)) + _chunk(b"IEND", b""))


def png_wrap(W: int, H: int, channels: int, zstream: bytes) -> bytes:
    """The PNG file around a finished zlib stream of the scanline data (Context.png_encode builds such streams on the device): signature,
    IHDR (8-bit; colour type 0 gray / 2 RGB / 6 RGBA, as encode_png writes them), one IDAT, IEND."""
    ctype = {1: 0, 3: 2, 4: 6}.get(channels)
    if ctype is None:
        raise ValueError(f"png_wrap: channels must be 1, 3 or 4, got {channels}")
    if W < 1 or H < 1:
        raise ValueError(f"png_wrap: empty image {W} x {H}")
    crc = zlib.crc32(zstream, zlib.crc32(b"IDAT")) & 0xFFFFFFFF          # the stream is read in place: a memoryview is as good as bytes
    return b"".join((PNG_MAGIC, _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, ctype, 0, 0, 0)), struct.pack(">I", len(zstream)), b"IDAT",
                     zstream, struct.pack(">I", crc), _chunk(b"IEND", b"")))


def imwrite(path: str, img: np.ndarray) -> bool:
    """cv2.imwrite(path, img) for PNG files of 8-bit gray or BGR(A) images (the reference writes its result images with it,
    processor.py:364-374).  Returns True; ValueError for another extension or image type, OSError when the file cannot be written."""
    if not path.lower().endswith(".png"):
        raise ValueError(f"imwrite: only .png files are written here, got {path!r}")
    data = encode_png(img)
    with open(path, "wb") as f:
        f.write(data)
    return True


class PngSequenceCapture:
    """cv2.VideoCapture('.../image_%05d.png') for a PNG sequence: frames are the files pattern % k for k = start, start + 1, ... until
    one is missing (OpenCV's image-sequence capture starts at the first existing index among 0 and 1; here: `start`, default the same
    probe).  read() -> (ok, BGR frame) like cv2; get(3) / get(4) / get(7) = width / height / frame count; set(1, k) seeks."""

    def __init__(self, pattern: str, start: Optional[int] = None, decoder: str = "host", ahead: int = 64, ctx=None) -> None:
        """decoder="host": every read() decodes one file on the host (imread).  decoder="device": a read() whose frame is not in hand
        decodes the next `ahead` files in one device call (imread_many: compressed bytes up, BGR frames back); the frames are the
        same.  ctx: the context whose stream the device route runs on (its size does not matter); None: one of the capture's own,
        created at the first device decode and closed by release()."""
        if decoder not in ("host", "device"):
            raise ValueError(f"decoder must be 'host' or 'device', got {decoder!r}")
        if ahead < 1:
            raise ValueError(f"ahead must be at least 1, got {ahead}")
        self.pattern = pattern
        self.decoder, self.ahead = decoder, int(ahead)
        self._ctx, self._own_ctx, self._ahead = ctx, False, {}
        if start is None:
            start = 0 if os.path.exists(pattern % 0) else 1
        self.start = self.pos = start
        first = self._frame(start)
        self._opened = first is not None
        self._size = (first.shape[1], first.shape[0]) if self._opened else (0, 0)
        self._count = None

    def _frame(self, k: int):
        """frame k as imread returns it, or None"""
        if self.decoder == "host":
            return imread(self.pattern % k)
        if k not in self._ahead:
            paths = [self.pattern % j for j in range(k, k + self.ahead)]
            while len(paths) > 1 and not os.path.exists(paths[-1]):
                paths.pop()
            if self._ctx is None:
                try:
                    with open(paths[0], "rb") as fh:
                        W, H = png_chunks(fh.read(), "small")[0][:2]
                except (OSError, ValueError, struct.error):
                    return None
                self._ctx, self._own_ctx = _lib.Context(W, H, 1), True
            got = imread_many(paths, self._ctx, "bgr")
            self._ahead = {k + j: f for j, f in enumerate(got.frames)}
        return self._ahead.get(k)

    def isOpened(self) -> bool:
        return self._opened

    def read(self):
        if not self._opened:
            return False, None
        frame = self._frame(self.pos)
        if frame is None:
            return False, None
        self.pos += 1
        return True, frame

    def get(self, prop: int) -> float:
        if prop == 3:
            return float(self._size[0])
        if prop == 4:
            return float(self._size[1])
        if prop == 7:                                # CAP_PROP_FRAME_COUNT
            if self._count is None:
                k = self.start
                while os.path.exists(self.pattern % k):
                    k += 1
                self._count = k - self.start
            return float(self._count)
        if prop == 1:                                # CAP_PROP_POS_FRAMES
            return float(self.pos - self.start)
        return 0.0

    def set(self, prop: int, value: float) -> bool:
        if prop == 1:
            self.pos = self.start + int(value)
            return True
        return False

    def release(self) -> None:
        self._opened = False
        self._ahead = {}
        if self._own_ctx and self._ctx is not None:
            self._ctx.close()
            self._ctx, self._own_ctx = None, False
