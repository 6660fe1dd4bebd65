"""Minimal PNG codec for the trajectory layout (8-bit RGB, no interlace).

The reference writes ``images{c}/im_{t}.png`` with OpenCV (``visual_mpc/sim/simulator.py:82-86``,
``cv2.imwrite(..., images[t, i, :, :, ::-1])`` - the ``::-1`` undoes OpenCV's BGR convention, so the
file holds the frame in RGB).  OpenCV is not part of this stack; a PNG of this kind is a zlib
stream of filter-0 scanlines between three chunks, which the standard library covers.
"""
import struct
import zlib

import numpy as np

_SIG = b'\x89PNG\r\n\x1a\n'


def _chunk(tag, data):
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)


def write_png(path, rgb):
    """Write a uint8 ``[H, W, 3]`` RGB array."""
    rgb = np.ascontiguousarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError('write_png takes a uint8 [H, W, 3] array, got %s %s' % (rgb.dtype, rgb.shape))
    h, w = rgb.shape[:2]
    raw = np.zeros((h, 1 + 3 * w), np.uint8)        # filter byte 0 ("None") in front of every scanline
    raw[:, 1:] = rgb.reshape(h, 3 * w)
    with open(path, 'wb') as f:
        f.write(_SIG)
        f.write(_chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)))
        f.write(_chunk(b'IDAT', zlib.compress(raw.tobytes(), 6)))
        f.write(_chunk(b'IEND', b''))


def read_png(path):
    """Read back a PNG written by ``write_png`` (8-bit RGB, filter 0 only) -> uint8 ``[H, W, 3]``."""
    with open(path, 'rb') as f:
        blob = f.read()
    if blob[:8] != _SIG:
        raise ValueError('%s is not a PNG file' % path)
    pos, idat, shape = 8, b'', None
    while pos < len(blob):
        n, tag = struct.unpack('>I4s', blob[pos:pos + 8])
        data = blob[pos + 8:pos + 8 + n]
        if struct.unpack('>I', blob[pos + 8 + n:pos + 12 + n])[0] != (zlib.crc32(tag + data) & 0xffffffff):
            raise ValueError('bad CRC in chunk %r' % tag)
        if tag == b'IHDR':
            w, h, depth, ctype, _, _, interlace = struct.unpack('>IIBBBBB', data)
            if (depth, ctype, interlace) != (8, 2, 0):
                raise ValueError('only 8-bit non-interlaced RGB is supported')
            shape = (h, w)
        elif tag == b'IDAT':
            idat += data
        pos += 12 + n
    h, w = shape
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    if raw[:, 0].any():
        raise ValueError('only filter type 0 scanlines are supported')
    return raw[:, 1:].reshape(h, w, 3).copy()


# ---------------------------------------------------------------------------------------------- animated PNG
# An APNG is a PNG whose first frame is the ordinary image plus three more chunk kinds: ``acTL`` (frame and loop counts)
# before the image data, one ``fcTL`` (geometry and delay) in front of every frame, and ``fdAT`` (a sequence number +
# the zlib stream) for every frame after the first.  A viewer without APNG support shows the first frame - so does
# ``read_png`` above, which skips the chunks it does not know.  Lossless, standard library only.
def _scanlines(rgb):
    h, w = rgb.shape[:2]
    raw = np.zeros((h, 1 + 3 * w), np.uint8)
    raw[:, 1:] = rgb.reshape(h, 3 * w)
    return zlib.compress(raw.tobytes(), 6)


def write_apng(path, frames, fps=4):
    """Write a uint8 ``[T, H, W, 3]`` RGB movie as an animated PNG that loops forever at ``fps`` frames per second."""
    frames = np.ascontiguousarray(frames)
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
        raise ValueError('write_apng takes a uint8 [T >= 1, H, W, 3] array, got %s %s' % (frames.dtype, frames.shape))
    n, h, w = frames.shape[:3]
    seq = 0
    with open(path, 'wb') as f:
        f.write(_SIG)
        f.write(_chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)))
        f.write(_chunk(b'acTL', struct.pack('>II', n, 0)))
        for i in range(n):
            # sequence number, width, height, x / y offset, delay numerator / denominator, dispose 0, blend 0
            f.write(_chunk(b'fcTL', struct.pack('>IIIIIHHBB', seq, w, h, 0, 0, 1, int(fps), 0, 0)))
            seq += 1
            if i == 0:
                f.write(_chunk(b'IDAT', _scanlines(frames[i])))
            else:
                f.write(_chunk(b'fdAT', struct.pack('>I', seq) + _scanlines(frames[i])))
                seq += 1
        f.write(_chunk(b'IEND', b''))


def read_apng(path):
    """Read back an animated PNG written by ``write_apng`` -> uint8 ``[T, H, W, 3]``; the number of frames found is
    checked against the count the file announces.  A plain PNG reads as one frame."""
    with open(path, 'rb') as f:
        blob = f.read()
    if blob[:8] != _SIG:
        raise ValueError('%s is not a PNG file' % path)
    pos, shape, announced, streams = 8, None, None, []
    while pos < len(blob):
        n, tag = struct.unpack('>I4s', blob[pos:pos + 8])
        data = blob[pos + 8:pos + 8 + n]
        if struct.unpack('>I', blob[pos + 8 + n:pos + 12 + n])[0] != (zlib.crc32(tag + data) & 0xffffffff):
            raise ValueError('bad CRC in chunk %r' % tag)
        if tag == b'IHDR':
            w, h, depth, ctype, _, _, interlace = struct.unpack('>IIBBBBB', data)
            if (depth, ctype, interlace) != (8, 2, 0):
                raise ValueError('only 8-bit non-interlaced RGB is supported')
            shape = (h, w)
        elif tag == b'acTL':
            announced = struct.unpack('>II', data)[0]
        elif tag == b'fcTL':
            fw, fh, x0, y0 = struct.unpack('>IIII', data[4:20])
            if (fh, fw, x0, y0) != shape + (0, 0):
                raise ValueError('only full-size frames are supported')
            streams.append(b'')
        elif tag == b'IDAT':
            if not streams:
                streams.append(b'')     # a plain PNG has no frame control chunk
            streams[0] += data
        elif tag == b'fdAT':
            streams[-1] += data[4:]
        pos += 12 + n
    if announced is not None and announced != len(streams):
        raise ValueError('%s announces %d frames and holds %d' % (path, announced, len(streams)))
    h, w = shape
    out = np.empty((len(streams), h, w, 3), np.uint8)
    for i, s in enumerate(streams):
        raw = np.frombuffer(zlib.decompress(s), np.uint8).reshape(h, 1 + 3 * w)
        if raw[:, 0].any():
            raise ValueError('only filter type 0 scanlines are supported')
        out[i] = raw[:, 1:].reshape(h, w, 3)
    return out
