"""Host reference for the device PNG encoder (vf_png.hip).  NumPy and the standard library only.

* `read_png`: a strict reader of the subset the encoder writes — signature, IHDR first, IDAT chunks in one run, IEND
  last, every chunk CRC (zlib.crc32), the zlib stream of the concatenated IDAT data (zlib.decompress, which checks the
  Adler-32), filter types 0-4 undone.  Raises PngError for anything else.
* `float_to_bytes`: image.savePNG's rule for float tensors, b = (uint8) trunc(255f * min(max(x, 0), 1)) in float32,
  NaN -> 0.  Restated from memory of the 2016-era `image` package (it is not part of the reference): saturate, `mul(255)`
  in the tensor's type, then libpng_wrapper's C cast to png_byte, which truncates.
* `choose_filters` / `filter_stream`: libpng's default heuristic for 8-bit non-palette images, restated: every row tries
  None, Sub, Up, Average, Paeth (the row before the first is zeros) and keeps the one with the smallest sum of the
  filtered bytes' absolute values read as signed; the first in that order wins a tie.
* `huffman_only_size`: the size yardstick S_H of the tests — the same filtered rows, cut into the encoder's chunks, each
  raw-deflated by zlib with Z_HUFFMAN_ONLY and a sync flush, plus the encoder's framing bytes.
"""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHUNK = 8192                                  # video_filler_amd.backend.PNG_CHUNK


class PngError(ValueError):
    pass


def float_to_bytes(x):
    """float array -> uint8, image.savePNG's rule (see the module text)."""
    x = np.asarray(x, np.float32)
    v = np.minimum(np.maximum(np.where(np.isnan(x), np.float32(0), x), np.float32(0)), np.float32(1))
    return np.trunc(np.float32(255) * v.astype(np.float32)).astype(np.uint8)


def chw_to_hwc_bytes(x):
    """float N x C x H x W -> the uint8 N x H x W x C a decoded file must hold."""
    return np.ascontiguousarray(float_to_bytes(x).transpose(0, 2, 3, 1))


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def _filtered_rows(img):
    """img uint8 H x W x C -> int array [5][H][W*C] of the five filters' output bytes."""
    H, W, C = img.shape
    x = img.reshape(H, W * C).astype(np.int32)
    a = np.zeros_like(x)
    a[:, C:] = x[:, :-C]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, C:] = x[:-1, :-C]
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - _paeth(a, b, c)]) & 255


def choose_filters(img):
    """uint8 H x W x C -> (filter type per row, the five candidates)."""
    f = _filtered_rows(img)
    cost = np.where(f < 128, f, 256 - f).sum(axis=2)          # [5][H]
    return np.argmin(cost, axis=0).astype(np.uint8), f        # argmin: the first minimum


def filter_stream(img):
    """uint8 H x W x C -> the bytes a zlib stream of this image holds under the heuristic: filter byte + row, per row."""
    img = np.asarray(img)
    types, f = choose_filters(img)
    H = img.shape[0]
    rows = f[types, np.arange(H)].astype(np.uint8)
    return np.concatenate([types[:, None], rows], axis=1).tobytes()


def framing_bytes(stream_len, chunk=CHUNK):
    nch = -(-stream_len // chunk)
    return 8 + 25 + 12 * nch + 2 + 4 + 12


def huffman_only_size(img, chunk=CHUNK, level=6):
    """S_H: file size of an encoder with zlib's dynamic Huffman codes, the encoder's chunks and no matcher."""
    s = filter_stream(img)
    total = framing_bytes(len(s), chunk)
    for o in range(0, len(s), chunk):
        z = zlib.compressobj(level, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
        part = s[o:o + chunk]
        total += len(z.compress(part) + (z.flush(zlib.Z_FINISH) if o + chunk >= len(s) else z.flush(zlib.Z_SYNC_FLUSH)))
    return total


def read_png(data, want_filters=False):
    """bytes of one PNG file -> uint8 H x W x C (and the filter byte of every row, and the IDAT data lengths)."""
    data = bytes(data)
    if data[:8] != SIGNATURE:
        raise PngError("bad signature")
    pos, chunks = 8, []
    while pos < len(data):
        if pos + 12 > len(data):
            raise PngError("truncated chunk header at %d" % pos)
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        typ = data[pos + 4:pos + 8]
        if pos + 12 + n > len(data):
            raise PngError("chunk %r runs past the end" % typ)
        body = data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        if zlib.crc32(typ + body) != crc:
            raise PngError("CRC of chunk %r at %d" % (typ, pos))
        chunks.append((typ, body))
        pos += 12 + n
        if typ == b"IEND":
            break
    if pos != len(data):
        raise PngError("bytes after IEND")
    names = [t for t, _ in chunks]
    if len(names) < 3 or names[0] != b"IHDR" or names[-1] != b"IEND" or set(names[1:-1]) != {b"IDAT"}:
        raise PngError("chunk order %r" % names[:4])
    if len(chunks[0][1]) != 13 or len(chunks[-1][1]) != 0:
        raise PngError("IHDR / IEND length")
    W, H, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    if depth != 8 or ctype not in (0, 2) or comp != 0 or filt != 0 or lace != 0 or W == 0 or H == 0:
        raise PngError("IHDR fields %r" % ((W, H, depth, ctype, comp, filt, lace),))
    C = 3 if ctype == 2 else 1
    try:
        raw = zlib.decompress(b"".join(b for _, b in chunks[1:-1]))
    except zlib.error as e:
        raise PngError("zlib stream: %s" % e) from None
    rb = W * C
    if len(raw) != H * (rb + 1):
        raise PngError("%d bytes inflated, %d expected" % (len(raw), H * (rb + 1)))
    rows = np.frombuffer(raw, np.uint8).reshape(H, rb + 1)
    types = rows[:, 0].copy()
    if types.max() > 4:
        raise PngError("filter type %d" % types.max())
    out = np.zeros((H, rb), np.uint8)
    prev = np.zeros(rb, np.int32)
    for y in range(H):
        t, line = int(types[y]), rows[y, 1:].astype(np.int32)
        if t == 0:
            cur = line
        elif t == 2:
            cur = (line + prev) & 255
        elif t == 1:
            cur = line.reshape(W, C).cumsum(axis=0).reshape(rb) & 255
        else:
            ln, pv, cur = line.tolist(), [0] * C + prev.tolist(), [0] * (rb + C)       # plain ints: this loop is serial
            for i in range(rb):
                a, b = cur[i], pv[i + C]
                if t == 3:
                    p = (a + b) >> 1
                else:
                    c = pv[i]
                    pp = a + b - c
                    pa, pb, pc = abs(pp - a), abs(pp - b), abs(pp - c)
                    p = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[i + C] = (ln[i] + p) & 255
            cur = np.array(cur[C:], np.int32)
        out[y] = cur
        prev = cur
    img = out.reshape(H, W, C)
    if want_filters:
        return img, types, [len(b) for _, b in chunks[1:-1]]
    return img
