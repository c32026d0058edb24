"""Host restatement of `image.load` for PNG files: the reference of the device decoder (vf_png_decode.hip).
NumPy, zlib and the standard library only; tests/test_png_load_ref.py pins it against Pillow.

Recalled from the 2016-era `image` package (png.c, init.lua; the package is not part of the reference):
* libpng runs with png_set_expand_gray_1_2_4_to_8 for grey below 8 bits, which is bit replication: 1-bit gives 0 or 255,
  2-bit multiplies by 85, 4-bit by 17; and with png_set_expand for palettes: RGB from PLTE.
* The tensor has 1, 2, 3 or 4 channels; 'float' divides by 255.
* image.load(path, 3) replicates grey, takes the grey of grey+alpha and drops the alpha of RGBA.  image.load(path, 1) on
  a colour file goes through rgb2y in float: not a byte rule, so `load` refuses it.
Decided here (Torch's loader writes 4-channel rows into a 3-channel tensor for it): a palette with tRNS gives RGBA for
channels=None, alpha 255 past the end of tRNS, and RGB for channels=3.  A palette index at or past the PLTE length is an
error (libpng's too).  tRNS on grey and RGB files would become alpha in the file's own channels: refused.

`parse` walks the chunks under the rules of vf_png_inspect; `load` returns uint8 H x W x C; `load_float` divides by 255."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHECKED = (b"IHDR", b"PLTE", b"tRNS", b"IDAT", b"IEND")
SAMPLES = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


class PngError(ValueError):
    pass


class PngUnsupported(PngError):
    pass


def parse(data):
    """bytes of one file -> dict(width, height, bit_depth, color_type, interlace, channels, idat (list of payloads),
    plte (n x 3 or None), trns (bytes or None), supported, reason, inflated_bytes).  PngError for a malformed file."""
    data = bytes(data)
    if data[:8] != SIGNATURE:
        raise PngError("bad signature")
    pos, first, seen_idat, idat_done, iend = 8, True, False, False, False
    d = dict(idat=[], plte=None, trns=None)
    while pos < len(data):
        if pos + 12 > len(data):
            raise PngError("truncated chunk header at byte %d" % pos)
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        typ = data[pos + 4:pos + 8]
        if pos + 12 + n > len(data):
            raise PngError("chunk %r runs past the end of the file" % typ)
        body = data[pos + 8:pos + 8 + n]
        if first != (typ == b"IHDR"):
            raise PngError("IHDR is not the first chunk" if first else "more than one IHDR")
        if typ in CHECKED and zlib.crc32(typ + body) != struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]:
            raise PngError("wrong CRC on chunk %r" % typ)
        if seen_idat and typ != b"IDAT":
            idat_done = True
        if typ == b"IHDR":
            if n != 13:
                raise PngError("IHDR length")
            W, H, depth, ct, comp, filt, lace = struct.unpack(">IIBBBBB", body)
            ok = depth in (1, 2, 4, 8, 16) and (ct == 0 or (ct == 3 and depth <= 8) or (ct in (2, 4, 6) and depth >= 8))
            if not ok or not 1 <= W < 2 ** 31 or not 1 <= H < 2 ** 31 or comp or filt or lace > 1:
                raise PngError("illegal IHDR %r" % ((W, H, depth, ct, comp, filt, lace),))
            d.update(width=W, height=H, bit_depth=depth, color_type=ct, interlace=lace)
            first = False
        elif typ == b"PLTE":
            ct = d["color_type"]
            if seen_idat:
                raise PngError("PLTE after IDAT")
            if d["plte"] is not None or n == 0 or n % 3 or n > 768 or ct in (0, 4) or (ct == 3 and n // 3 > 1 << d["bit_depth"]):
                raise PngError("illegal PLTE")
            d["plte"] = np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif typ == b"tRNS":
            ct = d["color_type"]
            ok = not seen_idat and d["trns"] is None and (
                (ct == 3 and d["plte"] is not None and 1 <= n <= len(d["plte"])) or (ct == 0 and n == 2) or (ct == 2 and n == 6))
            if not ok:
                raise PngError("illegal tRNS")
            d["trns"] = body
        elif typ == b"IDAT":
            if idat_done:
                raise PngError("IDAT chunks are not consecutive")
            if d["color_type"] == 3 and d["plte"] is None:
                raise PngError("no PLTE before IDAT for colour type 3")
            seen_idat = True
            d["idat"].append(body)
        elif typ == b"IEND":
            if n:
                raise PngError("IEND length")
            iend = True
            break
        elif not typ[0] & 0x20:
            raise PngError("unknown critical chunk %r" % typ)
        pos += 12 + n
    if first:
        raise PngError("no IHDR")
    if not iend:
        raise PngError("no IEND chunk")
    if not seen_idat:
        raise PngError("no IDAT chunk")
    z = b"".join(d["idat"])
    if len(z) < 2:
        raise PngError("zlib header: too short")
    if z[0] & 15 != 8 or z[0] >> 4 > 7 or z[1] & 0x20 or (z[0] * 256 + z[1]) % 31:
        raise PngError("bad zlib header")
    ct, depth = d["color_type"], d["bit_depth"]
    key = d["trns"] is not None
    d["channels"] = (4 if key else 3) if ct == 3 else SAMPLES[ct] + (1 if key and ct in (0, 2) else 0)
    d["rowbytes"] = (d["width"] * SAMPLES[ct] * depth + 7) // 8
    d["inflated_bytes"] = d["height"] * (1 + d["rowbytes"])
    why = ""
    if depth == 16:
        why = "16-bit samples"
    elif d["interlace"]:
        why = "Adam7 interlace"
    elif max(d["width"], d["height"]) > 16384:
        why = "larger than 16384 per side"
    d["supported"], d["reason"] = not why, why
    return d


def unfilter(raw, H, rb, bpp):
    """the inflated stream (filter byte + rb bytes per row) -> uint8 H x rb.  PngError for a filter byte above 4."""
    rows = np.frombuffer(raw, np.uint8).reshape(H, rb + 1)
    out = np.zeros((H, rb), np.uint8)
    prev = [0] * rb
    for y in range(H):
        t, ln = int(rows[y, 0]), rows[y, 1:].tolist()
        if t > 4:
            raise PngError("bad filter: type %d on row %d" % (t, y))
        cur = [0] * rb
        for i in range(rb):
            a = cur[i - bpp] if i >= bpp else 0
            b = prev[i]
            if t == 0:
                p = 0
            elif t == 1:
                p = a
            elif t == 2:
                p = b
            elif t == 3:
                p = (a + b) >> 1
            else:
                c = prev[i - bpp] if i >= bpp else 0
                pp = a + b - c
                pa, pb, pc = abs(pp - a), abs(pp - b), abs(pp - c)
                p = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            cur[i] = (ln[i] + p) & 255
        out[y] = cur
        prev = cur
    return out


def load(data, channels=None):
    """image.load(path[, channels]) as bytes: uint8 H x W x C.  PngError for malformed or corrupt files (the message
    names what vf_png_decode's status word names), PngUnsupported for what the byte rule does not cover."""
    d = parse(data)
    if not d["supported"]:
        raise PngUnsupported(d["reason"])
    ct, depth, W, H = d["color_type"], d["bit_depth"], d["width"], d["height"]
    if channels is None and d["trns"] is not None and ct != 3:
        raise PngUnsupported("tRNS on colour type %d with the file's channels" % ct)
    if channels == 1 and ct in (2, 3, 6):
        raise PngUnsupported("colour file with channels=1")
    z = zlib.decompressobj()
    try:
        raw = z.decompress(b"".join(d["idat"]))
    except zlib.error as e:
        raise PngError("zlib stream: %s" % e) from None
    if not z.eof:
        raise PngError("short data: the zlib stream does not end")
    if len(raw) != d["inflated_bytes"]:
        raise PngError("bad length: %d bytes inflated, %d expected" % (len(raw), d["inflated_bytes"]))
    rb = d["rowbytes"]
    rows = unfilter(raw, H, rb, max(1, SAMPLES[ct] * depth // 8))
    if depth < 8:                                                 # one sample per pixel, most significant bits first
        bits = np.unpackbits(rows, axis=1)[:, :W * depth].reshape(H, W, depth)
        s = bits.dot(1 << np.arange(depth - 1, -1, -1)).astype(np.uint8)[..., None]
        if ct == 0:
            s = s * np.uint8(255 // ((1 << depth) - 1))          # bit replication
    else:
        s = rows.reshape(H, W, SAMPLES[ct])
    if ct == 3:
        ix = s[..., 0]
        if int(ix.max()) >= len(d["plte"]):
            raise PngError("bad palette index: %d with %d entries" % (int(ix.max()), len(d["plte"])))
        img = d["plte"][ix]
        if d["trns"] is not None and channels is None:
            al = np.full(256, 255, np.uint8)
            al[:len(d["trns"])] = np.frombuffer(d["trns"], np.uint8)
            img = np.concatenate([img, al[ix][..., None]], axis=2)
    elif channels is None or channels == s.shape[2]:
        img = s
    elif channels == 1:
        img = s[..., :1]                                          # grey, or the grey of grey+alpha
    elif ct in (0, 4):
        img = np.repeat(s[..., :1], 3, axis=2)
    else:
        img = s[..., :3]                                          # RGB, or RGBA without its alpha
    return np.ascontiguousarray(img)


def load_float(data, channels=None):
    """image.load(path, channels, 'float') in H x W x C: an IEEE float32 division by 255."""
    return load(data, channels).astype(np.float32) / np.float32(255)
