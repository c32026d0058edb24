"""Host restatement of the full PNG rule: Adam7-interlaced and 16-bit files on top of png_load_ref (which stays the
reference of the default route and keeps calling these files unsupported).  The reference of vf_png_inspect_full and
vf_png_decode_full (vf_png_decode.hip); tests/test_png_full_ref.py pins it against Pillow.

Adam7: the inflated stream holds up to seven sub-images, pass p taking the pixels (x0 + i dx, y0 + j dy) of ADAM7[p];
w_p = ceil((W - x0) / dx), h_p = ceil((H - y0) / dy); a pass with w_p = 0 or h_p = 0 is absent (no filter bytes, no rows);
each present pass has its own row length, its own filter byte per row and zeros above its first row; sub-byte samples are
packed per pass row, most significant bits first.  The pixels are those of the same image stored without interlace.

16-bit samples are big-endian; the filter unit is samples * 2 bytes.  Decided: the uint8 result is each sample's HIGH
byte (libpng's png_set_strip_16; what Pillow returns for colour types 2, 4, 6, and its I;16 array >> 8 for colour type
0).  Recalled from `image`'s init.lua and not checked against Torch: 'float' of a 16-bit file is sample / 65535 on the
whole sample, an IEEE float32 division; it is not highbyte / 255.

Still unsupported: what png_load_ref.load refuses by channels, a side above 16384, and an expected inflated size of 2^31
bytes or more (the decoder's sizes are int32)."""
import zlib

import numpy as np

import png_load_ref
from png_load_ref import SAMPLES, PngError, PngUnsupported, unfilter

ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))   # x0, y0, dx, dy


def passes(W, H, samples, depth, interlace):
    """the seven passes' (w_p, h_p, rb_p), zeros for an absent pass; a plain file is one pass, the first"""
    if not interlace:
        return [(W, H, (W * samples * depth + 7) // 8)] + [(0, 0, 0)] * 6
    out = []
    for x0, y0, dx, dy in ADAM7:
        w, h = max(0, (W - x0 + dx - 1) // dx), max(0, (H - y0 + dy - 1) // dy)
        out.append((w, h, (w * samples * depth + 7) // 8) if w and h else (0, 0, 0))
    return out


def parse(data):
    """png_load_ref.parse with the full rule's supported / reason / inflated_bytes, and passes: seven (w, h, rowbytes)"""
    d = png_load_ref.parse(data)
    d["passes"] = passes(d["width"], d["height"], SAMPLES[d["color_type"]], d["bit_depth"], d["interlace"])
    d["inflated_bytes"] = sum(h * (1 + rb) for w, h, rb in d["passes"])
    why = ""
    if max(d["width"], d["height"]) > 16384:
        why = "larger than 16384 per side"
    elif sum(len(c) for c in d["idat"]) > 1 << 28:
        why = "IDAT data above 256 MiB"
    elif d["inflated_bytes"] >= 1 << 31:
        why = "inflated size of 2^31 bytes or more (the decoder's sizes are int32)"
    d["supported"], d["reason"] = not why, why
    return d


def samples(data, channels=None):
    """-> (H x W x C array, the sample maximum): uint16 samples and 65535 for a 16-bit file, else what png_load_ref.load
    gives (uint8 after expansion) and 255.  Errors as png_load_ref.load."""
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
    rc, bpp = SAMPLES[ct], max(1, SAMPLES[ct] * depth // 8)
    s = np.zeros((H, W, rc), np.uint16 if depth == 16 else np.uint8)
    at = 0
    for (w, h, rb), (x0, y0, dx, dy) in zip(d["passes"], ADAM7 if d["interlace"] else ((0, 0, 1, 1),) * 7):
        if not h:
            continue
        try:
            rows = unfilter(raw[at:at + h * (1 + rb)], h, rb, bpp)
        except PngError as e:
            raise PngError("%s (of the pass whose rows are %d bytes)" % (e, rb)) from None
        at += h * (1 + rb)
        if depth < 8:
            bits = np.unpackbits(rows, axis=1)[:, :w * depth].reshape(h, w, depth)
            sub = bits.dot(1 << np.arange(depth - 1, -1, -1)).astype(np.uint8)[..., None]
        elif depth == 8:
            sub = rows.reshape(h, w, rc)
        else:
            sub = rows.reshape(h, w, rc, 2).astype(np.uint16)
            sub = sub[..., 0] << 8 | sub[..., 1]
        s[y0::dy, x0::dx] = sub
    if depth < 8 and ct == 0:
        s = s * np.uint8(255 // ((1 << depth) - 1))                   # bit replication
    if ct == 3:
        ix = s[..., 0]
        if int(ix.max()) >= len(d["plte"]):
            raise PngError("bad palette index: %d with %d entries" % (int(ix.max()), len(d["plte"])))
        img = d["plte"][ix]
        if d["trns"] is not None and channels is None:
            al = np.full(256, 255, np.uint8)
            al[:len(d["trns"])] = np.frombuffer(d["trns"], np.uint8)
            img = np.concatenate([img, al[ix][..., None]], axis=2)
    elif channels is None or channels == rc:
        img = s
    elif channels == 1:
        img = s[..., :1]
    elif ct in (0, 4):
        img = np.repeat(s[..., :1], 3, axis=2)
    else:
        img = s[..., :3]
    return np.ascontiguousarray(img), (65535 if depth == 16 else 255)


def load(data, channels=None):
    """uint8 H x W x C: a 16-bit file's high bytes, every other file's bytes"""
    s, top = samples(data, channels)
    return (s >> 8).astype(np.uint8) if top == 65535 else s


def load_float(data, channels=None):
    """float32 H x W x C: sample / 65535 of a 16-bit file, byte / 255 of every other"""
    s, top = samples(data, channels)
    return s.astype(np.float32) / np.float32(top)
