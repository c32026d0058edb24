"""Regenerate tests/golden/png_decode_cases.npz: the PNG files the device decoder's tests (tests/test_gpu_png_decode.py,
tests/test_png_load_ref.py) read, so the tests need neither Pillow nor the reference tree.

Keys: `good/<name>` (the bytes of one file the decoder must take; expected pixels come from tests/png_load_ref.py at test
time), `bad/<name>` with `status/<name>` (a file whose headers are fine and whose data is corrupt, and the VF_PNG_* status
the decoder must report).  Good files: the reference's seven masks byte for byte (`mask/...`), a Pillow-written matrix
(`pil/...`) and hand-assembled files (`hand/...`: zlib.compressobj streams or deflate blocks written bit by bit here, inside
this file's own chunk writer).  For every bad file the generator asserts that zlib.decompress rejects the stream, or
Pillow the file; where neither looks (inflated size against IHDR, palette index against PLTE: Pillow pads or truncates
silently) it asserts that the size or the index is indeed off, which libpng reports.
Usage: python tests/golden/make_png_decode_golden.py [reference-dir]"""
import io
import os
import struct
import sys
import zlib

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import png_load_ref  # noqa: E402
import png_ref  # noqa: E402

MASKS = ("mask", "maskplus", "mask5p", "maskpp", "maskppp", "mask6p", "maskpppp")
OK, BAD_CODE, SHORT_DATA, BAD_DISTANCE, BAD_LENGTH, BAD_FILTER, BAD_ADLER, BAD_INDEX = range(8)
ZHDR = b"\x78\x01"


# ------------------------------------------------------------------------------------------------ chunk writer
def chunk(typ, body=b""):
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body))


def mk_png(W, H, depth, ct, zstream, plte=None, trns=None, before_plte=(), after_plte=(), idat_cuts=None):
    out = [png_ref.SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, ct, 0, 0, 0))]
    out += list(before_plte)
    if plte is not None:
        out.append(chunk(b"PLTE", bytes(plte)))
    out += list(after_plte)
    if trns is not None:
        out.append(chunk(b"tRNS", bytes(trns)))
    pos = 0
    for n in (idat_cuts or [len(zstream)]):
        out.append(chunk(b"IDAT", zstream[pos:pos + n]))
        pos += n
    assert pos == len(zstream)
    out.append(chunk(b"IEND"))
    return b"".join(out)


def zwrap(raw_deflate, data):
    return ZHDR + raw_deflate + struct.pack(">I", zlib.adler32(data))


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flushes=()):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    out, pos = b"", 0
    for p, mode in flushes:
        out += c.compress(data[pos:p]) + c.flush(mode)
        pos = p
    return out + c.compress(data[pos:]) + c.flush()


def filtered(img, types):
    """uint8 H x W x C and a filter type per row -> the stream's bytes"""
    f = png_ref._filtered_rows(img)
    H = img.shape[0]
    types = np.asarray(types, np.uint8)
    rows = f[types, np.arange(H)].astype(np.uint8)
    return np.concatenate([types[:, None], rows], axis=1).tobytes()


# ------------------------------------------------------------------------------------------------ deflate by hand
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, nbits):                       # least significant bit first (extra bits, header fields)
        self.acc |= v << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, nbits):                      # a Huffman code: most significant bit first
        self.put(int(format(c, "0%db" % nbits)[::-1], 2), nbits)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def done(self):
        self.align()
        return bytes(self.out)


def canon(lens):
    """code lengths -> {symbol: (code, length)}"""
    code, out = 0, {}
    for ln in range(1, 16):
        for s, v in enumerate(lens):
            if v == ln:
                out[s] = (code, ln)
                code += 1
        code <<= 1
    return out


LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
         12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
FLAT_LIT = [9] * 256 + [5, 5] + [6] * 28          # a complete code over the 286 symbols
FLAT_DIST = [4, 4] + [5] * 28
CL_LENS = [4] * 13 + [5] * 6                       # a complete code-length code over all 19 symbols
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def put_tokens(b, tokens, lit, dist):
    """tokens: int (a literal), (length, distance), ("lit", symbol) a raw literal/length symbol, ("dist", length symbol,
    distance code) a raw pair without extra bits; then the end-of-block code"""
    L, D = canon(lit), canon(dist)
    for t in tokens:
        if isinstance(t, int):
            b.code(*L[t])
        elif t[0] == "lit":
            b.code(*L[t[1]])
        elif t[0] == "dist":
            b.code(*L[t[1]])
            b.code(*D[t[2]])
        else:
            ln, ds = t
            i = max(k for k in range(29) if LBASE[k] <= ln and (k == 28) == (ln == 258))
            b.code(*L[257 + i])
            b.put(ln - LBASE[i], LEXT[i])
            j = max(k for k in range(30) if DBASE[k] <= ds)
            b.code(*D[j])
            b.put(ds - DBASE[j], DEXT[j])
    b.code(*L[256])


def fixed_block(b, tokens, final):
    b.put(final, 1)
    b.put(1, 2)
    put_tokens(b, tokens, FIXED_LIT, FIXED_DIST)


def dyn_block(b, tokens, final, lit, dist, ops=None, cl_lens=None):
    """ops: the code-length symbols of the header as (symbol, extra value) pairs; default: every length spelled out"""
    cl_lens = cl_lens or CL_LENS
    b.put(final, 1)
    b.put(2, 2)
    b.put(len(lit) - 257, 5)
    b.put(len(dist) - 1, 5)
    b.put(19 - 4, 4)
    for s in CL_ORDER:
        b.put(cl_lens[s], 3)
    cl = canon(cl_lens)
    for sym, extra in (ops if ops is not None else [(v, 0) for v in list(lit) + list(dist)]):
        b.code(*cl[sym])
        if sym >= 16:
            b.put(extra, {16: 2, 17: 3, 18: 7}[sym])
    if tokens is not None:
        put_tokens(b, tokens, lit, dist)


def stored_block(b, data, final, nlen=None):
    b.put(final, 1)
    b.put(0, 2)
    b.align()
    b.put(len(data), 16)
    b.put((~len(data) & 0xffff) if nlen is None else nlen, 16)
    b.out += data


# ------------------------------------------------------------------------------------------------ images
def smooth(H, W, C, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([(xx * (3 + c) + yy * (5 - c) + (xx * yy) // 7) & 255 for c in range(C)], -1)
    return ((img + rng.integers(0, 3, img.shape)) & 255).astype(np.uint8)


def pil_bytes(im, **kw):
    bio = io.BytesIO()
    im.save(bio, "PNG", **kw)
    return bio.getvalue()


def pillow_matrix():
    out = {}
    rng = np.random.default_rng(7)
    pal = rng.integers(0, 256, 768, dtype=np.uint8).tolist()
    H, W = 17, 23
    for lvl in (0, 1, 6, 9):
        g = smooth(H, W, 1, lvl)[..., 0]
        out["L8_l%d" % lvl] = pil_bytes(Image.fromarray(g), compress_level=lvl)
        out["1bit_l%d" % lvl] = pil_bytes(Image.fromarray(g > 100), compress_level=lvl)
        out["RGB_l%d" % lvl] = pil_bytes(Image.fromarray(smooth(H, W, 3, lvl)), compress_level=lvl)
        out["RGBA_l%d" % lvl] = pil_bytes(Image.fromarray(smooth(H, W, 4, lvl), "RGBA"), compress_level=lvl)
        out["LA_l%d" % lvl] = pil_bytes(Image.fromarray(smooth(H, W, 2, lvl), "LA"), compress_level=lvl)
        for bits in (1, 2, 4, 8):
            p = Image.fromarray((smooth(H, W, 1, 9 + bits)[..., 0].astype(np.int32) % (1 << bits)).astype(np.uint8), "P")
            p.putpalette(pal[:3 << bits])
            out["P%d_l%d" % (bits, lvl)] = pil_bytes(p, compress_level=lvl, bits=bits)
            out["P%d_trns_l%d" % (bits, lvl)] = pil_bytes(p, compress_level=lvl, bits=bits,
                                                           transparency=bytes(rng.integers(0, 256, max(1, (1 << bits) - 1), dtype=np.uint8)))
    for name, (h, w) in dict(s1x1=(1, 1), s1xH=(31, 1), sWx1=(1, 29)).items():
        out["RGB_" + name] = pil_bytes(Image.fromarray(smooth(h, w, 3, 3)))
        out["L8_" + name] = pil_bytes(Image.fromarray(smooth(h, w, 1, 4)[..., 0]))
    for w in (1, 7, 8, 9):
        out["1bit_w%d" % w] = pil_bytes(Image.fromarray(smooth(11, w, 1, w)[..., 0] > 90))
    for h in (63, 64, 65, 255, 256, 257):                              # the band seams of the unfilter wavefront
        out["RGB_h%d" % h] = pil_bytes(Image.fromarray(smooth(h, 5, 3, h)))
        out["L8_h%d" % h] = pil_bytes(Image.fromarray(smooth(h, 6, 1, h + 1)[..., 0]))
    return out


def grey_png(img, raw_deflate=None, data=None, **kw):
    """8-bit grey H x W (x 1) -> file; the stream is zlib level 6 of filter-0 rows unless given"""
    img = img.reshape(img.shape[0], img.shape[1], 1)
    data = filtered(img, [0] * img.shape[0]) if data is None else data
    z = zlib.compress(data, 6) if raw_deflate is None else zwrap(raw_deflate, data)
    assert zlib.decompress(z) == data
    return mk_png(img.shape[1], img.shape[0], 8, 0, z, **kw)


def hand_files():
    out = {}
    rgb = smooth(37, 40, 3, 11)
    for t in range(5):
        out["filter%d" % t] = mk_png(40, 37, 8, 2, zlib.compress(filtered(rgb, [t] * 37), 6))
    mixed = filtered(rgb, [(3 * y + y // 5) % 5 for y in range(37)])
    out["filter_mixed"] = mk_png(40, 37, 8, 2, zlib.compress(mixed, 6))
    ga = smooth(9, 13, 2, 12)
    out["filter_mixed_ga"] = mk_png(13, 9, 8, 4, zlib.compress(filtered(ga, [4, 3, 1, 2, 0, 4, 4, 3, 1]), 9))
    rgba = smooth(70, 11, 4, 13)
    out["filter_mixed_rgba"] = mk_png(11, 70, 8, 6, zlib.compress(filtered(rgba, [(y * 7 + 4) % 5 for y in range(70)]), 9))
    for depth in (2, 4):                                                # grey below 8 bits, which Pillow does not write
        W, H = 13, 9
        rb = (W * depth + 7) // 8
        packed = smooth(H, rb, 1, depth)
        out["grey%d" % depth] = mk_png(W, H, depth, 0, zlib.compress(filtered(packed, [y % 5 for y in range(H)]), 6))
    for name, st in (("fixed", zlib.Z_FIXED), ("huffman_only", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE)):
        out["strategy_" + name] = mk_png(40, 37, 8, 2, ZHDR + deflate(mixed, 6, st, -15) + struct.pack(">I", zlib.adler32(mixed)))
    for wb in (9, 15):
        out["wbits%d" % wb] = mk_png(40, 37, 8, 2, deflate(mixed, 9, wbits=wb))
    # a stored block of 65535 bytes, an empty one, and the last byte
    big = np.tile(np.arange(255, dtype=np.uint8), (256, 1))
    data = filtered(big[..., None], [0] * 256)
    b = Bits()
    stored_block(b, data[:65535], 0)
    stored_block(b, b"", 0)
    stored_block(b, data[65535:], 1)
    out["stored_65535"] = grey_png(big, b.done(), data)
    # Z_FULL_FLUSH in mid-row
    out["full_flush"] = mk_png(40, 37, 8, 2, deflate(mixed, 6, flushes=[(len(mixed) // 2 + 17, zlib.Z_FULL_FLUSH)]))
    # dist 1, len 258 chains far longer than one token batch
    flat = np.full((300, 300), 0, np.uint8)
    out["run_dist1"] = grey_png(flat)
    # a match at distance exactly 32768 (rows of 128 bytes; row 256 repeats row 0), written with fixed codes
    row0 = [0] + [(i * 37 + 5) & 255 for i in range(127)]
    toks = list(row0)
    left = 32768 - 128
    while left:
        n = min(258, left) if left - min(258, left) not in (1, 2) else 255
        toks.append((n, 128))
        left -= n
    toks.append((128, 32768))
    img = np.tile(np.array(row0[1:], np.uint8), (257, 1))
    b = Bits()
    fixed_block(b, toks, 1)
    out["dist_32768"] = grey_png(img, b.done())
    # sources in the deflate block before, and in the token batch before (the repeat lies 9088 bytes back)
    rng = np.random.default_rng(5)
    half = rng.integers(0, 256, (71, 127), dtype=np.uint8)
    img = np.concatenate([half, half])
    data = filtered(img[..., None], [0] * 142)
    raw = deflate(data, 9, wbits=-15, flushes=[(71 * 128, zlib.Z_SYNC_FLUSH)])
    out["prev_block_and_batch"] = grey_png(img, raw, data)
    # a dynamic block with 15-bit codes, and no distance code at all
    lit = list(range(1, 15)) + [15] + [0] * 241 + [15]
    img = np.array([[(x * y + x) % 15 for x in range(20)] for y in range(12)], np.uint8)
    data = filtered(img[..., None], [0] * 12)
    b = Bits()
    dyn_block(b, list(data), 1, lit, [0])
    out["dyn_15bit_no_dist"] = grey_png(img, b.done(), data)
    # a dynamic block with a single distance code (one bit, the other one-bit code unused)
    img = np.tile(np.array([0, 9, 200, 31], np.uint8), (10, 5))[:, :19]
    data = filtered(img[..., None], [0] * 10)
    toks = list(data[:20]) + [(len(data) - 20, 20)] if len(data) - 20 <= 258 else None
    b = Bits()
    dyn_block(b, toks, 1, FLAT_LIT, [0] * 8 + [1])                       # distance code 8: 17-24
    out["dyn_single_dist"] = grey_png(img, b.done(), data)
    # a hand-written header whose zero repeat (17, four times) runs from literal/length 258-259 into distance 0-1
    lit = [8] * 254 + [9, 9, 9, 9, 0, 0]
    dist = [0, 0, 1]
    cl = [0] * 19
    cl[16], cl[8], cl[9], cl[17], cl[1] = 1, 2, 3, 4, 4
    ops = [(8, 0)] + [(16, 3)] * 42 + [(8, 0)] + [(9, 0)] * 4 + [(17, 1), (1, 0)]
    img = np.array([[(7 * x + y) % 250 for x in range(15)] for y in range(6)], np.uint8)
    img[:, 3:6] = img[:, 0:3]
    data = filtered(img[..., None], [0] * 6)
    toks = []
    for y in range(6):
        r = data[16 * y:16 * y + 16]
        toks += list(r[:4]) + [(3, 3)] + list(r[7:])
    b = Bits()
    dyn_block(b, toks, 1, lit, dist, ops, cl)
    out["dyn_repeat_crosses"] = grey_png(img, b.done(), data)
    # IDAT cut into 1-byte chunks with zero-length ones among them
    img = smooth(8, 8, 1, 3)
    z = zlib.compress(filtered(img, [1] * 8), 6)
    cuts = []
    for i in range(len(z)):
        cuts += [1] + ([0] if i % 5 == 0 else [])
    out["idat_1byte"] = mk_png(8, 8, 8, 0, z, idat_cuts=[0] + cuts)
    # ancillary chunks before and after PLTE (and a tIME behind the data is the reference's own mask.png)
    pidx = (smooth(9, 14, 1, 8) % 6).astype(np.uint8)
    plte = bytes(range(10, 28))
    z = zlib.compress(filtered(pidx, [0, 1, 2, 3, 4, 0, 1, 2, 3]), 6)
    out["ancillary_around_plte"] = mk_png(14, 9, 8, 3, z, plte=plte, trns=b"\x00\x80",
                                          before_plte=[chunk(b"gAMA", struct.pack(">I", 45455)), chunk(b"tEXt", b"Title\x00x")],
                                          after_plte=[chunk(b"bKGD", b"\x01"), chunk(b"pHYs", struct.pack(">IIB", 2835, 2835, 1))])
    # tRNS on grey and on RGB (a colour key): ignored for channels 1 and 3, no byte rule for the file's own channels
    g = smooth(9, 13, 1, 31)
    out["grey_trns"] = mk_png(13, 9, 8, 0, zlib.compress(filtered(g, [y % 5 for y in range(9)]), 6),
                              trns=struct.pack(">H", int(g[2, 3, 0])))
    c = smooth(9, 13, 3, 32)
    out["rgb_trns"] = mk_png(13, 9, 8, 2, zlib.compress(filtered(c, [(y + 2) % 5 for y in range(9)]), 6),
                             trns=struct.pack(">HHH", *[int(v) for v in c[4, 5]]))
    return out


def bad_files():
    """name -> (file, status)"""
    out = {}
    img = smooth(24, 31, 1, 21)
    data = filtered(img, [y % 5 for y in range(24)])
    H, W = 24, 31

    def g(z, h=H, w=W):
        return mk_png(w, h, 8, 0, z)
    z = zlib.compress(data, 6)
    out["truncated"] = (g(z[:len(z) // 2]), SHORT_DATA)
    out["wrong_adler"] = (g(z[:-1] + bytes([z[-1] ^ 1])), BAD_ADLER)
    out["one_byte_too_many"] = (g(zlib.compress(data + b"\x00", 6)), BAD_LENGTH)
    out["one_row_too_few"] = (g(zlib.compress(data[:-(W + 1)], 6)), BAD_LENGTH)
    d5 = bytearray(data)
    d5[3 * (W + 1)] = 5
    out["filter_byte_5"] = (g(zlib.compress(bytes(d5), 6)), BAD_FILTER)

    def hand(build):
        b = Bits()
        build(b)
        return g(ZHDR + b.done() + struct.pack(">I", zlib.adler32(data)))
    out["distance_before_start"] = (hand(lambda b: fixed_block(b, [0, 7, (3, 5)] + list(data[5:]), 1)), BAD_DISTANCE)
    out["symbol_286"] = (hand(lambda b: fixed_block(b, list(data[:40]) + [("lit", 286)] + list(data[40:]), 1)), BAD_CODE)
    out["distance_code_30"] = (hand(lambda b: fixed_block(b, list(data[:40]) + [("dist", 257, 30)] + list(data[40:]), 1)), BAD_CODE)

    def type3(b):
        fixed_block(b, list(data[:100]), 0)
        b.put(1, 1)
        b.put(3, 2)
        b.put(0, 13)
    out["block_type_3"] = (hand(type3), BAD_CODE)
    out["len_nlen_mismatch"] = (hand(lambda b: stored_block(b, data, 1, nlen=0x1234)), BAD_CODE)
    out["oversubscribed"] = (hand(lambda b: dyn_block(b, list(data), 1, [8] * 257 + [3], FLAT_DIST)), BAD_CODE)
    out["no_end_of_block_code"] = (hand(lambda b: dyn_block(b, None, 1, [8] * 256 + [0], FLAT_DIST)), BAD_CODE)
    pidx = (smooth(9, 14, 1, 8) % 6).astype(np.uint8)
    zp = zlib.compress(filtered(pidx, [0] * 9), 6)
    out["palette_index_past_plte"] = (mk_png(14, 9, 8, 3, zp, plte=bytes(range(15))), BAD_INDEX)
    return out


def rejected_elsewhere(name, f):
    """who else refuses the file: "zlib", "pillow", or the restated check that libpng makes"""
    d = png_load_ref.parse(f)
    try:
        raw = zlib.decompress(b"".join(d["idat"]))
    except zlib.error:
        return "zlib"
    try:
        Image.open(io.BytesIO(f)).load()
    except Exception:
        return "pillow"
    if len(raw) != d["inflated_bytes"]:
        return "size %d against %d" % (len(raw), d["inflated_bytes"])
    if d["color_type"] == 3 and max(raw[i] for i in range(len(raw)) if i % (d["rowbytes"] + 1)) >= len(d["plte"]):
        return "palette index against %d entries" % len(d["plte"])
    raise AssertionError("%s: nothing rejects it" % name)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else None
    path = os.path.join(HERE, "png_decode_cases.npz")
    arrays = {}
    if ref is None:                                    # keep the masks of the file that is there
        old = np.load(path)
        for k in old.files:
            if k.startswith("good/mask/"):
                arrays[k] = old[k]
    else:
        for m in MASKS:
            with open(os.path.join(ref, m + ".png"), "rb") as fh:
                arrays["good/mask/" + m] = np.frombuffer(fh.read(), np.uint8)
    assert len([k for k in arrays if k.startswith("good/mask/")]) == 7
    for group, files in (("pil", pillow_matrix()), ("hand", hand_files())):
        for name, f in files.items():
            arrays["good/%s/%s" % (group, name)] = np.frombuffer(f, np.uint8)
    for k in [k for k in arrays if k.startswith("good/")]:
        f = arrays[k].tobytes()
        d = png_load_ref.parse(f)
        mine = png_load_ref.load(f, None if (d["trns"] is None or d["color_type"] == 3) else 3)
        assert mine.shape[:2] == (d["height"], d["width"]), k
    for name, (f, st) in bad_files().items():
        png_load_ref.parse(f)                          # the headers are fine
        try:
            png_load_ref.load(f)
            raise AssertionError("%s: the restatement takes it" % name)
        except png_load_ref.PngError as e:
            print("%-26s status %d  %-8s %s" % (name, st, rejected_elsewhere(name, f), e))
        arrays["bad/" + name] = np.frombuffer(f, np.uint8)
        arrays["status/" + name] = np.int32(st)
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes;", len(arrays), "entries")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "jpeg_cases.npz")) // 2


if __name__ == "__main__":
    main()
