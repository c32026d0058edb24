"""The JPEG encoding rule of DESIGN.md 5.8 in numpy: libjpeg's default compression (jpeg_set_defaults, jpeg_set_quality,
the fixed Annex K Huffman tables, no restart intervals, the islow DCT), whole files, byte for byte what Pillow's
save(format="JPEG", quality=q, subsampling=s) writes.  encode(frame, quality, subsampling) -> bytes is the definition the
kernels of csrc/vf_jpeg_enc.hip are held to; nothing here needs Pillow.

The tables below were read out of a file Pillow wrote at quality 50 (where the scaled tables are the base tables): the two
quantisation tables in the file's zig-zag order, and the four Huffman tables as their DHT segments carry them."""
import numpy as np

QUANT_ZZ = (
    (16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51,
     56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101,
     103, 99),
    (17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99),
)
# (table class << 4 | id, BITS[16], HUFFVAL) in the order of the file: DC0, AC0, DC1, AC1
HUFF = (
    (0x00, (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)),
    (0x10, (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125),
     (1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240,
      36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73,
      74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132,
      133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178,
      179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217,
      218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250)),
    (0x01, (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)),
    (0x11, (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119),
     (0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240,
      21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71,
      72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130,
      131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169,
      170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215,
      216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250)),
)
SUBSAMPLING = {"444": (1, 1), "422": (2, 1), "420": (2, 2)}      # luma sampling factors (h, v); chroma is 1 x 1


def _zigzag():
    """zz[k] = row-major position in the 8 x 8 block of the k-th coefficient of the zig-zag order."""
    order = sorted(((y, x) for y in range(8) for x in range(8)), key=lambda p: (p[0] + p[1], p[0] if (p[0] + p[1]) % 2 else p[1]))
    return np.array([8 * y + x for y, x in order])


ZZ = _zigzag()


def quant_tables(quality):
    """The two tables in zig-zag order, scaled by jpeg_set_quality's rule."""
    q = int(quality)
    assert 1 <= q <= 100
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return [np.clip((np.array(t, np.int64) * scale + 50) // 100, 1, 255) for t in QUANT_ZZ]


def _codes(bits, vals):
    """symbol -> (code, length) of the canonical code of a DHT segment."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


CODES = {tc_th: _codes(bits, vals) for tc_th, bits, vals in HUFF}


def header(H, W, C, quality, subsampling="420"):
    """Everything in front of the entropy-coded data: SOI, APP0, DQT, SOF0, DHT, SOS."""
    hs, vs = SUBSAMPLING[subsampling] if C == 3 else (1, 1)
    qt = quant_tables(quality)
    seg = lambda marker, body: bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t in range(2 if C == 3 else 1):
        out += seg(0xDB, bytes([t]) + bytes(qt[t].astype(np.uint8).tolist()))
    comps = [(1, hs << 4 | vs, 0), (2, 0x11, 1), (3, 0x11, 1)][:C]
    out += seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([C]) + b"".join(bytes(c) for c in comps))
    for tc_th, bits, vals in HUFF[:4 if C == 3 else 2]:
        out += seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    out += seg(0xDA, bytes([C]) + b"".join(bytes([i + 1, 0x00 if i == 0 else 0x11]) for i in range(C)) + bytes([0, 63, 0]))
    return out


def _ycc(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return [y, cb, cr]


def _pad_edge(a, rows, cols):
    return np.pad(a, ((0, rows - a.shape[0]), (0, cols - a.shape[1])), mode="edge")


def planes(frame, subsampling="420"):
    """The component planes padded to whole MCUs: columns of the SOURCE replicated to the MCU width, rows of the source to
    a multiple of the luma vertical factor, then the downsampling, then the component's own last row down to the MCU height."""
    f = np.asarray(frame)
    assert f.dtype == np.uint8 and f.ndim == 3 and f.shape[2] in (1, 3)
    H, W, C = f.shape
    hs, vs = SUBSAMPLING[subsampling] if C == 3 else (1, 1)
    mw, mh = 8 * hs, 8 * vs
    Wp, Hv, Hp = -(-W // mw) * mw, -(-H // vs) * vs, -(-H // mh) * mh
    comps = _ycc(f) if C == 3 else [f[..., 0].astype(np.int64)]
    out = []
    for i, c in enumerate(comps):
        c = _pad_edge(c, Hv, Wp)
        if i > 0 and (hs, vs) == (2, 1):
            bias = np.tile([0, 1], Wp // 4 + 1)[:Wp // 2]
            c = (c[:, 0::2] + c[:, 1::2] + bias) >> 1
        elif i > 0 and (hs, vs) == (2, 2):
            bias = np.tile([1, 2], Wp // 4 + 1)[:Wp // 2]
            c = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        rows = Hp if i == 0 else Hp // vs
        out.append(_pad_edge(c, rows, c.shape[1]))
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """One pass of jfdctint.c along the last axis of d (..., 8)."""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 13 - 2 if first else 13 + 2
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    o[7] = _descale(t4 + z1 + z3, n)
    o[5] = _descale(t5 + z2 + z4, n)
    o[3] = _descale(t6 + z2 + z3, n)
    o[1] = _descale(t7 + z1 + z4, n)
    return np.stack(o, -1)


def coefficients(plane, qt_zz):
    """Quantised coefficients of every 8 x 8 block of a padded plane: (block rows, block columns, 64) in zig-zag order."""
    h, w = plane.shape
    b = plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128
    b = _fdct_pass(b, True)                                             # rows
    b = _fdct_pass(b.swapaxes(-1, -2), False).swapaxes(-1, -2)          # columns
    c = b.reshape(h // 8, w // 8, 64)[..., ZZ]
    d = 8 * qt_zz
    return np.sign(c) * ((np.abs(c) + d // 2) // d)


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 255
            self.out.append(byte)
            if byte == 255:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1


def _put_block(bw, zz, pred, dc, ac):
    diff = int(zz[0]) - pred
    n = abs(diff).bit_length()
    bw.put(*dc[n])
    if n:
        bw.put((diff if diff >= 0 else diff - 1) & ((1 << n) - 1), n)
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bw.put(*ac[0xF0])
            run -= 16
        n = abs(v).bit_length()
        bw.put(*ac[run << 4 | n])
        bw.put((v if v >= 0 else v - 1) & ((1 << n) - 1), n)
        run = 0
    if run:
        bw.put(*ac[0x00])


def encode(frame, quality=75, subsampling="420", stats=None):
    """One frame, uint8 H x W x C (C = 1 or 3; H x W is taken as H x W x 1) -> the file's bytes.  stats, a dict, receives
    what the stream contained: counts of dummy blocks to the right and below, of 0xF0 symbols, the largest DC category."""
    f = np.asarray(frame)
    if f.ndim == 2:
        f = f[..., None]
    H, W, C = f.shape
    hs, vs = SUBSAMPLING[subsampling] if C == 3 else (1, 1)
    qt = quant_tables(quality)
    comp = [coefficients(p, qt[0 if i == 0 else 1]) for i, p in enumerate(planes(f, subsampling))]
    real = [(-(-H // 8), -(-W // 8))] + [(-(-(-(-H // vs)) // 8), -(-(-(-W // hs)) // 8))] * (C - 1)    # real blocks: rows, columns
    bw, pred = _Bits(), [0] * C
    st = stats if stats is not None else {}
    for key in ("dummy_right", "dummy_below", "zrl", "dc_cat_max"):
        st.setdefault(key, 0)
    for my in range(-(-H // (8 * vs))):
        for mx in range(-(-W // (8 * hs))):
            for i in range(C):
                fh, fv = (hs, vs) if i == 0 else (1, 1)
                dc, ac = CODES[0x00 if i == 0 else 0x01], CODES[0x10 if i == 0 else 0x11]
                for by in range(fv):
                    for bx in range(fh):
                        y, x = my * fv + by, mx * fh + bx
                        if y >= real[i][0] or x >= real[i][1]:          # a dummy: DC difference 0, no AC, predictor kept
                            st["dummy_below" if y >= real[i][0] else "dummy_right"] += 1
                            bw.put(*dc[0])
                            bw.put(*ac[0x00])
                            continue
                        zz = comp[i][y, x]
                        st["dc_cat_max"] = max(st["dc_cat_max"], abs(int(zz[0]) - pred[i]).bit_length())
                        nz = np.flatnonzero(zz[1:])
                        if nz.size:
                            gaps = np.diff(np.concatenate(([-1], nz))) - 1
                            st["zrl"] += int((gaps // 16).sum())
                        _put_block(bw, zz, pred[i], dc, ac)
                        pred[i] = int(zz[0])
    if bw.n:
        bw.put((1 << (8 - bw.n)) - 1, 8 - bw.n)
    return header(H, W, C, quality, subsampling) + bytes(bw.out) + b"\xff\xd9"
