"""A small PNG writer (NumPy and zlib) and the fixtures of the full PNG rule (tests/png_full_ref.py):
every legal (colour type, bit depth) pair, Adam7-interlaced or plain, a filter type drawn per row from a fixed seed, the
IDAT split wherever asked.  Pillow cannot write Adam7, so every fixture is made here at import; none is a golden file.

GOOD: name -> dict(file, pixels (the samples written, H x W x samples), color_type, bit_depth, interlace, H, W).
BAD: name -> (file, status word).  The benchmark script uses write_png too."""
import struct
import zlib

import numpy as np

ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))   # x0, y0, dx, dy
SAMPLES = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
PAIRS = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]
SIZES = [(1, 1), (1, 2), (2, 1), (3, 3), (4, 5), (5, 4), (7, 9), (8, 8), (9, 17), (17, 23)]            # H, W
STATUS = {"bad code": 1, "short data": 2, "bad distance": 3, "bad length": 4, "bad filter": 5, "bad Adler-32": 6,
          "bad palette index": 7}


def chunk(typ, body=b""):
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body))


def _filtered(rows, bpp, types):
    """rows (h x rb uint8) -> the filtered stream of one pass: a filter byte (types[r]; above 4 stores the row as it is) and
    the row's bytes per row"""
    h, rb = rows.shape
    cur = rows.astype(np.int16)
    a = np.zeros_like(cur)
    a[:, bpp:] = cur[:, :rb - bpp] if rb > bpp else 0
    b = np.zeros_like(cur)
    b[1:] = cur[:-1]
    c = np.zeros_like(cur)
    c[:, bpp:] = b[:, :rb - bpp] if rb > bpp else 0
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    pred = np.stack([np.zeros_like(cur), a, b, (a + b) >> 1, paeth])
    t = np.asarray(types, np.int64)
    out = np.empty((h, rb + 1), np.uint8)
    out[:, 0] = t
    out[:, 1:] = (cur - pred[np.where(t > 4, 0, t), np.arange(h)]) & 255
    return out.tobytes()


def pass_rows(pix, depth, interlace):
    """the samples (H x W x samples) -> per pass (7 entries, None for an absent one) its packed rows, h x rb uint8"""
    H, W, rc = pix.shape
    out = []
    for x0, y0, dx, dy in (ADAM7 if interlace else ((0, 0, 1, 1),)):
        sub = pix[y0::dy, x0::dx]
        h, w = sub.shape[:2]
        if not h or not w:
            out.append(None)
        elif depth == 16:
            v = sub.astype(np.uint16)
            out.append(np.stack([v >> 8, v & 255], -1).astype(np.uint8).reshape(h, w * rc * 2))
        elif depth == 8:
            out.append(sub.astype(np.uint8).reshape(h, w * rc))
        else:
            bits = (sub.reshape(h, w, 1).astype(np.uint8) >> np.arange(depth - 1, -1, -1)) & 1
            out.append(np.packbits(bits.reshape(h, w * depth), axis=1))
    return out + [None] * (7 - len(out))


def write_png(pix, color_type, depth, interlace=False, seed=0, plte=None, trns=None, level=6, split=(), force_filter=None,
              ihdr_interlace=None, filters=None, used=None):
    """One PNG file.  pix: the samples, H x W x samples, each below 2^depth.  A filter type 0 - 4 per row from `seed` (or
    `filters`, one type for all rows); force_filter {(pass, row): type} overrides single rows; split: stream positions at
    which a new IDAT chunk begins; ihdr_interlace: the flag written, if not the layout's; used: a set that receives every
    (pass, filter type) written."""
    pix = np.asarray(pix)
    H, W, rc = pix.shape
    assert rc == SAMPLES[color_type] and int(pix.max()) < 1 << depth
    rng = np.random.default_rng(seed)
    bpp = max(1, rc * depth // 8)
    raw = []
    for p, rows in enumerate(pass_rows(pix, depth, interlace)):
        if rows is None:
            continue
        types = rng.integers(0, 5, len(rows)) if filters is None else np.full(len(rows), filters)
        for (fp, fr), ft in (force_filter or {}).items():
            if fp == p:
                types[fr] = ft
        if used is not None:
            used.update((p, int(t)) for t in types)
        raw.append(_filtered(rows, bpp, types))
    z = zlib.compress(b"".join(raw), level)
    cuts = [0] + sorted(split) + [len(z)]
    lace = int(interlace) if ihdr_interlace is None else ihdr_interlace
    out = [b"\x89PNG\r\n\x1a\n", chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, color_type, 0, 0, lace))]
    if plte is not None:
        out.append(chunk(b"PLTE", np.asarray(plte, np.uint8).tobytes()))
    if trns is not None:
        out.append(chunk(b"tRNS", bytes(trns)))
    out += [chunk(b"IDAT", z[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    return b"".join(out + [chunk(b"IEND")])


def palette(depth, seed=5):
    """a palette for indices of `depth` bits: fewer entries than the depth allows at depths 4 and 8"""
    n = {1: 2, 2: 4, 4: 13, 8: 200}[depth]
    return np.random.default_rng(seed).integers(0, 256, (n, 3), dtype=np.uint8)


def random_pixels(H, W, color_type, depth, seed):
    rng = np.random.default_rng(seed)
    top = len(palette(depth)) if color_type == 3 else 1 << depth
    pix = rng.integers(0, top, (H, W, SAMPLES[color_type]))
    if H * W > 16:                                        # a smooth part too, so that the filters see more than noise
        yy, xx = np.mgrid[0:H, 0:W]
        pix[:, :W // 2] = ((yy * 3 + xx * 5)[:, :W // 2, None] * (top // 16 + 1) + np.arange(pix.shape[2])) % top
    return pix


USED = set()          # every (pass, filter type) the good cases hold
GOOD, BAD = {}, {}


def _add(H, W, ct, depth, lace, **kw):
    name = "c%dd%d_%s_%dx%d%s" % (ct, depth, "lace" if lace else "plain", H, W, kw.pop("tag", ""))
    seed = zlib.crc32(name.encode())
    pix = random_pixels(H, W, ct, depth, seed)
    if ct == 3:
        kw.setdefault("plte", palette(depth))
    GOOD[name] = dict(file=write_png(pix, ct, depth, lace, seed=seed, used=USED if lace else None, **kw), pixels=pix,
                      color_type=ct, bit_depth=depth, interlace=int(lace), H=H, W=W)
    return name


for _ct, _d in PAIRS:
    for _H, _W in SIZES:
        _add(_H, _W, _ct, _d, True)
        if _d == 16:
            _add(_H, _W, _ct, _d, False)
# pass 7 of 131 rows has 65 of them: it crosses a 64-row band of the unfilter kernel
BAND = [_add(131, 19, ct, d, True) for ct, d in ((3, 1), (0, 2), (3, 4), (2, 8), (4, 8), (0, 16), (6, 16))]
TRNS = _add(9, 17, 3, 4, True, trns=bytes([0, 128, 255, 7, 9]), tag="_trns")
# stored blocks (level 0): stream byte 2 + 5 + k is inflated byte k.  17 x 23 x 3: pass 1 is 3 rows of 1 + 9 bytes, pass 2
# follows at 30; the cuts fall inside a row of pass 1, inside a row of pass 2 and inside the last pass
SPLIT = _add(17, 23, 2, 8, True, level=0, split=(1, 7 + 14, 7 + 35, 7 + 36, 7 + 1000), tag="_split")
assert {t for p, t in USED} == {0, 1, 2, 3, 4} and all({t for q, t in USED if q == p} == {0, 1, 2, 3, 4} for p in range(7)), \
    "every filter type occurs in every pass across the set"


def _bad():
    rgb = random_pixels(17, 23, 2, 8, 11)
    BAD["filter5_pass5"] = (write_png(rgb, 2, 8, True, seed=1, force_filter={(4, 2): 5}), STATUS["bad filter"])
    laced, plain = write_png(rgb, 2, 8, True, seed=2, ihdr_interlace=0), write_png(rgb, 2, 8, False, seed=2, ihdr_interlace=1)
    BAD["lace_flag_cleared"] = (laced, STATUS["bad length"])
    BAD["lace_flag_set"] = (plain, STATUS["bad length"])
    ix = random_pixels(9, 17, 3, 4, 12)
    ix[3, 6] = 14                                          # an odd row: pass 7; the palette has 13 entries
    BAD["index_pass7"] = (write_png(ix % 16, 3, 4, True, seed=3, plte=palette(4)), STATUS["bad palette index"])
    deep = write_png(random_pixels(17, 23, 6, 16, 13), 6, 16, True, seed=4)
    at = deep.index(b"IDAT")
    (n,) = struct.unpack(">I", deep[at - 4:at])
    body = deep[at + 4:at + 4 + n // 2]
    BAD["deep_cut_short"] = (deep[:at - 4] + chunk(b"IDAT", body) + chunk(b"IEND"), STATUS["short data"])


_bad()
