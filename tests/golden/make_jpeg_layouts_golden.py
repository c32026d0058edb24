"""Regenerate tests/golden/jpeg_layouts_cases.npz: JPEG files in the layouts decode_jpeg(layouts=True) adds (DESIGN.md
5.2: other sampling factors, RGB, sequential files of several scans) with Pillow's decode of each, so the tests
(tests/test_jpeg_layouts_ref.py, tests/test_jpeg_layouts_cabi.py, tests/test_gpu_jpeg_layouts.py) need no Pillow.

Keys: `jpg/<name>` (uint8 file bytes), `ref/<name>` (Pillow's decode, convert("RGB") or "L"; uint8 H x W x C, C = 1 for
grey) and `bad/<name>` (file bytes only) for files the decoder must refuse.

Pillow cannot write most of these layouts, so `write` below is a small sequential writer of its own: any sampling
factors per component, any split of the components over scans, a restart interval per scan, SOF0 or SOF1, any table
slots, JFIF / Adobe / no marker, any component ids.  It takes the tables, the forward DCT and the block coding from
tests/jpeg_enc_ref.py.  It is a test tool and no encoder to match: it decimates by plain block means, and only Pillow's
decode of the bytes it writes counts.  Usage: python tests/golden/make_jpeg_layouts_golden.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_enc_ref as E  # noqa: E402
from make_jpeg_golden import content, encode, pillow_decode  # noqa: E402
from make_jpeg_progressive_golden import photo  # noqa: E402

LAYOUTS = {            # (h, v) of Y, Cb, Cr
    "440": ((1, 2), (1, 1), (1, 1)),
    "411": ((4, 1), (1, 1), (1, 1)),
    "410": ((4, 2), (1, 1), (1, 1)),                  # 10 blocks in the MCU
    "1x4": ((1, 4), (1, 1), (1, 1)),
    "3x1": ((3, 1), (1, 1), (1, 1)),                  # an MCU 24 wide
    "22_21_11": ((2, 2), (2, 1), (1, 1)),             # Cb h1v2, Cr h2v2
    "22_12_21": ((2, 2), (1, 2), (2, 1)),             # Cb h2v1, Cr h1v2
    "11_22_22": ((1, 1), (2, 2), (2, 2)),             # luma is the upsampled one
    "420": ((2, 2), (1, 1), (1, 1)),
    "444": ((1, 1), (1, 1), (1, 1)),
}
SIZES = [(1, 1), (7, 5), (16, 16), (17, 33), (37, 53)]
KINDS = ["noise", "smooth", "flat", "checker"]
QUALS = [50, 90, 100, 20]


def cdiv(a, b):
    return -(-a // b)


def _seg(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def write(frame, factors=((1, 1),), scans=None, dri=0, quality=75, sof=0xC0, slots=(0, 1), marker="jfif", ids=(1, 2, 3),
          rgb=False):
    """One frame (uint8 H x W x 3, or H x W x 1 for a grey file) as a sequential file.  factors: (h, v) per component;
    scans: lists of component numbers, one list per scan (default: one scan of them all); dri: the restart interval, one
    number or one per scan; slots: the Huffman slot (DC and AC alike) of component 0 and of the others; marker: "jfif",
    "adobe0", "adobe1" or None; rgb: the components are the frame's R, G, B, not Y, Cb, Cr."""
    f = np.asarray(frame)
    H, W, C = f.shape
    assert C == len(factors) and C in (1, 3)
    scans = scans or [list(range(C))]
    dris = [dri] * len(scans) if isinstance(dri, int) else list(dri)
    hmax, vmax = max(h for h, _ in factors), max(v for _, v in factors)
    one = C == 1                                                        # its factors are ignored: the MCU is one block
    mcux, mcuy = (cdiv(W, 8), cdiv(H, 8)) if one else (cdiv(W, 8 * hmax), cdiv(H, 8 * vmax))
    qt = E.quant_tables(quality)
    src = [f[..., 0].astype(np.int64)] if one else [f[..., i].astype(np.int64) for i in range(3)] if rgb else E._ycc(f)
    coef, real = [], []
    for c, (h, v) in enumerate(factors):
        rh, rv = (1, 1) if one else (hmax // h, vmax // v)
        ch, cw = cdiv(H, rv), cdiv(W, rh)
        p = E._pad_edge(src[c], ch * rv, cw * rh).reshape(ch, rv, cw, rh).mean((1, 3)).round().astype(np.int64)
        hh, vv = (1, 1) if one else (h, v)
        coef.append(E.coefficients(E._pad_edge(p, mcuy * 8 * vv, mcux * 8 * hh), qt[0 if c == 0 or rgb else 1]))
        real.append((cdiv(ch, 8), cdiv(cw, 8)))
    out = b"\xff\xd8"
    if marker == "jfif":
        out += _seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    elif marker in ("adobe0", "adobe1"):
        out += _seg(0xEE, b"Adobe" + bytes([0, 100, 0, 0, 0, 0, int(marker[-1])]))
    for t in range(1 if one or rgb else 2):
        out += _seg(0xDB, bytes([t]) + bytes(qt[t].astype(np.uint8).tolist()))
    out += _seg(sof, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([C]) +
                b"".join(bytes([ids[c], factors[c][0] << 4 | factors[c][1], 0 if c == 0 or rgb else 1]) for c in range(C)))
    for k, (tc_th, bits, vals) in enumerate(E.HUFF[:2 if one else 4]):    # DC0, AC0, DC1, AC1 of the rule, in the slots asked for
        out += _seg(0xC4, bytes([(tc_th & 0x10) | slots[k // 2]]) + bytes(bits) + bytes(vals))
    last_dri = 0
    for comps, ri in zip(scans, dris):
        if ri != last_dri:
            out += _seg(0xDD, ri.to_bytes(2, "big"))
            last_dri = ri
        out += _seg(0xDA, bytes([len(comps)]) + b"".join(bytes([ids[c], 0x11 * slots[0 if c == 0 else 1]]) for c in comps) +
                    bytes([0, 63, 0]))
        if len(comps) > 1:
            units = [[(c, my * factors[c][1] + y, mx * factors[c][0] + x) for c in comps for y in range(factors[c][1])
                      for x in range(factors[c][0])] for my in range(mcuy) for mx in range(mcux)]
        else:
            c = comps[0]
            units = [[(c, y, x)] for y in range(real[c][0]) for x in range(real[c][1])]
        bw, pred = E._Bits(), [0] * C
        for n, unit in enumerate(units):
            if ri and n and n % ri == 0:
                if bw.n:
                    bw.put((1 << (8 - bw.n)) - 1, 8 - bw.n)
                bw.out += bytes([0xFF, 0xD0 + (n // ri - 1) % 8])
                pred = [0] * C
            for c, y, x in unit:
                t = 0 if c == 0 else 1
                zz = coef[c][y, x]
                E._put_block(bw, zz, pred[c], E.CODES[t], E.CODES[0x10 | t])
                pred[c] = int(zz[0])
        if bw.n:
            bw.put((1 << (8 - bw.n)) - 1, 8 - bw.n)
        out += bytes(bw.out)
    return out + b"\xff\xd9"


def patched_sof(data, old, new, sof=0xC2):
    """The file with the luma sampling byte of its SOF replaced: the same entropy-coded data read under another layout."""
    b = bytearray(data)
    at = b.index(bytes([0xFF, sof])) + 11
    assert b[at] == old, hex(b[at])
    b[at] = new
    return bytes(b)


def keep_rgb(a, subsampling, **kw):
    bio = io.BytesIO()
    Image.fromarray(a).save(bio, "JPEG", quality=90, keep_rgb=True, subsampling=subsampling, **kw)
    return bio.getvalue()


def without_adobe_as_rgb_ids(data):
    """The keep_rgb file with its Adobe segment removed and its component ids patched to 'R', 'G', 'B'."""
    b = bytearray(data)
    at = b.index(b"\xff\xeeAdobe"[:2] + b"\x00\x0eAdobe")
    del b[at:at + 16]
    for marker, first, step in ((0xC0, 10, 3), (0xDA, 5, 2)):
        m = b.index(bytes([0xFF, marker]))
        for c in range(3):
            assert b[m + first + step * c] in (c + 1, b"RGB"[c])         # libjpeg gives an RGB file these ids itself
            b[m + first + step * c] = b"RGB"[c]
    return bytes(b)


def cases():
    rng = np.random.default_rng(20261020)
    out = []
    n = 0
    for name, fac in LAYOUTS.items():
        if name in ("420", "444"):
            continue
        for h, w in SIZES + ([(3, 3), (2, 6)] if name.startswith("22_") else []):   # cw <= 2 for the (2, 1) and (2, 2) components
            kind, q = KINDS[n % 4], QUALS[(n // 2) % 4]
            n += 1
            out.append(("%s_%dx%d_%s_q%d" % (name, h, w, kind, q), write(content(kind, h, w, rng), fac, quality=q, dri=(0, 1, 3)[n % 3])))
    for h, w in SIZES:                                                              # grey, 2x2 in its SOF: the factors are ignored
        out.append(("L22_%dx%d" % (h, w), write(content("noise", h, w, rng)[..., :1], ((2, 2),), quality=80, dri=(0, 2)[h % 2])))
    # colour
    a = content("smooth", 24, 40, rng) // 2 + content("noise", 24, 40, rng) // 2
    f = keep_rgb(a, 0)                                                              # Pillow writes keep_rgb at 4:4:4 only
    out.append(("rgb_adobe0_sub0_24x40", f))
    out.append(("rgb_ids_sub0_24x40", without_adobe_as_rgb_ids(f)))
    out.append(("rgb_adobe0_sub2_24x40", write(a, LAYOUTS["420"], marker="adobe0", rgb=True)))   # R at 2x2, G and B at 1x1
    out.append(("rgb_ids_sub2_24x40", write(a, LAYOUTS["420"], marker=None, ids=(82, 71, 66), rgb=True)))
    out.append(("ycc_nomarker_24x40", write(a, LAYOUTS["420"], marker=None)))
    out.append(("ycc_adobe1_24x40", write(a, LAYOUTS["420"], marker="adobe1")))
    out.append(("rgb_adobe0_writer_411_24x40", write(a, LAYOUTS["411"], marker="adobe0", rgb=True)))
    # scans
    b = content("noise", 37, 53, rng) // 2 + content("smooth", 37, 53, rng) // 2
    for sname, split, lay in (("y_cb_cr", [[0], [1], [2]], "444"), ("y_cbcr", [[0], [1, 2]], "444"), ("ycb_cr", [[0, 1], [2]], "420"),
                              ("y_cb_cr", [[0], [1], [2]], "420")):
        for ri in (0, 3):
            out.append(("scans_%s_%s_37x53_dri%d" % (sname, lay, ri), write(b, LAYOUTS[lay], split, dri=ri, quality=85)))
    out.append(("scans_y_cb_cr_420_37x53_drichange", write(b, LAYOUTS["420"], [[0], [1], [2]], dri=[5, 0, 2], quality=85)))
    out.append(("scans_cr_y_cb_444_17x33", write(b[:17, :33], LAYOUTS["444"], [[2], [0], [1]], dri=[0, 4, 0])))
    out.append(("sof1_slots23_420_37x53", write(b, LAYOUTS["420"], sof=0xC1, slots=(2, 3), quality=85)))
    out.append(("sof1_slots23_y_cbcr_17x33", write(b[:17, :33], LAYOUTS["444"], [[0], [1, 2]], sof=0xC1, slots=(3, 2))))
    out.append(("scans_y_cb_cr_440_37x53", write(b, LAYOUTS["440"], [[0], [1], [2]], dri=[0, 2, 0])))
    out.append(("scans_y_cb_cr_410_37x53", write(b, LAYOUTS["410"], [[0], [1], [2]])))
    # progressive: Pillow's files read under another header
    for h, w in ((16, 16), (32, 32), (16, 32)):
        c = content("noise", h, w, rng) // 2 + content("smooth", h, w, rng) // 2
        out.append(("prog_440_%dx%d" % (h, w), patched_sof(encode(c, "422", 90, progressive=True), 0x21, 0x12)))
        if (h, w) != (16, 16):                                                      # 4:1:1 needs a whole number of 32-wide MCUs
            out.append(("prog_411_%dx%d" % (h, w), patched_sof(encode(c, "420", 90, progressive=True), 0x22, 0x41)))
    out.append(("prog_rgb_adobe0_24x40", keep_rgb(a, 0, progressive=True)))
    # two larger files
    p = photo(360, 480, rng)
    out.append(("440_360x480_photo_q75", write(p, LAYOUTS["440"], quality=75)))
    out.append(("scans_y_cb_cr_420_360x480_smooth_q75_dri60",
                write(content("smooth", 360, 480, rng), LAYOUTS["420"], [[0], [1], [2]], dri=[60, 30, 30], quality=75)))
    return out


def refused():
    """fractional: 3x1 with 2x1; blocks18: 4x4 luma; twice: Cb in two scans; missing: no scan has Cr; cmyk."""
    a = content("smooth", 24, 40, np.random.default_rng(1))
    f = write(a, LAYOUTS["444"], [[0], [1], [2]])
    sos = [i for i in range(len(f) - 1) if f[i] == 0xFF and f[i + 1] == 0xDA]
    assert len(sos) == 3
    twice = bytearray(f)
    assert twice[sos[2] + 5] == 3
    twice[sos[2] + 5] = 2
    bio = io.BytesIO()
    Image.new("CMYK", (40, 24), (10, 20, 30, 40)).save(bio, "JPEG")
    frac = bytearray(write(a, LAYOUTS["3x1"]))          # Cb's factors patched to 2x1: 3 / 2 is no whole number
    at = frac.index(b"\xff\xc0") + 14
    assert frac[at] == 0x11
    frac[at] = 0x21
    return [("fractional", bytes(frac)), ("blocks18", write(a, ((4, 4), (1, 1), (1, 1)))),
            ("twice", bytes(twice)), ("missing", f[:sos[2]] + b"\xff\xd9"), ("cmyk", bio.getvalue())]


LIBJPEG_REFUSES = ("fractional", "blocks18")      # the others it decodes, with a warning or as another colour space


def main():
    arrays = {}
    for name, data in cases():
        assert "jpg/" + name not in arrays, name
        im = Image.open(io.BytesIO(data))
        ref = np.asarray(im.convert("L" if im.mode == "L" else "RGB"))
        arrays["jpg/" + name] = np.frombuffer(data, np.uint8)
        arrays["ref/" + name] = ref[..., None] if ref.ndim == 2 else ref
    for name, data in refused():
        arrays["bad/" + name] = np.frombuffer(data, np.uint8)
        if name in LIBJPEG_REFUSES:
            try:
                pillow_decode(data)
            except Exception:
                continue
            raise AssertionError("Pillow decodes bad/%s" % name)
    path = os.path.join(HERE, "jpeg_layouts_cases.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", sum(k.startswith("jpg/") for k in arrays), "supported cases")


if __name__ == "__main__":
    main()
