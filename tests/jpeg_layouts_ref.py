"""The decoding rule of DESIGN.md 5.2, "Other samplings, RGB and several scans", as a whole decoder in numpy: markers ->
per-scan Huffman decode -> dequantise, islow IDCT -> per-component upsampling -> colour -> crop.  `decode(file)` is the
definition vf_jpeg_decode_layouts is held to; `coefficients(file)` and `mcu_layout` give what
vf_jpeg_layouts_coefficients_host returns.  The entropy rule of progressive files is tests/jpeg_prog_ref.py's.  No
Pillow, no GPU."""
import numpy as np

import jpeg_prog_ref as PR
from jpeg_prog_ref import NATURAL, Bits, cdiv, extend, huff_codes, huff_decode, markers


def parse(f):
    """jpeg_prog_ref.parse for SOF0 / SOF1 / SOF2, with what the pixels need as well: sof, quant {component: 64 values in
    zig-zag order, latched at the component's first scan}, colour ("grey", "YCbCr" or "RGB", by jdapimin.c's
    default_decompress_parms)."""
    f = bytes(f)
    dht, dqt, dri, comps, W, H, sof, scans, pending, quant = {}, {}, 0, None, 0, 0, None, [], None, {}
    jfif, adobe = False, None
    for _, m, seg in markers(f):
        if m == 0xC4:
            j = 0
            while j < len(seg):
                cnt = list(seg[j + 1:j + 17])
                n = sum(cnt)
                dht[seg[j]] = huff_codes(cnt, list(seg[j + 17:j + 17 + n]))
                j += 17 + n
        elif m == 0xDB:
            j = 0
            while j < len(seg):
                pq, tq = seg[j] >> 4, seg[j] & 15
                if pq:
                    dqt[tq] = [(seg[j + 1 + 2 * k] << 8) | seg[j + 2 + 2 * k] for k in range(64)]
                else:
                    dqt[tq] = list(seg[j + 1:j + 65])
                j += 1 + 64 * (2 if pq else 1)
        elif m == 0xDD:
            dri = (seg[0] << 8) | seg[1]
        elif m == 0xE0 and seg[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe = seg[11]
        elif m in (0xC0, 0xC1, 0xC2):
            sof = m
            H, W = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(seg[5])]
        elif m == 0xDA:
            ns = seg[0]
            ids = [c[0] for c in comps]
            cs = [ids.index(seg[1 + 2 * c]) for c in range(ns)]
            for c in cs:
                quant.setdefault(c, list(dqt[comps[c][3]]))
            pending = dict(components=cs, Ss=seg[1 + 2 * ns], Se=seg[2 + 2 * ns], Ah=seg[3 + 2 * ns] >> 4, Al=seg[3 + 2 * ns] & 15,
                           restart_interval=dri, tables=dict(dht),
                           sel={c: (seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15) for k, c in enumerate(cs)})
        elif m == "data":
            begin, end = seg
            segs, cur, j = [], bytearray(), begin
            while j < end:
                if f[j] == 0xFF and j + 1 < end:
                    if f[j + 1] == 0:
                        cur.append(0xFF)
                    else:                       # RSTn
                        segs.append(bytes(cur))
                        cur = bytearray()
                    j += 2
                    continue
                cur.append(f[j])
                j += 1
            segs.append(bytes(cur))
            pending.update(begin=begin, end=end, segments=segs)
            scans.append(pending)
    if len(comps) == 1:
        colour = "grey"
    elif jfif:
        colour = "YCbCr"
    elif adobe is not None:
        colour = "RGB" if adobe == 0 else "YCbCr"
    else:
        colour = "RGB" if [c[0] for c in comps] == [82, 71, 66] else "YCbCr"
    return dict(width=W, height=H, comps=comps, scans=scans, sof=sof, quant=quant, colour=colour)


def coefficients(f):
    """jpeg_prog_ref.coefficients for a file of either kind: (coef, bw, bh), coef[c] int64 [block rows (MCU-padded), block
    columns, 64] in zig-zag order.  A sequential scan (jdhuff.c decode_mcu): per block the DC difference, then (run, size)
    symbols up to EOB or the 64th coefficient; the predictors start at 0 in every scan and after every RSTn; the dummy
    blocks only an interleaved scan would have coded stay zero."""
    P = parse(f)
    if P["sof"] == 0xC2:
        return PR.coefficients(f)
    hs, vs, mcux, mcuy, bw, bh = PR.geometry(P)
    coef = [np.zeros((mcuy * vs[c], mcux * hs[c], 64), np.int64) for c in range(len(P["comps"]))]
    for sc in P["scans"]:
        units = PR.scan_units(P, sc)
        tabs, sel = sc["tables"], sc["sel"]
        ri = sc["restart_interval"] or len(units)
        assert len(sc["segments"]) == cdiv(len(units), ri), (len(sc["segments"]), len(units), ri)
        for si, sg in enumerate(sc["segments"]):
            b, pred = Bits(sg), [0] * len(coef)
            for u in units[si * ri:(si + 1) * ri]:
                for c, y, x in u:
                    blk = coef[c][y, x]
                    s = huff_decode(b, tabs[sel[c][0]])
                    pred[c] += extend(b.bits(s), s)
                    blk[0] = pred[c]
                    t, k = tabs[0x10 | sel[c][1]], 1
                    while k < 64:
                        rs = huff_decode(b, t)
                        r, s = rs >> 4, rs & 15
                        if s:
                            k += r
                            blk[min(k, 63)] = extend(b.bits(s), s)
                            k += 1
                        elif r == 15:
                            k += 16
                        else:
                            break
    return coef, bw, bh


def mcu_layout(f, coef):
    """`coefficients` in vf_jpeg_layouts_coefficients_host's layout (jpeg_prog_ref.mcu_layout, for either kind)."""
    P = parse(f)
    hs, vs, mcux, mcuy, _, _ = PR.geometry(P)
    out = np.zeros((mcuy * mcux, sum(h * v for h, v in zip(hs, vs)), 64), np.int16)
    b = 0
    for c in range(len(coef)):
        for y in range(vs[c]):
            for x in range(hs[c]):
                out[:, b, NATURAL] = coef[c][y::vs[c], x::hs[c]].reshape(mcuy * mcux, 64)
                b += 1
    return out.reshape(-1, 64)


# ---- jidctint.c jpeg_idct_islow
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_pass(d, n):
    """One pass along the last axis of d (..., 8), descaled by n."""
    z2, z3 = d[..., 2], d[..., 6]
    z1 = (z2 + z3) * 4433
    tmp2, tmp3 = z1 - z3 * 15137, z1 + z2 * 6270
    tmp0, tmp1 = (d[..., 0] + d[..., 4]) << 13, (d[..., 0] - d[..., 4]) << 13
    t10, t13, t11, t12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    o = [t10 + tmp3, t11 + tmp2, t12 + tmp1, t13 + tmp0, t13 - tmp0, t12 - tmp1, t11 - tmp2, t10 - tmp3]
    return np.stack([_descale(v, n) for v in o], -1)


def idct_plane(coef_zz, q_zz):
    """[block rows, block columns, 64] zig-zag coefficients -> the uint8 plane (dequantise, islow, range limit)."""
    br, bc, _ = coef_zz.shape
    nat = np.zeros((br, bc, 64), np.int64)
    nat[..., NATURAL] = coef_zz * np.asarray(q_zz, np.int64)
    blk = nat.reshape(br, bc, 8, 8)
    ws = _idct_pass(blk.swapaxes(-1, -2), 13 - 2).swapaxes(-1, -2)     # pass 1: columns
    px = _idct_pass(ws, 13 + 2 + 3)                                    # pass 2: rows
    j = px & 1023                                                      # idct_range_limit (the +128 is in the table)
    px = np.where(j < 128, j + 128, np.where(j < 512, 255, np.where(j < 896, 0, j - 896)))
    return px.transpose(0, 2, 1, 3).reshape(br * 8, bc * 8).astype(np.int64)


# ---- jdsample.c
def upsampler(rh, rv, cw):
    """jinit_upsampler's choice for a component that is 1 / rh by 1 / rv of the image and cw samples wide."""
    if (rh, rv) == (1, 1):
        return "copy"
    if (rh, rv) == (2, 1) and cw > 2:
        return "h2v1_fancy"
    if (rh, rv) == (2, 2) and cw > 2:
        return "h2v2_fancy"
    if (rh, rv) == (1, 2):
        return "h1v2_fancy"
    return "int"


def _rows_3_1(p):
    """Output rows 2r and 2r + 1 as 3 * in[r] + in[r -+ 1], the rows beyond the edges repeating the edge rows."""
    up, dn = np.vstack([p[:1], p[:-1]]), np.vstack([p[1:], p[-1:]])
    return 3 * p + up, 3 * p + dn


def upsample(p, rh, rv, method):
    """p: the component's REAL samples (ch x cw) -> (ch * rv) x (cw * rh)."""
    ch, cw = p.shape
    if method == "copy":
        return p
    if method == "int":
        return np.repeat(np.repeat(p, rv, 0), rh, 1)
    if method == "h1v2_fancy":
        a, b = _rows_3_1(p)
        out = np.empty((2 * ch, cw), np.int64)
        out[0::2], out[1::2] = (a + 1) >> 2, (b + 2) >> 2
        return out

    def h2(rows, lo, hi, sh, edge):
        # rows: per-sample sums; an output pair (3 * s[i] + s[i - 1] + lo) >> sh, (3 * s[i] + s[i + 1] + hi) >> sh, the
        # first and last outputs from their one sample alone
        out = np.empty((rows.shape[0], 2 * cw), np.int64)
        out[:, 2::2] = (3 * rows[:, 1:] + rows[:, :-1] + lo) >> sh
        out[:, 1:-1:2] = (3 * rows[:, :-1] + rows[:, 1:] + hi) >> sh
        out[:, 0], out[:, -1] = edge(rows[:, 0], lo), edge(rows[:, -1], hi)
        return out
    if method == "h2v1_fancy":
        return h2(p, 1, 2, 2, lambda s, _: s)
    a, b = _rows_3_1(p)                                                # h2v2_fancy
    out = np.empty((2 * ch, 2 * cw), np.int64)
    out[0::2] = h2(a, 8, 7, 4, lambda s, bias: (4 * s + bias) >> 4)
    out[1::2] = h2(b, 8, 7, 4, lambda s, bias: (4 * s + bias) >> 4)
    return out


def decode(f, channels=3):
    """The file -> uint8 H x W x channels, byte for byte libjpeg's default decompression."""
    P = parse(f)
    coef, _, _ = coefficients(f)
    W, H = P["width"], P["height"]
    hs, vs, _, _, _, _ = PR.geometry(P)
    hmax, vmax = max(hs), max(vs)
    full = []
    for c in range(len(coef)):
        cw, ch = cdiv(W * hs[c], hmax), cdiv(H * vs[c], vmax)
        p = idct_plane(coef[c], P["quant"][c])[:ch, :cw]
        rh, rv = hmax // hs[c], vmax // vs[c]
        full.append(upsample(p, rh, rv, upsampler(rh, rv, cw))[:H, :W])
    if P["colour"] == "grey":
        return np.repeat(full[0][..., None], channels, 2).astype(np.uint8)
    assert channels == 3
    if P["colour"] == "RGB":
        return np.stack(full, -1).astype(np.uint8)
    y, cb, cr = full[0], full[1] - 128, full[2] - 128                  # jdcolor.c ycc_rgb_convert
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)
