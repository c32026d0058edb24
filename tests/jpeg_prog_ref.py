"""The progressive-JPEG entropy rule (jdphuff.c) in plain Python / numpy: file -> quantised coefficients per component.

`parse(file)` walks the markers: frame geometry and the scan list with the Huffman tables and the restart interval in
force at each SOS and the scan's restart segments (unstuffed).  `coefficients(file)` runs the four decoders
(decode_mcu_DC_first, decode_mcu_AC_first, decode_mcu_DC_refine, decode_mcu_AC_refine) over them.  `mcu_layout` puts
the per-component arrays into the block order of vf_jpeg_prog_coefficients_host.  No Pillow, no GPU."""
import numpy as np

NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                    54, 47, 55, 62, 63])


def cdiv(a, b):
    return -(-a // b)


class Bits:
    """MSB-first bits of one unstuffed segment; past its end the bits are 0 (a valid file never asks for them)."""

    def __init__(self, data):
        self.d, self.pos, self.acc, self.n = data, 0, 0, 0

    def bit(self):
        if self.n == 0:
            self.acc = self.d[self.pos] if self.pos < len(self.d) else 0
            self.pos += 1
            self.n = 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, k):
        v = 0
        for _ in range(k):
            v = (v << 1) | self.bit()
        return v


def huff_codes(counts, vals):
    """{(length, code): symbol} of a DHT table (canonical codes)."""
    codes, code, i = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            codes[(length, code)] = vals[i]
            i += 1
            code += 1
        code <<= 1
    return codes


def huff_decode(b, table):
    code = 0
    for length in range(1, 17):
        code = (code << 1) | b.bit()
        if (length, code) in table:
            return table[(length, code)]
    raise ValueError("bad code")


def extend(v, s):
    """HUFF_EXTEND"""
    return v - ((1 << s) - 1) if s and v < (1 << (s - 1)) else v


def markers(f):
    """[(offset, marker, payload)] of the file's marker segments up to EOI; an SOS's payload is its header, and
    (offset, 'data', (begin, end)) follows it with the byte range of its entropy-coded data."""
    out, i = [], 2
    while i + 1 < len(f):
        assert f[i] == 0xFF, "marker expected at %d" % i
        m = f[i + 1]
        if m == 0xD9:
            out.append((i, m, b""))
            break
        L = (f[i + 2] << 8) | f[i + 3]
        out.append((i, m, f[i + 4:i + 2 + L]))
        i += 2 + L
        if m == 0xDA:
            j = i
            while j + 1 < len(f) and not (f[j] == 0xFF and f[j + 1] != 0 and not 0xD0 <= f[j + 1] <= 0xD7):
                j += 1
            if j + 1 >= len(f):
                j = len(f)
            out.append((i, "data", (i, j)))
            i = j
    return out


def parse(f):
    """dict(width, height, comps [(id, h, v, tq)], scans [dict(components, Ss, Se, Ah, Al, restart_interval, begin, end,
    segments (list of unstuffed bytes), tables {0x00|id: DC, 0x10|id: AC}, sel {component: (td, ta)})])."""
    f = bytes(f)
    dht, dri, comps, W, H, scans, pending = {}, 0, None, 0, 0, [], None
    for _, m, seg in markers(f):
        if m == 0xC4:
            j = 0
            while j < len(seg):
                cnt = list(seg[j + 1:j + 17])
                n = sum(cnt)
                dht[seg[j]] = huff_codes(cnt, list(seg[j + 17:j + 17 + n]))
                j += 17 + n
        elif m == 0xDD:
            dri = (seg[0] << 8) | seg[1]
        elif m == 0xC2:
            H, W = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(seg[5])]
        elif m == 0xDA:
            ns = seg[0]
            ids = [c[0] for c in comps]
            cs = [ids.index(seg[1 + 2 * c]) for c in range(ns)]
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
    return dict(width=W, height=H, comps=comps, scans=scans)


def geometry(P):
    """(h, v per component, mcux, mcuy, real blocks per row, real block rows) — a single component counts as 1 x 1."""
    comps, W, H = P["comps"], P["width"], P["height"]
    hs = [1] if len(comps) == 1 else [c[1] for c in comps]
    vs = [1] if len(comps) == 1 else [c[2] for c in comps]
    hmax, vmax = max(hs), max(vs)
    mcux, mcuy = cdiv(W, 8 * hmax), cdiv(H, 8 * vmax)
    bw = [cdiv(cdiv(W * h, hmax), 8) for h in hs]
    bh = [cdiv(cdiv(H * v, vmax), 8) for v in vs]
    return hs, vs, mcux, mcuy, bw, bh


def scan_units(P, scan):
    """The scan's units in order: each a list of (component, block row, block column)."""
    hs, vs, mcux, mcuy, bw, bh = geometry(P)
    cs = scan["components"]
    if len(cs) > 1:
        order = [(c, y, x) for c in cs for y in range(vs[c]) for x in range(hs[c])]
        return [[(c, my * vs[c] + y, mx * hs[c] + x) for c, y, x in order] for my in range(mcuy) for mx in range(mcux)]
    c = cs[0]
    return [[(c, y, x)] for y in range(bh[c]) for x in range(bw[c])]


def coefficients(f):
    """-> (coef, bw, bh): coef[c] int64 [block rows (MCU-padded), block columns, 64] in ZIG-ZAG order; the real blocks
    are coef[c][:bh[c], :bw[c]]."""
    P = parse(f)
    hs, vs, mcux, mcuy, bw, bh = geometry(P)
    coef = [np.zeros((mcuy * vs[c], mcux * hs[c], 64), np.int64) for c in range(len(P["comps"]))]
    for sc in P["scans"]:
        units = scan_units(P, sc)
        Ss, Se, Ah, Al, tabs, sel = sc["Ss"], sc["Se"], sc["Ah"], sc["Al"], sc["tables"], sc["sel"]
        ri = sc["restart_interval"] or len(units)
        assert len(sc["segments"]) == cdiv(len(units), ri), (len(sc["segments"]), len(units), ri)
        for si, sg in enumerate(sc["segments"]):
            b, pred, eobrun = Bits(sg), [0] * len(coef), 0
            for u in units[si * ri:(si + 1) * ri]:
                for c, y, x in u:
                    blk = coef[c][y, x]
                    if Ss == 0:
                        if Ah == 0:                                    # decode_mcu_DC_first
                            s = huff_decode(b, tabs[sel[c][0]])
                            pred[c] += extend(b.bits(s), s)
                            blk[0] = pred[c] << Al
                        elif b.bit():                                  # decode_mcu_DC_refine
                            blk[0] |= 1 << Al
                        continue
                    t = tabs[0x10 | sel[c][1]]
                    if Ah == 0:                                        # decode_mcu_AC_first
                        if eobrun:
                            eobrun -= 1
                            continue
                        k = Ss
                        while k <= Se:
                            rs = huff_decode(b, t)
                            r, s = rs >> 4, rs & 15
                            if s:
                                k += r
                                blk[k] = extend(b.bits(s), s) * (1 << Al)
                                k += 1
                            elif r == 15:
                                k += 16
                            else:
                                eobrun = (1 << r) + (b.bits(r) if r else 0) - 1
                                break
                        continue
                    p1, m1, k = 1 << Al, -(1 << Al), Ss                # decode_mcu_AC_refine

                    def refine(k):
                        if b.bit() and (int(blk[k]) & p1) == 0:
                            blk[k] += p1 if blk[k] >= 0 else m1
                    if eobrun == 0:
                        while k <= Se:
                            rs = huff_decode(b, t)
                            r, s = rs >> 4, rs & 15
                            if s:
                                assert s == 1, "bad code"
                                s = p1 if b.bit() else m1
                            elif r != 15:
                                eobrun = (1 << r) + (b.bits(r) if r else 0)
                                break
                            while k <= Se:
                                if blk[k] != 0:
                                    refine(k)
                                else:
                                    r -= 1
                                    if r < 0:
                                        break
                                k += 1
                            if s:
                                blk[k] = s
                            k += 1
                    if eobrun > 0:
                        while k <= Se:
                            if blk[k] != 0:
                                refine(k)
                            k += 1
                        eobrun -= 1
    return coef, bw, bh


def mcu_layout(f, coef):
    """The per-component zig-zag arrays of `coefficients` in vf_jpeg_prog_coefficients_host's layout: int16 [blocks, 64],
    block m * bpm + b = block b of MCU m (components in frame order, each one's blocks in raster order), natural order."""
    P = parse(f)
    hs, vs, mcux, mcuy, _, _ = geometry(P)
    bpm = sum(h * v for h, v in zip(hs, vs))
    out = np.zeros((mcuy * mcux, bpm, 64), np.int16)
    b = 0
    for c in range(len(coef)):
        for y in range(vs[c]):
            for x in range(hs[c]):
                blocks = coef[c][y::vs[c], x::hs[c]].reshape(mcuy * mcux, 64)
                out[:, b, NATURAL] = blocks
                b += 1
    return out.reshape(-1, 64)
