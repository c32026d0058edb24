"""The progressive form of the JPEG encoding rule of DESIGN.md 5.8 in numpy, on top of tests/jpeg_enc_ref.py and
jpeg_enc_opts_ref.gen_optimal_table: libjpeg's jpeg_simple_progression and jcphuff.c (the four scan kinds, their EOB runs and
correction bits, one optimal table per scan), whole files, byte for byte what Pillow's save(format="JPEG", quality=q,
subsampling=s, progressive=True) writes.  encode(frame, quality, subsampling) -> bytes is the definition vf_jpeg_encode_prog
(csrc/vf_jpeg_enc.hip) is held to; nothing here needs Pillow but make_golden(), which writes
tests/golden/jpeg_encode_prog_cases.npz (python tests/jpeg_enc_prog_ref.py)."""
import os

import numpy as np

import jpeg_enc_opts_ref as O
import jpeg_enc_ref as R

MAX_RUN = 0x7FFF
MAX_BE = 937                  # jcphuff.c: MAX_CORR_BITS - DCTSIZE2 + 1; a run is flushed once it buffers more bits than this

# (components, Ss, Se, Ah, Al) in the order of the file: jcparam.c's jpeg_simple_progression
SCANS_COLOUR = (((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
                ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0))
SCANS_GREY = (((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0))


def scan_script(C):
    return SCANS_COLOUR if C == 3 else SCANS_GREY


# ------------------------------------------------------------------------------------------------------ frames made by formula
def flat_grey_long():
    """136 x 16384 grey, flat: 34 816 blocks, so every AC scan is one EOB run that is cut once at 0x7FFF."""
    return np.full((136, 16384, 1), 77, np.uint8)


def busy_left_frame():
    """16 x 4096 grey: the left 64 columns busy, the rest flat, so the EOB runs of a block row cross the 256-block tiles and
    end at the busy blocks of the next row."""
    y, x = np.mgrid[0:16, 0:4096]
    busy = (x * 37 + y * 101 + (x * y) % 23 * 9) & 255
    return np.where(x < 64, busy, 90).astype(np.uint8)[..., None]


def flush_frame(rng):
    """8 x 224 grey for quality 100.  64 x 64 noise at quality 100 never buffers 937 correction bits: a block of noise nearly
    always has a coefficient that becomes non-zero in the scan, and its symbol ends the run.  So the first 24 blocks are
    picked from black-and-white noise to have no AC coefficient of magnitude 1, 2 or 3: in both refinement scans they bring
    no symbol and some 60 correction bits each, and the run is flushed after 16 of them.  The last 4 blocks are faint noise
    (127 .. 129, two of them on a tenth of the pixels only), whose few small coefficients behind long zero runs give
    refinement ZRLs in both refinement scans."""
    qt, blocks = R.quant_tables(100)[0], []
    while len(blocks) < 24:
        b = rng.integers(0, 2, (8, 8), dtype=np.uint8) * 255
        ac = np.abs(R.coefficients(b, qt)[0, 0, 1:])
        if ((ac == 0) | (ac >= 4)).all() and (ac >= 4).sum() >= 60:
            blocks.append(b)
    for share in (1.0, 1.0, 0.1, 0.1):
        blocks.append(np.where(rng.random((8, 8)) < share, rng.integers(127, 130, (8, 8)), 128).astype(np.uint8))
    return np.concatenate(blocks, 1)[..., None]


def zrl_frame():
    """24 x 24 RGB for quality 90, 4:4:4: every block is 128 plus three DCT basis functions: a low one and a high one (index
    40 and up) in grey, and one of index 20 and up in red minus blue.  Luma band 6 - 63 and both chroma scans 1 - 63 then
    meet zero runs above 15 in front of a coefficient: AC-first ZRL."""
    n = np.arange(8)
    cos = np.cos((2 * n[None, :] + 1) * n[:, None] * np.pi / 16) * np.where(n == 0, np.sqrt(0.5), 1.0)[:, None] / 2   # [u][x]
    basis = lambda k: np.outer(cos[int(R.ZZ[k]) // 8], cos[int(R.ZZ[k]) % 8])
    f = np.zeros((3, 3, 8, 8, 3))
    for i in range(9):
        grey, chroma = 40 * basis(1 + i % 3) + 200 * basis(40 + 2 * i), 240 * basis(20 + 3 * i)
        f[i // 3, i % 3] = 128 + np.stack([grey + chroma, grey, grey - chroma], -1)
    return np.clip(np.rint(f), 0, 255).astype(np.uint8).transpose(0, 2, 1, 3, 4).reshape(24, 24, 3)


# ------------------------------------------------------------------------------------------------------------------- the scans
def _geometry(H, W, C, subsampling):
    hs, vs = R.SUBSAMPLING[subsampling] if C == 3 else (1, 1)
    real = [(-(-H // 8), -(-W // 8))] + [(-(-(-(-H // vs)) // 8), -(-(-(-W // hs)) // 8))] * (C - 1)      # rows, columns
    return hs, vs, real, -(-W // (8 * hs)), -(-H // (8 * vs))


def _dc_blocks(comp, comps, H, W, C, subsampling):
    """The DC values of a DC scan's walk, [(component, dc)].  One component: its real blocks in raster order.  Interleaved: MCU
    by MCU, and a dummy carries the DC of the block libjpeg replicates (jccoefct.c), which is the previous real block of its
    component in scan order, as in the baseline rule."""
    hs, vs, real, mcux, mcuy = _geometry(H, W, C, subsampling)
    if len(comps) == 1:
        c = comps[0]
        return [(c, int(comp[c][y, x, 0])) for y in range(real[c][0]) for x in range(real[c][1])]
    out, last = [], [0] * C
    for my in range(mcuy):
        for mx in range(mcux):
            for i in comps:
                fh, fv = (hs, vs) if i == 0 else (1, 1)
                for by in range(fv):
                    for bx in range(fh):
                        y, x = my * fv + by, mx * fh + bx
                        if y < real[i][0] and x < real[i][1]:
                            last[i] = int(comp[i][y, x, 0])
                        out.append((i, last[i]))
    return out


def _ac_first_block(zz, ss, se, al):
    """-> ([(symbol, extra, count)], joins the EOB run)"""
    out, run = [], 0
    for k in range(ss, se + 1):
        v = int(zz[k])
        a = abs(v) >> al
        if a == 0:
            run += 1
            continue
        while run > 15:
            out.append((0xF0, 0, 0))
            run -= 16
        n = a.bit_length()
        out.append((run << 4 | n, (a if v >= 0 else ~a) & ((1 << n) - 1), n))
        run = 0
    return out, run > 0


def _ac_refine_block(zz, ss, se, al):
    """-> ([(symbol, sign bit, 1) or (None, correction bits, their count)] in the order of the stream, the trailing correction
    bits as a list, joins the EOB run)"""
    absv = [abs(int(zz[k])) >> al for k in range(ss, se + 1)]
    eob = max([k for k, a in zip(range(ss, se + 1), absv) if a == 1], default=0)
    out, run, br = [], 0, []
    for k, a in zip(range(ss, se + 1), absv):
        if a == 0:
            run += 1
            continue
        while run > 15 and k <= eob:
            out.append((0xF0, 0, 0))
            run -= 16
            out.append((None, br, len(br)))
            br = []
        if a > 1:
            br.append(a & 1)
            continue
        out.append((run << 4 | 1, 0 if int(zz[k]) < 0 else 1, 1))
        out.append((None, br, len(br)))
        br, run = [], 0
    return out, br, run > 0 or len(br) > 0


def _ac_scan(blocks, ss, se, ah, al, st):
    """One AC scan over `blocks` (each 64 coefficients, zig-zag): the items of the stream, ('s', symbol, extra, count) or
    ('b', [bits]).  jcphuff.c's EOBRUN and BE: the run is emitted in front of the next block with a symbol, at 0x7FFF, when a
    refinement scan buffers more than 937 bits, and at the end."""
    items, run, buffered = [], 0, []
    band = np.abs(np.asarray(blocks)[:, ss:se + 1]) >> al

    def flush():
        nonlocal run, buffered
        if run:
            n = run.bit_length() - 1
            items.append(("s", n << 4, run & ((1 << n) - 1), n))
            items.append(("b", buffered))
            st["eob_runs"] += 1
            run, buffered = 0, []

    quiet = ~band.any(axis=1)
    for zz, q in zip(blocks, quiet):
        if q:                                        # nothing in the band: joins the run, no symbol, no bits
            syms, tail, joins = [], [], True
        elif ah == 0:
            (syms, joins), tail = _ac_first_block(zz, ss, se, al), []
        else:
            syms, tail, joins = _ac_refine_block(zz, ss, se, al)
        if syms:
            flush()
            for sym, extra, n in syms:
                if sym is None:
                    items.append(("b", extra))
                else:
                    items.append(("s", sym, extra, n))
                    if sym == 0xF0:
                        st["zrl_refine" if ah else "zrl_first"] += 1
        if joins:
            run += 1
            buffered = buffered + tail
            if run == MAX_RUN:
                st["cut_7fff"] += 1
                flush()
            elif len(buffered) > MAX_BE:
                st["flush_937"] += 1
                flush()
    flush()
    return items


def _walk(comp_c, rows, cols):
    return [comp_c[y, x] for y in range(rows) for x in range(cols)]


def encode(frame, quality=75, subsampling="420", info=None):
    """One frame, uint8 H x W x C (C = 1 or 3; H x W is taken as H x W x 1) -> the file's bytes.  info, a dict, receives
    "scans": per scan a dict of `counts` ({table selector: 256 symbol counts}), `eob_runs`, `cut_7fff` (runs cut at 0x7FFF),
    `flush_937` (refinement runs flushed by the 937-bit limit), `zrl_first`, `zrl_refine`, `bytes` (stuffed), and
    `max_unlimited`, the longest code length of any scan's table before the limiting to 16 bits."""
    f = np.asarray(frame)
    if f.ndim == 2:
        f = f[..., None]
    H, W, C = f.shape
    hs, vs, real, mcux, mcuy = _geometry(H, W, C, subsampling)
    qt = R.quant_tables(quality)
    comp = [R.coefficients(p, qt[0 if i == 0 else 1]).astype(np.int64) for i, p in enumerate(R.planes(f, subsampling))]
    seg = lambda marker, body: bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)
    base = R.header(H, W, C, quality, subsampling)
    sof = base.index(b"\xff\xc0")
    out = bytearray(base[:sof] + b"\xff\xc2" + base[sof + 2:base.index(b"\xff\xc4")])
    tinfo = {}
    scans = []
    for comps, ss, se, ah, al in scan_script(C):
        st = dict(counts={}, eob_runs=0, cut_7fff=0, flush_937=0, zrl_first=0, zrl_refine=0)
        items = []                                   # ('s', table 0 luma / 1 chroma, symbol, extra, count) or ('b', bits)
        if se == 0 and ah == 0:
            pred = [0] * C
            for i, dc in _dc_blocks(comp, comps, H, W, C, subsampling):
                diff = (dc >> al) - pred[i]
                pred[i] = dc >> al
                n = abs(diff).bit_length()
                items.append(("s", int(i > 0), n, (diff if diff >= 0 else diff - 1) & ((1 << n) - 1), n))
        elif se == 0:
            items = [("b", [(dc >> al) & 1]) for _, dc in _dc_blocks(comp, comps, H, W, C, subsampling)]
        else:
            c = comps[0]
            for it in _ac_scan(_walk(comp[c], *real[c]), ss, se, ah, al, st):
                items.append(("s", int(c > 0)) + it[1:] if it[0] == "s" else it)
        for it in items:
            if it[0] == "s":
                st["counts"].setdefault(it[1], np.zeros(256, np.int64))[it[2]] += 1
        cls = 0 if se == 0 else 1
        codes = {}
        for t in sorted(st["counts"]):
            bits, vals = O.gen_optimal_table(st["counts"][t], tinfo)
            out += seg(0xC4, bytes([cls << 4 | t]) + bytes(bits) + bytes(vals))
            codes[t] = R._codes(bits, vals)
        # jcmarker.c: a DC scan names no AC table, a DC refinement no table at all, an AC scan no DC table
        sel = lambda i: int(i > 0) if se else (0 if ah else int(i > 0) << 4)
        out += seg(0xDA, bytes([len(comps)]) + b"".join(bytes([i + 1, sel(i)]) for i in comps) + bytes([ss, se, ah << 4 | al]))
        bw = R._Bits()
        for it in items:
            if it[0] == "s":
                bw.put(*codes[it[1]][it[2]])
                if it[4]:
                    bw.put(it[3], it[4])
            else:
                for b in it[1]:
                    bw.put(b, 1)
        if bw.n:
            bw.put((1 << (8 - bw.n)) - 1, 8 - bw.n)
        st["bytes"] = len(bw.out)
        out += bw.out
        scans.append(st)
    if info is not None:
        info.update(scans=scans, max_unlimited=tinfo.get("max_unlimited", 0))
    return bytes(out) + b"\xff\xd9"


# ---------------------------------------------------------------------------------------------------------------- the fixtures
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_encode_prog_cases.npz")
FORMULAS = {"flat_grey_long": flat_grey_long, "busy_left_frame": busy_left_frame, "zrl_frame": zrl_frame,
            "fibonacci_frame": O.fibonacci_frame}


def cases():
    """(name, frame or the name of its formula, quality, sampling); grey cases carry "420", which the encoder ignores"""
    rng = np.random.default_rng(20261020)
    noise = lambda h, w, c=3: rng.integers(0, 256, (h, w, c), dtype=np.uint8)

    def photo(h, w, c):                              # smooth ramps under a little noise: a few symbols per block, runs of EOBs
        y, x = np.mgrid[0:h, 0:w]
        p = np.stack([(3 * x + 2 * y + 40 * np.sin(x / 5.0 + k) + 30 * np.cos(y / 7.0 - k)) for k in range(c)], -1)
        return np.clip(p + rng.normal(0, 6, p.shape) + 60, 0, 255).astype(np.uint8)

    out = []
    for side in (1, 8):
        out.append(("%dx%d_grey" % (side, side), photo(side, side, 1) if side > 1 else noise(1, 1, 1), 75, "420"))
        rgb = photo(side, side, 3) if side > 1 else noise(1, 1, 3)
        out += [("%dx%d_%s" % (side, side, s), rgb, 75, s) for s in ("444", "422", "420")]
    p = photo(37, 53, 3)
    out += [("37x53_%s_q%d" % (s, q), p, q, s) for s in ("444", "422", "420") for q in (75, 95)]
    out += [("37x53_b_420_q75", photo(37, 53, 3), 75, "420"), ("37x53_c_420_q75", noise(37, 53), 75, "420")]     # for the batch
    out += [("flat16_grey", np.full((16, 16, 1), 200, np.uint8), 75, "420"), ("flat16_rgb", np.full((16, 16, 3), 31, np.uint8), 75, "420")]
    out.append(("flat_grey_long", "flat_grey_long", 75, "420"))
    out.append(("noise_q100_444", noise(64, 64), 100, "444"))
    out.append(("flush_grey_q100", flush_frame(rng), 100, "420"))
    out.append(("100x200_noise_q95_444", noise(100, 200), 95, "444"))
    out.append(("busy_left_grey", "busy_left_frame", 75, "420"))
    out.append(("zrl_444_q90", "zrl_frame", 90, "444"))
    out.append(("fibonacci_grey_q50", "fibonacci_frame", 50, "420"))
    return out


def load_golden():
    """name -> (frame, quality, sampling, Pillow's file)"""
    z = np.load(GOLD)
    out = {}
    for n in z["names"].tolist():
        frame = z["frame/" + n] if "frame/" + n in z.files else FORMULAS[str(z["formula/" + n])]()
        out[n] = (frame, int(z["quality/" + n]), str(z["sampling/" + n]), z["file/" + n].tobytes())
    return out


def pillow_file(frame, quality, sampling, **kw):
    import io

    from PIL import Image
    bio = io.BytesIO()
    kw = dict(format="JPEG", quality=quality, progressive=True, **kw)
    if frame.shape[2] == 1:
        Image.fromarray(frame[..., 0]).save(bio, **kw)
    else:
        Image.fromarray(frame).save(bio, subsampling={"444": 0, "422": 1, "420": 2}[sampling], **kw)
    return bio.getvalue()


def make_golden():
    """Writes the fixture: `names`; `frame/<name>` uint8 H x W x C or `formula/<name>`, a key of FORMULAS; `file/<name>`,
    Pillow's file; `quality/<name>`; `sampling/<name>`.  Asserts the rule against every file."""
    arrays, names, info = {}, [], {}
    for name, frame, q, s in cases():
        assert name not in names
        names.append(name)
        if isinstance(frame, str):
            arrays["formula/" + name] = np.array(frame)
            frame = FORMULAS[frame]()
        else:
            arrays["frame/" + name] = frame
        f = pillow_file(frame, q, s)
        info[name] = {}
        assert encode(frame, q, s, info[name]) == f, name
        arrays["file/" + name] = np.frombuffer(f, np.uint8)
        arrays["quality/" + name] = np.array(q, np.int64)
        arrays["sampling/" + name] = np.array(s)
        print(name, len(f))
    total = lambda n, key: [sc[key] for sc in info[n]["scans"]]
    assert total("flat_grey_long", "cut_7fff") == [0, 1, 1, 1, 0, 1] and total("flat_grey_long", "eob_runs") == [0, 2, 2, 2, 0, 2]
    assert sum(total("noise_q100_444", "flush_937")) == 0        # which is why flush_grey_q100 exists
    assert total("flush_grey_q100", "flush_937")[3] >= 1 and total("flush_grey_q100", "flush_937")[5] >= 1
    assert sum(total("flush_grey_q100", "zrl_refine")) >= 1
    z = total("zrl_444_q90", "zrl_first")
    assert z[4] >= 1 and z[2] >= 1 and z[3] >= 1, z
    assert info["fibonacci_grey_q50"]["max_unlimited"] >= 17
    assert b"\xff\x00" in arrays["file/100x200_noise_q95_444"].tobytes()
    arrays["names"] = np.array(names)
    np.savez_compressed(GOLD, **arrays)
    print(GOLD, os.path.getsize(GOLD), "bytes")
    assert os.path.getsize(GOLD) < 512 * 1024


if __name__ == "__main__":
    make_golden()
