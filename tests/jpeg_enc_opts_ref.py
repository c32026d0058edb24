"""The two options of the JPEG encoding rule of DESIGN.md 5.8 in numpy, on top of tests/jpeg_enc_ref.py: restart intervals
(jchuff.c's emit_restart, jcmarker.c's DRI) and optimised Huffman tables (the gather pass and jpeg_gen_optimal_table), whole
files, byte for byte what Pillow's save(format="JPEG", quality=q, subsampling=s, restart_marker_rows=r, restart_marker_blocks=b,
optimize=o) writes.  encode(frame, quality, subsampling, restart_rows, restart_blocks, optimize) -> bytes is the definition
the opts path of csrc/vf_jpeg_enc.hip is held to; with every option off it is jpeg_enc_ref.encode.  Nothing here needs Pillow."""
import numpy as np

import jpeg_enc_ref as R


def clamp_frame():
    """264 x 16384 grey, 33 rows of 2048 MCUs: restart_rows=32 asks for 65536 MCUs and gets DRI 0xFFFF and one RST0."""
    y, x = np.mgrid[0:264, 0:16384]
    return ((x // 8 * 7 + y // 8 * 13) & 255).astype(np.uint8)[..., None]


def fibonacci_frame():
    """848 x 512 grey for quality 50 (where the scaled tables are the base tables): 6784 blocks, 6764 of them with exactly one
    AC coefficient, of value 1, at zig-zag index k; k = 1 .. 18 occur 1, 1, 2, 3, ... 2584 times, blocks in scan order, the
    last 20 flat.  The symbol counts of the AC table are then Fibonacci numbers and the optimal code reaches 18 bits, so
    jpeg_gen_optimal_table's limiting to 16 has work to do.  A block is 128 + the rounded 8 x 8 DCT basis function times
    the quantiser's entry."""
    q = R.quant_tables(50)[0]
    n = np.arange(8)
    cosines = np.cos((2 * n[None, :] + 1) * n[:, None] * np.pi / 16) * np.where(n == 0, np.sqrt(0.5), 1.0)[:, None] / 2   # [u][x]
    fib, ks = [1, 1], []
    while len(fib) < 18:
        fib.append(fib[-1] + fib[-2])
    for k, count in enumerate(fib, 1):
        ks += [k] * count
    frame = np.full((848 // 8, 512 // 8, 8, 8), 128, np.int64)
    for b, k in enumerate(ks):
        v, u = divmod(int(R.ZZ[k]), 8)
        frame[b // 64, b % 64] += np.rint(q[k] * np.outer(cosines[v], cosines[u])).astype(np.int64)
    return frame.transpose(0, 2, 1, 3).reshape(848, 512, 1).astype(np.uint8)


def restart_interval(H, W, C, subsampling="420", restart_rows=0, restart_blocks=0):
    """The interval in MCUs (0: none): rows of MCUs win over blocks, and are clamped to what DRI can say (jcmaster.c)."""
    hs, _ = R.SUBSAMPLING[subsampling] if C == 3 else (1, 1)
    assert 0 <= restart_rows <= 65535 and 0 <= restart_blocks <= 65535
    return min(restart_rows * -(-W // (8 * hs)), 65535) if restart_rows > 0 else restart_blocks


def block_symbols(zz, pred):
    """jchuff.c's encode_one_block as symbols: [(class 0 DC / 1 AC, symbol, extra bits, their count)]; zz None is a dummy."""
    if zz is None:
        return [(0, 0, 0, 0), (1, 0, 0, 0)]
    diff = int(zz[0]) - pred
    n = abs(diff).bit_length()
    out = [(0, n, (diff if diff >= 0 else diff - 1) & ((1 << n) - 1), n)]
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append((1, 0xF0, 0, 0))
            run -= 16
        n = abs(v).bit_length()
        out.append((1, run << 4 | n, (v if v >= 0 else v - 1) & ((1 << n) - 1), n))
        run = 0
    if run:
        out.append((1, 0x00, 0, 0))
    return out


def scan_symbols(frame, quality=75, subsampling="420", interval=0):
    """The scan as libjpeg walks it: a list of segments (one per restart interval), each a list of (table 0 luma / 1 chroma,
    class, symbol, extra, count).  The DC predictors start at 0 in every segment; a dummy codes difference 0 and keeps them."""
    f = np.asarray(frame)
    H, W, C = f.shape
    hs, vs = R.SUBSAMPLING[subsampling] if C == 3 else (1, 1)
    qt = R.quant_tables(quality)
    comp = [R.coefficients(p, qt[0 if i == 0 else 1]) for i, p in enumerate(R.planes(f, subsampling))]
    real = [(-(-H // 8), -(-W // 8))] + [(-(-(-(-H // vs)) // 8), -(-(-(-W // hs)) // 8))] * (C - 1)
    mcux, mcuy = -(-W // (8 * hs)), -(-H // (8 * vs))
    segments, pred = [], [0] * C
    for m in range(mcux * mcuy):
        if m == 0 or (interval and m % interval == 0):
            segments.append([])
            pred = [0] * C
        my, mx = divmod(m, mcux)
        for i in range(C):
            fh, fv = (hs, vs) if i == 0 else (1, 1)
            for by in range(fv):
                for bx in range(fh):
                    y, x = my * fv + by, mx * fh + bx
                    zz = comp[i][y, x] if y < real[i][0] and x < real[i][1] else None
                    segments[-1] += [(int(i > 0),) + s for s in block_symbols(zz, pred[i])]
                    if zz is not None:
                        pred[i] = int(zz[0])
    return segments


def gen_optimal_table(counts, info=None):
    """jpeg_gen_optimal_table: 256 symbol counts -> (BITS[16], HUFFVAL).  info, a dict, receives the longest code length
    before the limiting to 16 bits."""
    freq = [int(c) for c in counts] + [1]                # the reserved code point: no real symbol gets the all-ones code
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, 1 << 62
        for i in range(257):
            if freq[i] and freq[i] <= v:
                v, c1 = freq[i], i
        c2, v = -1, 1 << 62
        for i in range(257):
            if freq[i] and freq[i] <= v and i != c1:
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 33
    for i in range(257):
        if codesize[i]:
            assert codesize[i] <= 32
            bits[codesize[i]] += 1
    if info is not None:
        info["max_unlimited"] = max(info.get("max_unlimited", 0), max(i for i in range(33) if bits[i]))
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [s for length in range(1, 33) for s in range(256) if codesize[s] == length]
    return tuple(bits[1:17]), tuple(vals)


def header(H, W, C, quality, subsampling, tables, interval):
    """jpeg_enc_ref.header with the DHT segments of `tables` ((Tc << 4 | Th, BITS, HUFFVAL) each) and, for a non-zero
    interval, DRI between the last DHT and SOS."""
    base = R.header(H, W, C, quality, subsampling)
    dht, sos = base.index(b"\xff\xc4"), len(base) - (2 + 6 + 2 * C)
    assert base[sos:sos + 2] == b"\xff\xda"
    seg = lambda marker, body: bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)
    out = base[:dht]
    for tc_th, bits, vals in tables:
        out += seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    if interval:
        out += seg(0xDD, interval.to_bytes(2, "big"))
    return out + base[sos:]


def encode(frame, quality=75, subsampling="420", restart_rows=0, restart_blocks=0, optimize=False, info=None):
    """One frame, uint8 H x W x C (C = 1 or 3; H x W is taken as H x W x 1) -> the file's bytes.  info, a dict, receives the
    interval, the number of segments, the header's length and, with optimize, the longest unlimited code length."""
    f = np.asarray(frame)
    if f.ndim == 2:
        f = f[..., None]
    H, W, C = f.shape
    interval = restart_interval(H, W, C, subsampling, restart_rows, restart_blocks)
    segments = scan_symbols(f, quality, subsampling, interval)
    tables = list(R.HUFF[:4 if C == 3 else 2])
    if optimize:
        counts = np.zeros((2, 2, 256), np.int64)         # [table][class][symbol]
        for seg in segments:
            for t, cls, sym, _, _ in seg:
                counts[t, cls, sym] += 1
        tables = [(cls << 4 | t,) + gen_optimal_table(counts[t, cls], info) for t in range(2 if C == 3 else 1) for cls in (0, 1)]
    codes = {tc_th: R._codes(bits, vals) for tc_th, bits, vals in tables}
    head = header(H, W, C, quality, subsampling, tables, interval)
    out = bytearray()
    for s, seg in enumerate(segments):
        bw = R._Bits()
        for t, cls, sym, extra, n in seg:
            bw.put(*codes[cls << 4 | t][sym])
            if n:
                bw.put(extra, n)
        if bw.n:
            bw.put((1 << (8 - bw.n)) - 1, 8 - bw.n)      # 1-bits to the byte; put() stuffs the byte if it comes out 0xFF
        out += bw.out
        if s + 1 < len(segments):
            out += bytes([0xFF, 0xD0 + (s & 7)])
    if info is not None:
        info.update(interval=interval, segments=len(segments), header=len(head))
    return head + bytes(out) + b"\xff\xd9"
