"""Host restatement of what is new in the PNG encoder's level 1 (k_png_deflate_dense in vf_png.hip): the
matcher and the parse of one chunk.  NumPy and the standard library only.  The Huffman construction, the block header and
the framing are level 0's and are not restated, so the tests demand equal TOKENS, not equal files.

The rule, for chunk k of a frame's filtered stream s (png_ref.filter_stream), n = its bytes, begin = k * CHUNK:

* The window is the HIST bytes before the chunk (none for chunk 0; never another frame's) and the chunk.  Only chunk
  positions emit tokens; window positions before the chunk are match sources only.
* Every window position with two bytes behind it inside the window has the hash ((b0 | b1 << 8 | b2 << 16) * 0x9E3779B1
  mod 2^32) >> (32 - HASH_BITS); prev(i) is the nearest earlier window position with the same hash.
* A literal byte b costs cost[b] sixteenths of a bit, from the chunk's own byte histogram exactly as level 0 prices it;
  a match of (length, distance) costs 8 + 5 bits and the extra bits of both codes.
* A chunk position p (window position i) looks at distance 1, then at prev(i), prev(prev(i)), ... up to CANDIDATES chain
  entries, in that order.  A candidate's length is the common prefix, at most 258 and never past the chunk's end.  Only a
  candidate LONGER than every one before it is priced; its gain is the price of the literals it covers less its own; it
  becomes the position's match if its gain is at least MATCH_GAIN and above the gain held so far.  The walk ends at a
  candidate that reaches the longest possible length.
* Lazy step: a position's match is dropped if the next chunk position holds a longer match (as found above, before any
  dropping).
* Parse: from the chunk's start, a position with a match emits (length, distance) and moves on by length; one without
  emits its byte.
* Fallback: prices are estimates, so on photographic rows these tokens can code a little larger than level 0's.  The
  kernel codes the chunk with level 0's tokens too and keeps those where their block is strictly smaller, so no chunk's
  IDAT is larger than level 0's.  Which of the two a chunk shows depends on the Huffman construction, which is not
  restated here: a chunk of a level-1 file holds the tokens below, or exactly level 0's IDAT.
"""
import math
import struct
import zlib

import numpy as np

import png_ref

CHUNK = png_ref.CHUNK
HIST = 8192                 # PNG_HIST of vf_png.hip
HASH_BITS = 12
CANDIDATES = 64
MIN_MATCH, MAX_MATCH = 3, 258
MATCH_GAIN = 16

_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
              6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def _len_sym(length):
    for s in range(28, -1, -1):
        if length >= _LEN_BASE[s]:
            return 257 + s, _LEN_EXTRA[s]


def _dist_sym(dist):
    for s in range(29, -1, -1):
        if dist >= _DIST_BASE[s]:
            return s, _DIST_EXTRA[s]


_LEN_EB = np.zeros(MAX_MATCH + 1, np.int64)
for _l in range(MIN_MATCH, MAX_MATCH + 1):
    _LEN_EB[_l] = _len_sym(_l)[1]
_DIST_EB = np.zeros(32769, np.int64)
for _s in range(30):
    _DIST_EB[_DIST_BASE[_s]:] = _DIST_EXTRA[_s]


def literal_costs(chunk):
    """cost[256] in 1/16 bit from the chunk's byte histogram: log2(n / count) by the leading bit and four mantissa bits of
    the ratio, at least one bit, 15 bits for a byte that does not occur (level 0's rule)."""
    n = len(chunk)
    fr = np.bincount(np.frombuffer(chunk, np.uint8), minlength=256)
    cost = np.full(256, 15 * 16, np.int64)
    for b in range(256):
        if fr[b]:
            r = (n << 8) // int(fr[b])
            e = r.bit_length() - 1
            cost[b] = min(max(((e - 8) << 4) + ((r >> (e - 4)) & 15), 16), 15 * 16)
    return cost


def _common(u64, i, q, maxl):
    """common prefix lengths of window positions i and q (arrays), capped at maxl, eight bytes at a time"""
    out = np.zeros(len(i), np.int64)
    act = np.arange(len(i))
    while len(act):
        x = u64[i[act] + out[act]] ^ u64[q[act] + out[act]]
        same = x == 0
        nz = (x[~same].view(np.uint8).reshape(-1, 8) != 0).argmax(axis=1)
        out[act[~same]] += nz
        out[act[same]] += 8
        act = act[same]
        act = act[out[act] < maxl[act]]
    return np.minimum(out, maxl)


def matches(stream, chunk_index, candidates=None):
    """(length[n], distance[n]) of every chunk position before the lazy step; length 0 where there is no match"""
    candidates = CANDIDATES if candidates is None else candidates
    begin = chunk_index * CHUNK
    n = min(CHUNK, len(stream) - begin)
    h0 = min(HIST, begin)
    w = np.frombuffer(stream[begin - h0:begin + n], np.uint8)
    m = h0 + n
    pad = np.concatenate([w, np.zeros(MAX_MATCH + 16, np.uint8)])
    u64 = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(pad, 8)).view("<u8").reshape(-1)
    b = pad.astype(np.uint64)
    nh = max(m - 2, 0)
    h = (((b[:nh] | (b[1:nh + 1] << np.uint64(8)) | (b[2:nh + 2] << np.uint64(16))) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) \
        >> np.uint64(32 - HASH_BITS)
    prev = np.full(m, -1, np.int64)
    order = np.argsort(h, kind="stable")
    if nh > 1:
        same = h[order[1:]] == h[order[:-1]]
        prev[order[1:][same]] = order[:-1][same]
    cost = literal_costs(stream[begin:begin + n])
    pre = np.concatenate([[0], np.cumsum(cost[w[h0:]])])
    p = np.arange(n)
    i = p + h0
    maxl = np.minimum(MAX_MATCH, n - p)
    best_l, best_d, best_g = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    longest = np.zeros(n, np.int64)
    live = np.ones(n, bool)
    cand = i - 1                                       # distance 1 first
    live &= cand >= 0
    nxt = prev[i]
    for step in range(candidates + 1):
        idx = np.nonzero(live)[0]
        if not len(idx):
            break
        ln = _common(u64, i[idx], cand[idx], maxl[idx])
        d = i[idx] - cand[idx]
        longer = ln > longest[idx]
        longest[idx] = np.maximum(longest[idx], ln)
        ok = longer & (ln >= MIN_MATCH)
        g = np.zeros(len(idx), np.int64)
        g[ok] = pre[p[idx][ok] + ln[ok]] - pre[p[idx][ok]] - 16 * (13 + _LEN_EB[ln[ok]] + _DIST_EB[d[ok]])
        take = ok & (g >= MATCH_GAIN) & (g > best_g[idx])
        best_l[idx[take]], best_d[idx[take]], best_g[idx[take]] = ln[take], d[take], g[take]
        done = np.zeros(n, bool)
        done[idx[ln >= maxl[idx]]] = True
        if step == 0:
            live = np.ones(n, bool)
        live &= ~done
        cand = nxt
        live &= cand >= 0
        nxt = np.where(cand >= 0, prev[np.maximum(cand, 0)], -1)
    return best_l, best_d


def tokens(stream, chunk_index, candidates=None):
    """the chunk's tokens under the rule: an int for a literal byte, (length, distance) for a match"""
    ln, ds = matches(stream, chunk_index, candidates)
    n = len(ln)
    drop = np.zeros(n, bool)
    drop[:-1] = (ln[:-1] > 0) & (ln[1:] > ln[:-1])
    ln = np.where(drop, 0, ln).tolist()
    ds = ds.tolist()
    begin = chunk_index * CHUNK
    out, p = [], 0
    while p < n:
        if ln[p]:
            out.append((ln[p], ds[p]))
            p += ln[p]
        else:
            out.append(stream[begin + p])
            p += 1
    return out


def replay(toks, history=b""):
    """the bytes a token list stands for, behind `history`"""
    buf = bytearray(history)
    for t in toks:
        if isinstance(t, tuple):
            ln, d = t
            if d > len(buf):
                raise ValueError("distance %d reaches before the history (%d bytes)" % (d, len(buf)))
            for _ in range(ln):
                buf.append(buf[-d])
        else:
            buf.append(t)
    return bytes(buf[len(history):])


# --------------------------------------------------------------------------------------------------------- a recording inflate
class _Bits:
    def __init__(self, data, pos=0):
        self.d, self.pos = data, pos * 8

    def get(self, nbits):
        v = 0
        for k in range(nbits):
            bit = (self.d[self.pos >> 3] >> (self.pos & 7)) & 1
            v |= bit << k
            self.pos += 1
        return v


def _decoder(lengths):
    """canonical code (RFC 1951 3.2.2) -> {(length, code): symbol}"""
    count = [0] * 16
    for ln in lengths:
        count[ln] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    table = {}
    for sym, ln in enumerate(lengths):
        if ln:
            table[(ln, nxt[ln])] = sym
            nxt[ln] += 1
    return table


def _symbol(br, table):
    code = 0
    for ln in range(1, 16):
        code = (code << 1) | br.get(1)
        s = table.get((ln, code))
        if s is not None:
            return s
    raise ValueError("no such code")


_FIXED_LIT = _decoder([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
_FIXED_DIST = _decoder([5] * 30)
_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def tokens_of(zlib_stream, raw=False, kinds=False):
    """A small inflate that keeps the tokens: a zlib stream (raw deflate with raw=True) -> a list with one token list per
    deflate block (an int per literal, (length, distance) per match; a stored block gives its bytes as literals).  Empty
    stored blocks, which byte-align the encoder's chunks, are skipped.  With kinds, also the blocks' types: "stored",
    "fixed" or "dynamic" each."""
    data = bytes(zlib_stream)
    br = _Bits(data, 0 if raw else 2)
    blocks, types = [], []
    while True:
        final, btype = br.get(1), br.get(2)
        if btype == 0:
            br.pos = (br.pos + 7) & ~7
            at = br.pos >> 3
            ln, nln = struct.unpack("<HH", data[at:at + 4])
            if ln ^ nln != 0xFFFF:
                raise ValueError("stored block lengths")
            if ln:
                blocks.append(list(data[at + 4:at + 4 + ln]))
                types.append("stored")
            br.pos = (at + 4 + ln) * 8
        elif btype == 3:
            raise ValueError("block type 3")
        else:
            if btype == 1:
                lit, dist = _FIXED_LIT, _FIXED_DIST
            else:
                hlit, hdist, hclen = br.get(5) + 257, br.get(5) + 1, br.get(4) + 4
                cl = [0] * 19
                for k in range(hclen):
                    cl[_CL_ORDER[k]] = br.get(3)
                clt = _decoder(cl)
                lens = []
                while len(lens) < hlit + hdist:
                    s = _symbol(br, clt)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + br.get(2))
                    elif s == 17:
                        lens += [0] * (3 + br.get(3))
                    else:
                        lens += [0] * (11 + br.get(7))
                if len(lens) != hlit + hdist:
                    raise ValueError("code lengths overrun")
                lit, dist = _decoder(lens[:hlit]), _decoder(lens[hlit:])
            toks = []
            while True:
                s = _symbol(br, lit)
                if s < 256:
                    toks.append(s)
                elif s == 256:
                    break
                else:
                    ln = _LEN_BASE[s - 257] + br.get(_LEN_EXTRA[s - 257])
                    ds = _symbol(br, dist)
                    toks.append((ln, _DIST_BASE[ds] + br.get(_DIST_EXTRA[ds])))
            blocks.append(toks)
            types.append("fixed" if btype == 1 else "dynamic")
        if final:
            return (blocks, types) if kinds else blocks


# -------------------------------------------------------------------------------------------------------------- yardsticks
def zlib_chunked_size(img, level, hist, chunk=CHUNK):
    """S_Z(level, hist): png_ref.huffman_only_size's framing with zlib's default strategy at `level` on every chunk by
    itself, the `hist` bytes of the stream before the chunk given as the dictionary."""
    s = png_ref.filter_stream(img)
    total = png_ref.framing_bytes(len(s), chunk)
    for o in range(0, len(s), chunk):
        zd = s[max(0, o - hist):o] if hist else b""
        if zd:
            z = zlib.compressobj(level, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY, zd)
        else:
            z = zlib.compressobj(level, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY)
        total += len(z.compress(s[o:o + chunk]) + (z.flush(zlib.Z_FINISH) if o + chunk >= len(s) else z.flush(zlib.Z_SYNC_FLUSH)))
    return total


HEADER_FIXED_BITS = 17 + 19 * 3      # a dynamic block's fixed fields and its code-length code
HEADER_SYMBOL_BITS = 4               # allowance per used symbol in the two length tables


def chunk_estimate(toks, n, last):
    """bytes of one chunk's IDAT data: the tokens at their symbols' entropies, or a stored block if that is smaller"""
    fl, fd, extra = {256: 1}, {}, 0
    for t in toks:
        if isinstance(t, tuple):
            ls, le = _len_sym(t[0])
            ds, de = _dist_sym(t[1])
            fl[ls] = fl.get(ls, 0) + 1
            fd[ds] = fd.get(ds, 0) + 1
            extra += le + de
        else:
            fl[t] = fl.get(t, 0) + 1
    bits = float(extra + HEADER_FIXED_BITS + (0 if last else 3))
    for f in (fl, fd):
        bits += HEADER_SYMBOL_BITS * len(f)
        tot = sum(f.values())
        bits += sum(c * max(math.log2(tot / c), 1.0) for c in f.values())
    return min(int(math.ceil(bits / 8)) + (0 if last else 4), n + 5)


def estimate_size(img, candidates=None):
    """A CPU-only sanity figure of the level-1 file size of a frame (see chunk_estimate)."""
    s = png_ref.filter_stream(img)
    nch = -(-len(s) // CHUNK)
    total = png_ref.framing_bytes(len(s))
    for k in range(nch):
        n = min(CHUNK, len(s) - k * CHUNK)
        total += chunk_estimate(tokens(s, k, candidates), n, k == nch - 1)
    return total
