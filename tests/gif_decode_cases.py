"""Files shared by the GIF decoder's tests (test_gif_decode_ref.py, test_gif_decode_cabi.py, test_gpu_gif_decode.py): a small
general GIF writer, the hand-assembled files made with it from fixed seeds, the corrupt, malformed and unsupported ones, and
the Pillow-written files of tests/golden/gif_decode_cases.npz (made by tests/golden/make_gif_decode_golden.py).

Every fixture is a Case: its bytes, its kind (good, corrupt, malformed, unsupported), for a corrupt one the status word it
must give, and `pillow`: whether it belongs to the PILLOW-AGREED class, on which Pillow's seek(k) + convert("RGBA") equals the
rule of gif_decode_ref.py (alpha plane, and RGB where alpha is 255).  The class: the first frame covers the whole screen with
no transparent pixel; disposal 1 or 3 anywhere, disposal 0 behind a frame of disposal 0 or 1 (Pillow lets "unspecified"
inherit the method of the frame before it; the rule reads 0 as "keep"); disposal 2 only on a frame whose successor repaints
that rectangle opaquely.  Outside it Pillow fills disposed areas with the background colour and composes a partial first frame
differently: there gif_decode_ref.py alone is the rule, and nothing is compared with Pillow.  A fixture that fails the comparison belongs
to the other label, never to a tolerance: every comparison here is exact.
"""
import collections
import os
import struct

import numpy as np

import gif_cases
import gif_decode_ref as R
import gif_ref

TOKENS = 1984                                  # video_filler_amd.backend.GIF_DECODE_TOKENS: tokens per batch of k_gifd_lzw
Case = collections.namedtuple("Case", "data kind pillow status what")
HERE = os.path.dirname(os.path.abspath(__file__))


# ---------------------------------------------------------------------------------------------------------------- writer
def lzw_codes(idx, m, policy="standard"):
    """indices (< 1 << m) -> the codes of one frame, Clear and EOI included.  policy: "standard" — a Clear at the start and
    another whenever the dictionary has reached 4096 entries; "deferred" — a Clear at the start only: a full dictionary
    stays as it is; "none" — standard without the Clear at the start."""
    assert policy in ("standard", "deferred", "none") and 2 <= m <= 8
    clear, eoi = 1 << m, (1 << m) + 1
    px = [int(v) for v in np.asarray(idx).reshape(-1)]
    assert px and max(px) < clear
    codes = [] if policy == "none" else [clear]
    d, nxt, prefix = {}, eoi + 1, px[0]
    for b in px[1:]:
        key = (prefix, b)
        if key in d:
            prefix = d[key]
            continue
        codes.append(prefix)
        prefix = b
        if nxt < 4096:
            d[key] = nxt
            nxt += 1
            if nxt == 4096 and policy != "deferred":
                codes.append(clear)
                d, nxt = {}, eoi + 1
    return codes + [prefix, eoi]


def pack_codes(codes, m):
    """codes -> bytes, each at the width a decoder reads it at (the decoder's state is followed; the codes need not be a
    valid stream)"""
    clear, eoi = 1 << m, (1 << m) + 1
    acc, nbits = 0, 0
    width, nxt, prev = m + 1, eoi + 1, False
    for c in codes:
        assert c < 1 << width, "code %d does not fit %d bits" % (c, width)
        acc |= c << nbits
        nbits += width
        if c == clear:
            width, nxt, prev = m + 1, eoi + 1, False
        elif c != eoi:
            if prev and nxt < 4096:
                nxt += 1
                if nxt == 1 << width and width < 12:
                    width += 1
            prev = True
    return acc.to_bytes((nbits + 7) // 8, "little")


def sub_blocks(data, size=255):
    out = bytearray()
    for o in range(0, len(data), size):
        out.append(len(data[o:o + size]))
        out += data[o:o + size]
    return bytes(out) + b"\x00"


def table_bytes(table):
    """uint8 [n][3], n a power of two from 2 to 256 -> (the three size bits, the bytes)"""
    t = np.asarray(table, np.uint8).reshape(-1, 3)
    bits = {2 << k: k for k in range(8)}[len(t)]
    return bits, t.tobytes()


def gce(disposal=0, trans=None, delay=0):
    return b"\x21\xf9\x04" + bytes([disposal << 2 | (trans is not None)]) + struct.pack("<H", delay) + bytes([trans or 0, 0])


def image(idx, x=0, y=0, m=8, table=None, interlace=False, policy="standard", codes=None, stream=None, block=255, size=None):
    """One image block.  idx: h x w indices in display order (an interlaced frame's rows are reordered here).  codes / stream
    replace the encoder's output (corrupt files); size = (w, h) replaces idx's shape in the descriptor."""
    idx = np.asarray(idx, np.uint8)
    h, w = idx.shape
    if stream is None:
        rows = idx[R.lace_order(h)] if interlace else idx
        stream = pack_codes(lzw_codes(rows, m, policy) if codes is None else codes, m)
    if size is not None:
        w, h = size
    packed, tb = interlace << 6, b""
    if table is not None:
        bits, tb = table_bytes(table)
        packed |= 0x80 | bits
    return b"\x2c" + struct.pack("<HHHHB", x, y, w, h, packed) + tb + bytes([m]) + sub_blocks(stream, block)


def gif(W, H, blocks, table=None, version=b"GIF89a", loop=None, trailer=b"\x3b", background=0):
    packed, tb = 0x70, b""
    if table is not None:
        bits, tb = table_bytes(table)
        packed |= 0x80 | bits
    net = b"" if loop is None else b"\x21\xff\x0bNETSCAPE2.0\x03\x01" + struct.pack("<H", loop) + b"\x00"
    return version + struct.pack("<HHBBB", W, H, packed, background, 0) + tb + net + b"".join(blocks) + trailer


def palette(n, seed):
    """n distinct colours, none of them black (a painted pixel is never mistaken for an untouched one)"""
    rng = np.random.default_rng(seed)
    keys = rng.choice((1 << 24) - 1, n, replace=False) + 1
    return np.stack([keys >> 16, (keys >> 8) & 255, keys & 255], axis=1).astype(np.uint8)


def noise_idx(h, w, n, seed):
    return np.random.default_rng(seed).integers(0, n, (h, w), dtype=np.uint8)


def no_pair_twice(n):
    """n indices (n <= 8192) in which no pair of neighbours repeats: the coder makes one code per index"""
    seq = np.concatenate([(np.arange(256) * s) & 255 for s in range(1, 64, 2)]).astype(np.uint8)
    return seq[:n]


# ------------------------------------------------------------------------------------------------------------- fixtures
def _hand():
    fx = {}

    def add(name, data, kind="good", pillow=False, status=0, what=""):
        assert name not in fx
        fx["hand/" + name] = Case(bytes(data), kind, pillow, status, what)
    P2, P4, P8, P16, P256 = (palette(n, n) for n in (2, 4, 8, 16, 256))

    add("screen_1x1", gif(1, 1, [image([[1]], m=2)], table=P2), pillow=True)
    add("screen_3x5_87a", gif(3, 5, [image(noise_idx(5, 3, 4, 1), m=2, table=P4), image(noise_idx(5, 3, 16, 2), m=4, table=P16)],
                             version=b"GIF87a"), pillow=True)
    # 12 x 10: a full cover, then rectangles that touch each edge, a 1-pixel rectangle, transparency; disposal 0 and 1
    full = noise_idx(10, 12, 16, 3)
    rects = [(0, 0, 4, 3), (8, 7, 4, 3), (5, 5, 1, 1), (0, 4, 12, 2), (3, 0, 2, 10), (11, 9, 1, 1)]

    def rect_frames(disposals, seed, trans=7):
        out = [gce(disposals[0], None, 3), image(full, m=4)]
        for k, (x, y, w, h) in enumerate(rects):
            out += [gce(disposals[(k + 1) % len(disposals)], trans, 4 + k), image(noise_idx(h, w, 16, seed + k), x, y, m=4)]
        return out
    add("rects_d01", gif(12, 10, rect_frames([0, 1], 10), table=P16, loop=0), pillow=True)
    add("rects_d013", gif(12, 10, rect_frames([0, 3, 1, 3, 3, 1, 0], 20), table=P16, loop=3), pillow=True)
    add("d0_after_d3", gif(12, 10, rect_frames([1, 3, 0, 3, 3], 20), table=P16),
        what="Pillow lets a frame of disposal 0 inherit the method of the frame before it")
    add("rects_d4567", gif(12, 10, rect_frames([4, 5, 6, 7], 30), table=P16), what="disposal 4 .. 7 is 1 here")
    # disposal 2 on a frame whose successor covers the whole screen opaquely
    def d2_cover(d):
        return gif(12, 10, [gce(1), image(full, m=4), gce(2, 7), image(noise_idx(3, 4, 16, 40), 8, 7, m=4), gce(d),
                            image(noise_idx(10, 12, 16, 41), m=4), gce(2, 7), image(noise_idx(2, 12, 16, 42), 0, 4, m=4),
                            gce(1), image(noise_idx(10, 12, 16, 43), m=4)], table=P16)
    add("d2_then_cover", d2_cover(1), pillow=True)
    add("d0_after_d2", d2_cover(0), what="Pillow lets a frame of disposal 0 inherit the method of the frame before it")
    # outside the class: the rule alone
    add("partial_first", gif(12, 10, [gce(1), image(noise_idx(3, 4, 16, 50), 2, 2, m=4), gce(1, 3), image(noise_idx(10, 12, 16, 51), m=4)],
                             table=P16), what="a first frame that leaves canvas untouched")
    add("first_transparent", gif(12, 10, [gce(1, 5), image(noise_idx(10, 12, 16, 52), m=4), gce(3, 5), image(noise_idx(4, 4, 16, 53), 1, 1, m=4),
                                         gce(0, 5), image(noise_idx(2, 2, 16, 54), 9, 0, m=4)], table=P16),
        what="transparent pixels in the first frame")
    add("d2_left_open", gif(12, 10, [gce(2), image(full, m=4), gce(2, 7), image(noise_idx(3, 4, 16, 55), 8, 7, m=4), gce(1, 7),
                                    image(noise_idx(5, 5, 16, 56), 0, 0, m=4), gce(3), image(noise_idx(2, 2, 16, 57), 6, 6, m=4),
                                    gce(1, 2), image(noise_idx(10, 12, 16, 58), m=4)], table=P16),
        what="disposal 2 that nothing repaints: cleared to transparent")
    # interlace: heights 1, 2, 3, 4, 5, 8, 9 and 17 — every pass empty for some, non-empty for others
    lace = [gce(1), image(noise_idx(17, 7, 8, 60), m=3, interlace=True)]
    for k, h in enumerate((1, 2, 3, 4, 5, 8, 9)):
        lace += [gce(1, 0), image(noise_idx(h, 7 - k % 3, 8, 61 + k), k % 3, 17 - h - (k % 2 if h < 16 else 0), m=3, interlace=True)]
    add("interlaced", gif(7, 17, lace, table=P8), pillow=True)
    add("interlaced_local", gif(5, 9, [image(noise_idx(9, 5, 4, 70), m=2, table=P4, interlace=True),
                                      image(noise_idx(8, 5, 2, 71), 0, 1, m=2, table=P2, interlace=True)]), pillow=True)
    # every minimum code size, each frame with its own table
    sizes = [image(noise_idx(7, 9, 1 << m, 80 + m), m=m, table=palette(1 << m, 90 + m)) for m in range(2, 9)]
    add("code_sizes", gif(9, 7, sizes), pillow=True)
    # the token batch of k_gifd_lzw: one code per index, TOKENS - 1, TOKENS and TOKENS + 1 of them
    for n, (w, h) in ((TOKENS - 1, (661, 3)), (TOKENS, (64, 31)), (TOKENS + 1, (397, 5))):
        assert w * h == n
        codes = lzw_codes(no_pair_twice(n), 8)
        assert len(codes) == n + 2
        add("tokens_%d" % n, gif(w, h, [image(no_pair_twice(n).reshape(h, w), m=8)], table=P256), pillow=True)
    # the encoder's own boundary frame: the code width changes at a chunk's last code
    add("boundary_71x59", gif_ref.encode(gif_cases.boundary(71, 59)[None], 10), pillow=True)
    # 80 x 64 noise: the dictionary fills; under the deferred policy it stays full
    big = noise_idx(64, 80, 256, 100)
    assert len(lzw_codes(big, 8, "deferred")) > 4096 and lzw_codes(big, 8).count(256) == 2
    add("noise_deferred", gif(80, 64, [image(big, m=8, policy="deferred")], table=P256), pillow=True)
    add("noise_standard", gif(80, 64, [image(big, m=8)], table=P256), pillow=True)
    add("noise_no_clear", gif(80, 64, [image(big, m=8, policy="none", block=100)], table=P256), pillow=True)
    add("noise_deferred_m3", gif(80, 64, [image(noise_idx(64, 80, 8, 101), m=3, policy="deferred", interlace=True)], table=P8), pillow=True)
    # a long constant run: KwKwK chains, the longest strings, batches that end for want of room
    add("constant_200x200", gif(200, 200, [image(np.full((200, 200), 3, np.uint8), m=2)], table=P4), pillow=True)
    run = np.full((90, 90), 1, np.uint8)
    run[::7, ::5] = 2
    add("runs_90x90", gif(90, 90, [image(run, m=2, policy="none")], table=P4), pillow=True)
    # 70 frames: more than a wave's worth
    many = [gce(1, None, 2), image(noise_idx(4, 6, 16, 110), m=4)]
    for k in range(69):
        x, y = k % 5, k % 3
        many += [gce((1, 3, 1)[k % 3], 15, k), image(noise_idx(2, 2, 16, 111 + k), x, y, m=4)]
    add("frames_70", gif(6, 4, many, table=P16, loop=0), pillow=True)
    # extensions that are skipped, a loop count, bytes behind the trailer
    ext = [b"\x21\xfe" + sub_blocks(b"a comment that takes more than one sub-block" * 8, 100),
           b"\x21\xff\x0bXMP DataXMP" + sub_blocks(b"<x/>"), b"\x21\x01\x0c" + bytes(12) + sub_blocks(b"text"), gce(1, None, 7),
           image(noise_idx(4, 5, 4, 120), m=2), b"\x21\xfe" + sub_blocks(b"between"), gce(0, 2, 9), image(noise_idx(2, 3, 4, 121), 1, 1, m=2)]
    add("extensions", gif(5, 4, ext, table=P4, loop=7, trailer=b"\x3b" + b"junk behind the trailer \x2c\x00"), pillow=True)
    add("extra_codes_behind_full", gif(4, 4, [image(np.zeros((4, 4), np.uint8), m=2, codes=lzw_codes(noise_idx(4, 4, 4, 122), 2)[:-1]
                                                       + [1, 2, 3, 0, 1])], table=P4), what="codes behind the full rectangle, no EOI")

    # corrupt streams: each its own status
    z = np.zeros((4, 4), np.uint8)
    add("bad_code_above_next", gif(4, 4, [image(z, m=8, codes=[256, 5, 300, 1, 257])], table=P256), "corrupt", status=R.BAD_CODE)
    add("bad_first_after_clear", gif(4, 4, [image(z, m=8, codes=[256, 300, 1, 257])], table=P256), "corrupt", status=R.BAD_CODE)
    whole = pack_codes(lzw_codes(noise_idx(8, 8, 256, 130), 8), 8)
    add("short_cut", gif(8, 8, [image(np.zeros((8, 8), np.uint8), m=8, stream=whole[:len(whole) // 2])], table=P256), "corrupt",
        status=R.SHORT_DATA)
    add("short_eoi_early", gif(4, 4, [image(z, m=8, codes=[256, 1, 2, 3, 257])], table=P256), "corrupt", status=R.SHORT_DATA)
    add("short_no_data", gif(4, 4, [image(z, m=8, stream=b"")], table=P256), "corrupt", status=R.SHORT_DATA)
    add("bad_index", gif(4, 4, [image(np.array([[0, 1, 2, 3], [3, 2, 1, 0], [0, 5, 0, 0], [1, 1, 1, 1]]), m=3)], table=P4), "corrupt",
        status=R.BAD_INDEX)
    add("second_frame_short", gif(4, 4, [image(noise_idx(4, 4, 4, 131), m=2), image(z, 0, 0, m=2, codes=[4, 1, 5])], table=P4), "corrupt",
        status=R.SHORT_DATA)

    # malformed: refused on the host
    ok = gif(4, 4, [image(noise_idx(4, 4, 4, 140), m=2)], table=P4)
    add("no_trailer", ok[:-1], "malformed", what="no trailer")
    add("rect_off_screen", gif(4, 4, [image(noise_idx(4, 4, 4, 141), 1, 0, m=2)], table=P4), "malformed", what="leaves the")
    add("no_table", gif(4, 4, [image(noise_idx(4, 4, 4, 142), m=2)]), "malformed", what="no local colour table")
    at = 13 + 12 + 10                             # header and screen, the table of 4, the image descriptor
    assert ok[at] == 2
    add("min_code_9", ok[:at] + b"\x09" + ok[at + 1:], "malformed", what="minimum code size 9")
    add("bad_signature", b"GIF88a" + ok[6:], "malformed", what="signature")
    add("cut_in_table", ok[:15], "malformed", what="global colour table")
    add("no_frame", gif(4, 4, [gce(1)], table=P4), "malformed", what="no frame")
    # unsupported: refused with a reason, or handed to the fallback
    add("wide_16385", gif(16385, 1, [image([[1]], m=2)], table=P2), "unsupported", what="16384")
    return fx


def _pillow_written():
    z = np.load(os.path.join(HERE, "golden", "gif_decode_cases.npz"))
    agreed = set(str(s) for s in z["agreed"])
    return {k: Case(z[k].tobytes(), "good", k in agreed, 0, "") for k in z.files if k.startswith("pil/")}


_ALL = None


def fixtures():
    """name -> Case, made once"""
    global _ALL
    if _ALL is None:
        _ALL = dict(_hand())
        _ALL.update(_pillow_written())
    return _ALL


def of_kind(kind):
    return sorted(k for k, c in fixtures().items() if c.kind == kind)


_REF = {}


def reference(name):
    """(RGBA frames, status, meta) of a fixture by gif_decode_ref, computed once and left unchanged (read-only array)"""
    if name not in _REF:
        out, status, meta = R.decode(fixtures()[name].data, alpha=True)
        out.setflags(write=False)
        _REF[name] = (out, status, meta)
    return _REF[name]


def pillow_rgba(data):
    """Pillow's frames: seek(k), convert("RGBA")"""
    import io

    from PIL import Image
    im = Image.open(io.BytesIO(data))
    out = []
    for k in range(im.n_frames):
        im.seek(k)
        out.append(np.asarray(im.convert("RGBA")).copy())
    return np.stack(out)


def agrees_with_pillow(data, ref_rgba):
    """alpha planes equal, and RGB equal where alpha is 255"""
    got = pillow_rgba(data)
    if got.shape != ref_rgba.shape or not np.array_equal(got[..., 3], ref_rgba[..., 3]):
        return False
    opaque = ref_rgba[..., 3] == 255
    return bool(np.array_equal(got[..., :3][opaque], ref_rgba[..., :3][opaque]))
