"""tests/apng_ref.py, the definition of the file vf_apng_encode writes, against an independent reader: a file assembled
from Pillow-written PNGs opens in Pillow with the frame count, the exact frames, the duration and the loop count, and
its sequence numbers and CRCs are what the APNG specification asks for."""
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

import apng_ref


def pillow_png(frame, **kw):
    b = io.BytesIO()
    Image.fromarray(frame).save(b, format="PNG", **kw)
    return b.getvalue()


def frames(n, H, W, C, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for j in range(n):
        g = ((xx * (j + 2) + yy * 3 + j * 17) & 255).astype(np.uint8)
        if j % 2:
            g = rng.integers(0, 256, (H, W), dtype=np.uint8)
        out.append(g if C == 1 else np.stack([g, 255 - g, (g // 2 + j) .astype(np.uint8)], -1))
    return out


@pytest.mark.parametrize("n,H,W,C,delay,loop", [(1, 5, 7, 3, 10, 0), (2, 33, 85, 3, 0, 3), (5, 64, 128, 1, 65535, 0),
                                                (3, 1, 1, 3, 7, 65535), (4, 64, 128, 3, 5, 1)])
def test_pillow_reads_what_assemble_writes(n, H, W, C, delay, loop):
    fr = frames(n, H, W, C)
    f = apng_ref.assemble([pillow_png(x) for x in fr], delay, loop)
    im = Image.open(io.BytesIO(f))
    assert im.format == "PNG" and im.size == (W, H) and getattr(im, "n_frames", 1) == n
    if n > 1:
        assert im.is_animated and im.info["loop"] == loop
    for k in range(n):
        im.seek(k)
        assert np.array_equal(np.asarray(im.convert("L" if C == 1 else "RGB")), fr[k]), "frame %d" % k
        if n > 1:
            assert im.info["duration"] == 10 * delay


def test_small_idat_chunks_become_one_fdat_each_and_numbers_have_no_gaps():
    """Pillow's own IDATs are 64 KiB; re-chunk a frame's stream into pieces of 1, 2, 3, ... bytes to see one fdAT per IDAT"""
    fr = frames(3, 16, 24, 3)
    files = []
    for x in fr:
        ch = apng_ref.chunks(pillow_png(x))
        z = b"".join(d for t, d in ch if t == b"IDAT")
        parts, at, k = [], 0, 1
        while at < len(z):
            parts.append(z[at:at + k])
            at += k
            k += 1
        files.append(apng_ref.SIGNATURE + apng_ref.chunk(b"IHDR", ch[0][1]) + b"".join(apng_ref.chunk(b"IDAT", p) for p in parts) +
                     apng_ref.chunk(b"IEND", b""))
    f = apng_ref.assemble(files, 4, 2)
    r = apng_ref.read(f)                                   # checks every CRC
    assert r["frames"] == 3 and r["loop"] == 2 and r["delays"] == [(4, 100)] * 3
    assert r["seqs"] == list(range(len(r["seqs"])))
    counts = [sum(t == b"IDAT" for t, _ in apng_ref.chunks(x)) for x in files]
    assert len(r["seqs"]) == 3 + counts[1] + counts[2] and counts[1] > 5
    for k in range(3):
        raw = zlib.decompress(r["streams"][k])
        assert len(raw) == 16 * (24 * 3 + 1)
    im = Image.open(io.BytesIO(f))
    for k in range(3):
        im.seek(k)
        assert np.array_equal(np.asarray(im.convert("RGB")), fr[k])


def test_the_file_is_a_png_of_frame_0_and_its_layout_is_the_rule():
    fr = frames(2, 8, 8, 3)
    p0, p1 = (pillow_png(x) for x in fr)
    f = apng_ref.assemble([p0, p1], 10, 0)
    ch = apng_ref.chunks(f)
    assert [t for t, _ in ch] == [b"IHDR", b"acTL", b"fcTL", b"IDAT", b"fcTL", b"fdAT", b"IEND"]
    assert ch[1][1] == struct.pack(">II", 2, 0)
    assert ch[2][1] == struct.pack(">IIIIIHHBB", 0, 8, 8, 0, 0, 10, 100, 0, 0)
    assert ch[3][1] == apng_ref.chunks(p0)[1][1]
    assert ch[5][1] == struct.pack(">I", 2) + apng_ref.chunks(p1)[1][1]
    assert len(f) == 8 + 25 + 20 + 38 + (12 + len(ch[3][1])) + 38 + (16 + len(ch[5][1]) - 4) + 12


def test_the_fdat_crc_identity_the_device_uses():
    """reg(fdAT || seq || data) = reg(IDAT || data) ^ (S(F, 'IDAT') ^ S(F, 'fdAT' || seq)) * x^(8 * len(data)): the raw CRC
    register is linear in its start value, for lengths around a chunk's and the smallest"""
    poly = 0xEDB88320

    def raw(reg, data):
        for b in data:
            reg ^= b
            for _ in range(8):
                reg = (reg >> 1) ^ poly if reg & 1 else reg >> 1
        return reg

    def mulmod(a, b):                                       # reflected: bit 31 is x^0
        p = 0
        for i in range(32):
            if a & (0x80000000 >> i):
                p ^= b
            b = (b >> 1) ^ poly if b & 1 else b >> 1
        return p

    def xpow(n):                                            # x^(8 n)
        r, sq = 0x80000000, 0x00800000
        while n:
            if n & 1:
                r = mulmod(r, sq)
            sq = mulmod(sq, sq)
            n >>= 1
        return r
    rng = np.random.default_rng(3)
    F = 0xFFFFFFFF
    for n in (0, 1, 2, 3, 255, 256, 4097, 8199, 8201):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        seq = struct.pack(">I", int(rng.integers(0, 1 << 31)))
        r_idat = raw(F, b"IDAT" + data)
        assert r_idat ^ F == zlib.crc32(b"IDAT" + data)
        got = r_idat ^ mulmod(raw(F, b"IDAT") ^ raw(F, b"fdAT" + seq), xpow(n))
        assert got ^ F == zlib.crc32(b"fdAT" + seq + data), n


@pytest.mark.parametrize("n,C", [(1, 3), (2, 1), (5, 3)])
def test_the_decoder_s_walk_takes_what_assemble_writes(n, C):
    """sequence numbers, CRCs and geometry pass apng_decode_ref.parse, and its canvases are the frames"""
    import apng_decode_ref
    fr = frames(n, 33, 85, C)
    f = apng_ref.assemble([pillow_png(x) for x in fr], 6, 4)
    d = apng_decode_ref.parse(f)
    assert d["frames"] == n and d["num_plays"] == 4 and d["animated"] and d["default_is_frame"] and d["supported"]
    assert all((x["x"], x["y"], x["w"], x["h"], x["delay_num"], x["delay_den"], x["dispose"], x["blend"]) == (0, 0, 85, 33, 6, 100, 0, 0)
               for x in d["frame_info"])
    got = apng_decode_ref.decode(f)
    for k in range(n):
        assert np.array_equal(got[k], np.repeat(fr[k][..., None], 3, axis=2) if C == 1 else fr[k])
