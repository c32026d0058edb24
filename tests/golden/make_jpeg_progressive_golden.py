"""Regenerate tests/golden/jpeg_progressive_cases.npz: progressive JPEG files written by Pillow (libjpeg's default scan
script: 10 scans for colour, 6 for grey), Pillow's decode of each and, for the small cases, the source pixels, so the
progressive decoder's tests (tests/test_jpeg_prog_ref.py, tests/test_jpeg_prog_cabi.py,
tests/test_gpu_jpeg_progressive.py) need no Pillow.

Keys: `jpg/<name>` (uint8 file bytes), `ref/<name>` (Pillow's decode, uint8 H x W x C, C = 1 for grey) and `src/<name>`
(the pixels that were encoded; small cases only); `bad/<name>` (file bytes only) for files the decoder must refuse.  Case
names read <mode>_<H>x<W>_<content>_q<quality>_<restart> as in make_jpeg_golden.py; `perm<k>_...` are one file with its
scans reordered (each DHT / DRI ... SOS ... data group moved whole, DC first kept first, every refinement behind the
scan it refines), which decode to the same pixels.  Usage: python tests/golden/make_jpeg_progressive_golden.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_jpeg_golden import KINDS, MODES, RSTS, SIZES, content, encode, pillow_decode  # noqa: E402

QUALS = [5, 50, 90, 100]
PERMS = [[0, 2, 3, 1, 4, 6, 5, 8, 7, 9], [0, 6, 1, 2, 3, 4, 5, 7, 8, 9], [0, 4, 3, 2, 1, 5, 6, 7, 8, 9]]


def photo(h, w, rng):
    """Photo-like: smooth gradients, an edge, and grain over the left sixth."""
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([128 + 90 * np.sin(xx / 37.0) * np.cos(yy / 53.0), 128 + 100 * np.cos((xx + yy) / 71.0), 40 + 160.0 * (xx > w // 2)], -1)
    a[:, :w // 6] += rng.normal(0, 12, (h, w // 6, 3))
    return np.clip(a, 0, 255).astype(np.uint8)


def cases():
    """(name, file bytes, source pixels or None).  Quality, restart option and content rotate with size and mode as in
    make_jpeg_golden.py, so that each mode meets all of them (`coverage`)."""
    rng = np.random.default_rng(20261019)
    out = []
    for si, (h, w) in enumerate(SIZES):
        for mi, mode in enumerate(MODES):
            q = QUALS[(si + mi) % len(QUALS)]
            rst = RSTS[(si + mi) % len(RSTS)]
            kind = KINDS[(si + si // 2 + mi) % len(KINDS)]
            a = content(kind, h, w, rng)
            src = None if h * w > 4096 else a[..., :1] if mode == "L" else a     # the source pixels of the small cases only
            out.append(("%s_%dx%d_%s_q%d_%s" % (mode, h, w, kind, q, rst or "none"), encode(a, mode, q, rst, progressive=True), src))
    for mode, q, rst in (("420", 90, None), ("422", 50, "r1")):
        out.append(("%s_360x480_photo_q%d_%s" % (mode, q, rst or "none"), encode(photo(360, 480, rng), mode, q, rst, progressive=True), None))
    return out


def coverage(names):
    for mode in MODES:
        parts = [n.split("_") for n in names if n.startswith(mode + "_") and "360x480" not in n]
        assert {p[3] for p in parts} == {"q%d" % q for q in QUALS}, mode
        assert {p[-1] for p in parts} == {r or "none" for r in RSTS}, mode
        assert {p[2] for p in parts} == set(KINDS), mode


def scan_groups(f):
    """(head, groups): the bytes before the first scan's tables, and one byte string per scan: the DHT / DRI markers in
    front of its SOS, the SOS and its entropy-coded data."""
    marks, i = [], 2
    while True:
        m = f[i + 1]
        marks.append((i, m))
        if m == 0xD9:
            break
        i += 2 + ((f[i + 2] << 8) | f[i + 3])
        if m == 0xDA:
            while not (f[i] == 0xFF and f[i + 1] != 0 and not 0xD0 <= f[i + 1] <= 0xD7):
                i += 1
    starts, prev = [], -1
    for n, (_, m) in enumerate(marks):
        if m == 0xDA:
            b = n
            while b - 1 > prev and marks[b - 1][1] in (0xC4, 0xDD):
                b -= 1
            starts.append(marks[b][0])
            prev = n
    ends = starts[1:] + [marks[-1][0]]
    return f[:starts[0]], [f[s:e] for s, e in zip(starts, ends)]


def permuted():
    a = np.random.default_rng(2).integers(0, 256, (40, 56, 3), dtype=np.uint8)
    f = encode(a, "420", 85, None, progressive=True, restart_marker_blocks=5)
    head, G = scan_groups(f)
    assert len(G) == 10
    ref = pillow_decode(f)
    out = []
    for k, perm in enumerate(PERMS):
        g = head + b"".join(G[p] for p in perm) + b"\xff\xd9"
        assert np.array_equal(pillow_decode(g), ref), perm
        out.append(("perm%d_420_40x56_noise_q85_b5" % k, g, a))
    return out


def refused():
    """incomplete: the last scan dropped; disorder: the luma refinement moved in front of the scans it refines; badsos: the
    first refinement's Ah/Al byte patched to Ah=3, Al=1 (Al is not Ah - 1); cmyk: a progressive CMYK file."""
    a = content("smooth", 24, 40, np.random.default_rng(1))
    f = encode(a, "420", 90, progressive=True)
    head, G = scan_groups(f)
    assert not np.array_equal(pillow_decode(head + b"".join(G[:9]) + b"\xff\xd9"), pillow_decode(f))
    bad = bytearray(f)
    at = len(head) + sum(len(g) for g in G[:5]) + G[5].index(b"\xff\xda")
    assert bad[at + 9] == 0x21, hex(bad[at + 9])   # SOS: length 2, Ns 1, (component, tables) 2, Ss, Se, AhAl
    bad[at + 9] = 0x31
    bio = io.BytesIO()
    Image.new("CMYK", (40, 24), (10, 20, 30, 40)).save(bio, "JPEG", progressive=True)
    return [("incomplete", head + b"".join(G[:9]) + b"\xff\xd9"),
            ("disorder", head + G[0] + G[5] + b"".join(G[1:5]) + b"".join(G[6:]) + b"\xff\xd9"),
            ("badsos", bytes(bad)), ("cmyk", bio.getvalue())]


def main():
    arrays = {}
    cs = cases()
    coverage([n for n, _, _ in cs])
    for name, data, src in cs + permuted():
        arrays["jpg/" + name] = np.frombuffer(data, np.uint8)
        arrays["ref/" + name] = pillow_decode(data)
        if src is not None:
            arrays["src/" + name] = src
    for name, data in refused():
        arrays["bad/" + name] = np.frombuffer(data, np.uint8)
    path = os.path.join(HERE, "jpeg_progressive_cases.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", sum(k.startswith("jpg/") for k in arrays), "supported cases")


if __name__ == "__main__":
    main()
