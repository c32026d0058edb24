"""Regenerate tests/golden/jpeg_cases.npz: JPEG files written by Pillow and Pillow's decode of each (libjpeg's default
decompression), so the device decoder's tests (tests/test_gpu_jpeg.py, tests/test_jpeg_inspect.py) need no Pillow.

Keys: `jpg/<name>` (uint8 file bytes) and `ref/<name>` (uint8 H x W x C, C = 1 for grayscale) for the supported cases;
`bad/<name>` (file bytes only) for files the decoder must report as unsupported.  Case names read
<mode>_<H>x<W>_<content>_q<quality>[_opt]_<restart>: mode 444 / 422 / 420 / L; restart none, b1 (every block / MCU), b4,
r1 (every MCU row).  Usage: python tests/golden/make_jpeg_golden.py"""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(1, 1), (7, 9), (8, 8), (3, 4), (17, 33), (127, 129)]
MODES = ["444", "422", "420", "L"]
QUALS = [(5, False), (50, False), (90, False), (100, False), (75, True)]
RSTS = [None, "b1", "b4", "r1"]
KINDS = ["noise", "smooth", "flat", "checker"]


def content(kind, h, w, rng):
    """noise; smooth gradients; flat (long EOB / ZRL runs); 4-pixel checkerboard."""
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "smooth":
        return np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 127 // max(h + w - 2, 1)],
                        -1).astype(np.uint8)
    if kind == "flat":
        return np.full((h, w, 3), (40, 170, 90), np.uint8)
    return ((((xx // 4) + (yy // 4)) % 2) * 255).astype(np.uint8)[..., None].repeat(3, -1)


def encode(a, mode, quality, restart=None, optimize=False, **extra):
    im = Image.fromarray(a[..., 0]) if mode == "L" else Image.fromarray(a)
    kw = dict(quality=quality, optimize=optimize, **extra)
    if mode != "L":
        kw["subsampling"] = {"444": 0, "422": 1, "420": 2}[mode]
    if restart == "b1":
        kw["restart_marker_blocks"] = 1
    elif restart == "b4":
        kw["restart_marker_blocks"] = 4
    elif restart == "r1":
        kw["restart_marker_rows"] = 1
    bio = io.BytesIO()
    im.save(bio, "JPEG", **kw)
    return bio.getvalue()


def pillow_decode(data):
    im = Image.open(io.BytesIO(data))
    a = np.asarray(im)
    return a[..., None] if a.ndim == 2 else a


def cases():
    """(name, file bytes) of the supported cases: every size meets every mode.  Quality, restart interval and content
    are indexed by size and mode together, so that across the six sizes each mode meets every quality, every restart
    interval and every content (checked by `coverage`)."""
    rng = np.random.default_rng(20261016)
    out = []
    for si, (h, w) in enumerate(SIZES):
        for mi, mode in enumerate(MODES):
            q, opt = QUALS[(si + mi) % len(QUALS)]
            rst = RSTS[(si + mi) % len(RSTS)]
            kind = KINDS[(si + si // 2 + mi) % len(KINDS)]
            name = "%s_%dx%d_%s_q%d%s_%s" % (mode, h, w, kind, q, "_opt" if opt else "", rst or "none")
            out.append((name, encode(content(kind, h, w, rng), mode, q, rst, opt)))
    for mode, kind, q, rst in (("420", "noise", 90, None), ("422", "smooth", 50, "r1")):
        out.append(("%s_360x480_%s_q%d_%s" % (mode, kind, q, rst or "none"), encode(content(kind, 360, 480, rng), mode, q, rst)))
    return out


def coverage(names):
    """Fail unless every mode meets every quality, restart interval and content among the small cases."""
    for mode in MODES:
        parts = [n.split("_") for n in names if n.startswith(mode + "_") and "360x480" not in n]
        assert {p[3] + ("_opt" if "opt" in p else "") for p in parts} == {"q%d%s" % (q, "_opt" if o else "") for q, o in QUALS}
        assert {p[-1] for p in parts} == {r or "none" for r in RSTS}, mode
        assert {p[2] for p in parts} == set(KINDS), mode


def with_luma_sampling(data, hv):
    """The file with its SOF0 luma sampling byte replaced (Pillow's subsampling="4:1:1" writes 2x2, so a 4:1:1 or 4:4:0
    header is made this way; only the inspector reads it)."""
    b = bytearray(data)
    sof = b.index(b"\xff\xc0")
    b[sof + 11] = hv
    return bytes(b)


def unsupported():
    a = content("smooth", 24, 40, np.random.default_rng(1))
    bio = io.BytesIO()
    Image.new("CMYK", (40, 24), (10, 20, 30, 40)).save(bio, "JPEG")
    f444 = encode(a, "444", 90)
    return [("progressive", encode(a, "420", 90, progressive=True)), ("cmyk", bio.getvalue()),
            ("411", with_luma_sampling(f444, 0x41)), ("440", with_luma_sampling(f444, 0x12))]


def main():
    arrays = {}
    cs = cases()
    coverage([n for n, _ in cs])
    for name, data in cs:
        arrays["jpg/" + name] = np.frombuffer(data, np.uint8)
        arrays["ref/" + name] = pillow_decode(data)
    for name, data in unsupported():
        arrays["bad/" + name] = np.frombuffer(data, np.uint8)
    path = os.path.join(HERE, "jpeg_cases.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", sum(k.startswith("jpg/") for k in arrays), "supported cases")


if __name__ == "__main__":
    main()
