"""Regenerate tests/golden/jpeg_encode_opts_cases.npz: the frames the tests of the JPEG encoder's options encode and the files
Pillow (libjpeg-turbo) makes of them with Image.save(format="JPEG", quality=q, subsampling=s, restart_marker_rows=r,
restart_marker_blocks=b, optimize=o), so the tests need neither Pillow nor a random generator.

Keys: `names` (the cases, in order); `frame/<name>` uint8 H x W x C, or `formula/<name>`, the name of the function of
tests/jpeg_enc_opts_ref.py that makes the frame (the two large ones); `file/<name>` uint8, Pillow's file;
`options/<name>` int64 [quality, restart_rows, restart_blocks, optimize]; `sampling/<name>` ("444", "422", "420"; grey cases
carry "420", which the encoder ignores); `decoded/<name>`, Pillow's decode of the file (uint8 H x W x 3) for the small
cases: what a round trip through the device decoder must give.  The generator asserts what the cases must contain: a
stuffed pad byte in front of a marker (FF 00 FF Dn), a marker numbering that wraps, the clamp, an unlimited code length
of at least 17, and the file sizes the cases were designed to.  Usage: python tests/golden/make_jpeg_encode_opts_golden.py"""
import io
import os
import re
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import jpeg_enc_opts_ref  # noqa: E402
from make_jpeg_encode_golden import PILLOW_SUBSAMPLING, photo  # noqa: E402


def cases():
    """(name, frame or the name of its formula, quality, sampling, restart_rows, restart_blocks, optimize)"""
    rng = np.random.default_rng(20261019)
    noise = lambda h, w, c=3: rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    p = photo(37, 53, 3, rng)
    grey = p[..., 1:2].copy()
    out = []
    for tag, frame, s in (("420", p, "420"), ("422", p, "422"), ("444", p, "444"), ("grey", grey, "420")):
        for rr, rb in ((0, 1), (0, 3), (1, 0), (2, 0)):                       # dummies to the right and below at a segment's start
            out.append(("37x53_%s_r%d_b%d" % (tag, rr, rb), frame, 75, s, rr, rb, False))
    out.append(("37x53_420_r1_b5", p, 75, "420", 1, 5, False))                # both: rows win
    out += [("1x1_b1", noise(1, 1), 75, "420", 0, 1, False), ("8x8_b1", photo(8, 8, 3, rng), 75, "444", 0, 1, False),
            ("8x8_grey_r1", photo(8, 8, 1, rng), 75, "420", 1, 0, False)]     # DRI and no marker
    out.append(("100x200_noise_q95_b7", noise(100, 200), 95, "444", 0, 7, False))
    out.append(("clamp_r32", "clamp_frame", 75, "420", 32, 0, False))
    out += [("flat128_opt", np.full((24, 40, 3), 128, np.uint8), 75, "420", 0, 0, True),        # one-symbol tables
            ("flat7_grey_opt", np.full((9, 9, 1), 7, np.uint8), 90, "420", 0, 0, True),
            ("33x47_noise_420_opt", noise(33, 47), 90, "420", 0, 0, True),    # Cb and Cr share tables
            ("37x53_420_opt", p, 75, "420", 0, 0, True), ("37x53_grey_opt", grey, 75, "420", 0, 0, True),
            ("37x53_420_b3_opt", p, 75, "420", 0, 3, True),                   # predictor resets in the counts
            ("37x53_444_r1_opt", p, 92, "444", 1, 0, True),
            ("fibonacci_opt", "fibonacci_frame", 50, "444", 0, 0, True)]      # the limiting to 16 bits
    return out


def pillow_file(frame, quality, sampling, rr, rb, opt):
    bio = io.BytesIO()
    kw = dict(format="JPEG", quality=quality, restart_marker_rows=rr, restart_marker_blocks=rb, optimize=opt)
    if frame.shape[2] == 1:
        Image.fromarray(frame[..., 0]).save(bio, **kw)
    else:
        Image.fromarray(frame).save(bio, subsampling=PILLOW_SUBSAMPLING[sampling], **kw)
    return bio.getvalue()


def main():
    arrays, names, files, info = {}, [], {}, {}
    for name, frame, q, s, rr, rb, opt in cases():
        assert name not in names
        names.append(name)
        if isinstance(frame, str):
            arrays["formula/" + name] = np.array(frame)
            frame = getattr(jpeg_enc_opts_ref, frame)()
        else:
            arrays["frame/" + name] = frame
        f = pillow_file(frame, q, s, rr, rb, opt)
        info[name] = {}
        assert jpeg_enc_opts_ref.encode(frame, q, s, rr, rb, opt, info[name]) == f, name      # the rule against Pillow
        files[name] = f
        arrays["file/" + name] = np.frombuffer(f, np.uint8)
        arrays["options/" + name] = np.array([q, rr, rb, int(opt)], np.int64)
        arrays["sampling/" + name] = np.array(s)
        if max(frame.shape[:2]) <= 64:
            arrays["decoded/" + name] = np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
    scan = lambda n: files[n][info[n]["header"]:-2]
    assert info["37x53_444_r0_b1"]["segments"] == 35 and scan("37x53_444_r0_b1").count(b"\xff\xd0") >= 5       # wraps four times
    assert info["37x53_420_r1_b5"]["interval"] == 4 and info["1x1_b1"]["segments"] == 1
    assert re.search(b"\xff\x00\xff[\xd0-\xd7]", scan("100x200_noise_q95_b7")) and info["100x200_noise_q95_b7"]["segments"] == 47
    assert info["clamp_r32"] == dict(interval=65535, segments=2, header=info["clamp_r32"]["header"])
    assert b"\xff\xdd\x00\x04\xff\xff" in files["clamp_r32"][:400] and 80000 < len(files["clamp_r32"]) < 90000
    assert info["fibonacci_opt"]["max_unlimited"] >= 17 and len(files["fibonacci_opt"]) == 7774
    print(len(names), "cases;", {n: len(f) for n, f in files.items()})
    arrays["names"] = np.array(names)
    path = os.path.join(HERE, "jpeg_encode_opts_cases.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    main()
