"""Regenerate tests/golden/png_cases.npz: the frames the device PNG encoder's tests (tests/test_gpu_png.py) encode and
the size yardsticks they are held to, so the tests need neither Pillow nor a random generator.

Keys: `frame/<name>` (uint8 H x W x C) for every fixture; `sh/<name>` the yardstick S_H (tests/png_ref.py
`huffman_only_size`: the heuristic's filtered rows in the encoder's chunks, zlib Z_HUFFMAN_ONLY + sync flush, the
encoder's framing) and `s6/<name>` Pillow's compress_level=6 file size, for the photo-like, real-decode and padded
frames; `chunk` the chunk size the yardsticks were cut with.  Frames: photo (synthetic, photo-like), decode (Pillow's
decode of jpeg_cases.npz's 360 x 480 4:2:2 case), padded (the same zero-padded to 384 x 512, the shape of a whole-frame
output), flat (constant), hramp / vramp / dramp (ramps along x, y and both), noise (uniform random bytes), and grey
versions of photo, flat and noise.  Usage: python tests/golden/make_png_golden.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import png_ref  # noqa: E402

SIZED = ("photo", "decode", "padded")


def photo(h, w, rng):
    """Smooth shading, a few hard-edged shapes and sensor-like noise: what a video frame looks like to a filter."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, 3))
    for c in range(3):
        img[..., c] = 120 + 60 * np.sin(xx / (37.0 + 11 * c) + c) * np.cos(yy / (53.0 - 7 * c)) + 0.08 * (xx - yy)
    for _ in range(12):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(10, 70)
        col = rng.uniform(-70, 70, 3)
        img[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] += col
    for _ in range(6):
        y0, x0 = int(rng.uniform(0, h - 40)), int(rng.uniform(0, w - 60))
        img[y0:y0 + int(rng.uniform(8, 40)), x0:x0 + int(rng.uniform(8, 60))] = rng.uniform(20, 235, 3)
    img += rng.normal(0, 2.5, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def frames():
    rng = np.random.default_rng(20261017)
    z = np.load(os.path.join(HERE, "jpeg_cases.npz"))
    dec = np.ascontiguousarray(z["ref/422_360x480_smooth_q50_r1"])
    pad = np.zeros((384, 512, 3), np.uint8)
    pad[:360, :480] = dec
    ph = photo(384, 512, rng)
    yy, xx = np.mgrid[0:96, 0:160]
    hr = np.stack([xx * 255 // 159, 255 - xx * 255 // 159, (xx * 3) & 255], -1).astype(np.uint8)
    vr = np.stack([yy * 255 // 95, (yy * 7) & 255, 255 - yy * 255 // 95], -1).astype(np.uint8)
    dr = np.stack([(xx + yy) & 255, (2 * xx + 3 * yy) & 255, (xx * yy // 8) & 255], -1).astype(np.uint8)
    noise = rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)
    return {"photo": ph, "decode": dec, "padded": pad, "flat": np.full((128, 128, 3), (40, 170, 90), np.uint8),
            "hramp": hr, "vramp": vr, "dramp": dr, "noise": noise,
            "photo_grey": np.ascontiguousarray(ph[64:192, 64:192, 1:2]), "flat_grey": np.full((64, 200, 1), 77, np.uint8),
            "noise_grey": np.ascontiguousarray(noise[:, :, :1])}


def pillow_size(a, level):
    bio = io.BytesIO()
    Image.fromarray(a[..., 0] if a.shape[2] == 1 else a).save(bio, "PNG", compress_level=level)
    assert np.array_equal(png_ref.read_png(bio.getvalue()), a)          # the reader against Pillow's writer
    return len(bio.getvalue())


def main():
    arrays = {"chunk": np.int64(png_ref.CHUNK)}
    seen = set()
    for name, a in frames().items():
        arrays["frame/" + name] = a
        seen |= set(png_ref.choose_filters(a)[0].tolist())
        if name in SIZED:
            arrays["sh/" + name] = np.int64(png_ref.huffman_only_size(a))
            arrays["s6/" + name] = np.int64(pillow_size(a, 6))
            print(name, "S_H", int(arrays["sh/" + name]), "S_6", int(arrays["s6/" + name]))
    assert seen == {0, 1, 2, 3, 4}, "the fixtures must make the heuristic choose every filter type: %s" % sorted(seen)
    path = os.path.join(HERE, "png_cases.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "jpeg_cases.npz"))


if __name__ == "__main__":
    main()
