"""Regenerate tests/golden/jpeg_encode_cases.npz: the frames the JPEG encoder's tests encode and the files Pillow
(libjpeg-turbo) makes of them with Image.save(format="JPEG", quality=q, subsampling=s) and nothing else set, so the tests
need neither Pillow nor a random generator.

Keys: `names` (the cases, in order); `frame/<name>` uint8 H x W x C; `file/<name>` uint8, Pillow's file; `quality/<name>`;
`sampling/<name>` ("444", "422", "420"; grey cases carry "420", which the encoder ignores); `decoded/<name>`, Pillow's
decode of the file (uint8 H x W x 3), for the 37x53 and 100x75 frames at each sampling: what a round trip through the
device decoder must give.  No side is above 100.  The generator asserts that the cases together contain what a test
must reach: a stuffed 0xFF 0x00, a 0xF0 run symbol, a DC category of 11 and dummy blocks at both edges.  Usage: python tests/golden/make_jpeg_encode_golden.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_enc_ref  # noqa: E402

PILLOW_SUBSAMPLING = {"444": 0, "422": 1, "420": 2}
ROUND_TRIP = ("37x53", "37x53_422", "37x53_444", "100x75", "100x75_422", "100x75_444")


def photo(h, w, c, rng):
    """smooth shading, a hard-edged shape and a little noise"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([120 + 70 * np.sin(xx / (9.0 + 3 * k) + k) * np.cos(yy / (13.0 - 2 * k)) + 0.5 * (xx - yy) for k in range(c)], -1)
    img[h // 3:h // 3 + max(h // 4, 1), w // 4:w // 4 + max(w // 3, 1)] = rng.uniform(20, 235, c)
    img += rng.normal(0, 3.0, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def cases():
    """(name, frame, quality, sampling)"""
    rng = np.random.default_rng(20261018)
    noise = lambda h, w, c=3: rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    out = [("1x1", noise(1, 1), 75, "420"), ("1x1_grey", noise(1, 1, 1), 75, "420"),
           ("7x9", noise(7, 9), 75, "420"),                                   # a dummy row of blocks
           ("8x8", photo(8, 8, 3, rng), 75, "420"),                           # dummies to the right and below
           ("10x8", noise(10, 8), 90, "420"), ("20x24", photo(20, 24, 3, rng), 75, "420"),     # the even-height row rule
           ("12x40_noise", noise(12, 40), 100, "420"),
           ("17x33", photo(17, 33, 3, rng), 75, "420"), ("37x53", photo(37, 53, 3, rng), 75, "420"),
           ("16x16", photo(16, 16, 3, rng), 75, "420"), ("64x48", photo(64, 48, 3, rng), 75, "420")]     # no padding
    p, p2 = photo(37, 53, 3, rng), photo(100, 75, 3, rng)
    out += [("100x75", p2, 75, "420"), ("100x75_422", p2, 75, "422"), ("100x75_444", p2, 75, "444")]
    out += [("37x53_422", p, 75, "422"), ("37x53_444", p, 75, "444"), ("37x53_grey", p[..., 1:2].copy(), 75, "420"),
            ("8x8_grey", photo(8, 8, 1, rng), 75, "420"), ("17x33_422_noise", noise(17, 33), 90, "422"),
            ("9x17_444_noise", noise(9, 17), 30, "444")]
    for q in (1, 30, 75, 90, 100):                                            # the table rule and its clamps
        out.append(("37x53_q%d" % q, p, q, "420"))
    for q in (1, 100):
        out.append(("24x24_noise_q%d" % q, noise(24, 24), q, "444"))
    for v in (0, 128, 255):                                                   # EOB-only blocks
        out.append(("flat%d" % v, np.full((24, 40, 3), v, np.uint8), 75, "420"))
    out.append(("flat255_grey", np.full((9, 9, 1), 255, np.uint8), 90, "420"))
    step = np.zeros((8, 16, 1), np.uint8)
    step[:, 8:] = 255
    out += [("step_grey_q100", step, 100, "420"), ("step_q100", np.repeat(step, 3, 2), 100, "444")]     # DC category 11
    yy, xx = np.mgrid[0:32, 0:32]
    checker = (((yy + xx) & 1) * 255).astype(np.uint8)[..., None]
    out += [("checker_grey_q100", checker, 100, "420"), ("checker_q100", np.repeat(checker, 3, 2), 100, "444"),
            ("checker_420_q100", np.repeat(checker, 3, 2), 100, "420")]       # the largest AC magnitudes
    ramp = np.clip(40 + 2 * xx + yy, 0, 255).astype(np.uint8)
    ramp[7::8, 7::8] = 255                                                    # one bright pixel per block: long zero runs
    out += [("ramp_spike_grey_q90", ramp[..., None].copy(), 90, "420"),
            ("ramp_spike_q90", np.stack([ramp, ramp[::-1], ramp.T], -1).copy(), 90, "420")]
    out += [("100x75_noise_q100", noise(100, 75), 100, "420"), ("47x31_noise_grey_q100", noise(47, 31, 1), 100, "420"),
            ("33x100_noise_422_q95", noise(33, 100), 95, "422")]
    return out


def pillow_file(frame, quality, sampling):
    bio = io.BytesIO()
    if frame.shape[2] == 1:
        Image.fromarray(frame[..., 0]).save(bio, format="JPEG", quality=quality)
    else:
        Image.fromarray(frame).save(bio, format="JPEG", quality=quality, subsampling=PILLOW_SUBSAMPLING[sampling])
    return bio.getvalue()


def main():
    arrays, names, stats, stuffed = {}, [], {}, 0
    for name, frame, q, s in cases():
        assert max(frame.shape[:2]) <= 100 and name not in names
        f = pillow_file(frame, q, s)
        assert jpeg_enc_ref.encode(frame, q, s, stats) == f, name            # the rule against Pillow, and the statistics
        stuffed += f[len(jpeg_enc_ref.header(*frame.shape, q, s)):-2].count(b"\xff\x00")
        names.append(name)
        arrays["frame/" + name] = frame
        arrays["file/" + name] = np.frombuffer(f, np.uint8)
        arrays["quality/" + name] = np.int64(q)
        arrays["sampling/" + name] = np.array(s)
        if name in ROUND_TRIP:
            arrays["decoded/" + name] = np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
    print(len(names), "cases;", stats, "stuffed", stuffed)
    assert stuffed > 0 and stats["zrl"] > 0 and stats["dc_cat_max"] == 11 and stats["dummy_right"] > 0 and stats["dummy_below"] > 0
    arrays["names"] = np.array(names)
    path = os.path.join(HERE, "jpeg_encode_cases.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < os.path.getsize(os.path.join(HERE, "jpeg_cases.npz")) // 2


if __name__ == "__main__":
    main()
