"""The frames of the level-1 PNG encoder's tests (tests/test_gpu_png_dense.py, tests/test_png_dense_ref.py) and the reader
of their recorded fixture, tests/golden/png_dense_cases.npz (made by tests/golden/make_png_dense_golden.py).  Integer
arithmetic only: no random generator, so the frames are the same everywhere.

Small cases, each at most a few chunks of 8192 filtered bytes:
* the small fixtures of png_cases.npz (SMALL_FIXTURES) as they are;
* decode_crop: 96 x 128 x 3 cut from `decode` (5 chunks); padded_band: a cut of `padded` across its zero band;
* one_chunk / two_chunks: grey, 127 wide (rows of 128 filtered bytes), 64 and 128 rows: streams of exactly 8192 and 16384;
* row9000: 1 x 9000 x 1, whose second chunk is 809 bytes behind a full history;
* flat_run: a constant grey frame of three chunks, one run of equal bytes across both chunk boundaries;
* period_hist / period_longer: noise rows of 128 filtered bytes repeating every 64 rows (a byte period of exactly
  HIST = 8192) and every 65 rows (8320, out of the window's reach for all but the chunk's last bytes), 192 and 195 rows.
"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_dense_cases.npz")
PNG_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_cases.npz")
SMALL_FIXTURES = ("flat", "hramp", "vramp", "dramp", "noise", "photo_grey", "flat_grey", "noise_grey")
SIZED = ("photo", "decode", "padded")


def noise_bytes(count, seed):
    """`count` bytes of a 64-bit mixing function of the index: noise to a compressor, the same on every machine"""
    h = (np.arange(count, dtype=np.uint64) + np.uint64((seed * 0x632BE59BD9B4E019) & (2 ** 64 - 1))) * np.uint64(0x9E3779B97F4A7C15)
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    return (h & np.uint64(255)).astype(np.uint8)


def texture(H, W, C):
    """texture, flat bands and noisy bands (the mix of tests/test_gpu_png.py's synth, by this module's own arithmetic)"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    planes = []
    for c in range(C):
        v = (xx * xx * 3 + yy * 7 + (xx * yy) // 5 + 31 * c) & 255
        v = np.where((yy // 16) % 3 == 1, 200 - 40 * c, v)
        v = np.where((yy // 16) % 3 == 2, noise_bytes(H * W, 7 + c).reshape(H, W), v)
        planes.append(v)
    return np.stack(planes, -1).astype(np.uint8)


def periodic(rows, period):
    """grey rows x 127: row y is noise row y % period"""
    base = noise_bytes(period * 127, 3).reshape(period, 127)
    return np.ascontiguousarray(base[np.arange(rows) % period])[:, :, None]


def fixtures():
    z = np.load(PNG_GOLD)
    return {k[6:]: z[k] for k in z.files if k.startswith("frame/")}


def small_cases(fx=None):
    fx = fixtures() if fx is None else fx
    cases = {name: fx[name] for name in SMALL_FIXTURES}
    cases["decode_crop"] = np.ascontiguousarray(fx["decode"][100:196, 200:328])
    cases["padded_band"] = np.ascontiguousarray(fx["padded"][330:384, 400:512])
    cases["one_chunk"] = texture(64, 127, 1)
    cases["two_chunks"] = texture(128, 127, 1)
    cases["row9000"] = texture(1, 9000, 1)
    cases["flat_run"] = np.full((192, 127, 1), 0, np.uint8)
    cases["period_hist"] = periodic(192, 64)
    cases["period_longer"] = periodic(195, 65)
    return cases


def pack_tokens(chunks):
    """a list of token lists -> (int16 [tokens][2], int32 [chunks]): a literal is (byte, 0), a match (length, distance)"""
    rows = [(t if isinstance(t, tuple) else (t, 0)) for toks in chunks for t in toks]
    return np.array(rows, np.int16).reshape(-1, 2), np.array([len(t) for t in chunks], np.int32)


def unpack_tokens(tok, cnt):
    out, at = [], 0
    for c in cnt.tolist():
        out.append([(int(a), int(b)) if b else int(a) for a, b in tok[at:at + c].tolist()])
        at += c
    return out


def recorded():
    """-> (the npz, {case: recorded token lists per chunk})"""
    z = np.load(GOLD)
    return z, {k[4:]: unpack_tokens(z[k], z["cnt/" + k[4:]]) for k in z.files if k.startswith("tok/")}


def load():
    """-> (the npz, {case: frame}, {case: recorded token lists per chunk}); the frames of SMALL_FIXTURES come from
    png_cases.npz, every other from the recorded file"""
    z, toks = recorded()
    fx = fixtures()
    frames = {name: fx[name] for name in SMALL_FIXTURES}
    frames.update({k[6:]: z[k] for k in z.files if k.startswith("frame/")})
    return z, frames, toks
