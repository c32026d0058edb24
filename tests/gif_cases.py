"""Frames shared by the GIF tests (test_gif_ref.py, test_gif_cabi.py, test_gpu_gif.py): made from fixed seeds and integer
arithmetic, nothing read from disk.  Every maker returns uint8 H x W x 3."""
import numpy as np

import gif_ref


def constant(H, W):
    return np.full((H, W, 3), (17, 130, 251), np.uint8)


def two_colour(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    m = ((yy * 3 + xx * 5) // 11) % 2 == 0
    return np.where(m[..., None], np.array([255, 255, 255], np.uint8), np.array([0, 32, 0], np.uint8)).astype(np.uint8)


def n_colours(H, W, n, seed=3):
    """exactly n distinct colours (n <= H * W), spread over many histogram cells and placed in a fixed shuffled order"""
    assert n <= H * W
    rng = np.random.default_rng(seed)
    keys = rng.choice(1 << 24, n, replace=False)
    pal = np.stack([keys >> 16, (keys >> 8) & 255, keys & 255], axis=1).astype(np.uint8)
    pick = np.concatenate([np.arange(n), rng.integers(0, n, H * W - n)])
    return pal[rng.permutation(pick)].reshape(H, W, 3)


def noise(H, W, seed=4):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _lowpass(a, r):
    for ax in (0, 1):
        for _ in range(3):                                          # three box filters: nearly Gaussian
            pad = np.concatenate([np.repeat(a.take([0], ax), r, ax), a, np.repeat(a.take([-1], ax), r, ax)], ax)
            c = np.cumsum(pad, ax, dtype=np.float64)
            c = np.concatenate([np.zeros_like(c.take([0], ax)), c], ax)
            n = a.shape[ax]
            a = (c.take(range(2 * r + 1, 2 * r + 1 + n), ax) - c.take(range(0, n), ax)) / (2 * r + 1)
    return a


def photo(H, W, seed=5):
    """low-passed noise stretched over the whole range, with a little sensor noise on top: smooth gradients, thousands of
    colours"""
    rng = np.random.default_rng(seed)
    a = _lowpass(rng.normal(0, 1, (H, W, 3)), max(2, min(H, W) // 8))
    a = (a - a.min((0, 1))) / np.maximum(a.max((0, 1)) - a.min((0, 1)), 1e-12)
    return np.clip(np.rint(a * 255 + rng.normal(0, 1.5, a.shape)), 0, 255).astype(np.uint8)


def smooth(H, W, seed=6):
    """the same without the noise, low-passed harder: long runs of equal indices after quantisation"""
    rng = np.random.default_rng(seed)
    a = _lowpass(rng.normal(0, 1, (H, W, 3)), max(2, min(H, W) // 4))
    a = (a - a.min((0, 1))) / np.maximum(a.max((0, 1)) - a.min((0, 1)), 1e-12)
    return np.rint(a * 255).astype(np.uint8)


def boundary(H, W, codes=None):
    """grey frame (<= 256 colours, so index == rank of the grey level) whose first chunk makes exactly codes[0] codes, so
    that the Clear behind it is one bit wider than its last code; where the frame ends inside a later chunk of at least
    codes[1] pixels, that tail makes codes[1] codes before EOI."""
    n = H * W
    assert n >= gif_ref.CHUNK
    if codes is None:
        codes = (1791, 767) if n % gif_ref.CHUNK >= 767 else (767, 255)
    idx = np.full(n, 7, np.uint8)
    idx[:gif_ref.CHUNK] = gif_ref.boundary_chunk(codes[0])
    tail = n % gif_ref.CHUNK
    if tail >= codes[1]:
        idx[n - tail:] = gif_ref.boundary_chunk(codes[1], tail)
    # the indices are the ranks of the grey levels: a relabelling, which keeps the number of codes
    return np.repeat(idx.reshape(H, W, 1), 3, axis=2)


def contents(H, W):
    """name -> frame, every content kind that fits the geometry"""
    out = {"constant": constant(H, W), "two_colour": two_colour(H, W), "noise": noise(H, W), "photo": photo(H, W)}
    if H * W >= 257:
        out["colours_256"] = n_colours(H, W, 256)
        out["colours_257"] = n_colours(H, W, 257)
    if H * W >= gif_ref.CHUNK:
        out["boundary"] = boundary(H, W)
    return out
