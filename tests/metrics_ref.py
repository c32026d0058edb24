"""The scoring rule of DESIGN.md 5.7 in NumPy — its one restatement, which vf_metrics.hip equals exactly.

Everything is computed on BYTES: a float batch N x C x H x W goes through image.savePNG's rule first
(png_ref.float_to_bytes), a uint8 batch N x H x W x C is taken as it is.  `frame_table` gives the int64 table
[N][2][6] of the device call: per frame and region (0: every pixel of the valid rectangle; 1: those under the mask),
summed over the channels, the columns COLUMNS.  Every column is an integer sum (int64 throughout; the largest, sse of a
16384 x 16384 x 3 frame, stays below 2^46).  The one floating-point step is a window's SSIM, which is pinned to two
IEEE double divisions and one multiplication of exact integers, then rounded to a multiple of 2^-30.  `scores` is the
host side: float64 from the integers.
"""
import numpy as np

import png_ref

COLUMNS = ("n", "sse", "sae", "ssim_q", "ssim_n", "flicker")
WIN = 7                      # uniform window, NP = 49 samples
Q = 1 << 30                  # fixed point of a window's SSIM
C1_E4 = 65025                # 10^4 * (0.01 * 255)^2
C2_E4 = 585225               # 10^4 * (0.03 * 255)^2


def to_bytes(x):
    """float N x C x H x W in [0,1] or uint8 N x H x W x C -> uint8 N x H x W x C, the bytes save_frames writes."""
    x = np.asarray(x)
    assert x.ndim == 4
    if x.dtype == np.uint8:
        return x
    return np.ascontiguousarray(png_ref.float_to_bytes(x).transpose(0, 2, 3, 1))


def _box(x):
    """Sums over every WIN x WIN window that lies inside the int64 plane x: (h - 6) x (w - 6), entry (i, j) is the
    window whose centre is (i + 3, j + 3)."""
    h, w = x.shape
    s = np.zeros((h + 1, w + 1), np.int64)
    s[1:, 1:] = x.cumsum(0).cumsum(1)
    return s[WIN:, WIN:] - s[:-WIN, WIN:] - s[WIN:, :-WIN] + s[:-WIN, :-WIN]


def window_q(a, b):
    """int64 planes a, b (bytes) -> llrint(SSIM * 2^30) of every window inside them, (h - 6) x (w - 6)."""
    n = WIN * WIN
    Sx, Sy, Sxx, Syy, Sxy = _box(a), _box(b), _box(a * a), _box(b * b), _box(a * b)
    p = Sx * Sy
    vx, vy, cxy = n * Sxx - Sx * Sx, n * Syy - Sy * Sy, n * Sxy - p
    N1 = 20000 * p + n * n * C1_E4
    D1 = 10000 * (Sx * Sx + Sy * Sy) + n * n * C1_E4
    N2 = 20000 * cxy + n * (n - 1) * C2_E4
    D2 = 10000 * (vx + vy) + n * (n - 1) * C2_E4
    assert max(int(np.abs(v).max()) for v in (N1, D1, N2, D2)) < 1 << 53
    s = (N1.astype(np.float64) / D1.astype(np.float64)) * (N2.astype(np.float64) / D2.astype(np.float64))
    return np.rint(s * float(Q)).astype(np.int64)            # to nearest, ties to even


def frame_table(a, b, mask=None, valid=None, clip=True):
    """-> int64 [N][2][len(COLUMNS)].  a, b: both float N x C x H x W or both uint8 N x H x W x C; mask: H x W, non-zero =
    hole, or None; valid: (vh, vw), rows / columns that count, default the whole frame; clip: flicker runs over the
    batch (frames t >= 1), else it is 0."""
    A, B = to_bytes(a).astype(np.int64), to_bytes(b).astype(np.int64)
    assert A.shape == B.shape
    N, H, W, C = A.shape
    vh, vw = (H, W) if valid is None else valid
    assert 1 <= vh <= H and 1 <= vw <= W
    A, B = A[:, :vh, :vw], B[:, :vh, :vw]
    hole = None if mask is None else np.asarray(mask)[:vh, :vw] != 0
    windows = vh >= WIN and vw >= WIN
    out = np.zeros((N, 2, len(COLUMNS)), np.int64)
    for t in range(N):
        d = A[t] - B[t]
        fl = np.abs(d - (A[t - 1] - B[t - 1])) if clip and t > 0 else np.zeros_like(d)
        q = np.stack([window_q(A[t, :, :, c], B[t, :, :, c]) for c in range(C)], -1) if windows else None
        for reg in (0, 1):
            if reg == 1 and hole is None:
                continue
            pix = np.ones((vh, vw), bool) if reg == 0 else hole
            row = out[t, reg]
            row[0] = int(pix.sum()) * C
            row[1] = (d * d)[pix].sum()
            row[2] = np.abs(d)[pix].sum()
            if windows:
                centre = pix[3:vh - 3, 3:vw - 3]          # a window belongs to the region its centre pixel is in
                row[3] = q[centre].sum()
                row[4] = int(centre.sum()) * C
            row[5] = fl[pix].sum()
    return out


def scores(table):
    """The host side: the int64 table -> {psnr, ssim, mae, flicker and their hole_ forms: float64 [N]; "mean": the clip
    means}.  A region without samples, or without windows, gives nan; sse == 0 gives psnr inf.  The mean of flicker is
    over the frames t >= 1 (0.0 for a single frame)."""
    t = np.asarray(table, np.int64)
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for reg, pre in ((0, ""), (1, "hole_")):
            n, sse, sae, sq, sn, fl = (t[:, reg, k].astype(np.float64) for k in range(len(COLUMNS)))
            out[pre + "psnr"] = 10.0 * np.log10(65025.0 * n / sse)
            out[pre + "ssim"] = sq / (sn * float(Q))
            out[pre + "mae"] = sae / n
            out[pre + "flicker"] = fl / n
        out["mean"] = {k: (float(np.mean(v[1:])) if len(v) > 1 else 0.0) if k.endswith("flicker") else float(np.mean(v))
                       for k, v in out.items()}
    return out
