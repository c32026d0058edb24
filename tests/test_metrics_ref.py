"""tests/metrics_ref.py, the restatement of DESIGN.md 5.7 that vf_metrics.hip must equal exactly, pinned on the host:
hand cases of every column, the SSIM against an independent float64 form (scikit-image's recipe on
scipy.ndimage.uniform_filter), the float byte rule at its edges, and the host halves of the product (argument checks,
the table -> scores step), which need no GPU."""
from fractions import Fraction

import numpy as np
import pytest

import metrics_ref as R

N_, SSE, SAE, SQ, SN, FL = range(6)
Q = 1 << 30


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def test_columns_are_the_documented_ones():
    from video_filler_amd.backend import METRIC_COLUMNS
    assert R.COLUMNS == METRIC_COLUMNS == ("n", "sse", "sae", "ssim_q", "ssim_n", "flicker")


def test_identical_batches():
    a = noise((3, 9, 11, 3), 0)
    t = R.frame_table(a, a.copy())
    assert (t[:, 0, N_] == 9 * 11 * 3).all() and not t[:, 0, [SSE, SAE, FL]].any()
    assert (t[:, 0, SN] == 3 * 5 * 3).all() and (t[:, 0, SQ] == t[:, 0, SN] * Q).all()        # identical windows give exactly 2^30
    assert not t[:, 1].any()                                                                   # no mask: the hole is absent
    s = R.scores(t)
    assert np.isposinf(s["psnr"]).all() and (s["ssim"] == 1).all() and (s["mae"] == 0).all()
    assert np.isnan(s["hole_psnr"]).all() and np.isnan(s["hole_ssim"]).all()


@pytest.mark.parametrize("d", [1, 7, 100])
def test_constant_offset_without_saturation(d):
    a = np.random.default_rng(d).integers(0, 256 - d, (2, 8, 10, 3)).astype(np.uint8)
    t = R.frame_table(a, a + np.uint8(d))
    n = 8 * 10 * 3
    assert (t[:, 0, N_] == n).all() and (t[:, 0, SSE] == d * d * n).all() and (t[:, 0, SAE] == d * n).all()
    assert not t[:, 0, FL].any()                                         # the error does not change from frame to frame
    s = R.scores(t)
    assert np.allclose(s["psnr"], 10 * np.log10(255.0 ** 2 / d ** 2), rtol=1e-15) and (s["mae"] == d).all()


def test_frames_below_the_window_have_no_ssim():
    for h, w in ((6, 9), (9, 6), (1, 1)):
        t = R.frame_table(noise((2, h, w, 1), 1), noise((2, h, w, 1), 2))
        assert not t[:, 0, SN].any() and not t[:, 0, SQ].any() and (t[:, 0, N_] == h * w).all()
        s = R.scores(t)
        assert np.isnan(s["ssim"]).all() and np.isfinite(s["psnr"]).all()
    assert (R.frame_table(noise((1, 7, 7, 3), 1), noise((1, 7, 7, 3), 2))[:, 0, SN] == 3).all()       # one window per channel


def test_empty_mask_gives_nan_for_every_hole_score():
    t = R.frame_table(noise((2, 8, 8, 3), 3), noise((2, 8, 8, 3), 4), mask=np.zeros((8, 8), np.uint8))
    assert not t[:, 1].any()
    s = R.scores(t)
    for k in ("hole_psnr", "hole_ssim", "hole_mae", "hole_flicker"):
        assert np.isnan(s[k]).all() and np.isnan(s["mean"][k]), k
    assert np.isfinite(s["psnr"]).all()


def test_hole_membership_of_pixels_and_windows():
    a, b = noise((1, 9, 9, 3), 5), noise((1, 9, 9, 3), 6)
    m = np.zeros((9, 9), np.uint8)
    m[0, 0] = 255                                                        # a corner pixel: in no window's centre
    m[4, 5] = 1                                                          # any non-zero value is hole
    t = R.frame_table(a, b, mask=m)[0]
    d = a[0].astype(int) - b[0].astype(int)
    assert t[1, N_] == 6 and t[1, SSE] == (d[0, 0] ** 2).sum() + (d[4, 5] ** 2).sum()
    assert t[1, SN] == 3
    q = sum(int(R.window_q(a[0, 1:8, 2:9, c].astype(np.int64), b[0, 1:8, 2:9, c].astype(np.int64))[0, 0]) for c in range(3))
    assert t[1, SQ] == q                                                 # the window centred on (4, 5) spans rows 1..7, columns 2..8
    full = R.frame_table(a, b, mask=np.ones((9, 9), np.uint8))[0]
    assert (full[0] == full[1]).all()


def test_flicker():
    a, b = noise((1, 8, 8, 3), 7), noise((1, 8, 8, 3), 8)
    assert not R.frame_table(a, b)[:, :, FL].any()                       # one frame: nothing to compare with
    # the error of frame t is e * t: right in no frame, and steady — flicker sees e per sample from t = 1 on
    base = np.random.default_rng(9).integers(0, 100, (4, 8, 8, 3)).astype(np.uint8)
    e = 5
    res = (base + np.arange(4, dtype=np.uint8).reshape(4, 1, 1, 1) * np.uint8(e)).astype(np.uint8)
    t = R.frame_table(res, base)
    assert t[0, 0, FL] == 0 and (t[1:, 0, FL] == e * 8 * 8 * 3).all()
    assert not R.frame_table(res, base, clip=False)[:, :, FL].any()
    assert (R.frame_table(res, base, clip=False)[:, :, :FL] == t[:, :, :FL]).all()
    s = R.scores(t)
    assert (s["flicker"] == [0, e, e, e]).all() and s["mean"]["flicker"] == e
    # a result that is right in every other frame and off in between jumps: |d_t - d_{t-1}| = 10 everywhere
    alt = base.copy()
    alt[1::2] += 10
    assert (R.frame_table(alt, base)[1:, 0, FL] == 10 * 8 * 8 * 3).all()


def test_valid_rectangle_ignores_the_padding():
    a, b = noise((2, 12, 13, 3), 10), noise((2, 12, 13, 3), 11)
    m = noise((12, 13), 12) & 1
    want = R.frame_table(a[:, :9, :10], b[:, :9, :10], mask=m[:9, :10])
    a2, b2, m2 = a.copy(), b.copy(), m.copy()
    a2[:, 9:], a2[:, :, 10:], b2[:, 9:], b2[:, :, 10:], m2[9:], m2[:, 10:] = 1, 2, 3, 4, 1, 1
    assert (R.frame_table(a2, b2, mask=m2, valid=(9, 10)) == want).all()


def ssim_float64(x, y):
    """scikit-image's structural_similarity with its defaults for 8-bit data (uniform 7 x 7 filter, sample covariance,
    K1 0.01, K2 0.03, data_range 255), recalled: the mean over the windows that lie wholly inside the image."""
    from scipy.ndimage import uniform_filter
    x, y = x.astype(np.float64), y.astype(np.float64)
    NP = 49
    cov_norm = NP / (NP - 1)
    ux, uy = uniform_filter(x, 7), uniform_filter(y, 7)
    uxx, uyy, uxy = uniform_filter(x * x, 7), uniform_filter(y * y, 7), uniform_filter(x * y, 7)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    return S[3:-3, 3:-3].mean()


def ssim_cases():
    rng = np.random.default_rng(20)
    yy, xx = np.mgrid[0:40, 0:52]
    smooth = (127.5 + 100 * np.sin(yy / 7.0) * np.cos(xx / 9.0)).astype(np.uint8)
    rnd = rng.integers(0, 256, (40, 52), dtype=np.uint8)
    return {
        "random": (rnd, rng.integers(0, 256, (40, 52), dtype=np.uint8)),
        "random_close": (rnd, np.clip(rnd.astype(int) + rng.integers(-6, 7, rnd.shape), 0, 255).astype(np.uint8)),
        "smooth": (smooth, np.clip(smooth.astype(int) + rng.integers(-3, 4, smooth.shape), 0, 255).astype(np.uint8)),
        "flat": (np.full((40, 52), 255, np.uint8), np.full((40, 52), 255, np.uint8)),
        "flat_apart": (np.full((40, 52), 0, np.uint8), np.full((40, 52), 255, np.uint8)),
        "anti": (rnd, 255 - rnd),
    }


@pytest.mark.parametrize("name", sorted(ssim_cases()))
def test_ssim_against_the_float64_form(name):
    """Tolerance 1e-8 on the mean: the fixed point contributes at most 2^-31 per window, the filter's float rounding is
    far below C2."""
    x, y = ssim_cases()[name]
    t = R.frame_table(x[None, :, :, None], y[None, :, :, None])[0, 0]
    assert t[SN] == 34 * 46
    got, want = t[SQ] / (t[SN] * Q), ssim_float64(x, y)
    assert abs(got - want) <= 1e-8, (name, got, want)
    if name == "anti":
        assert got < -0.5                                                # the fixed point is signed
    if name == "flat":
        assert t[SQ] == t[SN] * Q


def test_window_rounding_is_to_nearest_even_and_signed():
    a, b = noise((16, 16), 30).astype(np.int64), noise((16, 16), 31).astype(np.int64)
    q = R.window_q(a, b)
    S = [R._box(v) for v in (a, b, a * a, b * b, a * b)]
    for i, j in ((0, 0), (9, 9), (3, 7)):
        sx, sy, sxx, syy, sxy = (int(v[i, j]) for v in S)
        n1, d1 = 20000 * sx * sy + 2401 * 65025, 10000 * (sx * sx + sy * sy) + 2401 * 65025
        n2 = 20000 * (49 * sxy - sx * sy) + 2352 * 585225
        d2 = 10000 * (49 * sxx - sx * sx + 49 * syy - sy * sy) + 2352 * 585225
        s = (float(n1) / float(d1)) * (float(n2) / float(d2))           # Python floats: IEEE doubles, the same three operations
        assert int(q[i, j]) == round(s * Q)                              # round(): to nearest, ties to even
        assert abs(Fraction(int(q[i, j]), Q) - Fraction(n1, d1) * Fraction(n2, d2)) < Fraction(1, Q)
    assert R.window_q(a, 255 - a).max() < 0


def test_float_byte_rule_at_its_edges():
    F = np.float32
    xs = []
    for k in range(256):
        x = F(k) / F(255)
        xs += [np.nextafter(x, F(-1)), x, np.nextafter(x, F(2))]
    xs = np.array(xs + [-0.0, -1e-30, -3.0, -np.inf, 1.0, 1.0000001, 7.0, np.inf, np.nan], F)
    want = []
    for x in xs.tolist():                                                # exact: a float32 times 255 has at most 32 significant bits
        if x != x or x <= 0:
            want.append(0)
        elif x >= 1:
            want.append(255)
        else:
            want.append(int(F(float(Fraction(255) * Fraction(x)))))      # one float32 rounding of the exact product, then truncation
    got = R.to_bytes(xs.reshape(1, 1, 1, -1))
    assert got.dtype == np.uint8 and got.shape == (1, 1, xs.size, 1)
    assert got.reshape(-1).tolist() == want
    assert want[3 * 255 + 1] == 255 and want[1] == 0 and 254 in want
    x = np.random.default_rng(40).uniform(-0.2, 1.2, (2, 3, 5, 4)).astype(F)
    assert (R.to_bytes(x) == np.trunc(F(255) * np.clip(x, 0, 1)).astype(np.uint8).transpose(0, 2, 3, 1)).all()
    # both forms of the same bytes give one table
    y = np.random.default_rng(41).uniform(-0.2, 1.2, (2, 3, 5, 4)).astype(F)
    assert (R.frame_table(x, y) == R.frame_table(R.to_bytes(x), R.to_bytes(y))).all()


def test_product_scores_from_the_table_match_the_restatement():
    from video_filler_amd import inference
    a, b = noise((3, 9, 9, 3), 50), noise((3, 9, 9, 3), 51)
    b[1] = a[1]                                                          # one perfect frame: psnr inf
    m = np.zeros((9, 9), np.uint8)
    m[2:6, 3:8] = 1
    for t in (R.frame_table(a, b, mask=m), R.frame_table(a, b), R.frame_table(a[:, :5], b[:, :5], mask=m[:5])):
        got, want = inference.scores_from_table(t), R.scores(t)
        assert sorted(got) == sorted(want) == sorted(["psnr", "ssim", "mae", "flicker", "hole_psnr", "hole_ssim", "hole_mae",
                                                      "hole_flicker", "mean"])
        for k in want:
            if k != "mean":
                assert got[k].dtype == np.float64 and np.array_equal(got[k], want[k], equal_nan=True), k
        assert sorted(got["mean"]) == sorted(k for k in want if k != "mean")
        for k, v in want["mean"].items():
            assert got["mean"][k] == v or (np.isnan(v) and np.isnan(got["mean"][k])), k
    s = R.scores(R.frame_table(a, b, mask=m))
    assert np.isposinf(s["psnr"][1]) and np.isposinf(s["mean"]["psnr"]) and s["ssim"][1] == 1


def test_argument_errors_are_raised_on_the_host():
    import torch
    from video_filler_amd.data import _check_metric_args as chk
    f = torch.zeros(2, 3, 8, 9)
    u = torch.zeros(2, 8, 9, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="both are float N x C x H x W or both uint8 N x H x W x C"):
        chk(f, torch.zeros(2, 3, 8, 8), None, None)
    with pytest.raises(ValueError, match="both are float"):
        chk(f, u.permute(0, 3, 1, 2), None, None)
    with pytest.raises(ValueError, match="both are float"):
        chk(f[0], f[0], None, None)
    with pytest.raises(ValueError, match="2 channels"):
        chk(torch.zeros(2, 2, 8, 9), torch.zeros(2, 2, 8, 9), None, None)
    with pytest.raises(ValueError, match="4 channels"):
        chk(torch.zeros(2, 8, 9, 4, dtype=torch.uint8), torch.zeros(2, 8, 9, 4, dtype=torch.uint8), None, None)
    with pytest.raises(ValueError, match=r"the mask is uint8 \(9, 8\); it is uint8 H x W = 8 x 9"):
        chk(u, u, torch.zeros(9, 8, dtype=torch.uint8), None)
    with pytest.raises(ValueError, match="the mask is float32"):
        chk(f, f, torch.zeros(8, 9), None)
    for bad in ((0, 9), (8, 10), (9, 9), (8, 0), (2.5, 3)):
        with pytest.raises(ValueError, match="outside 1..8 x 1..9"):
            chk(f, f, None, bad)
    a, b, m, valid = chk(f.double(), f, torch.ones(8, 9, dtype=torch.bool), (8, 9))
    assert a.dtype == b.dtype == torch.float32 and m.dtype == torch.uint8 and valid == (8, 9)
    assert chk(u, u, None, None)[3] == (8, 9)
