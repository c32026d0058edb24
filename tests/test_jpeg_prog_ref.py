"""The progressive entropy rule in Python (tests/jpeg_prog_ref.py) against the encoder's reference: the
coefficients it decodes from a Pillow progressive file are the quantised coefficients tests/jpeg_enc_ref.py computes from
the source pixels (libjpeg's forward path), on every real block.  Reads the committed fixtures
(tests/golden/jpeg_progressive_cases.npz); a random matrix runs when Pillow is importable."""
import io
import os

import numpy as np
import pytest

import jpeg_enc_ref as E
import jpeg_prog_ref as R

try:
    from PIL import Image
except ImportError:   # pragma: no cover - the fixtures cover the same ground
    Image = None

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_progressive_cases.npz"))
WITH_SRC = sorted(k[4:] for k in GOLDEN.files if k.startswith("src/"))


def _check(f, src, mode, quality):
    coef, bw, bh = R.coefficients(f)
    qt = E.quant_tables(quality)
    want = [E.coefficients(p, qt[0 if i == 0 else 1]) for i, p in enumerate(E.planes(src, "444" if mode == "L" else mode))]
    assert len(coef) == (1 if mode == "L" else 3)
    for i in range(len(coef)):
        np.testing.assert_array_equal(coef[i][:bh[i], :bw[i]], want[i][:bh[i], :bw[i]], err_msg="component %d" % i)


@pytest.mark.parametrize("name", WITH_SRC)
def test_rule_gives_the_encoders_coefficients(name):
    parts = name.split("_")
    if parts[0].startswith("perm"):
        parts = parts[1:]
    _check(GOLDEN["jpg/" + name].tobytes(), GOLDEN["src/" + name], parts[0], int(parts[3][1:]))


def test_scan_scripts_of_the_fixtures():
    for name in WITH_SRC:
        P = R.parse(GOLDEN["jpg/" + name].tobytes())
        assert len(P["scans"]) == (6 if len(P["comps"]) == 1 else 10), name
        first = P["scans"][0]
        assert (first["Ss"], first["Se"], first["Ah"], first["Al"]) == (0, 0, 0, 1) and len(first["components"]) == len(P["comps"])


def test_17x33_420_has_3x5_real_luma_blocks_in_a_4x6_plane():
    f = GOLDEN["jpg/420_17x33_noise_q90_b4"].tobytes()
    coef, bw, bh = R.coefficients(f)
    assert (bh[0], bw[0]) == (3, 5) and coef[0].shape[:2] == (4, 6)
    # the dummy row and column get DC values from the interleaved DC scans; no AC scan visits them
    assert not coef[0][3, :, 1:].any() and not coef[0][:, 5, 1:].any()


@pytest.mark.skipif(Image is None, reason="Pillow writes the files")
def test_pillow_random_matrix():
    rng = np.random.default_rng(5)
    for h, w in ((1, 1), (9, 23), (40, 56)):
        for sub, mode in ((0, "444"), (1, "422"), (2, "420"), (None, "L")):
            for q in (5, 50, 90, 100):
                for extra in ({}, {"restart_marker_blocks": 3}, {"restart_marker_rows": 1}):
                    yy, xx = np.mgrid[0:h, 0:w]
                    a = np.clip(np.stack([128 + 90 * np.sin(xx / 7), 128 + 90 * np.cos(yy / 5), rng.integers(0, 256, (h, w))], -1) +
                                rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8)
                    src = a[..., :1] if sub is None else a
                    im = Image.fromarray(src[..., 0]) if sub is None else Image.fromarray(src)
                    bio = io.BytesIO()
                    im.save(bio, "JPEG", quality=q, progressive=True, **({} if sub is None else {"subsampling": sub}), **extra)
                    _check(bio.getvalue(), src, mode, q)
