"""tests/jpeg_enc_ref.py, the JPEG encoding rule of DESIGN.md 5.8 in numpy, against libjpeg: whole files, the header
built from its own tables included.  Against the golden files Pillow wrote (no Pillow needed), and, where Pillow
imports, against Pillow itself on a randomised matrix."""
import io
import os

import numpy as np
import pytest

import jpeg_enc_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_encode_cases.npz")


def test_every_golden_case_whole_file():
    z = np.load(GOLD)
    names = z["names"].tolist()
    assert len(names) >= 35
    for name in names:
        got = jpeg_enc_ref.encode(z["frame/" + name], int(z["quality/" + name]), str(z["sampling/" + name]))
        assert got == z["file/" + name].tobytes(), name
    assert len(jpeg_enc_ref.header(37, 53, 3, 75, "420")) == 623


def test_against_pillow_on_a_randomised_matrix():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    bad, n = [], 0
    for H in range(1, 35):
        for W in (1, 8, 15, 16, 17, 40):
            s = ("444", "422", "420", "grey")[(n + H) % 4]
            q = int(rng.integers(1, 101))
            C = 1 if s == "grey" else 3
            a = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
            if rng.integers(2):                                          # photo-like: a ramp under a little noise
                a = (a // 8 + np.linspace(0, 200, W)[None, :, None] + np.arange(H)[:, None, None]).astype(np.uint8)
            bio = io.BytesIO()
            if C == 1:
                Image.fromarray(a[..., 0]).save(bio, format="JPEG", quality=q)
            else:
                Image.fromarray(a).save(bio, format="JPEG", quality=q, subsampling={"444": 0, "422": 1, "420": 2}[s])
            n += 1
            if jpeg_enc_ref.encode(a, q, "420" if C == 1 else s) != bio.getvalue():
                bad.append((H, W, s, q))
    assert n >= 200 and not bad, "%d of %d differ: %s" % (len(bad), n, bad[:10])
