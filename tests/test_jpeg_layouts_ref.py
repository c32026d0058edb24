"""The layouts rule in numpy (tests/jpeg_layouts_ref.py) against libjpeg: Pillow's decode stored with the
fixtures of tests/golden/jpeg_layouts_cases.npz, and, where Pillow is importable, a randomised sweep of the fixture
generator's writer over sampling factors, scan splits, sizes and restart intervals.  No GPU."""
import io
import os
import sys

import numpy as np
import pytest

import jpeg_layouts_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "jpeg_layouts_cases.npz"))
NAMES = sorted(k[4:] for k in GOLDEN.files if k.startswith("jpg/"))


@pytest.mark.parametrize("name", NAMES)
def test_rule_equals_pillow(name):
    ref = GOLDEN["ref/" + name]
    np.testing.assert_array_equal(R.decode(GOLDEN["jpg/" + name].tobytes(), ref.shape[2]), ref)


def test_every_upsampler_and_colour_space_is_among_the_fixtures():
    seen, colours, scans = set(), set(), set()
    for name in NAMES:
        P = R.parse(GOLDEN["jpg/" + name].tobytes())
        hs, vs = R.PR.geometry(P)[:2]
        for h, v in zip(hs, vs):
            seen.add(R.upsampler(max(hs) // h, max(vs) // v, R.cdiv(P["width"] * h, max(hs))))
        colours.add(P["colour"])
        scans.add((P["sof"], len(P["scans"])))
    assert seen == {"copy", "h2v1_fancy", "h2v2_fancy", "h1v2_fancy", "int"}
    assert colours == {"grey", "YCbCr", "RGB"}
    assert {(0xC0, 1), (0xC0, 2), (0xC0, 3), (0xC1, 1), (0xC1, 2), (0xC2, 10)} <= scans
    # the replicate fallback of the two fancy horizontal cases: a (2, 1) and a (2, 2) component at most 2 samples wide
    narrow = set()
    for name in NAMES:
        P = R.parse(GOLDEN["jpg/" + name].tobytes())
        hs, vs = R.PR.geometry(P)[:2]
        for h, v in zip(hs, vs):
            r = (max(hs) // h, max(vs) // v)
            if r in ((2, 1), (2, 2)) and R.cdiv(P["width"] * h, max(hs)) <= 2:
                narrow.add(r)
    assert narrow == {(2, 1), (2, 2)}


def test_writer_sweep_against_pillow():
    Image = pytest.importorskip("PIL.Image")
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_jpeg_layouts_golden as G
    rng = np.random.default_rng(77)
    factor_sets = [f for f in G.LAYOUTS.values()] + [((2, 1), (1, 1), (1, 1)), ((1, 1), (1, 2), (2, 1)), ((2, 4), (1, 1), (1, 2)),
                                                     ((4, 1), (2, 1), (1, 1)), ((1, 2), (1, 2), (1, 1))]
    splits = [None, [[0], [1], [2]], [[0], [1, 2]], [[0, 1], [2]], [[2], [1], [0]], [[0, 2], [1]]]
    for i in range(60):
        h, w = int(rng.integers(1, 71)), int(rng.integers(1, 71))
        a = np.clip(rng.integers(0, 256, (h, w, 3)) * rng.uniform(0, 1) + np.add.outer(np.arange(h) * 3, np.arange(w) * 2)[..., None], 0,
                    255).astype(np.uint8)
        if i % 10 == 9:
            f = G.write(a[..., :1], (tuple(int(x) for x in rng.integers(1, 5, 2)),), dri=int(rng.integers(0, 5)))
        else:
            split = splits[int(rng.integers(0, len(splits)))]
            dri = [int(rng.integers(0, 6)) for _ in (split or [0])]
            f = G.write(a, factor_sets[int(rng.integers(0, len(factor_sets)))], split, dri=dri, quality=int(rng.integers(10, 101)),
                        sof=(0xC0, 0xC1)[i % 2], slots=((0, 1), (1, 0), (2, 3))[i % 3 if i % 2 else 0],
                        marker=("jfif", "adobe1", None)[i % 3])
        im = Image.open(io.BytesIO(f))
        ref = np.asarray(im.convert("L" if im.mode == "L" else "RGB"))
        ref = ref[..., None] if ref.ndim == 2 else ref
        np.testing.assert_array_equal(R.decode(f, ref.shape[2]), ref, err_msg="case %d" % i)
