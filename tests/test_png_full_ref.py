"""tests/png_full_ref.py (the full PNG rule: Adam7 and 16-bit samples) against Pillow, exactly, on every
fixture of tests/png_full_cases.py, and the host-only inspection of the device decoder against it.  No GPU."""
import io

import numpy as np
import pytest
from PIL import Image

import png_full_cases as cases
import png_full_ref
import png_load_ref
import video_filler_amd  # noqa: F401
from video_filler_amd import data


def _pillow(f):
    im = Image.open(io.BytesIO(f))
    im.load()
    return im


def test_the_cases_are_the_ones_the_rule_needs():
    have = {(c["color_type"], c["bit_depth"], c["interlace"], c["H"], c["W"]) for c in cases.GOOD.values()}
    for ct, d in cases.PAIRS:
        for H, W in cases.SIZES:
            assert (ct, d, 1, H, W) in have and ((ct, d, 0, H, W) in have) == (d == 16)
    assert len(cases.PAIRS) == 15 and len(cases.BAND) == 7
    for p in range(7):
        assert {t for q, t in cases.USED if q == p} == {0, 1, 2, 3, 4}, "pass %d" % (p + 1)
    assert data.png_info(cases.GOOD[cases.SPLIT]["file"])["idat_chunks"] == 6
    # pass 7 of a 131-row file has 65 rows: more than one 64-row band of the unfilter kernel
    assert all(png_full_ref.parse(cases.GOOD[n]["file"])["passes"][6][1] == 65 for n in cases.BAND)
    # which passes exist: pass 2 only from W = 5, pass 3 only from H = 5
    sizes = lambda H, W: [p[:2] for p in png_full_ref.passes(W, H, 1, 8, 1)]
    assert sizes(1, 1) == [(1, 1)] + [(0, 0)] * 6
    assert sizes(4, 5)[1] == (1, 1) and sizes(4, 5)[2] == (0, 0) and sizes(5, 4)[1] == (0, 0) and sizes(5, 4)[2] == (1, 1)


@pytest.mark.parametrize("name", sorted(cases.GOOD))
def test_rule_equals_pillow_exactly(name):
    c = cases.GOOD[name]
    f, ct, depth = c["file"], c["color_type"], c["bit_depth"]
    im = _pillow(f)
    s, top = png_full_ref.samples(f)
    got = png_full_ref.load(f)
    assert got.shape[:2] == (c["H"], c["W"]) and got.dtype == np.uint8
    # the decoded samples are the ones the writer was given, whatever the layout
    if ct != 3:
        assert np.array_equal(s, c["pixels"] * (255 // ((1 << depth) - 1) if depth < 8 else 1)), "the writer's samples"
    if depth == 16:
        assert top == 65535 and s.dtype == np.uint16 and np.array_equal(got, (s >> 8).astype(np.uint8))
        if ct == 0:
            assert im.mode == "I;16"
            a = np.asarray(im).astype(np.uint16)
            assert np.array_equal(a, s[..., 0]) and np.array_equal((a >> 8).astype(np.uint8), got[..., 0])
        elif ct == 2:
            assert im.mode == "RGB" and np.array_equal(np.asarray(im), got)
        elif ct == 4:                                      # Pillow: RGBA, the grey in channel 0, the alpha in channel 3
            a = np.asarray(im)
            assert im.mode == "RGBA" and np.array_equal(a[..., 0], got[..., 0]) and np.array_equal(a[..., 3], got[..., 1])
        else:
            assert im.mode == "RGBA" and np.array_equal(np.asarray(im), got)
        want = s.astype(np.float32) / np.float32(65535)
        assert np.array_equal(png_full_ref.load_float(f).view(np.uint32), want.view(np.uint32))
        return
    mode = {0: "L", 2: "RGB", 4: "LA", 6: "RGBA"}.get(ct) or ("RGBA" if "_trns" in name else "RGB")
    a = np.asarray(im.convert(mode))
    assert np.array_equal(a.reshape(got.shape), got), "Pillow, mode %s from %s" % (mode, im.mode)
    if ct == 3:
        assert np.array_equal(png_full_ref.load(f, 3), np.asarray(im.convert("RGB")))


def test_plain_8_bit_files_equal_the_default_rule():
    n = 0
    for ct, depth in cases.PAIRS:
        if depth == 16:
            continue
        for H, W in cases.SIZES[3:]:
            pix = cases.random_pixels(H, W, ct, depth, 100 + n)
            f = cases.write_png(pix, ct, depth, False, seed=n, plte=cases.palette(depth) if ct == 3 else None)
            lace = cases.write_png(pix, ct, depth, True, seed=n + 1, plte=cases.palette(depth) if ct == 3 else None)
            for ch in (None, 1, 3):
                if ch == 1 and ct in (2, 3, 6):
                    with pytest.raises(png_load_ref.PngUnsupported):
                        png_full_ref.load(f, ch)
                    continue
                want = png_load_ref.load(f, ch)
                assert np.array_equal(png_full_ref.load(f, ch), want) and np.array_equal(png_full_ref.load(lace, ch), want)
                assert np.array_equal(png_full_ref.load_float(f, ch).view(np.uint32), png_load_ref.load_float(f, ch).view(np.uint32))
            n += 1
    assert n == 11 * 7


def test_channels_rules_on_16_bit_files():
    for ct in (0, 2, 4, 6):
        f = cases.GOOD["c%dd16_lace_17x23" % ct]["file"]
        s = png_full_ref.samples(f)[0]
        three = png_full_ref.samples(f, 3)[0]
        assert np.array_equal(three, np.repeat(s[..., :1], 3, 2) if ct in (0, 4) else s[..., :3])
        if ct in (0, 4):
            assert np.array_equal(png_full_ref.samples(f, 1)[0], s[..., :1])
        else:
            with pytest.raises(png_load_ref.PngUnsupported, match="channels=1"):
                png_full_ref.load(f, 1)


@pytest.mark.parametrize("name", sorted(cases.BAD))
def test_corrupt_cases_raise_what_their_status_names(name):
    f, st = cases.BAD[name]
    word = {v: k for k, v in cases.STATUS.items()}[st]
    with pytest.raises(png_load_ref.PngError, match=word) as e:
        png_full_ref.load(f)
    assert not isinstance(e.value, png_load_ref.PngUnsupported)
    assert png_full_ref.parse(f)["supported"] and data.png_info(f, full=True)["supported"]


def test_the_two_layouts_of_17x23x3_inflate_to_different_sizes():
    laced, plain = cases.BAD["lace_flag_cleared"][0], cases.BAD["lace_flag_set"][0]
    a, b = png_full_ref.parse(laced), png_full_ref.parse(plain)
    assert (a["interlace"], b["interlace"]) == (0, 1)
    assert a["inflated_bytes"] == 17 * (1 + 69) and b["inflated_bytes"] == sum(h * (1 + rb) for w, h, rb in b["passes"])
    assert a["inflated_bytes"] != b["inflated_bytes"]


@pytest.mark.parametrize("name", sorted(cases.GOOD)[::3] + [cases.TRNS, cases.SPLIT])
def test_png_info_full_equals_the_parse(name):
    f = cases.GOOD[name]["file"]
    want, got = png_full_ref.parse(f), data.png_info(f, full=True)
    for k in ("width", "height", "bit_depth", "color_type", "interlace", "channels", "supported", "reason", "inflated_bytes"):
        assert got[k] == want[k], k
    assert got["passes"] == want["passes"] and len(got["passes"]) == 7
    assert got["idat_chunks"] == len(want["idat"]) and got["idat_bytes"] == sum(map(len, want["idat"]))
    old = data.png_info(f)                                 # the default still says unsupported, and why
    assert "passes" not in old and not old["supported"]
    assert old["reason"] == ("16-bit samples" if want["bit_depth"] == 16 else "Adam7 interlace")
    assert not png_load_ref.parse(f)["supported"]
