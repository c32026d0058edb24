"""tests/apng_decode_ref.py, the definition of vf_apng_decode, against Pillow on every good fixture Pillow reads, against
hand-computed canvases where Pillow deviates, and on the malformed, unsupported and corrupt fixtures."""
import io

import numpy as np
import pytest
from PIL import Image

import apng_cases
import apng_decode_ref as ref
from png_load_ref import PngError

FX = apng_cases.fixtures()
# Pillow restores the DEFAULT IMAGE, not the empty canvas, when the first frame's disposal is PREVIOUS and the default image is
# not part of the animation; the rule here (and the specification) treats PREVIOUS on the first frame as BACKGROUND.  These
# fixtures have hand-computed expectations below.
PILLOW_RESTORES_DEFAULT_IMAGE = {"pillow_RGB_d2_default", "pillow_RGBA_d2_default", "previous_first_excluded_default"}
# Not read by Pillow 12: it raises on interlaced frames of an animation ("function takes at most 3 arguments") and does not
# identify a PNG with an fcTL but no acTL.  The Adam7 fixtures are compared with their non-interlaced twins instead.
PILLOW_DOES_NOT_READ = {"adam7_rgb", "adam7_palette2", "rgba16_adam7", "plain_png_stray_fctl"}
# Pillow clears a palette file to INDEX 0, not to black: with a colour at entry 0 its RGB differs from the rule's transparent black.
# Every other palette fixture has black there; this one has a hand-computed expectation below.
PILLOW_CLEARS_TO_INDEX_0 = {"palette_dispose1_colour0"}
# 16-bit grey (Pillow's I;16 does not convert to RGBA as bytes) is compared through its own array instead
PILLOW_MODE_I16 = {"grey16"}


def pillow_frames(data):
    """(N x H x W x 4 as Pillow composites them, default image excluded; whether the file carries alpha)"""
    im = Image.open(io.BytesIO(data))
    n = getattr(im, "n_frames", 1)
    skip = 1 if n > 1 and im.info.get("default_image") else 0
    out = []
    for k in range(skip, n):
        im.seek(k)
        out.append(np.asarray(im.convert("RGBA")))
    return np.stack(out)


@pytest.mark.parametrize("name", sorted(FX["good"]))
def test_reference_equals_pillow(name):
    f = FX["good"][name]
    d = ref.parse(f)
    got = ref.decode(f, alpha=True)
    assert got.shape == (d["frames"], d["height"], d["width"], 4)
    assert np.array_equal(ref.decode(f), got[..., :3])
    if name in PILLOW_RESTORES_DEFAULT_IMAGE or name in PILLOW_CLEARS_TO_INDEX_0:
        return
    if name in PILLOW_DOES_NOT_READ:
        with pytest.raises((TypeError, OSError)):
            pillow_frames(f)
        return
    if name in PILLOW_MODE_I16:
        im = Image.open(io.BytesIO(f))
        for k in range(d["frames"]):
            im.seek(k)
            # frames of this fixture are dispose 0 over a full first frame: the canvas is grey everywhere
            assert np.array_equal((np.asarray(im).astype(np.uint32) >> 8).astype(np.uint8), got[k, ..., 0]), k
        return
    want = pillow_frames(f)
    assert want.shape == got.shape, (want.shape, got.shape)
    has_alpha = d["color_type"] in (4, 6) or d["trns"] is not None
    if has_alpha:
        assert np.array_equal(got, want), "first differing frame %d" % next(k for k in range(len(got)) if not np.array_equal(got[k], want[k]))
    else:
        # files without alpha: Pillow clears to OPAQUE black where the rule clears to transparent black; the RGB agrees
        assert np.array_equal(got[..., :3], want[..., :3])
        painted = got[..., 3] == 255
        assert np.array_equal(got[..., 3][painted], want[..., 3][painted]) and not got[..., :3][~painted].any()


def test_previous_on_the_first_frame_is_background():
    """hand-computed: frame 0 (6 x 7 at (3,4), PREVIOUS) leaves an empty canvas behind, whatever the default image holds"""
    f = FX["good"]["previous_first_excluded_default"]
    d = ref.parse(f)
    assert not d["default_is_frame"] and d["frames"] == 2 and d["frame_info"][0]["dispose"] == 2
    got = ref.decode(f, alpha=True)
    p0 = ref.rgba(ref.png_full_ref.load(ref.frame_png(d, 0)))
    p1 = ref.rgba(ref.png_full_ref.load(ref.frame_png(d, 1)))
    want0 = np.zeros((14, 19, 4), np.uint8)
    want0[4:10, 3:10] = p0
    want1 = np.zeros((14, 19, 4), np.uint8)
    want1[1:5, 1:5] = p1
    assert np.array_equal(got[0], want0) and np.array_equal(got[1], want1)
    for name in sorted(PILLOW_RESTORES_DEFAULT_IMAGE - {"previous_first_excluded_default"}):
        g = ref.decode(FX["good"][name], alpha=True)
        fi = ref.parse(FX["good"][name])["frame_info"]
        x, y, w, h = (fi[0][k] for k in "xywh")
        fr1 = fi[1]
        # behind frame 0 the canvas is empty: outside frame 1's rectangle, output frame 1 is transparent black
        mask = np.ones(g.shape[1:3], bool)
        mask[fr1["y"]:fr1["y"] + fr1["h"], fr1["x"]:fr1["x"] + fr1["w"]] = False
        assert not g[1][mask].any(), name


def test_hand_computed_background_then_smaller():
    f = FX["good"]["background_then_smaller"]
    d = ref.parse(f)
    px = [ref.rgba(ref.png_full_ref.load(ref.frame_png(d, k))) for k in range(5)]
    got = ref.decode(f, alpha=True)
    c = px[0].copy()
    assert np.array_equal(got[0], c)
    c1 = c.copy()
    c1[3:11, 4:13] = px[1]
    assert np.array_equal(got[1], c1)
    c[3:11, 4:13] = 0                                       # BACKGROUND: transparent black, then the smaller frame inside it
    c2 = c.copy()
    c2[5:8, 6:9] = px[2]
    assert np.array_equal(got[2], c2) and got[2][3, 4, 3] == 0 and got[2][5, 6, 3] == 255
    c3 = c2.copy()
    c3[0:2, 0:5] = px[3]
    assert np.array_equal(got[3], c3)
    c3[0:2, 0:5] = 0
    c3[13, 18] = px[4][0, 0]
    assert np.array_equal(got[4], c3)


def test_adam7_frames_equal_their_plain_twins():
    W, H = 19, 14
    for name, ct, depth, kw in (("adam7_rgb", 2, 8, {}), ("adam7_palette2", 3, 2, dict(plte=apng_cases.pfc.palette(2))),
                                ("rgba16_adam7", 6, 16, {})):
        d = ref.parse(FX["good"][name])
        assert d["interlace"] == 1
        frames = []
        for k, f in enumerate(d["frame_info"]):
            px = ref.png_full_ref.samples(ref.frame_png(d, k))[0] if ct != 3 else None
            if ct == 3:                                      # the indices, not the colours
                one = dict(d, plte=None, trns=None, color_type=0)
                px = ref.png_full_ref.load(ref.frame_png(one, k)) // (255 // ((1 << depth) - 1))
            frames.append(apng_cases.frame(px, x=f["x"], y=f["y"], dispose=f["dispose"]))
        twin = apng_cases.build(W, H, ct, depth, frames, lace=False, **kw)
        assert ref.parse(twin)["interlace"] == 0
        assert np.array_equal(ref.decode(twin, alpha=True), ref.decode(FX["good"][name], alpha=True)), name
    assert np.array_equal(ref.decode(FX["good"]["plain_png_stray_fctl"]), ref.decode(FX["good"]["plain_png"]))


def test_background_clears_a_palette_file_to_transparent_black_not_to_entry_0():
    f = FX["good"]["palette_dispose1_colour0"]
    d = ref.parse(f)
    assert d["plte"][:3] != b"\0\0\0" and d["frame_info"][1]["dispose"] == 1
    got = ref.decode(f, alpha=True)
    assert not got[2][3:9, 2:7][np.ix_(range(6), range(3, 5))].any()         # inside frame 1's rectangle, outside frame 2's 3 x 3
    assert (got[2][9:, :, 3] == 255).all()


def test_metadata():
    d = ref.parse(FX["good"]["delay_den_0"])
    assert [(f["delay_num"], f["delay_den"]) for f in d["frame_info"]] == [(7, 0), (0, 0), (65535, 65535)]
    d = ref.parse(FX["good"]["pillow_RGB_d1_default"])
    assert d["animated"] and not d["default_is_frame"] and d["frames"] == 3 and d["num_plays"] == 2
    assert [f["delay_num"] * 1000 // f["delay_den"] for f in d["frame_info"]] == [30, 40, 50]
    crops = ref.parse(FX["good"]["pillow_RGB_d0_frame0"])["frame_info"]
    assert any((f["w"], f["h"]) != (17, 13) for f in crops), "Pillow's writer crops sub-rectangles"
    d = ref.parse(FX["good"]["plain_png_stray_fctl"])
    assert not d["animated"] and d["frames"] == 1 and d["num_plays"] == -1 and d["default_is_frame"]
    d = ref.parse(FX["good"]["many_fdats"])
    assert d["frames"] == 3 and d["supported"]
    import apng_ref
    f = apng_ref.assemble([apng_cases.pfc.write_png(apng_cases.pix(5, 6, 2, 8, s), 2, 8, split=(3, 4)) for s in range(3)], 7, 9)
    d = ref.parse(f)                                        # the encoder's rule passes the decoder's walk
    assert d["frames"] == 3 and d["num_plays"] == 9 and all((x["delay_num"], x["delay_den"]) == (7, 100) for x in d["frame_info"])


@pytest.mark.parametrize("name", sorted(FX["malformed"]))
def test_malformed_files_raise(name):
    f, word = FX["malformed"][name]
    with pytest.raises(ref.ApngError) as e:
        ref.parse(f)
    assert word in str(e.value)


@pytest.mark.parametrize("name", sorted(FX["unsupported"]))
def test_unsupported_files_say_why(name):
    f, word = FX["unsupported"][name]
    d = ref.parse(f)
    assert not d["supported"] and word in d["reason"]
    with pytest.raises(ref.ApngUnsupported):
        ref.decode(f)


@pytest.mark.parametrize("name", sorted(FX["corrupt"]))
def test_corrupt_streams_raise(name):
    f, status = FX["corrupt"][name]
    assert ref.parse(f)["supported"]
    words = {v: k for k, v in apng_cases.pfc.STATUS.items()}
    with pytest.raises(PngError) as e:
        ref.decode(f)
    assert words[status] in str(e.value) or (status == 6 and "incorrect data check" in str(e.value))
