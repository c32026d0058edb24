"""GPU tests of the full PNG rule (vf_png_decode_full, data.decode_png(full=True)): Adam7-interlaced and
16-bit files against tests/png_full_ref.py, byte for byte and bit for bit, on the fixtures of tests/png_full_cases.py; the
corrupt fixtures' status words; files of the default route in the same batch."""
import os

import numpy as np
import pytest
import torch

import png_full_cases as cases
import png_full_ref
import png_load_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "png_decode_cases.npz"))
OLD = ["mask/mask", "pil/RGBA_l9", "pil/P4_trns_l6", "hand/filter_mixed", "pil/L8_l6"]
NAMES = sorted(cases.GOOD)
WORD = {v: k for k, v in cases.STATUS.items()}
_REF = {}


def _file(name):
    return GOLDEN["good/" + name].tobytes() if name in OLD else cases.GOOD[name]["file"]


def _ref(name, channels=None, kind="load"):
    """the rule's decode, computed once per (file, channels, uint8 or float); None where the rule has none"""
    key = (name, channels, kind)
    if key not in _REF:
        try:
            _REF[key] = getattr(png_full_ref, kind)(_file(name), channels)
        except png_load_ref.PngUnsupported:
            _REF[key] = None
    return _REF[key]


def _same(got, want):
    return tuple(got.shape) == want.shape and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)


def _same_bits(got, want):
    return tuple(got.shape) == want.shape and got.dtype == torch.float32 and \
        np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("channels", [None, 1, 3])
def test_every_case_alone(hipb, channels):
    from video_filler_amd import data
    n = 0
    for name in NAMES:
        want = _ref(name, channels)
        if want is None:
            with pytest.raises(ValueError, match="item 0 is not supported .*channels=1"):
                data.decode_png([_file(name)], channels=channels, full=True)
            continue
        (got,) = data.decode_png([_file(name)], channels=channels, full=True)
        assert _same(got, want), name
        n += 1
    assert n == (len(NAMES) if channels != 1 else sum(cases.GOOD[m]["color_type"] in (0, 4) for m in NAMES))


@pytest.mark.parametrize("channels", [None, 1, 3])
def test_all_cases_in_one_batch_with_files_of_the_default_route(hipb, channels):
    from video_filler_amd import data
    names = [m for m in NAMES + OLD if _ref(m, channels) is not None]
    names = names[1::2] + names[0::2]                      # the old files among the new ones
    assert len(names) > 80 and (channels == 1 or set(OLD) <= set(names))
    got = data.decode_png([_file(m) for m in names], channels=channels, full=True)
    for m, g in zip(names, got):
        assert _same(g, _ref(m, channels)), m
    old = [m for m in OLD if m in names]
    for m, g in zip(old, data.decode_png([_file(m) for m in old], channels=channels)):
        assert _same(g, _ref(m, channels)) and np.array_equal(_ref(m, channels), png_load_ref.load(_file(m), channels)), m


def test_same_bytes_alone_twice_and_in_two_batches(hipb):
    from video_filler_amd import data
    pick = ["c6d16_lace_17x23", "mask/mask", "c3d2_lace_9x17", cases.BAND[0], "c0d16_plain_7x9", "pil/RGBA_l9", cases.BAND[6],
            cases.SPLIT, "c2d8_lace_4x5"]
    alone = [data.decode_png([_file(m)], full=True)[0].cpu().numpy() for m in pick]
    again = [data.decode_png([_file(m)], full=True)[0].cpu().numpy() for m in pick]
    b1 = [t.cpu().numpy() for t in data.decode_png([_file(m) for m in pick], full=True)]
    order = [3, 0, 5, 8, 5, 1, 4, 7, 2, 0, 6]
    b2 = [t.cpu().numpy() for t in data.decode_png([_file(pick[i]) for i in order], full=True)]
    for i, m in enumerate(pick):
        assert np.array_equal(alone[i], _ref(m)), m
        assert np.array_equal(alone[i], again[i]) and np.array_equal(alone[i], b1[i]), m
    for j, i in enumerate(order):
        assert np.array_equal(b2[j], alone[i]), pick[i]


@pytest.mark.parametrize("name", sorted(cases.BAD))
def test_corrupt_case_gives_its_status_and_names_the_item(hipb, name):
    from video_filler_amd import data
    bad, st = cases.BAD[name]
    around = ["c2d16_lace_17x23", "mask/mask", "c3d4_lace_9x17", cases.BAND[3]]
    files = [_file(around[0]), _file(around[1]), bad, _file(around[2]), _file(around[3])]
    for kind in (0, 1):
        status = hipb.png_decode_full(files, out_kind=kind)[2].cpu().tolist()
        print(name, "out_kind", kind, "status", status)
        assert status == [0, 0, st, 0, 0]
    with pytest.raises(ValueError, match=r"decode_png: item 2: .*\(%s\)" % WORD[st]):
        data.decode_png(files, full=True)
    for m, g in zip(around, data.decode_png([_file(m) for m in around], full=True)):
        assert _same(g, _ref(m)), m


def test_float_is_written_by_the_expansion_kernel_bit_for_bit(hipb):
    from video_filler_amd import data
    names = ["c2d8_lace_17x23", "c0d2_lace_9x17", "c6d16_lace_17x23", "c0d16_plain_17x23", "pil/RGBA_l9", "c4d16_lace_7x9",
             "c3d2_lace_9x17", cases.BAND[6], "mask/mask", "c2d16_plain_9x17"]
    for channels in (None, 3):
        got = data.decode_png([_file(m) for m in names], channels=channels, dtype="float", full=True)
        for m, g in zip(names, got):
            want = _ref(m, channels, "load_float")
            deep = m in cases.GOOD and cases.GOOD[m]["bit_depth"] == 16
            s = png_full_ref.samples(_file(m), channels)[0].astype(np.float32)
            assert np.array_equal(want, s / np.float32(65535 if deep else 255))
            assert _same_bits(g, want), m
            if deep:                                       # it is not highbyte / 255
                assert not np.array_equal(want, _ref(m, channels).astype(np.float32) / np.float32(255))
    # files of up to 8 bits: the bits of the default route's division
    for m in ("c2d8_lace_17x23", "pil/RGBA_l9"):
        (a,) = data.decode_png([_file(m)], dtype="float", full=True)
        b = hipb.png_bytes_to_float(data.decode_png([_file(m)], full=True)[0])
        assert torch.equal(a, b), m
    one = data.decode_png([_file("c6d16_lace_17x23")] * 2, dtype="float", full=True, stack=True)
    assert tuple(one.shape) == (2, 17, 23, 4) and _same_bits(one[1], _ref("c6d16_lace_17x23", None, "load_float"))


def test_decode_image_sorts_a_mixed_folder(hipb):
    from video_filler_amd import data
    jz = np.load(os.path.join(HERE, "golden", "jpeg_cases.npz"))
    jn = sorted(k[4:] for k in jz.files if k.startswith("jpg/") and "ref/" + k[4:] in jz.files)[0]
    items = ["c6d16_lace_9x17", jn, "c0d1_lace_17x23", "pil/RGBA_l9", "c4d16_plain_5x4"]
    files = [jz["jpg/" + m].tobytes() if m == jn else _file(m) for m in items]
    got = data.decode_image(files, full=True)
    for m, g in zip(items, got):
        want = _ref(m, 3) if m != jn else jz["ref/" + m]
        want = np.repeat(want[..., None], 3, 2) if want.ndim == 2 else want
        assert _same(g, want if want.shape[2] == 3 else np.repeat(want, 3, 2)), m
    with pytest.raises(ValueError, match="decode_png: item 0 is not supported by the device decoder: 16-bit samples"):
        data.decode_image(files)


def test_load_mask_of_an_interlaced_1_bit_mask(hipb):
    from video_filler_amd import data
    pix = (np.random.default_rng(8).integers(0, 5, (37, 53, 1)) > 0).astype(np.uint8)
    plain, laced = cases.write_png(pix, 0, 1, False, seed=1), cases.write_png(pix, 0, 1, True, seed=2)
    a, b, c = data.load_mask(plain), data.load_mask(laced, full=True), data.load_mask(plain, full=True)
    assert a.dtype == torch.uint8 and tuple(a.shape) == (37, 53) and torch.equal(a, b) and torch.equal(a, c)
    assert np.array_equal(a.cpu().numpy(), pix[..., 0])
    with pytest.raises(ValueError, match="Adam7 interlace"):
        data.load_mask(laced)


def test_fallback_takes_only_what_is_still_unsupported(hipb):
    from video_filler_amd import data
    keyed = GOLDEN["good/hand/grey_trns"].tobytes()
    seen = []

    def fb(b):
        seen.append(b)
        d = png_load_ref.parse(b)
        return np.full((d["height"], d["width"], 2), 7, np.uint8)
    names = ["c4d16_lace_9x17", "c4d8_lace_9x17"]
    got = data.decode_png([_file(names[0]), keyed, _file(names[1])], full=True, fallback=fb)
    assert seen == [keyed] and bool((got[1] == 7).all())
    assert _same(got[0], _ref(names[0])) and _same(got[2], _ref(names[1]))
    with pytest.raises(ValueError, match="item 1 is not supported by the device decoder: tRNS on colour type 0"):
        data.decode_png([_file(names[0]), keyed], full=True)
    fl = data.decode_png([_file(names[0]), keyed], full=True, fallback=fb, dtype="float")
    assert _same_bits(fl[0], _ref(names[0], None, "load_float")) and fl[1].dtype == torch.float32
    assert bool((fl[1].cpu().numpy() == np.float32(7) / np.float32(255)).all())
