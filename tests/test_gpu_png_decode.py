"""The device PNG decoder (vf_png_decode.hip) against the restated image.load of tests/png_load_ref.py, byte
for byte, on the fixtures of tests/golden/png_decode_cases.npz; the corrupt fixtures' status words; the round trip through
the device encoder; and the loaders fed with a decoded mask."""
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import png_load_ref
import png_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "png_decode_cases.npz"))
GOOD = sorted(k[5:] for k in GOLDEN.files if k.startswith("good/"))
BAD = sorted(k[4:] for k in GOLDEN.files if k.startswith("bad/"))
MASKS = [n for n in GOOD if n.startswith("mask/")]
STATUS_WORD = {1: "bad code", 2: "short data", 3: "bad distance", 4: "bad length", 5: "bad filter", 6: "bad Adler-32",
               7: "bad palette index"}
_REF = {}


def _file(name):
    return GOLDEN["good/" + name].tobytes()


def _ref(name, channels=None):
    """the restatement's decode, computed once per (file, channels); None where the rule has none"""
    key = (name, channels)
    if key not in _REF:
        try:
            _REF[key] = png_load_ref.load(_file(name), channels)
        except png_load_ref.PngUnsupported:
            _REF[key] = None
    return _REF[key]


def _same(got, want):
    return tuple(got.shape) == want.shape and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)


def test_every_fixture_alone(hipb):
    from video_filler_amd import data
    keyed = []
    for name in GOOD:
        if _ref(name) is None:                            # tRNS on grey / RGB: no byte rule for the file's own channels
            keyed.append(name)
            with pytest.raises(ValueError, match="item 0 is not supported .*tRNS on colour type"):
                data.decode_png([_file(name)])
            (got,) = data.decode_png([_file(name)], channels=3)
            assert _same(got, _ref(name, 3)), name
            continue
        (got,) = data.decode_png([_file(name)])
        assert _same(got, _ref(name)), name
    assert sorted(keyed) == ["hand/grey_trns", "hand/rgb_trns"]
    (got,) = data.decode_png([_file("hand/grey_trns")], channels=1)
    assert _same(got, _ref("hand/grey_trns", 1))


@pytest.mark.parametrize("channels", [None, 1, 3])
def test_mixed_batch(hipb, channels):
    from video_filler_amd import data
    names = [n for n in GOOD if _ref(n, channels) is not None]
    assert len(names) > 30
    got = data.decode_png([_file(n) for n in names], channels=channels)
    for n, g in zip(names, got):
        assert _same(g, _ref(n, channels)), n
    if channels == 1:
        with pytest.raises(ValueError, match="item 1 is not supported .*channels=1"):
            data.decode_png([_file("pil/L8_l6"), _file("pil/RGB_l6")], channels=1)


def test_same_bytes_alone_twice_and_in_two_batches(hipb):
    from video_filler_amd import data
    pick = ["hand/filter_mixed", "mask/mask", "hand/run_dist1", "pil/P4_trns_l6", "hand/dist_32768", "pil/RGBA_l9"]
    alone = [data.decode_png([_file(n)])[0].cpu().numpy() for n in pick]
    again = [data.decode_png([_file(n)])[0].cpu().numpy() for n in pick]
    b1 = [t.cpu().numpy() for t in data.decode_png([_file(n) for n in pick])]
    order = [3, 0, 5, 5, 1, 4, 2, 0]
    b2 = [t.cpu().numpy() for t in data.decode_png([_file(pick[i]) for i in order])]
    for i, n in enumerate(pick):
        assert np.array_equal(alone[i], again[i]) and np.array_equal(alone[i], b1[i]), n
    for j, i in enumerate(order):
        assert np.array_equal(b2[j], alone[i]), pick[i]


@pytest.mark.parametrize("name", BAD)
def test_corrupt_fixture_raises_its_status_and_names_the_item(hipb, name):
    from video_filler_amd import data
    bad = GOLDEN["bad/" + name].tobytes()
    st = int(GOLDEN["status/" + name])
    around = ["hand/filter_mixed", "mask/maskpp", "pil/P2_l1"]
    files = [_file(around[0]), _file(around[1]), bad, _file(around[2])]
    status = hipb.png_decode(files)[2].cpu().tolist()
    print(name, "status", status)
    assert status == [0, 0, st, 0]
    with pytest.raises(ValueError, match=r"decode_png: item 2: .*\(%s\)" % STATUS_WORD[st]):
        data.decode_png(files)
    for n, g in zip(around, data.decode_png([_file(n) for n in around])):
        assert _same(g, _ref(n)), n


def test_round_trip_through_the_device_encoder(hipb):
    from video_filler_amd import data
    rng = np.random.default_rng(3)
    x = rng.uniform(-0.3, 1.3, (3, 3, 65, 47)).astype(np.float32)
    got = data.decode_png(data.encode_png(torch.from_numpy(x)), stack=True)
    assert np.array_equal(got.cpu().numpy(), png_ref.chw_to_hwc_bytes(x))
    yy, xx = np.mgrid[0:384, 0:512]
    frame = np.stack([(xx * 3 + yy) & 255, (xx ^ yy) & 255, rng.integers(0, 256, (384, 512))], -1).astype(np.uint8)
    (f,) = data.encode_png(frame[None])
    assert data.png_info(f)["idat_chunks"] > 50
    (got,) = data.decode_png([f])
    assert _same(got, frame)


def _unsupported_files():
    lace = bytearray(_file("pil/RGB_l6"))
    lace[28] = 1
    lace[29:33] = struct.pack(">I", zlib.crc32(bytes(lace[12:29])))
    deep = bytearray(_file("pil/L8_l6"))
    deep[24] = 16
    deep[29:33] = struct.pack(">I", zlib.crc32(bytes(deep[12:29])))
    return bytes(deep), bytes(lace)


def test_fallback_takes_what_the_device_does_not(hipb):
    from video_filler_amd import data
    deep, lace = _unsupported_files()
    seen = []

    def fb(b):
        seen.append(b)
        return np.full((17, 23, 3), len(seen), np.uint8)
    got = data.decode_png([deep, _file("pil/RGB_l6"), lace], channels=3, fallback=fb)
    assert seen == [deep, lace]
    assert bool((got[0] == 1).all()) and bool((got[2] == 2).all()) and _same(got[1], _ref("pil/RGB_l6", 3))
    with pytest.raises(ValueError, match="item 0 is not supported by the device decoder: 16-bit samples"):
        data.decode_png([deep])
    with pytest.raises(ValueError, match="item 1 is not supported by the device decoder: Adam7 interlace"):
        data.decode_png([_file("pil/RGB_l6"), lace])
    with pytest.raises(ValueError, match="decode_png: item 1: .*signature"):
        data.decode_png([_file("pil/RGB_l6"), b"\x89PNG\r\n\x1a\r" + bytes(40)])


def test_decode_image_sorts_a_mixed_folder(hipb):
    from video_filler_amd import data
    jz = np.load(os.path.join(HERE, "golden", "jpeg_cases.npz"))
    jn = sorted(k[4:] for k in jz.files if k.startswith("jpg/") and "ref/" + k[4:] in jz.files)[:3]
    pn = ["pil/RGB_l6", "mask/maskplus", "pil/P8_l9", "hand/filter_mixed_rgba"]
    items = [("p", pn[0]), ("j", jn[0]), ("j", jn[1]), ("p", pn[1]), ("p", pn[2]), ("j", jn[2]), ("p", pn[3])]
    files = [_file(n) if k == "p" else jz["jpg/" + n].tobytes() for k, n in items]
    got = data.decode_image(files)
    for (k, n), g in zip(items, got):
        want = _ref(n, 3) if k == "p" else jz["ref/" + n]
        want = np.repeat(want[..., None], 3, 2) if want.ndim == 2 else want
        assert _same(g, want if want.shape[2] == 3 else np.repeat(want, 3, 2)), n
    with pytest.raises(ValueError, match="item 1 is neither"):
        data.decode_image([files[0], b"GIF89a" + bytes(20)])


def test_load_mask_feeds_the_loaders(hipb):
    from video_filler_amd import data, inference
    for n in MASKS:
        m = data.load_mask(_file(n))
        ref = _ref(n)
        want = (ref == 255).astype(np.uint8)
        want = want[..., 0] if want.shape[2] == 1 else want
        assert m.dtype == torch.uint8 and m.is_cuda and np.array_equal(m.cpu().numpy(), want), n
    one = _ref("mask/mask")
    assert set(np.unique(one).tolist()) <= {0, 255} and data.load_mask(_file("mask/mask")).max().item() == 1
    # the loaders take it as they take the host-decoded mask
    name = "mask/maskpp"
    dev, host = data.load_mask(_file(name)), data.byte_mask(_ref(name)[..., 0])
    a, b = data.ClipBatcher.__new__(data.ClipBatcher), data.ClipBatcher.__new__(data.ClipBatcher)
    a.set_mask(dev)
    b.set_mask(host)
    assert torch.equal(a.mask_state, b.mask_state)
    rng = np.random.default_rng(2)
    frames = rng.integers(0, 256, (2, 90, 120, 3), dtype=np.uint8)
    fa, pa = inference.load_whole_frames(frames, dev, loadSize=96, fineSize=64)
    fb, pb = inference.load_whole_frames(frames, host, loadSize=96, fineSize=64)
    assert torch.equal(fa, fb) and torch.equal(pa, pb)


def test_float_is_an_ieee_division_by_255(hipb):
    from video_filler_amd import data
    for n in ("pil/RGB_l6", "mask/mask6p", "pil/LA_l1"):
        (g,) = data.decode_png([_file(n)], dtype="float")
        want = _ref(n).astype(np.float32) / np.float32(255)
        assert g.dtype == torch.float32 and np.array_equal(g.cpu().numpy().view(np.uint32), want.view(np.uint32)), n
