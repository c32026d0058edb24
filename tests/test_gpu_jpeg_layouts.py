"""decode_jpeg(layouts=True) on the device (vf_jpeg.hip, DESIGN.md 5.2: other samplings, RGB, sequential files of several
scans) against libjpeg's decompression (Pillow's decode, stored with the files in tests/golden/jpeg_layouts_cases.npz),
byte for byte; mixed with the baseline and progressive fixtures in one buffer.  Deliberately corrupt entropy-coded data
is the host entry's matter (tests/test_jpeg_layouts_cabi.py), not the device's."""
import os

import numpy as np
import pytest
import torch

import video_filler_amd  # noqa: F401
from video_filler_amd import data
from video_filler_amd.backend import get_backend

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "jpeg_layouts_cases.npz"))
BASE = np.load(os.path.join(HERE, "golden", "jpeg_cases.npz"))
PROG = np.load(os.path.join(HERE, "golden", "jpeg_progressive_cases.npz"))
NAMES = sorted(k[4:] for k in GOLDEN.files if k.startswith("jpg/"))
GREY = [n for n in NAMES if n.startswith("L22_")]


def _names(z):
    return sorted(k[4:] for k in z.files if k.startswith("jpg/"))


def _file(name, z=GOLDEN):
    return z["jpg/" + name].tobytes()


def _one(prefix):
    """the fixture whose name starts so (content and quality rotate through the names)"""
    (name,) = [n for n in NAMES if n.startswith(prefix)]
    return name


def _ref(name, channels=3, z=GOLDEN):
    r = z["ref/" + name]
    return np.repeat(r, channels, -1) if r.shape[2] == 1 else r


@pytest.mark.parametrize("name", NAMES)
def test_fixture_one_by_one(name):
    (got,) = data.decode_jpeg([_file(name)], layouts=True)
    assert got.is_cuda and got.dtype == torch.uint8
    np.testing.assert_array_equal(got.cpu().numpy(), _ref(name))


def test_mixed_batch_with_baseline_and_progressive_files_is_one_buffer():
    lists = [[(_file(n, z), _ref(n, z=z), n) for n in _names(z)] for z in (GOLDEN, BASE, PROG)]
    items = [lst[i] for i in range(max(map(len, lists))) for lst in lists if i < len(lst)]   # interleaved
    got = data.decode_jpeg([f for f, _, _ in items], layouts=True)
    for (_, ref, name), g in zip(items, got):
        np.testing.assert_array_equal(g.cpu().numpy(), ref, err_msg=name)
    assert len({g.untyped_storage().data_ptr() for g in got}) == 1
    ptrs = [g.data_ptr() for g in got]
    assert ptrs == sorted(ptrs)                          # in item order, back to back
    assert all(b - a == g.numel() for a, b, g in zip(ptrs, ptrs[1:], got))


def test_subsequence_sizes_and_repeats_agree():
    files = [_file(n) for n in NAMES]
    want = np.concatenate([_ref(n).ravel() for n in NAMES])
    B = get_backend()
    for sub in (16, 1024, 16):
        buf, offs, status, rounds, levels = B.jpeg_decode_layouts(files, 3, sub)
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0] * len(files)
        assert rounds.item() >= 1
        assert levels == 3                               # the progressive fixtures' three; never a function of the file count
        np.testing.assert_array_equal(buf.cpu().numpy()[:want.size], want)
    seq = [f for f, n in zip(files, NAMES) if not n.startswith("prog_")]
    assert B.jpeg_decode_layouts(seq, 3, 256)[4] == 1    # sequential files alone: every scan in the one first launch
    assert B.jpeg_decode_layouts(seq[:3], 3, 256)[4] == 1


def test_grey_channels():
    assert len(GREY) >= 5
    for n, g in zip(GREY, data.decode_jpeg([_file(n) for n in GREY], channels=1, layouts=True)):
        np.testing.assert_array_equal(g.cpu().numpy(), GOLDEN["ref/" + n])
    for n, g in zip(GREY, data.decode_jpeg([_file(n) for n in GREY], channels=3, layouts=True)):
        np.testing.assert_array_equal(g.cpu().numpy(), _ref(n))
    with pytest.raises(ValueError, match="item 1 .*YCbCr file with channels=1"):
        data.decode_jpeg([_file(GREY[0]), _file(_one("440_16x16"))], channels=1, layouts=True)
    with pytest.raises(ValueError, match="item 0 .*RGB file with channels=1"):
        data.decode_jpeg([_file("rgb_adobe0_sub0_24x40")], channels=1, layouts=True)


@pytest.mark.parametrize("name,why", [("440_16x16", r"sampling 1x2,1x1,1x1 \(4:4:4, 4:2:2 and 4:2:0 only\)"),
                                      ("rgb_adobe0_sub0_24x40", r"RGB colour transform \(Adobe transform 0\)"),
                                      ("rgb_ids_sub0_24x40", "RGB components"),
                                      ("scans_y_cbcr_444_37x53_dri0", "multi-scan sequential"),
                                      ("sof1_slots23_420_37x53", "one beyond baseline's two"),
                                      ("prog_440_16x16", "progressive")])
def test_without_layouts_the_files_raise_as_before(name, why):
    name = _one(name)
    with pytest.raises(ValueError, match="item 0 is not supported by the device decoder: .*" + why):
        data.decode_jpeg([_file(name)])
    if not name.startswith("prog_"):
        with pytest.raises(ValueError, match="item 0 is not supported by the device decoder: .*" + why):
            data.decode_jpeg([_file(name)], progressive=True)


def test_refused_files_reach_the_fallback_or_raise():
    good = _file(_one("411_17x33"))
    for key, why in (("fractional", "fractional ratio"), ("blocks18", "18 blocks"), ("missing", "is in no scan"), ("cmyk", "4 components")):
        bad = GOLDEN["bad/" + key].tobytes()
        with pytest.raises(ValueError, match="item 1 .*" + why):
            data.decode_jpeg([good, bad], layouts=True)
        seen = []

        def fb(buf):
            seen.append(buf)
            return np.full((24, 40, 3), 7, np.uint8)

        got = data.decode_jpeg([good, bad], fallback=fb, layouts=True)
        assert seen == [bad] and got[1].is_cuda and int(got[1].float().mean()) == 7
    with pytest.raises(ValueError, match="item 2: .*scan 2: component 1 is coded in two scans"):
        data.decode_jpeg([good, good, GOLDEN["bad/twice"].tobytes()], fallback=lambda b: None, layouts=True)


def test_stack_is_a_view_of_the_buffer():
    big = [n for n in NAMES if "360x480" in n]
    assert len(big) == 2
    st = data.decode_jpeg([_file(big[0]), _file(big[1]), _file(big[0])], stack=True, layouts=True)
    assert tuple(st.shape) == (3, 360, 480, 3)
    for i, n in enumerate((big[0], big[1], big[0])):
        np.testing.assert_array_equal(st[i].cpu().numpy(), _ref(n))
    assert st.data_ptr() == st.untyped_storage().data_ptr() and st.is_contiguous()


def test_decode_image_on_a_jpeg_png_mix():
    import png_load_ref
    png = np.load(os.path.join(HERE, "golden", "png_decode_cases.npz"))
    pngs = [png["good/pil/RGB_l0"].tobytes(), png["good/pil/L8_l0"].tobytes()]
    a, b, c = _one("22_21_11_17x33"), "scans_y_cb_cr_440_37x53", _names(BASE)[0]
    items = [pngs[0], _file(a), _file(c, BASE), pngs[1], _file(b)]
    refs = [png_load_ref.load(pngs[0], 3), _ref(a), _ref(c, z=BASE), png_load_ref.load(pngs[1], 3), _ref(b)]
    for g, r in zip(data.decode_image(items, layouts=True), refs):
        np.testing.assert_array_equal(g.cpu().numpy(), r)
    with pytest.raises(ValueError, match="decode_jpeg: item 1 .*sampling"):
        data.decode_image(items, progressive=True)
