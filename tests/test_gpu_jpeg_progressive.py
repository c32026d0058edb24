"""Progressive JPEG decode on the device (vf_jpeg.hip) against libjpeg's decompression (Pillow's decode,
stored with the files in tests/golden/jpeg_progressive_cases.npz), byte for byte; mixed with baseline files in one
buffer; the loaders fed with it.  Deliberately corrupt refinement data is the host entry's matter
(tests/test_jpeg_prog_cabi.py), not the device's."""
import io
import os

import numpy as np
import pytest
import torch

import video_filler_amd  # noqa: F401
from video_filler_amd import data
from video_filler_amd.backend import get_backend, jpeg_scans_inspect

try:
    from PIL import Image
except ImportError:   # pragma: no cover
    Image = None

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "jpeg_progressive_cases.npz"))
BASE = np.load(os.path.join(HERE, "golden", "jpeg_cases.npz"))
NAMES = sorted(k[4:] for k in GOLDEN.files if k.startswith("jpg/"))
BASE_NAMES = sorted(k[4:] for k in BASE.files if k.startswith("jpg/"))
BIG = "420_360x480_photo_q90_none"


def _file(name, z=GOLDEN):
    return z["jpg/" + name].tobytes()


def _ref(name, channels=3, z=GOLDEN):
    r = z["ref/" + name]
    return np.repeat(r, channels, -1) if r.shape[2] == 1 else r


@pytest.mark.parametrize("name", NAMES)
def test_fixture_one_by_one(name):
    (got,) = data.decode_jpeg([_file(name)], progressive=True)
    assert got.is_cuda and got.dtype == torch.uint8
    np.testing.assert_array_equal(got.cpu().numpy(), _ref(name))


def test_default_still_refuses_progressive():
    with pytest.raises(ValueError, match="item 0 .*progressive"):
        data.decode_jpeg([_file(NAMES[0])])


def test_mixed_batch_with_baseline_files_is_one_buffer():
    items = []
    for i in range(max(len(NAMES), len(BASE_NAMES))):   # interleaved, so both kinds land between each other
        if i < len(NAMES):
            items.append((_file(NAMES[i]), _ref(NAMES[i]), NAMES[i]))
        if i < len(BASE_NAMES):
            items.append((_file(BASE_NAMES[i], BASE), _ref(BASE_NAMES[i], z=BASE), BASE_NAMES[i]))
    got = data.decode_jpeg([f for f, _, _ in items], progressive=True)
    for (_, ref, name), g in zip(items, got):
        np.testing.assert_array_equal(g.cpu().numpy(), ref, err_msg=name)
    assert len({g.untyped_storage().data_ptr() for g in got}) == 1
    ptrs = [g.data_ptr() for g in got]
    assert ptrs == sorted(ptrs)                          # in item order, back to back
    assert all(b - a == g.numel() for a, b, g in zip(ptrs, ptrs[1:], got))


def test_subsequence_sizes_and_repeats_agree():
    files = [_file(n) for n in NAMES]
    B = get_backend()
    outs = []
    for sub in (16, 1024, 16):
        buf, offs, status, rounds, levels = B.jpeg_prog_decode(files, 3, sub)
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0] * len(files)
        assert rounds.item() >= 1
        assert levels == 3                               # libjpeg's script: never a function of the file count
        outs.append(buf.cpu().numpy())
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(outs[0], outs[2])


def test_gray_channels():
    gray = [n for n in NAMES if n.startswith("L_")]
    for n, g in zip(gray, data.decode_jpeg([_file(n) for n in gray], channels=1, progressive=True)):
        np.testing.assert_array_equal(g.cpu().numpy(), GOLDEN["ref/" + n])
    for n, g in zip(gray, data.decode_jpeg([_file(n) for n in gray], channels=3, progressive=True)):
        assert g.shape[2] == 3
        np.testing.assert_array_equal(g.cpu().numpy(), _ref(n))
    with pytest.raises(ValueError, match="item 0"):
        data.decode_jpeg([_file(BIG)], channels=1, progressive=True)


def test_stack_is_a_view_of_the_buffer():
    base = [n for n in BASE_NAMES if n.startswith("420_360x480")][0]
    st = data.decode_jpeg([_file(BIG), _file(base, BASE), GOLDEN["jpg/" + BIG]], stack=True, progressive=True)
    assert tuple(st.shape) == (3, 360, 480, 3)
    np.testing.assert_array_equal(st[0].cpu().numpy(), _ref(BIG))
    np.testing.assert_array_equal(st[1].cpu().numpy(), _ref(base, z=BASE))
    np.testing.assert_array_equal(st[2].cpu().numpy(), _ref(BIG))
    assert st.data_ptr() == st.untyped_storage().data_ptr() and st.is_contiguous()


def test_truncated_last_scan_raises_after_sync():
    f = _file(BIG)
    last = jpeg_scans_inspect(f)["scans"][-1]
    cut = f[:last["begin"] + (last["end"] - last["begin"]) // 3] + b"\xff\xd9"
    with pytest.raises(ValueError, match="item 1.*short data"):
        data.decode_jpeg([_file(NAMES[0]), cut], progressive=True)
    (ok,) = data.decode_jpeg([f], progressive=True)
    np.testing.assert_array_equal(ok.cpu().numpy(), _ref(BIG))


def test_refused_files_reach_the_fallback_or_raise():
    good = _file(NAMES[0])
    for key, why in (("incomplete", "incomplete progression"), ("disorder", "progression out of order"), ("cmyk", "4 components")):
        bad = GOLDEN["bad/" + key].tobytes()
        with pytest.raises(ValueError, match="item 1 .*" + why):
            data.decode_jpeg([good, bad], progressive=True)
        seen = []

        def fb(buf):
            seen.append(buf)
            return np.full((24, 40, 3), 7, np.uint8)

        got = data.decode_jpeg([good, bad, good], fallback=fb, progressive=True)
        assert seen == [bad]
        assert got[1].is_cuda and tuple(got[1].shape) == (24, 40, 3) and int(got[1].float().mean()) == 7
        np.testing.assert_array_equal(got[0].cpu().numpy(), _ref(NAMES[0]))
        np.testing.assert_array_equal(got[2].cpu().numpy(), _ref(NAMES[0]))
    with pytest.raises(ValueError, match="item 2: .*scan 5: bad progression parameters"):
        data.decode_jpeg([good, good, GOLDEN["bad/badsos"].tobytes()], fallback=lambda b: None, progressive=True)


@pytest.mark.skipif(Image is None, reason="Pillow writes the round-trip files")
def test_pillow_round_trip_matrix(monkeypatch):
    from PIL import ImageFile
    monkeypatch.setattr(ImageFile, "MAXBLOCK", 1 << 22)   # Pillow writes a progressive file through one buffer of this size
    rng = np.random.default_rng(11)
    files, refs = [], []
    for i in range(32):
        h, w = int(rng.integers(1, 301)), int(rng.integers(1, 301))
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.clip(np.stack([128 + 90 * np.sin(xx / rng.uniform(3, 40)), 128 + 90 * np.cos(yy / rng.uniform(3, 40)),
                              rng.integers(0, 256, (h, w))], -1) + rng.normal(0, rng.uniform(0, 40), (h, w, 3)), 0, 255)
        a = a.astype(np.uint8)
        kw = dict(quality=int(rng.integers(1, 101)), optimize=bool(rng.integers(0, 2)), progressive=True)
        r = int(rng.integers(0, 4))
        if r == 1:
            kw["restart_marker_blocks"] = int(rng.integers(1, 9))
        elif r == 2:
            kw["restart_marker_rows"] = int(rng.integers(1, 4))
        gray = i % 5 == 4
        im = Image.fromarray(a[..., 0]) if gray else Image.fromarray(a)
        if not gray:
            kw["subsampling"] = int(rng.integers(0, 3))
        bio = io.BytesIO()
        im.save(bio, "JPEG", **kw)
        files.append(bio.getvalue())
        refs.append(np.asarray(Image.open(io.BytesIO(files[-1])).convert("RGB")))
    for r, g in zip(refs, data.decode_jpeg(files, progressive=True)):
        np.testing.assert_array_equal(g.cpu().numpy(), r)


def test_image_batcher_fed_by_progressive_decode():
    dec = data.decode_jpeg([_file(BIG)] * 4, stack=True, progressive=True)
    ref = torch.from_numpy(np.stack([_ref(BIG)] * 4))
    outs = []
    for src in (dec, ref):
        ib = data.ImageBatcher(4, 3, 64, 100, rng=np.random.default_rng(3))
        for i in range(4):
            ib.add(src[i])
        outs.append(ib.batch().clone().cpu())
    assert torch.equal(outs[0], outs[1])


def test_decode_image_on_a_jpeg_png_mix():
    import png_load_ref
    png = np.load(os.path.join(HERE, "golden", "png_decode_cases.npz"))
    pngs = [png["good/pil/RGB_l0"].tobytes(), png["good/pil/L8_l0"].tobytes()]
    base = BASE_NAMES[0]
    items = [pngs[0], _file(BIG), _file(base, BASE), pngs[1], _file(NAMES[0])]
    refs = [png_load_ref.load(pngs[0], 3), _ref(BIG), _ref(base, z=BASE), png_load_ref.load(pngs[1], 3), _ref(NAMES[0])]
    for g, r in zip(data.decode_image(items, progressive=True), refs):
        np.testing.assert_array_equal(g.cpu().numpy(), r)
    with pytest.raises(ValueError, match="decode_jpeg: item 1 .*progressive"):
        data.decode_image(items)
