"""Baseline JPEG decode on the device (vf_jpeg.hip) against libjpeg's default decompression (Pillow's
decode, stored with the files in tests/golden/jpeg_cases.npz), byte for byte; the loaders fed with it."""
import io
import os

import numpy as np
import pytest
import torch

import video_filler_amd  # noqa: F401
from video_filler_amd import data
from video_filler_amd.backend import get_backend
from video_filler_amd.inference import load_whole_frames

try:
    from PIL import Image
except ImportError:   # pragma: no cover
    Image = None

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz"))
NAMES = sorted(k[4:] for k in GOLDEN.files if k.startswith("jpg/"))


def _file(name):
    return GOLDEN["jpg/" + name].tobytes()


def _ref(name, channels=3):
    r = GOLDEN["ref/" + name]
    return np.repeat(r, channels, -1) if r.shape[2] == 1 else r


@pytest.mark.parametrize("name", NAMES)
def test_fixture_one_by_one(name):
    (got,) = data.decode_jpeg([_file(name)])
    assert got.is_cuda and got.dtype == torch.uint8
    np.testing.assert_array_equal(got.cpu().numpy(), _ref(name))


def test_fixtures_as_one_mixed_batch():
    got = data.decode_jpeg([_file(n) for n in NAMES])
    for n, g in zip(NAMES, got):
        np.testing.assert_array_equal(g.cpu().numpy(), _ref(n), err_msg=n)
    assert len({g.untyped_storage().data_ptr() for g in got}) == 1   # views into one buffer


def test_subsequence_sizes_and_repeats_agree():
    files = [_file(n) for n in NAMES]
    B = get_backend()
    outs = []
    for sub in (16, 1024, 16):
        buf, offs, status, rounds = B.jpeg_decode(files, 3, sub)
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0] * len(files)
        assert rounds.item() >= 1
        outs.append(buf.cpu().numpy())
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(outs[0], outs[2])


def test_gray_channels():
    gray = [n for n in NAMES if n.startswith("L_")]
    for n, g in zip(gray, data.decode_jpeg([_file(n) for n in gray], channels=1)):
        np.testing.assert_array_equal(g.cpu().numpy(), GOLDEN["ref/" + n])
    for n, g in zip(gray, data.decode_jpeg([_file(n) for n in gray], channels=3)):
        assert g.shape[2] == 3
        np.testing.assert_array_equal(g.cpu().numpy(), _ref(n))
    with pytest.raises(ValueError, match="item 0"):
        data.decode_jpeg([_file([n for n in NAMES if n.startswith("420")][0])], channels=1)


def test_stack_and_item_kinds(tmp_path):
    n = [x for x in NAMES if "360x480" in x][0]
    p = tmp_path / "a.jpg"
    p.write_bytes(_file(n))
    st = data.decode_jpeg([_file(n), GOLDEN["jpg/" + n], str(p)], stack=True)
    assert tuple(st.shape) == (3, 360, 480, 3)
    for i in range(3):
        np.testing.assert_array_equal(st[i].cpu().numpy(), _ref(n))
    with pytest.raises(AssertionError):
        data.decode_jpeg([_file(NAMES[0]), _file(n)], stack=True)


def test_fallback_for_unsupported():
    prog = GOLDEN["bad/progressive"].tobytes()
    with pytest.raises(ValueError, match="item 1 .*progressive"):
        data.decode_jpeg([_file(NAMES[0]), prog])
    seen = []

    def fb(buf):
        seen.append(buf)
        return np.full((24, 40, 3), 7, np.uint8)

    got = data.decode_jpeg([_file(NAMES[0]), prog], fallback=fb)
    assert seen == [prog]
    assert got[1].is_cuda and int(got[1].float().mean()) == 7
    np.testing.assert_array_equal(got[0].cpu().numpy(), _ref(NAMES[0]))


def test_corrupt_data_raises_after_sync():
    n = [x for x in NAMES if x.startswith("420_360x480")][0]
    buf = bytearray(_file(n))
    info = data.jpeg_info(bytes(buf))
    cut = bytes(buf[:info["scan_begin"] + 2000]) + b"\xff\xd9"   # most of the scan missing
    with pytest.raises(ValueError, match="item 0.*short data"):
        data.decode_jpeg([cut])


def _truncated():
    n = [x for x in NAMES if x.startswith("420_360x480")][0]
    buf = _file(n)
    return buf[:data.jpeg_info(buf)["scan_begin"] + 2000] + b"\xff\xd9"   # the file of test_corrupt_data_raises_after_sync


def test_default_entry_is_the_layouts_entry_on_baseline_files():
    # one scan of a baseline file is one sequential first scan of the shared pipeline: same bytes, statuses and rounds
    files = [_file(n) for n in NAMES]
    B = get_backend()
    for sub in (16, 1024):
        buf, offs, status, rounds = B.jpeg_decode(files, 3, sub)
        lbuf, loffs, lstatus, lrounds, levels = B.jpeg_decode_layouts(files, 3, sub)
        torch.cuda.synchronize()
        assert levels == 1 and list(offs) == list(loffs)
        assert torch.equal(buf, lbuf)
        assert status.cpu().tolist() == lstatus.cpu().tolist() == [0] * len(files)
        assert rounds.item() == lrounds.item() >= 1
    cut = [_truncated()]
    (_, _, status, _), (_, _, lstatus, _, _) = B.jpeg_decode(cut, 3, 256), B.jpeg_decode_layouts(cut, 3, 256)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == lstatus.cpu().tolist() and status.item() != 0
    # a run of zero bytes decodes as short blocks, so a restart segment's last block ends more than a 16-byte subsequence
    # before its data does: the bits behind it are skipped, as libjpeg skips them (the lane this entry once had read on)
    early = bytearray(_file("420_17x33_noise_q50_b4"))
    early[651:672] = bytes(21)
    for sub in (16, 256):
        (_, _, status, _), (_, _, lstatus, _, _) = B.jpeg_decode([bytes(early)], 3, sub), B.jpeg_decode_layouts([bytes(early)], 3, sub)
        torch.cuda.synchronize()
        assert status.cpu().tolist() == lstatus.cpu().tolist() == [0]


def test_malformed_files_raise_naming_the_item():
    good = _file(NAMES[0])
    b = bytearray(_file("420_360x480_noise_q90_none"))
    i = 0
    while True:   # every symbol of the first AC table at code length 1 (JERR_BAD_HUFF_TABLE in libjpeg)
        i = b.index(b"\xff\xc4", i)
        if b[i + 4] >> 4 == 1:
            break
        i += 2
    b[i + 5] = sum(b[i + 5:i + 21])
    b[i + 6:i + 21] = bytes(15)
    with pytest.raises(ValueError, match="item 1: .*bad Huffman table"):
        data.decode_jpeg([good, bytes(b)])
    # a restart marker out of sequence is found while the scan data is walked, inside the decode call
    r = bytearray(_file("422_360x480_smooth_q50_r1"))
    k = r.index(b"\xff\xd0", data.jpeg_info(bytes(r))["scan_begin"])
    r[k + 1] = 0xD3
    with pytest.raises(ValueError, match="item 2: .*restart marker out of sequence"):
        data.decode_jpeg([good, good, bytes(r)])
    (ok,) = data.decode_jpeg([good])
    np.testing.assert_array_equal(ok.cpu().numpy(), _ref(NAMES[0]))


@pytest.mark.skipif(Image is None, reason="Pillow writes the round-trip files")
def test_pillow_round_trip_matrix():
    rng = np.random.default_rng(7)
    files, refs = [], []
    for i in range(48):
        h, w = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.clip(np.stack([128 + 90 * np.sin(xx / rng.uniform(3, 40)), 128 + 90 * np.cos(yy / rng.uniform(3, 40)),
                              rng.integers(0, 256, (h, w))], -1) + rng.normal(0, rng.uniform(0, 40), (h, w, 3)), 0, 255)
        a = a.astype(np.uint8)
        kw = dict(quality=int(rng.integers(1, 101)), optimize=bool(rng.integers(0, 2)))
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
    for sub in (16, 1024):
        for f, r, g in zip(files, refs, data.decode_jpeg(files, subseq_bytes=sub)):
            np.testing.assert_array_equal(g.cpu().numpy(), r)


def _frames():
    n = [x for x in NAMES if x.startswith("420_360x480")][0]
    return n, data.decode_jpeg([_file(n)] * 4, stack=True), torch.from_numpy(np.stack([_ref(n)] * 4))


def test_image_batcher_fed_by_decode():
    n, dec, ref = _frames()
    outs = []
    for src in (dec, ref):
        ib = data.ImageBatcher(4, 3, 64, 100, rng=np.random.default_rng(3))
        for i in range(4):
            ib.add(src[i])
        outs.append(ib.batch().clone().cpu())
    assert torch.equal(outs[0], outs[1])


def test_clip_batcher_and_whole_frames_fed_by_decode():
    n, dec, ref = _frames()
    outs = []
    for src in (dec, ref):
        cb = data.ClipBatcher(1, 12, 64, rng=np.random.default_rng(5))
        m = np.zeros((360, 480), np.uint8)
        m[100:200, 100:300] = 1
        cb.set_mask(torch.from_numpy(m))
        while not cb.add_frames(src, 100):
            pass
        outs.append([t.clone().cpu() for t in cb.batch()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    m = np.zeros((360, 480), np.uint8)
    m[120:240, 160:320] = 1
    w = [load_whole_frames(src, torch.from_numpy(m), loadSize=200) for src in (dec, ref)]
    for a, b in zip(w[0], w[1]):
        assert torch.equal(a.cpu(), b.cpu())
