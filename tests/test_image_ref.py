"""CPU checks of the image.scale restatement (tests/image_ref.py) and of the loaders' size logic
(data.load_size, inference.whole_frame_sizes): the ground the device kernels of vf_image.hip are held to."""
import numpy as np
import pytest
import torch

import image_ref as R
import video_filler_amd  # noqa: F401
from video_filler_amd import data, inference


def test_same_size_is_a_copy():
    rng = np.random.default_rng(0)
    x = rng.uniform(0, 1, (3, 17, 23)).astype(np.float32)
    np.testing.assert_array_equal(R.scale(x, 23, 17), x)
    b = rng.integers(0, 256, (2, 9, 5), dtype=np.uint8)
    got = R.scale(b, 5, 9)
    assert got.dtype == np.uint8
    np.testing.assert_array_equal(got, b)


@pytest.mark.parametrize("H,W,h,w", [(36, 48, 35, 46), (10, 12, 31, 7), (5, 5, 1, 1), (1, 9, 4, 9)])
def test_constant_stays_constant(H, W, h, w):
    for v in (np.float32(0.25), np.float32(1.0), np.float32(0.0)):
        out = R.scale(np.full((2, H, W), v, np.float32), w, h)
        assert out.shape == (2, h, w)
        np.testing.assert_array_equal(out, v)
    np.testing.assert_array_equal(R.scale(np.full((1, H, W), 200, np.uint8), w, h), 200)


def test_upscale_keeps_the_endpoints():
    rng = np.random.default_rng(1)
    s = rng.uniform(0, 1, (4, 7)).astype(np.float32)
    d = R.rowcol(s, 19)
    np.testing.assert_array_equal(d[:, 0], s[:, 0])
    np.testing.assert_array_equal(d[:, -1], s[:, -1])
    # 7 -> 19: scale = 6/18 = 1/3, so every third destination sample lands on a source sample
    np.testing.assert_array_equal(d[:, ::3], s)


def test_integer_downscale_is_the_block_mean():
    rng = np.random.default_rng(2)
    # dyadic values: every partial sum and the division by 2 or 4 are exact in float32
    x = (rng.integers(0, 64, (3, 8, 12)) / np.float32(64)).astype(np.float32)
    got = R.scale(x, 6, 4)
    want = x.reshape(3, 4, 2, 6, 2).mean(axis=(2, 4), dtype=np.float64).astype(np.float32)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(R.rowcol(np.arange(8, dtype=np.float32), 1), [np.float32(3.5)])


def test_one_pixel_source_upscale():
    d = R.rowcol(np.array([[0.7]], np.float32), 5)
    np.testing.assert_array_equal(d, np.full((1, 5), np.float32(0.7)))
    np.testing.assert_array_equal(R.scale(np.array([[[9]]], np.uint8), 3, 4), np.full((1, 4, 3), 9, np.uint8))


def test_byte_rounding_and_clamping():
    np.testing.assert_array_equal(R.fi_byte([-3, -0.5, 0.49, 0.5, 254.4, 254.6, 300]), [0, 0, 0, 1, 254, 255, 255])
    # 4 -> 2: scale 2, blocks {10, 20} and {31, 40}: 15 -> 15.5 -> 15, 35.5 -> 36
    np.testing.assert_array_equal(R.rowcol(np.array([10, 20, 31, 40], np.float32), 2, byte=True), [15, 36])
    # 5 -> 2: scale 2.5: (0 + 10 + .5*20) / 2.5 = 8; (.5*20 + 30 + 41) / 2.5 = 32.4 -> 32
    np.testing.assert_array_equal(R.rowcol(np.array([0, 10, 20, 30, 41], np.float32), 2, byte=True), [8, 32])
    # 2 -> 5: scale .25: 0, 63.75 -> 64, 127.5 -> 128, 191.25 -> 191, 255
    np.testing.assert_array_equal(R.rowcol(np.array([0, 255], np.float32), 5, byte=True), [0, 64, 128, 191, 255])
    # the Float path keeps the fractions
    np.testing.assert_array_equal(R.rowcol(np.array([0, 255], np.float32), 5), np.float32([0, 63.75, 127.5, 191.25, 255]))


def test_byte_intermediate_is_rounded():
    """scaleBilinear's tmp has the source's type: on the Byte path the row pass is rounded before the column pass."""
    src = np.array([[[0, 255], [0, 0]]], np.uint8)                   # 1 x 2 x 2
    tmp = R.rowcol(src.astype(np.float32), 5, byte=True)             # row 0: 0 64 128 191 255
    want = R.rowcol(tmp.swapaxes(-1, -2), 3, byte=True).swapaxes(-1, -2)
    got = R.scale(src, 5, 3)
    np.testing.assert_array_equal(got, want.astype(np.uint8))
    np.testing.assert_array_equal(got[0, 1], [0, 32, 64, 96, 128])   # (64 / 2 = 32), (191 / 2 = 95.5 -> 96)


def test_decoded_byte_over_255_identity():
    """image.load(path, nc, 'float') divides in double and stores float; b / 255 in float32 is the same number."""
    b = np.arange(256, dtype=np.uint8)
    f32 = b.astype(np.float32) / np.float32(255)
    f64 = (b.astype(np.float64) / 255.0).astype(np.float32)
    np.testing.assert_array_equal(f32.view(np.uint32), f64.view(np.uint32))
    hwc = b[:255].reshape(5, 17, 3)
    np.testing.assert_array_equal(R.decoded_to_float(hwc)[:, 2, 4], f64[(2 * 17 + 4) * 3:(2 * 17 + 4) * 3 + 3])


def test_byte_mask_keeps_only_255():
    m = np.array([[0, 1, 128, 254, 255]], np.uint8)
    np.testing.assert_array_equal(R.byte_mask(m), [[0, 0, 0, 0, 1]])
    np.testing.assert_array_equal(data.byte_mask(torch.from_numpy(m)).numpy(), [[0, 0, 0, 0, 1]])


@pytest.mark.parametrize("loadSize,H,W,scalef,want", [
    (350, 360, 480, None, (350, 466)),       # landscape: 350 * 480 / 360 = 466.67 -> 466
    (350, 480, 360, None, (466, 350)),       # portrait
    (360, 360, 480, None, (360, 480)),
    (360, 683, 512, None, (480, 360)),       # 360 * 683 / 512 = 480.23
    (350, 512, 683, None, (350, 466)),       # 350 * 683 / 512 = 466.89
    (350, 300, 300, None, (350, 350)),
    (-1, 360, 480, 1.25, (600, 450)),        # image.scale(input, iH, iW): height = scalef * W, width = scalef * H
    (-1, 480, 360, 0.7, (251, 336)),        # 0.7 * 360 = 251.99999999999997 in double -> 251
    (-2, 360, 480, 2.1, (1008, 756)),        # 2.1 * 480 = 1008.0000000000001, 2.1 * 360 = 756.0000000000001
    (-2, 97, 131, 1.5, (196, 145)),          # 196.5 -> 196, 145.5 -> 145: truncated
    (0, 97, 131, None, (97, 131)),
])
def test_load_size(loadSize, H, W, scalef, want):
    assert data.load_size(H, W, loadSize, scalef) == want


def test_draw_scalef_ranges():
    rng = np.random.default_rng(4)
    a = [data.draw_scalef(-1, rng) for _ in range(200)]
    b = [data.draw_scalef(-2, rng) for _ in range(200)]
    assert 0.5 <= min(a) and max(a) < 1.5 and 1 <= min(b) and max(b) < 3
    assert max(a) - min(a) > 0.8 and max(b) - min(b) > 1.6


@pytest.mark.parametrize("loadSize,fs,want", [(360, 128, (360, 480, 384, 512)), (350, 128, (350, 466, 384, 512)),
                                              (96, 64, (96, 128, 128, 128)), (100, 64, (100, 133, 128, 192))])
def test_whole_frame_sizes(loadSize, fs, want):
    assert inference.whole_frame_sizes(loadSize, fs) == want
    assert R.whole_sizes(loadSize, fs) == want


def test_restated_callers_shapes_and_ranges():
    rng = np.random.default_rng(5)
    img = rng.uniform(0, 1, (3, 40, 52)).astype(np.float32)
    out = R.hook2d(img, 35, 46, 32, 7, 2, True)
    assert out.shape == (3, 32, 32) and out.min() >= -1 and out.max() <= 1
    np.testing.assert_array_equal(out[:, :, ::-1], R.hook2d(img, 35, 46, 32, 7, 2, False))
    frames = rng.uniform(0, 1, (2, 3, 40, 52)).astype(np.float32)
    mask = np.zeros((1, 40, 52), np.uint8)
    mask[:, 10:20, 15:30] = 1
    full, pm = R.whole_frames(frames, mask, 30, 32, 110 / 255)
    assert full.shape == (6, 32, 64) and pm.shape == (3, 32, 64)
    assert (full[:, 30:, :] == -1).all() and (full[:, :, 40:] == -1).all() and (pm[:, 30:, :] == 0).all()
    fill = np.float32(110 / 255) * np.float32(2) + np.float32(-1)
    assert (full.reshape(2, 3, 32, 64)[:, pm.astype(bool)] == fill).all() and pm.sum() > 0
