"""Scores of result frames on the device (vf_metrics.hip) against tests/metrics_ref.py: EXACT equality of
the whole int64 table, no tolerance — every column is an integer sum, and a window's SSIM is pinned to three IEEE double
operations on exact integers.  Shapes around the kernel's tile, both input forms, the valid rectangle, masks, the range
of the counters, the clip switch, argument errors, and the numbers-of-the-files claim of inference.evaluate_frames."""
import os
import re

import numpy as np
import pytest
import torch

import metrics_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 32                                      # the kernel's tile side (MT)
F = np.float32


def test_tile_side_is_the_kernels():
    src = open(os.path.join(ROOT, "video-filler_amd", "csrc", "vf_metrics.hip")).read()
    assert int(re.search(r"constexpr int MT = (\d+);", src).group(1)) == TILE


def dev(a, b, mask=None, valid=None, clip=True):
    from video_filler_amd import data
    as_t = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v))
    table, cols = data.frame_metrics(as_t(a), as_t(b), as_t(mask), valid, clip)
    assert cols == R.COLUMNS and table.dtype == torch.int64 and table.is_cuda
    return table.cpu().numpy()


def as_float(u8):
    """uint8 N x H x W x C -> a float32 N x C x H x W whose bytes under image.savePNG's rule are u8 (k/255 alone would
    truncate to k - 1 for some k: half a step is added)."""
    x = ((u8.astype(F) + F(0.5)) / F(255)).transpose(0, 3, 1, 2)
    assert (R.to_bytes(x) == u8).all()
    return np.ascontiguousarray(x)


def check(a, b, mask=None, valid=None, clip=True, floats=True):
    """device == restatement, for the uint8 form and (floats) the float form of the same bytes -> the table"""
    want = R.frame_table(a, b, mask, valid, clip)
    got = dev(a, b, mask, valid, clip)
    assert got.shape == want.shape and np.array_equal(got, want), "uint8 %s: columns differ\n%s\n%s" % (a.shape, got, want)
    if floats:
        gotf = dev(as_float(a), as_float(b), mask, valid, clip)
        assert np.array_equal(gotf, want), "float %s: columns differ\n%s\n%s" % (a.shape, gotf, want)
    return want


def frames(n, h, w, c, seed, close=True):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)
    if not close:
        return a, rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)
    return a, np.clip(a.astype(int) + rng.integers(-20, 21, a.shape), 0, 255).astype(np.uint8)


def blob_mask(h, w, seed):
    m = np.zeros((h, w), np.uint8)
    rng = np.random.default_rng(seed)
    y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
    m[y:y + max(1, h // 2), x:x + max(1, w // 2)] = 255
    return m


AROUND = (TILE - 1, TILE, TILE + 1, 2 * TILE + 6)
SHAPES = [(1, 1), (6, 9), (7, 7), (8, 8), (17, 23)] + [(h, 9) for h in AROUND] + [(9, w) for w in AROUND] + [(2 * TILE + 6, TILE + 1)]


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes_channels_and_batch_sizes(hipb, hw):
    h, w = hw
    for c, n in ((1, 1), (3, 2), (1, 3), (3, 3)):
        a, b = frames(n, h, w, c, seed=h * 100 + w + c + n)
        t = check(a, b, blob_mask(h, w, h + w))
        assert (t[:, 0, 0] == h * w * c).all() and (t[:, 0, 4] == max(h - 6, 0) * max(w - 6, 0) * c * (h >= 7 and w >= 7)).all()


def test_valid_rectangle_with_garbage_and_nan_in_the_padding(hipb):
    h, w, vh, vw = 2 * TILE + 8, TILE + 13, TILE + 5, TILE + 2
    a, b = frames(3, h, w, 3, seed=1)
    m = blob_mask(h, w, 2)
    m[vh:], m[:, vw:] = 7, 9
    want = check(a[:, :vh, :vw], b[:, :vh, :vw], m[:vh, :vw])
    assert np.array_equal(check(a, b, m, valid=(vh, vw)), want)
    fa, fb = as_float(a), as_float(b)
    rng = np.random.default_rng(3)
    for x in (fa, fb):
        x[:, :, vh:] = rng.standard_normal(x[:, :, vh:].shape) * 1e30
        x[:, :, :, vw:] = np.nan
    assert np.array_equal(dev(fa, fb, m, valid=(vh, vw)), want)
    assert np.array_equal(dev(fa, fb, None, valid=(vh, vw))[:, 0], want[:, 0])
    for valid in ((1, 1), (7, w), (h, 7), (TILE, TILE)):
        check(a, b, m, valid=valid, floats=False)


def test_masks(hipb):
    h, w, vh, vw = TILE + 9, 2 * TILE + 3, TILE + 2, TILE + 7
    a, b = frames(2, h, w, 3, seed=4)
    z = np.zeros((h, w), np.uint8)
    empty = check(a, b, z, valid=(vh, vw))
    assert not empty[:, 1].any()
    assert np.array_equal(empty, check(a, b, None, valid=(vh, vw)))
    full = check(a, b, np.full((h, w), 3, np.uint8), valid=(vh, vw))
    assert np.array_equal(full[:, 0], full[:, 1])
    for y, x in ((0, 0), (0, vw - 1), (vh - 1, 0), (vh - 1, vw - 1)):                 # the corners of the valid rectangle
        m = z.copy()
        m[y, x] = 1
        t = check(a, b, m, valid=(vh, vw))
        assert (t[:, 1, 0] == 3).all() and not t[:, 1, 4].any()                        # three samples, centre of no whole window
    m = z.copy()
    m[:10, :5] = 255                                                                  # touches the border: its windows are cut off
    m[vh - 4:, TILE - 2:] = 255
    t = check(a, b, m, valid=(vh, vw))
    assert (t[:, 1, 4] == 3 * ((10 - 3) * (5 - 3) + 1 * (vw - 3 - (TILE - 2)))).all()
    m = z.copy()
    m[vh:], m[:, vw:] = 255, 255                                                      # non-zero in the padding only
    assert np.array_equal(check(a, b, m, valid=(vh, vw)), empty)


def test_counter_range_and_negative_ssim(hipb):
    a, b = np.zeros((1, 160, 160, 3), np.uint8), np.full((1, 160, 160, 3), 255, np.uint8)
    t = check(a, b, np.ones((160, 160), np.uint8))
    assert t[0, 0, 1] == 160 * 160 * 3 * 65025 > 1 << 32 and t[0, 1, 1] == t[0, 0, 1]
    a = np.random.default_rng(5).integers(0, 256, (2, TILE + 5, TILE + 9, 3), dtype=np.uint8)
    t = check(a, 255 - a, blob_mask(TILE + 5, TILE + 9, 6))
    assert (t[:, 0, 3] < -(t[:, 0, 4] << 29)).all()                                    # mean SSIM below -0.5: the fixed point is signed
    a, b = frames(2, TILE + 5, TILE + 9, 3, seed=7, close=False)                       # unrelated noise: SSIM near 0, of either sign
    check(a, b)
    same = check(a, a.copy())
    assert (same[:, 0, 3] == same[:, 0, 4] << 30).all() and not same[:, 0, [1, 2, 5]].any()


def test_clip_switch_and_repeatability(hipb):
    a, b = frames(3, TILE + 3, TILE + 3, 3, seed=8)
    m = blob_mask(TILE + 3, TILE + 3, 9)
    clip, still = check(a, b, m), check(a, b, m, clip=False)
    assert clip[1:, :, 5].all() and not clip[0, :, 5].any() and not still[:, :, 5].any()
    assert np.array_equal(clip[:, :, :5], still[:, :, :5])
    assert np.array_equal(dev(a, b, m), dev(a, b, m))
    fa, fb = as_float(a), as_float(b)
    assert np.array_equal(dev(fa, fb, m), dev(fa, fb, m))


def test_argument_errors_raise_before_any_launch(hipb):
    from video_filler_amd import data
    from video_filler_amd._lib import VfError
    f = torch.zeros(2, 3, 8, 9)
    u = torch.zeros(2, 8, 9, 3, dtype=torch.uint8)
    hipb.prof_begin()
    with pytest.raises(ValueError, match="both are float N x C x H x W or both uint8 N x H x W x C"):
        data.frame_metrics(f, torch.zeros(2, 3, 9, 9))
    with pytest.raises(ValueError, match="both are float"):
        data.frame_metrics(f, u)
    with pytest.raises(ValueError, match="2 channels"):
        data.frame_metrics(torch.zeros(2, 2, 8, 9), torch.zeros(2, 2, 8, 9))
    with pytest.raises(ValueError, match="the mask is uint8"):
        data.frame_metrics(u, u, torch.zeros(8, 8, dtype=torch.uint8))
    for bad in ((0, 9), (9, 9), (8, 10)):
        with pytest.raises(ValueError, match="outside 1..8 x 1..9"):
            data.frame_metrics(f, f, None, bad)
    with pytest.raises(VfError, match="valid rectangle 9 x 9"):                        # the library checks for itself
        hipb.frame_metrics(f.cuda(), f.cuda(), None, (9, 9))
    assert not hipb.prof_end()                                                        # nothing was launched


def test_evaluate_frames_gives_the_numbers_of_the_files(hipb, tmp_path):
    """inference.evaluate_frames on tensors of the shape WholeImageInpainter returns == metrics_ref on the frames read
    back, with Pillow, from the files save_frames wrote."""
    from PIL import Image
    from video_filler_amd import inference
    predLen, nc, H, W, vh, vw = 4, 3, 2 * TILE, TILE + TILE // 2, TILE + 13, TILE + 1
    rng = np.random.default_rng(10)
    truth = rng.uniform(-0.05, 1.05, (predLen, nc, H, W)).astype(F)
    result = (truth + rng.standard_normal(truth.shape).astype(F) * F(0.05)).astype(F)
    padmask = np.zeros((nc, H, W), np.uint8)
    padmask[:, 10:TILE + 3, 5:TILE - 4] = 1
    got = inference.evaluate_frames(torch.from_numpy(result).cuda(), torch.from_numpy(truth).cuda(), torch.from_numpy(padmask).cuda(),
                                    valid=(vh, vw))
    paths = inference.save_frames(str(tmp_path), inpaintImages=torch.from_numpy(result), fullImages=torch.from_numpy(truth))
    read = np.stack([np.asarray(Image.open(p).convert("RGB")) for p in paths])
    want = R.scores(R.frame_table(read[:predLen], read[predLen:], padmask[0], (vh, vw)))
    for k in ("psnr", "ssim", "mae", "flicker", "hole_psnr", "hole_ssim", "hole_mae", "hole_flicker"):
        assert got[k].dtype == np.float64 and got[k].shape == (predLen,) and np.array_equal(got[k], want[k]), k
        assert np.isfinite(got[k]).all() and got["mean"][k] == want["mean"][k], k
    assert (got["ssim"] < 1).all() and (got["psnr"] > 15).all() and got["flicker"][0] == 0 and (got["flicker"][1:] > 0).all()
    # uint8 frames, as save_frames also accepts them, and host tensors: the same numbers
    again = inference.evaluate_frames(read[:predLen], read[predLen:], padmask[0], valid=(vh, vw))
    assert all(np.array_equal(again[k], got[k]) for k in got if k != "mean")
