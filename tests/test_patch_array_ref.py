"""The restatement of train_wholeim_input.lua's loader (tests/patch_array_ref.py) pinned on the host: against an index
formula on small hand-checkable cases, the zero bands, the full-width flip, the window numbering; the draw order of
data.draw_patch_array; the geometry the reference is not defined for."""
import numpy as np
import pytest

import image_ref as R
import patch_array_ref as PA

import video_filler_amd  # noqa: F401
from video_filler_amd import data

MV = 110.0 / 255.0


def _case(iH, iW, seed, block=True):
    rng = np.random.default_rng(seed)
    inp = rng.uniform(0.05, 1, (3, iH, iW)).astype(np.float32)
    mask = np.zeros((1, iH, iW), np.uint8)
    if block:
        mask[:, iH // 3:iH // 3 + iH // 4, iW // 4:iW // 4 + iW // 3] = 1
        mask[:, iH - 3:, iW - 5:] = 1                 # reaches the bottom-right corner: must move with the shift
    return inp, mask


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("crop_w,crop_h", [(1, 1), (100, 70), (37, 5)])
@pytest.mark.parametrize("iH,iW,ss,arrh,arrw", [(90, 130, 16, 3, 3), (80, 110, 12, 2, 2), (84, 121, 10, 4, 3)])
def test_restatement_equals_the_index_formula(iH, iW, ss, arrh, arrw, crop_w, crop_h, flip):
    inp, mask = _case(iH, iW, iH + crop_w)
    out, maskout, masked, s = PA.train_hook(inp, mask, ss, arrh, arrw, crop_w, crop_h, flip, MV)
    out2, maskout2, masked2 = PA.by_index(inp, mask, ss, arrh, arrw, crop_w, crop_h, flip, MV)
    np.testing.assert_array_equal(out, out2)
    np.testing.assert_array_equal(maskout, maskout2)
    np.testing.assert_array_equal(masked, masked2)
    assert out.dtype == maskout.dtype == masked.dtype == np.float32
    assert set(np.unique(maskout)) <= {0.0, 1.0}
    # masked == full wherever the mask is 0, on the four shared windows; maskValue wherever it is 1
    win = [0, 1, arrw, arrw + 1]
    shared = np.concatenate([masked[3 * p:3 * p + 3] for p in win])
    np.testing.assert_array_equal(shared[maskout == 0], out[maskout == 0])
    assert (shared[maskout == 1] == np.float32(MV) * np.float32(2) + np.float32(-1)).all()
    # the dark sum belongs to output window 0: (out + 1) / 2 undoes the [-1,1] map only to float32 rounding, hence the loose
    # bound — the exact statement (s == the double sum of the unmapped window) is test_windows_by_hand's
    top = (out[0:3].astype(np.float64) + 1) / 2
    assert abs(s - top.sum()) < 1e-3


def test_windows_by_hand():
    """3 x 3 windows of 4 pixels over a 10 x 12 frame whose value encodes its position: steps 3 and 4."""
    iH, iW, ss = 10, 12, 4
    pos = (np.arange(iH)[:, None] * 16 + np.arange(iW)[None, :]).astype(np.float32) / np.float32(256)
    inp = np.stack([pos, pos + np.float32(1 / 512), pos + np.float32(1 / 1024)])
    mask = np.zeros((1, iH, iW), np.uint8)
    mask[0, 4, 5] = 1
    out, maskout, masked, s = PA.train_hook(inp, mask, ss, 3, 3, 1, 1, False, MV)
    dec = lambda a: (a + 1) / 2                                       # exact: dyadic values
    np.testing.assert_array_equal(dec(masked[0:3]), inp[:, 0:4, 0:4])             # p = 0: (h, w) = (1, 1)
    np.testing.assert_array_equal(dec(masked[3 * 5:3 * 5 + 3]), inp[:, 3:7, 8:12])  # p = 5: (h, w) = (4, 9), no mask inside
    np.testing.assert_array_equal(dec(masked[3 * 8:3 * 8 + 3]), inp[:, 6:10, 8:12])
    # out windows: (h1, w1) = (0,0), (0,1), (1,0), (1,1) -> channels 0, 3, 6, 9
    np.testing.assert_array_equal(dec(out[3:6]), inp[:, 0:4, 4:8])
    np.testing.assert_array_equal(dec(out[6:9]), inp[:, 3:7, 0:4])
    np.testing.assert_array_equal(dec(out[9:12]), inp[:, 3:7, 4:8])
    assert maskout[9:12, 1, 1].tolist() == [1, 1, 1] and maskout.sum() == 3       # (4, 5) lies in window (1,1) alone
    assert s == float(inp[:, 0:4, 0:4].astype(np.float64).sum())


def test_zero_bands_and_full_width_flip():
    iH, iW, ss = 90, 130, 16
    inp, mask = _case(iH, iW, 5)
    mask[:] = 1                                                       # every real pixel is masked: the bands stand out
    crop_w, crop_h = 100, 70                                          # 31 columns and 21 rows of the frame survive
    out, maskout, masked, _ = PA.train_hook(inp, mask, ss, 3, 3, crop_w, crop_h, False, MV)
    mv = np.float32(MV) * np.float32(2) + np.float32(-1)
    # window 0 is all real; beyond the surviving pixels a ZERO band (-1 after the map, NOT maskValue), mask 0 there too
    assert (masked[0:3] == mv).all() and (maskout[0:3] == 1).all()
    np.testing.assert_array_equal(out[0:3], inp[:, 69:85, 99:115] * np.float32(2) + np.float32(-1))
    # window (0,1) starts at column 57 > 31: all band
    assert (masked[3:6] == -1).all() and (out[3:6] == -1).all() and (maskout[3:6] == 0).all()
    # window (1,0) starts at row 37 > 21
    assert (masked[9:12] == -1).all() and (out[6:9] == -1).all()
    # crop_h = 80: 11 rows survive, so window 0 is cut by the band
    out, maskout, masked, _ = PA.train_hook(inp, mask, ss, 3, 3, crop_w, 80, False, MV)
    assert (masked[0:3, :11] == mv).all() and (masked[0:3, 11:] == -1).all()
    assert (maskout[0:3, :11] == 1).all() and (maskout[0:3, 11:] == 0).all() and (out[0:3, 11:] == -1).all()
    # flipped over the FULL width: the real columns are now the last 31, so the band is on the LEFT and the real pixels
    # reach the right-most window (0,2), mirrored
    out, maskout, masked, s = PA.train_hook(inp, mask, ss, 3, 3, crop_w, crop_h, True, MV)
    assert (masked[0:3] == -1).all() and (out[0:3] == -1).all() and (maskout[0:3] == 0).all() and s == 0.0
    assert (masked[6:9, :16, :] == mv).all()                           # window (0,2): columns 114..129, all real
    # unmasked, to see the mirror: column X of the flipped frame is column 129 - X of the shifted one
    mask[:] = 0
    out, _, masked, _ = PA.train_hook(inp, mask, ss, 3, 3, crop_w, crop_h, True, MV)
    np.testing.assert_array_equal(masked[6:9], inp[:, 69:85, 99:115][:, :, ::-1] * np.float32(2) + np.float32(-1))


def test_sample_scales_frame_and_mask_state():
    rng = np.random.default_rng(2)
    img = R.decoded_to_float(rng.integers(0, 256, (40, 60, 3), dtype=np.uint8))
    mask = np.zeros((1, 40, 60), np.uint8)
    mask[:, 10:25, 20:45] = 1
    d = dict(height=90, width=135, crop_w=3, crop_h=2, flip=True)
    masked, out, maskout, s, state = PA.sample(img, mask, d, ss=16)
    np.testing.assert_array_equal(state, R.scale(mask, 135, 90))
    o2, m2, k2, s2 = PA.train_hook(R.scale(img, 135, 90), state, 16, 3, 3, 3, 2, True, MV)
    np.testing.assert_array_equal(masked, k2)
    np.testing.assert_array_equal(out, o2)
    np.testing.assert_array_equal(maskout, m2)
    assert s == s2 and masked.shape == (27, 16, 16) and out.shape == maskout.shape == (12, 16, 16)


class _Recorder:
    """Records the calls a loader makes on its rng and answers from a real generator."""

    def __init__(self, seed):
        self.g, self.calls = np.random.default_rng(seed), []

    def uniform(self, *a):
        self.calls.append(("uniform",) + a)
        return self.g.uniform(*a)

    def integers(self, *a):
        self.calls.append(("integers",) + a)
        return self.g.integers(*a)


@pytest.mark.parametrize("loadSize", [360, 0, -1, -2])
def test_draw_order(loadSize):
    H, W = 360, 480
    rec = _Recorder(7)
    d = data.draw_patch_array(H, W, loadSize, rec)
    scale = {-1: [("uniform", 0.5, 1.5)], -2: [("uniform", 1, 3)]}.get(loadSize, [])
    assert rec.calls == scale + [("integers", 1, 101), ("integers", 1, 71), ("uniform",)]   # crop_w, crop_h, flip
    g = np.random.default_rng(7)
    scalef = float(g.uniform(*scale[0][1:])) if scale else None
    height, width = data.load_size(H, W, loadSize, scalef)
    want = dict(height=height, width=width, crop_w=int(g.integers(1, 101)), crop_h=int(g.integers(1, 71)))
    want["flip"] = bool(g.uniform() > 0.6)
    assert d == want
    if loadSize == 360:
        assert (height, width) == (360, 480)
    if loadSize < 0:
        assert (height, width) == (int(scalef * W), int(scalef * H))   # the transposed aspect of loadSize < 0, kept
    ds = [data.draw_patch_array(H, W, 360, g) for _ in range(4000)]
    assert {x["crop_w"] for x in ds} == set(range(1, 101))             # torch.random(100): 1..100 inclusive
    assert {x["crop_h"] for x in ds} == set(range(1, 71))


BAD = [
    dict(height=360, width=480, fineSize=128, nc=1),                              # channel triples
    dict(height=360, width=480, fineSize=128, array_h=1),                         # (arrh - 1) = 0
    dict(height=360, width=480, fineSize=128, array_w=1),
    dict(height=130, width=480, fineSize=128),                                    # steph = 1
    dict(height=360, width=129, fineSize=128),                                    # stepw = 0
    dict(height=100, width=480, fineSize=128),                                    # smaller than a window
    dict(height=136, width=480, fineSize=128, array_h=4),                         # steph = 2 visits 5 rows of windows
    dict(height=360, width=480, fineSize=128, crop_h=361),
    dict(height=360, width=480, fineSize=128, crop_w=481),
    dict(height=360, width=480, fineSize=128, crop_w=0),
]


@pytest.mark.parametrize("kw", BAD)
def test_geometry_the_reference_is_not_defined_for_raises(kw):
    with pytest.raises(ValueError, match="patch array"):
        data.patch_array_steps(**kw)
    g = dict(dict(array_h=3, array_w=3, nc=3, crop_h=1, crop_w=1), **kw)
    inp = np.zeros((g["nc"], g["height"], g["width"]), np.float32)
    with pytest.raises(ValueError):                                               # the restatement agrees, by running the loop
        PA.train_hook(inp, np.zeros((1,) + inp.shape[1:], np.uint8), g["fineSize"], g["array_h"], g["array_w"], g["crop_w"],
                      g["crop_h"], False, MV)


def test_geometry_accepted():
    assert data.patch_array_steps(360, 480, 128) == (116, 176)
    assert data.patch_array_steps(300, 400, 128, 4, 3) == (57, 136)
    assert data.patch_array_steps(300, 400, 128, 2, 2, crop_h=70, crop_w=100) == (172, 272)
    assert data.patch_array_steps(132, 132, 128) == (2, 2)
