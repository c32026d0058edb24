"""GPU parity of Torch7's image.scale and the loaders built on it (vf_image.hip) against the float32
restatement in tests/image_ref.py: bit-exact everywhere except through the generator (the tolerance
test_gpu_pipeline.py uses for it)."""
import numpy as np
import pytest
import torch

import image_ref as R
from helpers import rel_err, to_np

pytestmark = pytest.mark.gpu

SIZES = [
    (360, 480, 350, 466),      # loadSize 350 on the reference's frames: non-integer downscale
    (360, 480, 128, 170),
    (97, 131, 300, 41),        # up in one axis, down in the other
    (64, 96, 32, 48),          # integer downscale
    (37, 45, 80, 100),         # upscale
    (1, 1, 5, 7),              # one-pixel source
    (1, 9, 4, 3),
    (5, 1, 1, 1),
    (40, 52, 40, 52),          # equal sizes: a copy
]


@pytest.mark.parametrize("N", [1, 12])
@pytest.mark.parametrize("H,W,h,w", SIZES)
def test_scale_float_and_decoded_bit_exact(H, W, h, w, N, hipb):
    from video_filler_amd import data
    rng = np.random.default_rng(H * 1000 + W + N)
    dec = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    planar = np.stack([R.decoded_to_float(f) for f in dec])
    want = R.scale(planar.reshape(N * 3, H, W), w, h).reshape(N, 3, h, w)
    got = data.image_scale(torch.from_numpy(dec), w, h, layout="hwc")
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, 3, h, w)
    np.testing.assert_array_equal(to_np(got), want)
    x = rng.uniform(0, 1, (N, 2, H, W)).astype(np.float32)
    got = data.image_scale(torch.from_numpy(x).to(hipb.device), w + 0.9, h + 0.5)     # fractional sizes truncate
    np.testing.assert_array_equal(to_np(got), R.scale(x.reshape(N * 2, H, W), w, h).reshape(N, 2, h, w))
    if N == 1:
        one = data.image_scale(torch.from_numpy(dec[0]), w, h, layout="hwc")
        np.testing.assert_array_equal(to_np(one), want[0])


@pytest.mark.parametrize("H,W,h,w", SIZES)
def test_scale_byte_bit_exact(H, W, h, w, hipb):
    from video_filler_amd import data
    rng = np.random.default_rng(H + W)
    b = rng.integers(0, 256, (2, H, W), dtype=np.uint8)
    got = data.image_scale(torch.from_numpy(b), w, h)
    assert got.dtype == torch.uint8
    np.testing.assert_array_equal(to_np(got), R.scale(b, w, h))
    m = np.zeros((1, H, W), np.uint8)
    m[:, H // 4:H // 2 + 1, W // 3:W // 3 + 2] = 1
    np.testing.assert_array_equal(to_np(data.image_scale(torch.from_numpy(m), w, h)), R.scale(m, w, h))


def test_repeated_mask_rescale_bit_exact(hipb):
    """The video loader rescales its module-global Byte mask from the previous scaled mask on every call."""
    from video_filler_amd import data
    m = np.zeros((1, 360, 480), np.uint8)
    m[:, 100:250, 150:330] = 1
    m[:, 20:23, 40:41] = 1
    d, want = torch.from_numpy(m), m
    for h, w in ((350, 466), (600, 450), (251, 336), (700, 1000), (180, 240)):
        d = data.image_scale(d, w, h)
        want = R.scale(want, w, h)
        np.testing.assert_array_equal(to_np(d), want)
    assert want.sum() > 0


@pytest.mark.parametrize("loadSize,H,W", [(350, 360, 480), (350, 512, 683), (-1, 360, 480), (150, 170, 140)])
def test_image_batcher_rows_feed_center_trainer(loadSize, H, W, oracle, hipb):
    from video_filler_amd.data import ImageBatcher, center_prepare, load_size
    from video_filler_amd.trainers import CenterTrainer
    rng = np.random.default_rng(abs(loadSize) + H)
    Bn, fs = 3, 128
    ib = ImageBatcher(Bn, 3, fs, loadSize, rng=np.random.default_rng(9))
    dec = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(Bn)]
    want, ds = [], []
    for k, img in enumerate(dec):
        d = ib.add(torch.from_numpy(img) if k % 2 else img)
        assert 0 <= d["h1"] <= d["height"] - fs and 0 <= d["w1"] <= d["width"] - fs
        ds.append(d)
        want.append(R.hook2d(R.decoded_to_float(img), d["height"], d["width"], fs, d["w1"], d["h1"], d["flip"]))
    want = np.stack(want)
    batch = ib.batch()
    assert tuple(batch.shape) == (Bn, 3, fs, fs) and batch.is_contiguous()
    np.testing.assert_array_equal(to_np(batch), want)
    # the draws follow the loader's order (data/donkey_folder.lua:52-82: scalef, h1, w1, flip) on the batcher's rng
    rng2 = np.random.default_rng(9)
    for d in ds:
        scalef = float(rng2.uniform(0.5, 1.5)) if loadSize == -1 else None
        h, w = load_size(H, W, loadSize, scalef)
        h1, w1 = int(np.ceil(rng2.uniform(1e-2, h - fs))), int(np.ceil(rng2.uniform(1e-2, w - fs)))
        assert d == dict(height=h, width=w, h1=min(h1, h - fs), w1=min(w1, w - fs), flip=bool(rng2.uniform() > 0.5))
    opt = dict(nBottleneck=64, wtl2=0.999, overlapPred=4, batchSize=Bn)
    want_ctx, want_center = oracle.center_prepare(want, 4)
    ctx, center = center_prepare(batch, 4)
    np.testing.assert_array_equal(to_np(ctx), want_ctx)
    np.testing.assert_array_equal(to_np(center), want_center)
    tr = CenterTrainer(opt)
    tr.set_batch(batch)
    tr.step()
    assert np.isfinite([v for v in tr.losses().values() if v is not None]).all()


@pytest.mark.parametrize("loadSize,centre_mask", [(140, True), (140, False), (-2, True), (0, False)])
def test_add_frames_matches_add_on_the_restated_clip(loadSize, centre_mask, hipb):
    """ClipBatcher.add_frames (device resize + mask state + device crop statistics) == ClipBatcher.add on the clip
    and mask restated on the host, with the same decisions — and those decisions are what `draw` takes from the same
    random stream on the host copies."""
    from video_filler_amd.data import ClipBatcher, draw_scalef, load_size
    rng = np.random.default_rng(loadSize + 7 * centre_mask)
    predLen, nc, H, W, fs = 2, 3, 150, 200, 128
    mask = np.zeros((1, H, W), np.uint8)
    if centre_mask:
        mask[:, 40:110, 50:160] = 1
    dev = ClipBatcher(4, predLen * nc, fs, rng=np.random.default_rng(3))
    host = ClipBatcher(4, predLen * nc, fs, rng=np.random.default_rng(3))
    dev.set_mask(torch.from_numpy(mask))
    state = mask
    added = 0
    for k in range(7):
        frames = rng.integers(0, 256, (predLen, H, W, nc), dtype=np.uint8)
        if k == 1:
            frames //= 64                           # a dark clip: mostly rejected (datavid/donkey_folder.lua:148-153)
        scalef = draw_scalef(loadSize, host.rng) if loadSize < 0 else None
        h, w = load_size(H, W, loadSize, scalef)
        clip = R.load_cont(np.stack([R.decoded_to_float(f) for f in frames]), h, w)
        state = R.scale(state, w, h)
        d_host = host.draw(clip, state)
        ok = dev.add_frames(frames, loadSize)
        np.testing.assert_array_equal(to_np(dev.mask_state), state)
        assert ok == (d_host is not None)
        if not ok:
            continue
        assert dev.last == dict(d_host, height=h, width=w)
        assert host.add(clip, state, d_host)
        added += 1
        if added == 4:
            break
    assert added == 4
    for a, b in zip(dev.batch(), host.batch()):
        np.testing.assert_array_equal(to_np(a), to_np(b))


@pytest.mark.parametrize("hwc", [True, False])
def test_load_whole_frames_feeds_the_inpainter(hwc, oracle, hipb):
    from test_gpu_pipeline import _small_netG
    from video_filler_amd.inference import WholeImageInpainter, load_whole_frames
    rng = np.random.default_rng(31)
    predLen, nc, fs, loadSize = 4, 3, 128, 200                      # 200 x 266 scaled, 256 x 384 padded
    dec = rng.integers(0, 256, (predLen, 90, 120, nc), dtype=np.uint8)
    planar = np.stack([R.decoded_to_float(f) for f in dec])
    decoded_mask = np.zeros((90, 120), np.uint8)
    decoded_mask[30:60, 40:95] = 255
    decoded_mask[10:20, 5:9] = 254                                   # not 255: not masked after :byte()
    mask = R.byte_mask(decoded_mask)[None]
    want_full, want_pm = R.whole_frames(planar, mask, loadSize, fs, 110.0 / 255.0)
    full, pm = load_whole_frames(torch.from_numpy(dec) if hwc else torch.from_numpy(planar), torch.from_numpy(mask),
                                 loadSize, fs, 110.0 / 255.0)
    assert full.dtype == torch.float32 and pm.dtype == torch.uint8
    np.testing.assert_array_equal(to_np(full), want_full)
    np.testing.assert_array_equal(to_np(pm), want_pm)
    assert want_pm.sum() > 0 and (want_full[:, 200:, :] == -1).all()
    ref, net = _small_netG(oracle, hipb, nc, nc, 5)
    want_out, want_inp, want_f = oracle.whole_image_inpaint(ref, want_full, want_pm, predLen, 1, fs, nc)
    out, inp, fullv = WholeImageInpainter(net, predLen, 1, fs, nc)(full, pm)
    assert rel_err(to_np(out), want_out) < 5e-5
    assert rel_err(to_np(inp), want_inp) < 5e-5
    np.testing.assert_array_equal(to_np(fullv).reshape(want_f.shape), want_f)


def test_image_entry_points_reject_bad_geometry(hipb):
    x = torch.zeros(1, 3, 64, 64, device=hipb.device)
    out = hipb.empty(3, 128, 128)
    with pytest.raises(RuntimeError, match="outside"):
        hipb.image_hook2d(x, False, out, 130, 130, 5, 0, False)
    with pytest.raises(RuntimeError, match="sides"):
        hipb.image_scale(x, False, hipb.empty(1, 3, 0, 5))
    with pytest.raises(RuntimeError, match="does not hold"):
        hipb.image_whole_frames(x, False, hipb.empty(1, 3, 64, 64), 70, 60, None, 0.4)
