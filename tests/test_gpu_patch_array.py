"""GPU parity of train_wholeim_input.lua's loader on the device (data.PatchArrayBatcher, vf_patch_array_prepare; DESIGN.md
5.1, quirk 4) against the NumPy restatement in tests/patch_array_ref.py: the three batch tensors bit for bit, the mask
state after every call, the dark rule's decisions against a host replay of the same random stream, the sum within the
bound of a fixed-order double sum."""
import os

import numpy as np
import pytest
import torch

import image_ref as R
import patch_array_ref as PA
from helpers import to_np

pytestmark = pytest.mark.gpu

MV = 110.0 / 255.0
FS = 128


def _logo_mask(H, W):
    m = np.zeros((1, H, W), np.uint8)
    m[:, H // 8:H // 8 + H // 5, W // 10:W // 10 + W // 3] = 1       # a logo-like block
    m[:, H - H // 6:H - 4, W // 2:W - 7] = 1                          # and a caption bar
    return m


def _as_input(dec, hwc, k, dev):
    """the sample as `add` accepts it: decoded uint8 HWC or float CHW, on the host (numpy / tensor) or on the device."""
    x = torch.from_numpy(dec if hwc else R.decoded_to_float(dec))
    return (dec if hwc else x.numpy(), x, x.to(dev))[k % 3]


def _check_row(pb, n, want_masked, want_full, want_mask):
    np.testing.assert_array_equal(to_np(pb.masked[n]), want_masked)
    np.testing.assert_array_equal(to_np(pb.full[n]), want_full)
    np.testing.assert_array_equal(to_np(pb.mask[n]), want_mask)


@pytest.mark.parametrize("hwc", [True, False])
@pytest.mark.parametrize("loadSize,H,W", [(360, 360, 480), (360, 512, 683), (-1, 360, 480), (0, 300, 400)])
def test_batch_bit_exact(loadSize, H, W, hwc, hipb):
    """Forced flips and the extreme crops, host and device inputs, a logo-like mask whose state is rescaled call by call."""
    from video_filler_amd.data import PatchArrayBatcher, draw_patch_array
    rng = np.random.default_rng(abs(loadSize) * 7 + H + hwc)
    Bn = 4
    pb = PatchArrayBatcher(Bn, 3, FS, loadSize, rng=np.random.default_rng(1))
    state = _logo_mask(H, W)
    pb.set_mask(torch.from_numpy(state))
    draws = np.random.default_rng(11)
    want = []
    for k in range(Bn):
        dec = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        d = draw_patch_array(H, W, loadSize, draws)
        d["flip"] = bool(k % 2)
        if k == 0:
            d.update(crop_w=1, crop_h=1)
        if k == 1:
            d.update(crop_w=100, crop_h=70)
        assert pb.add(_as_input(dec, hwc, k, hipb.device), decisions=d)
        masked, full, maskout, s, state = PA.sample(R.decoded_to_float(dec), state, d, FS, 3, 3, MV)
        np.testing.assert_array_equal(to_np(pb.mask_state), state)
        assert pb.last["rejected"] is False and {k2: pb.last[k2] for k2 in d} == d
        # relative bound; a top-left window that is all zero band (flip with a large crop_w) has s == 0.0, and the bound then
        # asks for the device sum to be exactly 0.0 too, which it must be
        assert abs(pb.last["mean"] * 3 * FS * FS - s) <= 1e-10 * abs(s)
        want.append((masked, full, maskout))
    assert state.sum() > 0
    got = pb.batch()
    assert [tuple(t.shape) for t in got] == [(Bn, 27, FS, FS), (Bn, 12, FS, FS), (Bn, 12, FS, FS)]
    for t in got:
        assert t.permute(0, 2, 3, 1).is_contiguous()                   # channels-last, as VidTrainer.set_batch reads them
    for j in range(3):
        np.testing.assert_array_equal(to_np(got[j]), np.stack([w[j] for w in want]))
    assert want[1][2].sum() > 0 or want[0][2].sum() > 0               # the mask reaches the output windows


@pytest.mark.parametrize("arrh,arrw,H,W", [(2, 2, 300, 400), (4, 3, 300, 400), (3, 3, 140, 150)])
def test_other_arrays_and_all_zero_mask(arrh, arrw, H, W, hipb):
    from video_filler_amd.data import PatchArrayBatcher
    rng = np.random.default_rng(arrh * 10 + arrw)
    pb = PatchArrayBatcher(2, 3, FS, 0, arrh, arrw, rng=np.random.default_rng(2))
    state = np.zeros((1, 77, 91), np.uint8)                           # a mask of another size: scaled to the frame's
    pb.set_mask(state)
    for k in range(2):
        dec = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        d = dict(height=H, width=W, crop_w=(100, 3)[k], crop_h=(2, 70)[k], flip=bool(k))
        assert pb.add(torch.from_numpy(dec).to(hipb.device), decisions=d)
        masked, full, maskout, s, state = PA.sample(R.decoded_to_float(dec), state, d, FS, arrh, arrw, MV)
        assert maskout.sum() == 0
        _check_row(pb, k, masked, full, maskout)
        np.testing.assert_array_equal(to_np(pb.mask_state), state)
    assert tuple(pb.batch()[0].shape) == (2, 3 * arrh * arrw, FS, FS)


@pytest.mark.parametrize("loadSize", [360, -2])
def test_mask_state_and_dark_rule_follow_the_random_stream(loadSize, hipb):
    """Dark frames (bytes // 64: mean about 0.006) are mostly rejected, bright ones (uniform bytes: about 0.5) never: both far
    from the 0.1 threshold, so the decision does not hang on the last bits of the mean.  The draws come from the batcher's
    rng in the loader's order, the extra uniform only for a dark sample; the mask state moves on rejected calls too; a
    rejected row is overwritten by the next sample."""
    from video_filler_amd.data import PatchArrayBatcher, draw_patch_array
    H, W, Bn = 180, 240, 3
    rng = np.random.default_rng(5)
    pb = PatchArrayBatcher(Bn, 3, FS, loadSize, rng=np.random.default_rng(17))
    replay = np.random.default_rng(17)
    state = _logo_mask(H, W)
    pb.set_mask(torch.from_numpy(state))
    want, rejected, k = [], 0, 0
    while len(want) < Bn:
        dec = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        dark = k % 2 == 0
        if dark:
            dec //= 64
        k += 1
        assert k < 60
        d = draw_patch_array(H, W, loadSize, replay)
        masked, full, maskout, s, state = PA.sample(R.decoded_to_float(dec), state, d, FS, 3, 3, MV)
        mean = s / (3 * FS * FS)
        assert (mean < 0.02) if dark else (mean > 0.12), "an input of this test, not a result: keep the mean far from 0.1"
        rej = bool(mean < 0.1 and replay.uniform() > 0.1)
        n = pb.n
        ok = pb.add(dec)
        np.testing.assert_array_equal(to_np(pb.mask_state), state)    # after every call, rejected ones included
        assert ok == (not rej) and pb.last["rejected"] == rej
        assert {k2: pb.last[k2] for k2 in d} == d
        assert abs(pb.last["mean"] - mean) <= 1e-10 * abs(mean)       # exact equality where the window is all zero band
        _check_row(pb, n, masked, full, maskout)                      # the row is written either way ...
        assert pb.n == n + (0 if rej else 1)                          # ... and kept only for an accepted sample
        rejected += rej
        if not rej:
            want.append((masked, full, maskout))
    assert rejected >= 1, "the stream of this seed must hold a rejected sample"
    got = pb.batch()
    for j in range(3):
        np.testing.assert_array_equal(to_np(got[j]), np.stack([w[j] for w in want]))
    assert replay.uniform() == pb.rng.uniform()                       # both streams stand at the same place


def test_sum_bound_and_repeatability(hipb):
    """The device sum against the restatement's double sum: a fixed-order double sum of 3 * 128^2 floats is off by at most
    about 49152 * 2^-53 = 5.5e-12 relative; 1e-10 is asserted.  Two launches on the same input give the same bits."""
    from video_filler_amd.backend import nhwc_empty
    rng = np.random.default_rng(3)
    H, W, h, w = 200, 260, 360, 468
    dec = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    mask = R.scale(_logo_mask(H, W), w, h)
    d = dict(height=h, width=w, crop_w=41, crop_h=13, flip=True)
    masked, full, maskout, s, _ = PA.sample(R.decoded_to_float(dec[0]), mask, d, FS, 3, 3, MV)
    src, dmask = torch.from_numpy(dec).to(hipb.device), torch.from_numpy(mask[0]).to(hipb.device)
    runs = []
    for _ in range(2):
        out = [nhwc_empty(1, c, FS, FS, hipb.device) for c in (27, 12, 12)]
        tot = hipb.empty(1, dtype=torch.float64)
        hipb.patch_array_prepare(src, True, dmask, out[0], out[1], out[2], tot, h, w, 3, 3, 41, 13, True, MV)
        runs.append([to_np(t) for t in out] + [to_np(tot)])
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
    np.testing.assert_array_equal(runs[0][0][0], masked)
    np.testing.assert_array_equal(runs[0][1][0], full)
    np.testing.assert_array_equal(runs[0][2][0], maskout)
    got = float(runs[0][3][0])
    print("device sum %.17g, restatement %.17g, relative difference %.3e" % (got, s, abs(got - s) / abs(s)))
    assert abs(got - s) <= 1e-10 * abs(s)
    # no mask (NULL): the all-zero mask
    out = [nhwc_empty(1, c, FS, FS, hipb.device) for c in (27, 12, 12)]
    hipb.patch_array_prepare(src, True, None, out[0], out[1], out[2], tot, h, w, 3, 3, 41, 13, True, MV)
    m0, f0, k0, _, _ = PA.sample(R.decoded_to_float(dec[0]), np.zeros_like(mask), d, FS, 3, 3, MV)
    np.testing.assert_array_equal(to_np(out[0])[0], m0)
    np.testing.assert_array_equal(to_np(out[1])[0], f0)
    assert float(out[2].abs().sum()) == 0 and k0.sum() == 0


def test_batch_feeds_the_wholeim_trainer(hipb):
    from video_filler_amd.data import PatchArrayBatcher
    from video_filler_amd.trainers import VidTrainer
    rng = np.random.default_rng(8)
    Bn, H, W = 4, 360, 480
    pb = PatchArrayBatcher(Bn, rng=np.random.default_rng(4))
    pb.set_mask(torch.from_numpy(_logo_mask(H, W)))
    while pb.n < Bn:
        pb.add(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
    ctx, full, mask = pb.batch()
    tr = VidTrainer(dict(nBottleneck=96, nc_in=27, nc_out=12, nef=32, ngf=32, ndf=32, weight_nomask=1, wtgdl=0.5), seed=2)
    tr.set_batch(ctx, full, mask)
    tr.step()
    assert np.isfinite([v for v in tr.losses().values() if v is not None]).all()


def test_fed_by_decode_jpeg(hipb):
    """decode_jpeg -> add: a view into the decoder's buffer gives what the host-decoded frame gives, and the restatement."""
    from video_filler_amd import data
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz"))
    name = [k[4:] for k in sorted(golden.files) if k.startswith("jpg/420_360x480")][0]       # Pillow-encoded 4:2:0
    ref = golden["ref/" + name]
    views = data.decode_jpeg([golden["jpg/" + name].tobytes()] * 2)
    d = dict(height=360, width=480, crop_w=9, crop_h=33, flip=True)
    pb = data.PatchArrayBatcher(2, rng=np.random.default_rng(6))
    pb.set_mask(_logo_mask(360, 480))
    assert pb.add(views[1], decisions=d) and pb.add(torch.from_numpy(ref), decisions=d)
    masked, full, maskout, _, _ = PA.sample(R.decoded_to_float(ref), _logo_mask(360, 480), d, FS, 3, 3, MV)
    for n in range(2):
        _check_row(pb, n, masked, full, maskout)


def test_bad_geometry_is_refused_before_anything_is_written(hipb):
    from video_filler_amd.backend import nhwc_empty
    from video_filler_amd.data import PatchArrayBatcher
    src = torch.zeros(1, 64, 64, 3, dtype=torch.uint8, device=hipb.device)
    out = [nhwc_empty(1, c, FS, FS, hipb.device) for c in (27, 12, 12)]
    out4 = nhwc_empty(1, 36, FS, FS, hipb.device)
    out1 = nhwc_empty(1, 9, FS, FS, hipb.device)
    for t in out + [out4, out1]:
        t.fill_(7.0)
    tot = hipb.empty(1, dtype=torch.float64).fill_(-3.0)

    def call(masked, h, w, arrh, arrw, crop_w, crop_h):
        hipb.patch_array_prepare(src, True, None, masked, out[1], out[2], tot, h, w, arrh, arrw, crop_w, crop_h, False, MV)

    with pytest.raises(RuntimeError, match="steps 1 and 176"):
        call(out[0], 130, 480, 3, 3, 1, 1)
    with pytest.raises(RuntimeError, match="steps 0 and"):
        call(out[0], 100, 480, 3, 3, 1, 1)
    with pytest.raises(RuntimeError, match="visit 5x3 windows"):
        call(out4, 136, 480, 4, 3, 1, 1)
    with pytest.raises(RuntimeError, match=r"crop \(481,1\) outside the 360x480"):
        call(out[0], 360, 480, 3, 3, 481, 1)
    with pytest.raises(RuntimeError, match=r"crop \(1,361\) outside"):
        call(out[0], 360, 480, 3, 3, 1, 361)
    with pytest.raises(RuntimeError, match="1x3 patch array"):
        call(out1, 360, 480, 1, 3, 1, 1)
    torch.cuda.synchronize()
    for t in out + [out4, out1]:
        assert bool((t == 7.0).all())
    assert float(tot[0]) == -3.0
    # the batcher names the geometry on the host, before its launch
    pb = PatchArrayBatcher(1, loadSize=130, rng=np.random.default_rng(1))
    pb.set_mask(np.zeros((1, 64, 64), np.uint8))
    with pytest.raises(ValueError, match="steps 1 and"):
        pb.add(np.zeros((64, 64 * 4, 3), np.uint8))
    assert tuple(pb.mask_state.shape) == (1, 64, 64)                   # a refused call leaves the state alone
    with pytest.raises(ValueError, match="nc=1"):
        PatchArrayBatcher(1, nc=1)
    assert pb.n == 0
