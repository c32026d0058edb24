"""The contact sheets on the device (vf_display.hip) against tests/display_ref.py: BIT equality, no
tolerance — both sides are the same float32 operations in the same order, and the only reductions are min / max.
display_tensor over shapes, grid widths, paddings, every argument combination of tests/test_display_ref.py and both
input layouts; center_finish; predict_center on a real generator; the files save_sheet / save_clip_sheet write."""
import numpy as np
import pytest
import torch

import display_ref as R
import png_ref
from test_display_ref import LASTBIT, pack

pytestmark = pytest.mark.gpu

F = np.float32


def dev(x, **kw):
    from video_filler_amd import inference
    return inference.display_tensor(x, **kw).cpu().numpy()


def check(x, **kw):
    got, want = dev(torch.from_numpy(x), **kw), R.to_display_tensor(x, **kw)
    assert got.dtype == F and got.shape == want.shape
    assert np.array_equal(got, want), "%s %s: %d of %d elements differ" % (x.shape, kw, (got != want).sum(), want.size)
    return got


# (5, 3, 37, 41): 22755 elements — three reduction slices, the last one partial and ending off a 16-byte boundary
SHAPES = [(1, 1, 1, 1), (3, 1, 1, 1), (7, 3, 5, 7), (6, 3, 64, 64), (13, 1, 33, 2), (5, 3, 37, 41)]


@pytest.mark.parametrize("shape", SHAPES)
def test_layout_over_grid_widths_and_paddings(hipb, shape):
    x = np.random.default_rng(sum(shape)).standard_normal(shape).astype(F)
    for nrow in (1, 4, 6, 10):                       # N < nrow, N % xmaps != 0, N % xmaps == 0
        for padding in (0, 2, 4):
            check(x, padding=padding, nrow=nrow)


def test_extremes_at_the_ends_and_inside_the_last_partial_slice(hipb):
    x = np.random.default_rng(1).uniform(-1, 1, (6, 3, 64, 64)).astype(F)
    x.reshape(-1)[0], x.reshape(-1)[-1] = -7.5, 9.25
    g = check(x, nrow=4, padding=2)
    assert g.min() == 0 and g.max() == 1 and g[0, 0, 0] == 1            # the padding holds the scaled maximum
    y = np.random.default_rng(2).uniform(-1, 1, (5, 3, 37, 41)).astype(F)
    y.reshape(-1)[-3], y.reshape(-1)[-700] = 11.0, -13.0
    g = check(y, nrow=2)
    assert g.min() == 0 and g.max() == 1


def test_every_argument_combination_of_the_host_cases(hipb):
    x = pack([2, 4, 3])
    assert np.array_equal(check(x, padding=0, nrow=2)[0], np.array([[0, 1], [0.5, 1]], F))
    assert check(x, padding=2, nrow=2).shape == (1, 6, 6)
    assert not check(np.full((2, 3, 2, 2), 0.75, F)).any()              # constant: all zeros
    assert not check(np.zeros((2, 1, 2, 2), F)).any()                   # zero: untouched
    v = pack([0, 1, 2, 3, 4, 0.5])
    for kw in (dict(min=0, max=2), dict(min=0, max=2, saturate=False), dict(), dict(min=1, max=3), dict(min=1, max=3, saturate=False),
               dict(max=2), dict(min=1), dict(min=1, symmetric=True), dict(max=5, symmetric=True), dict(symmetric=True, saturate=False)):
        check(v, nrow=6, **kw)
        check(v, nrow=4, padding=2, **kw)
    check(pack([-1, 3, 0, 1.5]), nrow=4, symmetric=True)
    c = LASTBIT
    a = check(pack(c["values"]), nrow=4, min=c["min"], saturate=False)
    b = check(pack(c["values"]), nrow=4, min=c["min"], max=c["tmax"], saturate=False)
    assert a[0, 0, 3] == F(1) and b[0, 0, 3] == np.nextafter(F(1), F(0))
    rng = np.random.default_rng(8)
    z = rng.standard_normal((6, 3, 64, 64)).astype(F)
    for kw in (dict(min=-0.5, max=0.7), dict(min=0.1), dict(max=0.3), dict(min=-1, max=1, saturate=False), dict(symmetric=True),
               dict(min=1, max=-1, saturate=False)):
        check(z, nrow=6, **kw)                                          # no cell or band to fill
        check(z, nrow=4, padding=2, **kw)


def test_scaleeach(hipb):
    x = np.zeros((3, 1, 1, 2), F)
    x[0, 0, 0], x[1, 0, 0], x[2, 0, 0] = (0, 10), (-1, 1), (5, 6)
    assert np.array_equal(check(x, nrow=2, scaleeach=True)[0], np.array([[0, 1, 0, 1], [0, 1, 1, 1]], F))
    check(x, nrow=3, padding=2, scaleeach=True, min=0, max=20)
    rng = np.random.default_rng(9)
    for shape in ((7, 3, 5, 7), (6, 3, 64, 64), (5, 3, 37, 41)):        # 105 elements an image: slices start off a 16-byte boundary
        z = rng.standard_normal(shape).astype(F) * np.arange(1, shape[0] + 1, dtype=F).reshape(-1, 1, 1, 1)
        for kw in (dict(), dict(symmetric=True), dict(min=-1, max=2), dict(min=-1, max=2, saturate=False), dict(min=0.25),
                   dict(min=1, max=-1, saturate=False)):                # a negative divisor: every image's map falls
            check(z, nrow=4, padding=2, scaleeach=True, **kw)
            check(z, nrow=shape[0], scaleeach=True, **kw)


def test_channels_last_input_is_read_in_place(hipb):
    rng = np.random.default_rng(10)
    for shape in ((7, 3, 5, 7), (6, 3, 64, 64)):
        x = rng.standard_normal(shape).astype(F)
        t = torch.from_numpy(x).cuda().contiguous(memory_format=torch.channels_last)
        assert not t.is_contiguous()
        for kw in (dict(nrow=4, padding=2), dict(nrow=6), dict(nrow=4, scaleeach=True), dict(nrow=3, min=-1, max=1)):
            assert np.array_equal(dev(t, **kw), R.to_display_tensor(x, **kw))
    s = torch.from_numpy(x).cuda()[:, :, ::2, 1::3]                     # neither dense layout: copied to planar
    assert np.array_equal(dev(s, nrow=4), R.to_display_tensor(x[:, :, ::2, 1::3], nrow=4))


def test_negative_only_and_a_minimum_of_exactly_zero(hipb):
    rng = np.random.default_rng(12)
    neg = -rng.uniform(0.5, 3, (7, 3, 5, 7)).astype(F)
    g = check(neg, nrow=4, padding=2)
    assert g.max() == 1 and g.min() == 0
    pos = rng.uniform(0.5, 3, (7, 3, 5, 7)).astype(F)
    pos[3, 1, 2, 2] = 0                                                 # min == 0: the add is skipped
    g = check(pos, nrow=4)
    assert np.array_equal(g[:, :5, :7], pos[0] / pos.max())


def test_the_grid_is_the_same_on_every_run(hipb):
    x = np.random.default_rng(13).standard_normal((6, 3, 64, 64)).astype(F)
    t = torch.from_numpy(x).cuda()
    first = dev(t, nrow=4, padding=2).tobytes()
    for _ in range(4):
        assert dev(t, nrow=4, padding=2).tobytes() == first
    dev(torch.from_numpy(np.random.default_rng(14).uniform(50, 60, (40, 3, 96, 96)).astype(F)), nrow=7, scaleeach=True)
    assert dev(t, nrow=4, padding=2).tobytes() == first                 # the workspace now holds another call's partials


def test_display_refusals_reach_the_library_too(hipb):
    x = torch.zeros(2, 3, 4, 4, device=hipb.device)
    with pytest.raises(RuntimeError, match="padding=3"):
        hipb.display_tensor(x, padding=3)
    with pytest.raises(RuntimeError, match="2 x 2 x 4 x 4"):
        hipb.display_tensor(torch.zeros(2, 2, 4, 4, device=hipb.device))


# ------------------------------------------------------------------------------------------------------- center_finish
def nhwc(a):
    return torch.from_numpy(a).cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


@pytest.mark.parametrize("fs,ov", [(8, 0), (8, 1), (64, 0), (64, 1), (64, 4)])
def test_center_finish(hipb, fs, ov):
    rng = np.random.default_rng(fs + ov)
    for B in (1, 3):
        for C in (1, 3):
            ctx = rng.uniform(-1, 1, (B, C, fs, fs)).astype(F)
            pred = rng.uniform(-1, 1, (B, C, fs // 2, fs // 2)).astype(F)
            want = R.center_finish(ctx, pred, ov)
            c, p = nhwc(ctx), nhwc(pred)
            outs = [hipb.empty(*w.shape).fill_(-9) for w in want]
            hipb.center_finish(c, p, ov, *outs)
            for g, w in zip(outs, want):
                assert np.array_equal(g.cpu().numpy(), w)
            only = hipb.empty(*want[0].shape).fill_(-9)
            hipb.center_finish(c, p, ov, only)                          # both optional outputs NULL
            assert np.array_equal(only.cpu().numpy(), want[0])


def test_center_finish_refusals(hipb):
    from video_filler_amd.backend import nhwc_empty
    d = hipb.device
    with pytest.raises(RuntimeError, match="overlapPred=2"):
        hipb.center_finish(nhwc_empty(1, 3, 8, 8, d), nhwc_empty(1, 3, 4, 4, d), 2, hipb.empty(2, 3, 8, 8))
    with pytest.raises(RuntimeError, match="fineSize=6"):
        hipb.center_finish(nhwc_empty(1, 3, 6, 6, d), nhwc_empty(1, 3, 3, 3, d), 0, hipb.empty(2, 3, 6, 6))


# ------------------------------------------------------------------------------------------- predict_center, the files
@pytest.fixture(scope="module")
def small_net(hipb):
    """train.lua's generator at the smallest sizes its layers allow: five stride-2 convolutions and the 4 x 4 valid
    bottleneck convolution need a 128 x 128 input (the prediction is 64 x 64); nef = ngf = 8, nBottleneck = 16.
    weights_init, with the convolutions widened so that the output depends on the input in evaluate() mode."""
    from video_filler_amd.trainers import build_netG, weights_init
    net = build_netG(3, 3, 8, 8, 16, False)
    net.getParameters()
    weights_init(net, torch.Generator().manual_seed(3))

    def widen(m):
        if "Convolution" in m.type_name():
            m.weight.mul_(6.0)
    net.apply(widen)
    net.evaluate()
    return net


@pytest.fixture(scope="module")
def center_results(hipb, small_net):
    """(ov -> (batch, the net's own prediction on center_prepare's input, predict_center's results)), computed once"""
    from video_filler_amd import data, inference
    rng = np.random.default_rng(15)
    batch = rng.uniform(-1, 1, (3, 3, 128, 128)).astype(F)
    out = {}
    for ov in (0, 4):
        ctx, center = data.center_prepare(torch.from_numpy(batch), ov)
        pred = small_net.forward(ctx).clone()
        got = inference.predict_center(small_net, torch.from_numpy(batch), ov)
        out[ov] = (ctx.cpu().numpy(), center.cpu().numpy(), pred.cpu().numpy(), [g.cpu().numpy() for g in got])
    return out


@pytest.mark.parametrize("ov", [0, 4])
def test_predict_center_on_a_real_net(center_results, ov):
    ctx, center, pred, got = center_results[ov]
    assert pred.shape == (3, 3, 64, 64) and np.ptp(pred[0] - pred[1]) > 1e-6, "the net's output must depend on its input"
    want = R.center_finish(ctx, pred, ov) + (R.unit(center),)
    assert len(got) == 4
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w)
    lo, hi = 32 + ov, 96 - ov
    assert np.all(got[0][0::2, :, lo:hi, lo:hi] == 1) and got[0].min() >= 0 and got[0].max() <= 1


def read(path):
    with open(path, "rb") as fh:
        return png_ref.read_png(fh.read())


def test_save_sheet_writes_the_scripts_file(hipb, center_results, tmp_path):
    from video_filler_amd import inference
    pretty = center_results[4][3][0]
    path = inference.save_sheet(str(tmp_path / "s.png"), torch.from_numpy(pretty), nrow=10)     # test.lua:129
    assert path == str(tmp_path / "s.png")
    want = png_ref.chw_to_hwc_bytes(R.to_display_tensor(pretty, 0, 10)[None])[0]
    img = read(path)
    assert img.shape == (128, 6 * 128, 3) and np.array_equal(img, want)
    path = inference.save_sheet(str(tmp_path / "d.png"), torch.from_numpy(pretty))              # demo.lua:96
    assert np.array_equal(read(path), png_ref.chw_to_hwc_bytes(R.to_display_tensor(pretty)[None])[0])


def test_save_clip_sheet_interleaves_input_and_prediction(hipb, tmp_path):
    from video_filler_amd import inference

    class Half:                                        # a stand-in generator: evaluate() and forward() are all the driver uses
        def evaluate(self):
            pass

        def forward(self, x):
            y = x.clone()
            hipb.scale_shift(y, 0.5, 0.1)
            return y
    predLen = 5
    clip = np.random.default_rng(16).uniform(-1, 1, (predLen, 3, 32, 32)).astype(F)
    inp, pred = inference.predict_clip(Half(), torch.from_numpy(clip))
    path = inference.save_clip_sheet(str(tmp_path / "clip.png"), inp, pred)
    pretty = np.empty((2 * predLen, 3, 32, 32), F)
    pretty[0::2], pretty[1::2] = inp.cpu().numpy(), pred.cpu().numpy()
    want = png_ref.chw_to_hwc_bytes(R.to_display_tensor(pretty, 0, 10)[None])[0]
    img = read(path)
    assert img.shape == (32, 320, 3) and np.array_equal(img, want)


def test_load_demo_images_scales_and_maps(hipb):
    from video_filler_amd import data, inference
    frames = np.random.default_rng(17).integers(0, 256, (3, 50, 70, 3), dtype=np.uint8)
    got = inference.load_demo_images(frames, 32)
    want = data.image_scale(frames, 32, 32, layout="hwc").cpu().numpy() * F(2) + F(-1)           # mul(2):add(-1)
    assert got.shape == (3, 3, 32, 32) and np.array_equal(got.cpu().numpy(), want)
