"""The 64-row tile form of the planes weight-gradient kernel (k_pwgrad_group, csrc/vf_pgemm.hip): a layer whose low-resolution
operand has 64 channels (the generator's second conv) takes vf_conv2d_bwd_weight_planes / vf_deconv2d_bwd_weight_planes on a
64 x 128 x 32 tile instead of falling back to the fp32-fed kernel.  Same six-term products as that kernel in another summation
order: 2e-6 of the max-norm between them (the bar of test_gpu_pgemm.py::test_weight_gradient_from_planes), 2e-5 against an
fp64 evaluation (the suite's bar for the fp32-grade conv passes).  Which kernel ran is asserted from the launch list."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

NEW_ALONE = "pwgrad_group_64x128x32"
NEW_MIXED = "pwgrad_group_64+128x128x32"
OLD_128 = "pwgrad_group_128x128x32"

# (Bn, Cin, H, Cout): conv Cin -> Cout on an H x H map; the low-resolution operand has Cout channels
ONE_TILE = (2, 64, 16, 64)          # 128 pixels: four K steps, no split-K, eight column tiles
SPLIT_K = (8, 64, 64, 64)           # 8192 pixels: split-K (32 slabs of 8 K steps) and the combine
TWO_COLS = (2, 128, 16, 64)         # 128 gathered channels: two column tiles per tap
REMAINDER = (4, 64, 8, 192)         # 192 = 128 + 64 rows: not served (only ONE row tile of 64 is), stays on the fp32-fed kernel
SERVED = [ONE_TILE, SPLIT_K, TWO_COLS]


def _rand(shape, seed, dev, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev)


def _act(Bn, C, H, seed, dev):
    return _rand((Bn, H, H, C), seed, dev).permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def _operands(case):
    """the two maps of a case on the CPU, and the weight gradient of the conv in fp64: computed once, shared, never modified.
    (The full-conv on the SAME pair of maps — the low-resolution tensor its input, the other its gradOutput — has the same
    physical gradient [low-res channels][kh][kw][high-res channels].)"""
    Bn, Cin, H, Cout = case
    x = _act(Bn, Cin, H, 3, "cpu")
    gy = _act(Bn, Cout, H // 2, 4, "cpu")
    wz = torch.zeros(Cout, Cin, 4, 4, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(x.double().contiguous(), wz, stride=2, padding=1).backward(gy.double().contiguous())
    return x, gy, wz.grad.detach()


def _on_device(case, hipb):
    x, gy, ref = _operands(case)
    dev = hipb.device
    # channels-last storage, as every activation of the library
    x = x.permute(0, 2, 3, 1).contiguous().to(dev).permute(0, 3, 1, 2)
    gy = gy.permute(0, 2, 3, 1).contiguous().to(dev).permute(0, 3, 1, 2)
    return x, gy, hipb.planes_split(x), hipb.planes_split(gy), ref


def _call(hipb, full, x, gy, xp, gp, gw, beta, planes=True):
    """conv: (input, gradOutput) = (x, gy); the full-conv on the same maps: (gy, x)"""
    if full:
        hipb.deconv2d_bwd_weight(gy, x, gw, None, 4, 2, 1, beta, *((gp, xp) if planes else ()))
    else:
        hipb.conv2d_bwd_weight(x, gy, gw, None, 4, 2, 1, beta, *((xp, gp) if planes else ()))


def _gw(case, dev, seed=7):
    Bn, Cin, H, Cout = case
    return _rand((Cout, 4, 4, Cin), seed, dev, 0.5).permute(0, 3, 1, 2)      # logical [Cout][Cin][4][4] over physical [Cout][4][4][Cin]


def _wgrad_names(prof):
    return sorted(n for n in prof if "wgrad" in n and not n.startswith("slab_reduce"))


@pytest.mark.parametrize("full", [False, True], ids=["conv", "fullconv"])
@pytest.mark.parametrize("case", SERVED, ids=str)
def test_64_row_layer_alone(case, full, hipb):
    """overwrite and accumulate against the fp32-fed kernel (2e-6) and fp64 (2e-5), on the new tile form by its launch name"""
    x, gy, xp, gp, ref = _on_device(case, hipb)
    for beta in (0.0, 1.0):
        want = _gw(case, hipb.device)
        got = want.permute(0, 2, 3, 1).clone().permute(0, 3, 1, 2)
        old = got.permute(0, 2, 3, 1).clone().permute(0, 3, 1, 2).double().cpu()
        _call(hipb, full, x, gy, xp, gp, want, beta, planes=False)
        hipb.prof_begin()
        _call(hipb, full, x, gy, xp, gp, got, beta)
        names = _wgrad_names(hipb.prof_end())
        assert names == [NEW_ALONE], names
        scale = float(want.abs().max())
        err32 = float((got - want).abs().max()) / scale
        want64 = ref + beta * old
        err64 = float((got.double().cpu() - want64).abs().max() / want64.abs().max())
        print("case", case, "full", full, "beta", beta, "vs fp32-fed %.3g  vs fp64 %.3g" % (err32, err64))
        assert err32 <= 2e-6, (beta, err32)
        assert err64 <= 2e-5, (beta, err64)


def test_192_rows_keep_the_fp32_fed_kernel(hipb):
    """Nu % 128 == 64 beyond ONE row tile is refused by the planes route (documented in vf_conv.hip's wgrad): the planes arguments
    change neither the kernel nor a bit of the result"""
    x, gy, xp, gp, ref = _on_device(REMAINDER, hipb)
    for full in (False, True):
        want, got = _gw(REMAINDER, hipb.device), _gw(REMAINDER, hipb.device)
        _call(hipb, full, x, gy, xp, gp, want, 0.0, planes=False)
        hipb.prof_begin()
        _call(hipb, full, x, gy, xp, gp, got, 0.0)
        names = _wgrad_names(hipb.prof_end())
        assert names and not any(n.startswith("pwgrad_group") for n in names), names
        assert torch.equal(got, want)
        assert float((got.double().cpu() - ref).abs().max() / ref.abs().max()) <= 2e-5


def test_one_plane_mode_keeps_its_route(hipb):
    """the bf16-operand mode has no 64-row form: a 64-row layer stays off k_pwgrad_group there"""
    x, gy, xp, gp, _ = _on_device(ONE_TILE, hipb)
    got = _gw(ONE_TILE, hipb.device)
    hipb.set_mfma_mode("bf16")
    try:
        hipb.prof_begin()
        _call(hipb, False, x, gy, xp, gp, got, 0.0)
        names = _wgrad_names(hipb.prof_end())
    finally:
        hipb.set_mfma_mode("f32_3xbf16")
    assert names and not any(n.startswith("pwgrad_group") for n in names), names


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("case", [ONE_TILE, SPLIT_K], ids=str)
def test_in_a_group_beside_a_128_row_layer(case, beta, hipb):
    """one launch for both tile forms: the 64-row layer's result is what it is alone, and so, bit for bit, is the 128-row layer's"""
    dev = hipb.device
    x, gy, xp, gp, ref = _on_device(case, hipb)
    big = (4, 64, 32, 128)                       # 128 low-resolution channels, 1024 pixels: split-K as well
    xb, gb_ = _act(big[0], big[1], big[2], 11, dev), _act(big[0], big[3], big[2] // 2, 12, dev)
    xbp, gbp = hipb.planes_split(xb), hipb.planes_split(gb_)

    def fresh():
        return _gw(case, dev), _gw(big, dev, 9)
    a64, a128 = fresh()
    hipb.prof_begin()
    _call(hipb, False, xb, gb_, xbp, gbp, a128, beta)
    assert _wgrad_names(hipb.prof_end()) == [OLD_128]
    _call(hipb, False, x, gy, xp, gp, a64, beta)
    g64, g128 = fresh()
    hipb.prof_begin()
    hipb.wgrad_group_begin()
    _call(hipb, False, xb, gb_, xbp, gbp, g128, beta)
    _call(hipb, False, x, gy, xp, gp, g64, beta)
    hipb.wgrad_group_end()
    prof = hipb.prof_end()
    assert _wgrad_names(prof) == [NEW_MIXED] and prof[NEW_MIXED]["launches"] == 1, prof.keys()
    assert torch.equal(g128, a128)
    assert torch.equal(g64, a64)
    old = _gw(case, dev).double().cpu()
    want64 = ref + beta * old
    assert float((g64.double().cpu() - want64).abs().max() / want64.abs().max()) <= 2e-5


def test_repeat_in_place_is_bit_identical(hipb):
    """the split-K case once more into the same output and workspace: same slabs, same gradient"""
    Bn, Cin, H, Cout = SPLIT_K
    x, gy, xp, gp, _ = _on_device(SPLIT_K, hipb)
    got = _gw(SPLIT_K, hipb.device)
    total = Cout * 16 * Cin
    nslab = 32                                   # 8192 pixels = 256 K steps of 32, 8 per block: 8 column tiles x 32 = 256 blocks
    nbytes = nslab * total * 4
    ws = hipb.workspace.view(torch.uint8).flatten()
    assert ws.numel() >= nbytes
    _call(hipb, False, x, gy, xp, gp, got, 0.0)
    first, slabs = got.clone(), ws[:nbytes].clone()
    # the slabs sum to the output (so these bytes ARE the slabs of this launch)
    s = slabs.view(torch.float32).view(nslab, total).double().sum(0)
    assert float((s - first.permute(0, 2, 3, 1).reshape(-1).double()).abs().max()) <= 1e-5 * float(first.abs().max())
    _call(hipb, False, x, gy, xp, gp, got, 0.0)
    assert torch.equal(got, first)
    assert torch.equal(ws[:nbytes], slabs)
