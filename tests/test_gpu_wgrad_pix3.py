"""The whole-pixel form of the fp32-fed weight-gradient kernel (k_wgrad, csrc/vf_conv.hip): a layer whose high-resolution side
has 3 channels (the nets' image-side convs) gathers each (pixel, tap) with ONE 12-byte load into a 64-column tile whose columns
are 4 * tap + c, c = 3 a phantom channel that is always zero.  The same call with the 3-channel tensor zero-padded to 4 channels
takes the 16-byte route with the same split over K and the same products in the same order, so the two weight gradients are equal
bit for bit; against an fp64 evaluation the bar is test_gpu_conv_sweep.py's for weight gradients (TOL with beta = 1, 2 * TOL
with beta = 0).  Which kernel ran is asserted from the launch list."""
import functools

import pytest
import torch

from helpers import assert_close

pytestmark = pytest.mark.gpu

TOL = 2e-5                          # tests/test_gpu_conv_sweep.py
NEW = "_pix3_"

# (B, H, W of the LOW-resolution map, its channels): the 3-channel map is 2H x 2W
CASES = [
    (3, 4, 4, 64),       # P = 48: one K step and a partial one
    (2, 8, 8, 64),       # P = 128: four steps
    (3, 16, 16, 64),     # P = 768: 24 steps, no split
    (2, 32, 32, 64),     # P = 2048: 64 steps, split over K with slabs
    (2, 8, 16, 64),      # non-square
    (2, 16, 4, 64),      # non-square, the other order
    (2, 8, 8, 128),      # the 128-row tile
    (2, 32, 32, 128),    # ... split over K
    (2, 8, 8, 100),      # a partial row tile, 16-byte loads still legal on the 100-channel side
    (1, 8, 8, 32),       # a 64-row tile half empty
]
FULL_CASES = [(2, 8, 8, 64), (2, 32, 32, 64)]


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


@functools.lru_cache(maxsize=None)
def _operands(case):
    """both maps and the initial gradient in physical (channels-last) order on the CPU, and the weight gradient of the conv
    3 -> Nu in fp64 as [Nu][kh][kw][3]: computed once, shared, never modified.  The full-conv Nu -> 3 on the same pair of maps
    (the low-resolution tensor its input, the image its gradOutput) has the same physical gradient."""
    B, H, W, Nu = case
    img = _rand((B, 2 * H, 2 * W, 3), 3)
    low = _rand((B, H, W, Nu), 4)
    gw0 = _rand((Nu, 4, 4, 3), 5, 0.5)
    wz = torch.zeros(Nu, 3, 4, 4, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(img.double().permute(0, 3, 1, 2), wz, stride=2, padding=1).backward(low.double().permute(0, 3, 1, 2))
    return img, low, gw0, wz.grad.detach().permute(0, 2, 3, 1).contiguous()


def _dev(t, hipb):
    """physical [..][C] on the device, seen as the logical channels-first tensor the backend takes"""
    return t.contiguous().to(hipb.device).permute(0, 3, 1, 2)


def _pad4(t):
    return torch.cat([t, torch.zeros(t.shape[:-1] + (1,), dtype=t.dtype)], dim=-1)


def _call(hipb, full, img, low, gw, gb, beta):
    if full:
        hipb.deconv2d_bwd_weight(low, img, gw, gb, 4, 2, 1, beta)
    else:
        hipb.conv2d_bwd_weight(img, low, gw, gb, 4, 2, 1, beta)


def _wgrad_names(prof):
    return sorted(n for n in prof if "wgrad" in n and not n.startswith("slab_reduce"))


def _run(hipb, case, full, beta, cv, group=None):
    """the weight gradient of `case` with cv = 3 (the layer) or 4 (zero-padded) image channels -> (gw physical [Nu][4][4][cv], gb,
    launch names).  group: a callable that records a planes layer first; the call is then made inside an open group."""
    img, low, gw0, _ = _operands(case)
    Nu = case[3]
    if cv == 4:
        img, gw0 = _pad4(img), _pad4(gw0)
    dimg, dlow, gw = _dev(img, hipb), _dev(low, hipb), _dev(gw0, hipb)
    # conv: gw is logical [Nu][cv][4][4]; full-conv: logical [Nu][cv][4][4] as well (input channels first): one physical layout
    gb = torch.full((cv if full else Nu,), 0.25, device=hipb.device)
    hipb.prof_begin()
    if group is not None:
        hipb.wgrad_group_begin()
        group()
    _call(hipb, full, dimg, dlow, gw, gb, beta)
    if group is not None:
        hipb.wgrad_group_end()
    names = _wgrad_names(hipb.prof_end())
    return gw.permute(0, 2, 3, 1).contiguous().cpu(), gb.cpu(), names


def _check(hipb, case, full, beta):
    _, _, gw0, ref = _operands(case)
    got, gb, names = _run(hipb, case, full, beta, 3)
    pad, gb4, names4 = _run(hipb, case, full, beta, 4)
    assert len(names) == 1 and NEW in names[0], names
    assert names4 and not any(NEW in n for n in names4), names4
    assert torch.equal(got, pad[..., :3]), "3-channel form differs from the zero-padded 16-byte route: max %.3g" % float(
        (got - pad[..., :3]).abs().max())
    assert torch.equal(pad[..., 3], beta * _pad4(gw0)[..., 3])                # exactly 0
    assert torch.equal(gb, gb4[:gb.numel()])
    want = ref + beta * gw0.double()
    assert_close(got.double().numpy(), want.numpy(), TOL if beta else 2 * TOL, "bwd_weight(beta=%g) %s full=%s" % (beta, case, full))


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_conv_side(case, beta, hipb):
    _check(hipb, case, False, beta)


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("case", FULL_CASES, ids=str)
def test_full_conv_side(case, beta, hipb):
    _check(hipb, case, True, beta)


@pytest.mark.parametrize("case", [(2, 8, 8, 64), (2, 32, 32, 128)], ids=str)
def test_one_plane_mode(case, hipb):
    """the bf16-operand mode takes the form too (two stage buffers instead of one): the same bits as its 16-byte route on the padded
    tensor, and the mode's own bar against fp64 (1e-2: operands rounded to bf16, backend.set_mfma_mode)"""
    _, _, _, ref = _operands(case)
    hipb.set_mfma_mode("bf16")
    try:
        got, _, names = _run(hipb, case, False, 0.0, 3)
        pad, _, names4 = _run(hipb, case, False, 0.0, 4)
    finally:
        hipb.set_mfma_mode("f32_3xbf16")
    assert len(names) == 1 and NEW in names[0] and names[0].endswith("_bf16"), names
    assert names4 and not any(NEW in n for n in names4), names4
    assert torch.equal(got, pad[..., :3])
    assert torch.equal(pad[..., 3], torch.zeros_like(pad[..., 3]))
    assert_close(got.double().numpy(), ref.numpy(), 1e-2, "bwd_weight, bf16 operands %s" % (case,))


def test_other_channel_counts_keep_their_kernels(hipb):
    """27 image channels (the scalar gather) and 4 (16-byte loads) do not run under the new name"""
    for cv in (27, 4):
        x = _dev(_rand((2, 16, 16, cv), 8), hipb)
        gy = _dev(_rand((2, 8, 8, 64), 9), hipb)
        gw = _dev(torch.zeros(64, 4, 4, cv), hipb)
        hipb.prof_begin()
        hipb.conv2d_bwd_weight(x, gy, gw, None, 4, 2, 1, 0.0)
        names = _wgrad_names(hipb.prof_end())
        assert names and not any(NEW in n for n in names), (cv, names)


@pytest.mark.parametrize("case", [(2, 8, 8, 64), (2, 32, 32, 64)], ids=str)
def test_inside_a_weight_gradient_group(case, hipb):
    """a planes layer recorded first, then the 3-channel layer while the group is open: launched at once, its slabs behind the
    recorded ones, the same bits as outside a group; the planes layer's result is what it is alone"""
    big = (4, 32, 32, 64, 128)                  # B, H, W, Cin, Cout: 1024 low-resolution pixels, split over K
    xb = _dev(_rand((big[0], big[1], big[2], big[3]), 11), hipb)
    gb_ = _dev(_rand((big[0], big[1] // 2, big[2] // 2, big[4]), 12), hipb)
    xbp, gbp = hipb.planes_split(xb), hipb.planes_split(gb_)

    def planes_layer(out):
        hipb.conv2d_bwd_weight(xb, gb_, out, None, 4, 2, 1, 0.0, xbp, gbp)
    alone_big = _dev(torch.zeros(big[4], 4, 4, big[3]), hipb)
    planes_layer(alone_big)
    alone, _, _ = _run(hipb, case, False, 0.0, 3)
    in_group_big = _dev(torch.zeros(big[4], 4, 4, big[3]), hipb)
    got, _, names = _run(hipb, case, False, 0.0, 3, group=lambda: planes_layer(in_group_big))
    assert sum(NEW in n for n in names) == 1 and any(n.startswith("pwgrad_group") for n in names), names
    assert torch.equal(got, alone)
    assert torch.equal(in_group_big, alone_big)
