"""tests/nonsquare_cases.py held to its own premises, on the CPU: the GPU test built on it (tests/test_gpu_nonsquare.py) cannot
pass vacuously.

  - the integer operands make every route exact: 8 significant bits, multiples of 2^-2, sums far below 2^24 ulps of 2^-4 — and a
    float32 evaluation on the CPU does equal the fp64 reference bit for bit;
  - an H / W mix-up shows: the same passes with the operands' channels-last bytes read as W x H maps differ from the reference in more
    than half of the elements, for every case of the table;
  - the comparison the GPU test uses rejects one element off by 2^-4, one NaN (an element no launch wrote), and the swapped reading;
  - every group of the table holds both orders of a non-square map."""
import numpy as np
import pytest
import torch

import nonsquare_cases as NS

IDS = [c.id for c in NS.CASES]
KEYS = ("fwd", "fwd_act", "fwd_relu", "fwd_lrelu", "bwd_data", "bwd_data_act", "scatter_fwd", "gw_b0", "gb_b0", "gw_b1", "gb_b1",
        "bn_fwd_sums", "bn_bwd", "bn_bwd_sums")


def test_case_ids_are_unique():
    assert len(set(IDS)) == len(IDS)


def _significant_bits(t):
    """bits from the leading one to the last set bit of |v| / 2^-2 (0 for 0)"""
    q = (t.double() * 4).abs()
    assert torch.equal(q, q.round()), "an operand is not a multiple of 2^-2"
    q = q.to(torch.int64).numpy()
    bits = 0
    for v in np.unique(q):
        v = int(v)
        if v:
            bits = max(bits, v.bit_length() - ((v & -v).bit_length() - 1))
    return bits


@pytest.mark.parametrize("case", NS.CASES, ids=IDS)
def test_integer_operands_make_every_route_exact(case):
    o = NS.operands(case, "int")
    for name, t in o.items():
        assert _significant_bits(t) <= 8, name
        assert torch.equal(NS.bf16_round(t), t), "%s: rounding to bf16 changes it" % name
    for name in ("xact", "bn_yact"):
        assert bool((o[name] != 0).all()), "%s holds a zero: the kink convention would matter" % name
    ref = NS.reference(case, "int")
    worst = max(float(ref[k].abs().max()) for k in KEYS)
    # every value and every partial sum of it is a multiple of 2^-4: exact in fp32 while 16 * |v| < 2^24.  (The BatchNorm sums
    # run over |terms|: a partial sum in any order stays below the sum of the magnitudes.)
    assert 16 * max(worst, ref["bn_abs_sums"]) < 2 ** 24, worst
    for k in KEYS:
        q = ref[k] * 16
        assert torch.equal(q, q.round()), "%s is not a multiple of 2^-4" % k
    # the same operations in float32 (another summation order than any kernel's, and than the fp64 evaluation's): the same bits
    f32 = NS.passes_of(case, o, torch.float32)
    for k in KEYS:
        assert f32[k].dtype == torch.float32
        assert NS.exact_mismatch(f32[k], ref[k]) is None, k
    # and the rounded-operand reference of the bf16 mode is the same reference
    rr = NS.reference(case, "int", rounded=True)
    for k in KEYS:
        assert torch.equal(rr[k], ref[k]), k


@pytest.mark.parametrize("case", NS.CASES, ids=IDS)
def test_a_height_width_mixup_shows(case):
    o = NS.operands(case, "int")
    ref = NS.reference(case, "int")
    sw = NS.swapped_passes(case, o)
    for k, t in sw.items():
        assert t.shape == ref[k].shape, k
        frac = float((t != ref[k]).double().mean())
        assert frac > 0.5, "%s: the swapped reading differs in only %.3f of the elements" % (k, frac)
        assert NS.exact_mismatch(t.float(), ref[k]) is not None


@pytest.mark.parametrize("case", [c for c in NS.CASES if c.group in ("igemm_conv", "thin_out", "generic_no_pow2")][::3],
                         ids=lambda c: c.id)
def test_comparison_helper_rejects_small_damage(case):
    ref = NS.reference(case, "int")
    for k in ("fwd", "bwd_data", "gw_b0"):
        good = ref[k].float()
        assert NS.exact_mismatch(good, ref[k]) is None
        for pos in (0, good.numel() // 2, good.numel() - 1):
            off = good.clone()
            off.view(-1)[pos] += 2.0 ** -4
            assert "1 of" in NS.exact_mismatch(off, ref[k])
            nan = good.clone()
            nan.view(-1)[pos] = float("nan")
            msg = NS.exact_mismatch(nan, ref[k])
            assert "1 of" in msg and "(1 NaN)" in msg
            assert not NS.rel_err(nan, ref[k]) <= 1.0, "a NaN passes the random run's bar"
        assert NS.exact_mismatch(good[:, :-1], ref[k]) is not None


def test_random_operands_and_bf16_rounding():
    c = NS.CASES[0]
    o = NS.operands(c, "rand")
    assert abs(float(o["w"].std()) - 0.05) < 0.01 and abs(float(o["x"].std()) - 1.0) < 0.1
    assert NS.operands(c, "rand") is o and NS.reference(c, "rand") is NS.reference(c, "rand")
    # round-to-nearest-even at the 8th significant bit: ties go to the even neighbour, both ways
    t = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0, 257.0, 259.0])
    assert NS.bf16_round(t).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.0, 256.0, 260.0]
    r, rr = NS.reference(c, "rand"), NS.reference(c, "rand", rounded=True)
    e = NS.rel_err(rr["fwd"], r["fwd"])
    assert 1e-5 < e < 1e-2, e      # operand rounding, 2^-9 relative per operand (tests/test_gpu_bf16.py's second bar)
    assert torch.equal(rr["gb_b0"], r["gb_b0"]), "the bias gradient is formed from the unrounded gradOutput"


def test_table_coverage():
    groups = {}
    for c in NS.CASES:
        assert c.H != c.W, c.id
        groups.setdefault(c.group, set()).add(c.H < c.W)
        assert set(c.routes) | set(c.refused) >= set(c.passes) - {"pwgrad_b0", "pwgrad_b1"}, c.id
        assert set(c.modes) <= set(NS.MODES) and 3 in c.modes
    for g, orders in groups.items():
        assert orders == {True, False} or g in NS.ONE_ORDER, "%s holds one order of its non-square maps only" % g
    # the groups and modes the table must hold
    want = {"igemm_conv": (3, 1, 0), "igemm_full": (3, 1, 0), "thin_in": (3,), "thin_in_grad": (3,), "thin_out": (3,), "col2im": (3,),
            "generic": (3, 0), "generic_no_pow2": (3, 0), "planes": (3, 1), "patch_gather": (3,), "patch_scatter": (3,), "bn": (3,)}
    assert set(groups) == set(want)
    for c in NS.CASES:
        assert c.modes == want[c.group], c.id
    maps = lambda g: sorted({(c.B, c.H, c.W) for c in NS.CASES if c.group == g})
    assert maps("igemm_conv") == maps("igemm_full") == maps("generic") == [(2, 8, 16), (3, 16, 4)]
    assert maps("planes") == maps("bn") == [(2, 16, 32), (3, 32, 8)]
    assert maps("thin_out") == maps("thin_in_grad") == [(2, 8, 16), (2, 16, 8)]
    assert maps("thin_in") == [(2, 16, 32), (2, 32, 16)] and maps("generic_no_pow2") == [(2, 6, 10), (2, 10, 6)]
    assert {(c.Cin, c.Cout) for c in NS.CASES if c.group == "planes"} == {(32, 64), (64, 128), (128, 64), (64, 33)}
    # the support rule mirrored here (which planes rows are run, which are asserted to be refused) has both outcomes in both modes
    pl = [c for c in NS.CASES if c.group == "planes"]
    for mode in (3, 1):
        for tr in (False, True):
            assert {NS.pconv_supported(mode, c, tr) for c in pl} == {True, False}
    assert {NS.pwgrad_route(m, c) for c in pl for m in (3, 1)} == {("pwgrad_group_",), ("wgrad_",)}


def test_net_chain_reference_runs_in_fp64():
    g = torch.Generator().manual_seed(5)
    shapes = [(64, 3, 4, 4), (64,), (128, 64, 4, 4), (128,), (128,), (128,), (64, 128, 4, 4), (64,), (64,), (64,),
              (64, 128, 4, 4), (128,), (128,), (128,), (128, 32, 4, 4), (32,), (32,), (32,), (32, 3, 4, 4), (3,)]
    params = [(torch.randn(s, generator=g, dtype=torch.float64) * 0.05).requires_grad_() for s in shapes]
    for shape in NS.NET_INPUTS:
        x = torch.randn(shape, generator=g, dtype=torch.float64, requires_grad=True)
        y = NS.torch_chain(params)(x)
        assert y.shape == shape and y.dtype == torch.float64
        y.backward(torch.ones_like(y))
        assert x.grad.shape == shape and all(p.grad is not None for p in params)
