"""tests/planes3_cases.py held to its own premises, on the CPU: the GPU test built on it (tests/test_gpu_planes3.py) cannot pass
vacuously.  For every (case, pass family) that test runs:

  - the restated truncation split gives the planes the recipe intends (hi +-1, mid +-2^-8 or 0, lo +-2^-16 or 0, one sign) and
    sums back bit for bit;
  - every term is a multiple of 2^-16 and the sum of |terms| behind every output element, epilogue included, is below 128 — the
    condition under which fp32 accumulation is exact in any order; the reference survives a round trip through float32;
  - the bf16 mode's reference on the same operands is exact likewise (multiples of 2^-14 below 2^10), and the ties went to even;
  - every mutant of the six-term rule differs from the reference in at least a quarter of the elements of every tensor the family's
    passes write (weight gradients, activations behind a ReLU included);
  - THE GAP: on the table's "rand" operands a lost second-order term moves the product by less than the 2e-5 bar of every random
    run in the suite — which is why this file exists."""
import numpy as np
import pytest
import torch

import nonsquare_cases as NS
import planes3_cases as P3

IDS = [c.id for c in P3.CASES]
MIN_SHARE = 0.25
GAP = {}
SHARE = {}      # (case, family) -> (the lowest share of elements a mutant moves, the largest sum of |terms|)


def families(case):
    return sorted({P3.FAMILY[p] for p in P3.passes(case)})


FAMS = [pytest.param(c, f, id="%s-%s" % (c.id, f)) for c in P3.CASES for f in families(c)]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if SHARE:
        k = min(SHARE, key=lambda k: SHARE[k][0])
        print("the lowest share of elements a mutant moves: %.3f at %s (bar %.2f)" % (SHARE[k][0], k, MIN_SHARE))
        k = max(SHARE, key=lambda k: SHARE[k][1])
        print("the largest sum of |terms| behind an element: %.1f at %s (cap %.0f)" % (SHARE[k][1], k, P3.CAP))
    for name in sorted({n for v in GAP.values() for n in v}):
        worst = max((v[name], k) for k, v in GAP.items() if name in v)
        print("the gap, %s: at most %.3e of the max-norm (bar 2e-5) at %s" % (name, worst[0], worst[1]))


def test_case_ids_are_unique_and_in_scope():
    assert len(set(IDS)) == len(IDS)
    table = {c.group for c in NS.CASES}
    assert set(P3.IN_SCOPE) <= table and table - set(P3.IN_SCOPE) == {"thin_out", "generic", "generic_no_pow2", "bn"}
    for c in P3.CASES:
        assert P3.passes(c) and all(p in P3.FAMILY for p in P3.passes(c)), c.id
        assert 3 in c.modes
    # every table case of an in-scope group rides along: both checks on one launch set
    assert [c for c in NS.CASES if c.group in P3.IN_SCOPE] == P3.CASES[:len(P3.CASES) - len(P3.EXTRA)]


def test_split_restatement():
    t = np.array([1.0, 1 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -16, -(1 + 2.0 ** -8 + 2.0 ** -16), 1 + 2.0 ** -16, 0.0, 3.14159274], np.float32)
    hi, mid, lo = P3.split_trunc(t)
    assert hi.tolist()[:6] == [1.0, 1.0, 1.0, -1.0, 1.0, 0.0]
    assert mid.tolist()[:6] == [0.0, 2.0 ** -8, 2.0 ** -8, -2.0 ** -8, 2.0 ** -16, 0.0]      # 1 + 2^-16: the residual is a MID plane
    assert lo.tolist()[:6] == [0.0, 0.0, 2.0 ** -16, -2.0 ** -16, 0.0, 0.0]
    assert np.array_equal(hi + mid + lo, t)
    for p in (hi, mid, lo):
        assert not (p.view(np.uint32) & 0xFFFF).any(), "a plane is not a bf16 number"
    # rounding instead: the tie goes to even, the third value rounds up and its mid plane turns negative
    assert P3.rne16(t)[:4].tolist() == [1.0, 1.0, 1 + 2.0 ** -7, -(1 + 2.0 ** -7)]
    rh, rm, rl = P3.split_rne(t)
    assert np.array_equal(rh + rm + rl, t) and rm[2] == -(2.0 ** -8) + 2.0 ** -16 and rl[2] == 0
    g = np.random.default_rng(3).standard_normal(4096).astype(np.float32)
    assert np.array_equal(np.sum(P3.split_trunc(g), 0, dtype=np.float64), g.astype(np.float64))


@pytest.mark.parametrize("case,family", FAMS)
def test_operands_reference_and_mutants(case, family):
    o = P3.operands(case)[family]
    _, na, nb = P3.bilinear(case, family)
    # ---- the planes the recipe intends, from the split's restatement
    for name in (na, nb):
        t = o[name].numpy()
        hi, mid, lo = P3.split_trunc(t)
        assert np.array_equal(hi + mid + lo, t), name
        assert np.isin(np.abs(hi), (0.0, 1.0)).all() and np.isin(np.abs(mid), (0.0, 2.0 ** -8)).all() and np.isin(np.abs(lo), (0.0, 2.0 ** -16)).all()
        assert (np.sign(mid) * np.sign(hi) >= 0).all() and (np.sign(lo) * np.sign(mid) > 0)[lo != 0].all(), "%s: a plane changes sign" % name
        nz = (t != 0).sum()
        assert (mid != 0).sum() > 0.7 * nz and (lo != 0).sum() > 0.4 * nz, "%s: too few low planes" % name
    dense = o[na]
    assert bool((dense != 0).all()), "%s is the dense operand" % na
    for name, t in o.items():
        if name not in (na, nb):
            assert torch.equal(t, t.round()), "%s is not integer-valued" % name
    assert bool((o["xact"] != 0).all()) if family == "tr" else True
    # ---- six terms, each a multiple of 2^-16 (plane i times plane j with i + j <= 2), and the cap
    ref = P3.reference(case, family)
    assert ref["abs"] < P3.CAP, "sum of |terms| %.1f reaches the cap" % ref["abs"]
    assert ref["abs"] > 8, "hardly any product behind an element"
    for k in P3.KEYS[family]:
        # the slope of a (Leaky)ReLU is one exact scaling of the finished sum, after the last addition
        q = ref[k] / (P3.UNIT if k in ("fwd", "bwd_data") or k[:2] in ("gw", "gb") else P3.UNIT * NS.SLOPE)
        assert torch.equal(q, q.round()), "%s is not a multiple of 2^-16" % k
        assert ref[k].dtype == torch.float64 and torch.equal(ref[k].float().double(), ref[k]), "%s is not an fp32 tensor" % k
        assert NS.exact_mismatch(ref[k].float(), ref[k]) is None
    # the six-term value is not the product: the low planes carry weight here
    exact = P3.family_passes(case, family, o, P3.EXACT)
    assert not torch.equal(exact[P3.PRODUCT_KEYS[family][0]], ref[P3.PRODUCT_KEYS[family][0]])
    # ---- the bf16 mode on the same operands
    if 1 in case.modes:
        rr = P3.reference(case, family, rounded=True)
        assert rr["abs"] < P3.CAP_ROUNDED
        for k in P3.KEYS[family]:
            q = rr[k] * (2.0 ** 16 if k.startswith("gb_") else 2.0 ** 14 / NS.SLOPE)     # the bias gradient sums the unrounded gradOutput
            assert torch.equal(q, q.round()) and torch.equal(rr[k].float().double(), rr[k]), k
        for name in (na, nb):
            t = o[name]
            r = torch.from_numpy(P3.rne16(t))
            assert torch.equal(r, NS.bf16_round(t))
            a = t.abs()
            assert bool((r.abs()[a == 1 + 2.0 ** -8] == 1.0).all()), "a tie did not go to even"
            assert bool((r.abs()[a == 1 + 2.0 ** -8 + 2.0 ** -16] == 1 + 2.0 ** -7).all())
            assert int((a == 1 + 2.0 ** -8).sum()) > 0
        k = P3.PRODUCT_KEYS[family][0]
        assert float((rr[k] != ref[k]).double().mean()) >= MIN_SHARE
    # ---- every mutant shows, in every tensor the passes of this family compare (the bias gradient is no product)
    f = P3.bilinear(case, family)[0]
    assert torch.equal(P3.Terms(f, o[na], o[nb]).value(P3.SIX), ref[P3.PRODUCT_KEYS[family][0]] - (
        o["bias"].double().view(1, -1, 1, 1) if family == "fwd" else 0)), "the two forms of the six-term sum differ"
    keys = [k for k in P3.KEYS[family] if not k.startswith("gb_")]
    low, lowest = [], 1.0
    for name, v in P3.mutant_values(f, o[na], o[nb]):
        m = P3.epilogues(case, family, o, v)
        for k in keys:
            share = float((m[k] != ref[k]).double().mean())
            lowest = min(lowest, share)
            if share < MIN_SHARE:
                low.append("%s in %s: %.3f" % (name, k, share))
    assert not low, "mutants that differ in less than %.2f of the elements: %s" % (MIN_SHARE, "; ".join(low))
    SHARE["%s %s" % (case.id, family)] = (lowest, ref["abs"])
    # the naming the GPU test's message relies on (on the small cases: it forms every mutant again)
    if ref[keys[0]].numel() > 1 << 20:
        return
    assert P3.which_mutant(case, family, keys[0], ref[keys[0]].float()) == []
    one =P3.epilogues(case, family, o, P3.Terms(f, o[na], o[nb]).value(P3.MUTANTS["mid.mid dropped"].coef))[keys[0]].float()
    assert "mid.mid dropped" in P3.which_mutant(case, family, keys[0], one)


@pytest.mark.parametrize("oc", P3.OUTERS, ids=lambda oc: oc.id)
def test_outer_product_operands(oc):
    o = P3.outer(oc)
    assert o["U"].shape == (oc.world * oc.K, oc.Nu) and o["V"].shape == (oc.world * oc.K, oc.Ncols)
    assert oc.K >= 64 and oc.K % 16 == 0, "below 64 rows, or off a multiple of 16, the fused kernel forms fp32 products: no planes"
    assert bool((o["U"] != 0).all())
    for t in (o["U"], o["V"]):
        hi, mid, lo = P3.split_trunc(t.numpy())
        assert np.isin(np.abs(hi), (0.0, 1.0)).all() and np.isin(np.abs(mid), (0.0, 2.0 ** -8)).all() and np.isin(np.abs(lo), (0.0, 2.0 ** -16)).all()
    assert 32 < o["abs"] < P3.CAP, o["abs"]
    q = o["g"] / (P3.UNIT / oc.world)
    assert torch.equal(q, q.round()) and torch.equal(o["g"].float().double(), o["g"])
    lowest = 1.0
    for name, v in P3.mutant_values(oc.f, o["U"], o["V"]):
        share = float((v != o["g"]).double().mean())
        lowest = min(lowest, share)
        assert share >= MIN_SHARE, "%s: %.3f" % (name, share)
    SHARE[oc.id] = (lowest, o["abs"])
    assert P3.which_outer_mutant(oc, o["g"].float()) == []


TABLE = [c for c in P3.CASES if c in NS.CASES]


@pytest.mark.parametrize("case", TABLE, ids=[c.id for c in TABLE])
def test_the_gap(case):
    """the table's "rand" operands: the six-term product is fp32-grade, and so — under the 2e-5 bar — is every form of it that
    loses one second-order term"""
    o = NS.operands(case, "rand")
    for family in families(case):
        f, na, nb = P3.bilinear(case, family)
        exact = P3.EXACT.product(f, o[na], o[nb])
        scale = float(exact.abs().max())
        err = lambda rule: float((rule.product(f, o[na], o[nb]) - exact).abs().max()) / scale
        e6 = err(P3.TRUNC6)
        assert e6 < 5e-7, "%s: the six-term product is %.3e from the product" % (family, e6)
        fig = GAP.setdefault("%s %s" % (case.id, family), {"six terms": e6})
        for name in P3.SECOND_ORDER_DROPS:
            fig[name] = e = err(P3.MUTANTS[name])
            assert 10 * e6 < e < 2e-5, "%s, %s: %.3e" % (family, name, e)
        for name in ("mid and lo swapped in the first operand", "mid and lo swapped in the second operand"):
            fig[name] = err(P3.MUTANTS[name])       # reported; the issue's figure for it was 1.2e-5
        print("%s %s: %s" % (case.id, family, ", ".join("%s %.2e" % kv for kv in fig.items())))
