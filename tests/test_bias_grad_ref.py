"""CPU checks of tests/bias_grad_ref.py, the yardstick tests/test_gpu_bias_grad.py holds the bias-gradient kernels to:
  - fp32 / fp64 arithmetic in the kernels' own order (as written and with the epilogue contracted to a fused multiply-add) stays
    inside the derived bound on every random case — so the bound is not tighter than a correct kernel;
  - the exact cases are exact: the emulation reproduces the integer sums bit for bit, and a dropped row does not;
  - every case still reaches the geometry it is in the table for, asked of the library's own vf_bias_grad_plan (float4 route) and of
    the restated slab arithmetic (scalar route; pinned on the device by test_gpu_bias_grad.py)."""
import numpy as np
import pytest

import bias_grad_ref as R

BETAS = (0.0, 1.0, 0.5)


def _routes(case):
    return ("single", "multi") if case["route"] == "f4" else ("single",)


def _n_t(case):
    geo = R.f4_geom(case["P"], case["C"]) if case["route"] == "f4" else R.scalar_geom(case["P"], case["C"])
    return R.rows_per_thread(case["route"], geo)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c["id"])
def test_emulation_stays_inside_the_bound(case):
    P, C = case["P"], case["C"]
    g, gb0 = R.random_g(P, C, 11), R.random_gb0(C, 11)
    n_t = _n_t(case)
    for stage2 in _routes(case):
        for beta in BETAS:
            ref, bnd = R.ref64(g, gb0, beta), R.bound(g, gb0, beta, n_t)
            for fused in ((False, True) if beta else (False,)):
                got = R.emulate(g, gb0, beta, case["route"], stage2, fused)
                err = np.abs(got.astype(np.float64) - ref)
                assert (err <= bnd).all(), "%s %s beta %g fused %s: %.3f times the bound" % (case["id"], stage2, beta, fused,
                                                                                          float((err / bnd).max()))


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c["id"])
def test_exact_cases_are_exact(case):
    P, C = case["P"], case["C"]
    g, gb0 = R.exact_g(P, C, 5), R.exact_gb0(C, 5)
    assert np.abs(g).max() <= 8 and (g == np.round(g)).all() and (gb0 % 2 == 0).all()
    assert P * 8 + 8 < 2 ** 24
    for stage2 in _routes(case):
        for beta in BETAS:
            want = R.ref64(g, gb0, beta)
            assert (want == np.round(want)).all()
            for fused in (False, True):
                got = R.emulate(g, gb0, beta, case["route"], stage2, fused)
                assert got.dtype == np.float32 and (got.astype(np.float64) == want).all(), (case["id"], stage2, beta, fused)
    # the sums tell a dropped row from the full set in every column where that row is not zero
    if P > 1:
        short = R.ref64(g[:-1], gb0, 0.0)
        assert ((short != R.ref64(g, gb0, 0.0)) == (g[-1] != 0)).all()


def test_exact_generator_is_not_degenerate():
    g = R.exact_g(4096, 64, 5)
    assert set(np.unique(g)) == set(range(-8, 9))
    assert (g[:-1] != g[1:]).mean() > 0.9 and (g[:, :-1] != g[:, 1:]).mean() > 0.9      # neighbouring rows / columns differ
    assert len(set(R.exact_gb0(4000, 5))) == 9


def test_case_table_reaches_its_geometry():
    from video_filler_amd import _lib
    lib = _lib.load()
    seen = dict(cq=set(), gy=set(), gx=set(), nslab=set())
    for c in R.CASES:
        if c["route"] == "f4":
            geo = R.plan_from_library(lib, c["P"], c["C"])
            assert geo == R.f4_geom(c["P"], c["C"]), "%s: the restated plan %s is not the library's %s" % (c["id"], R.f4_geom(c["P"], c["C"]), geo)
        else:
            geo = R.scalar_geom(c["P"], c["C"])
        for k, v in c["reach"].items():
            assert geo[k] == v, "%s no longer reaches %s = %d (now %d)" % (c["id"], k, v, geo[k])
            seen[k].add(v)
    for k, need in list(R.REQUIRED_F4.items()) + list(R.REQUIRED_SCALAR.items()):
        assert need <= seen[k], "no case is in the table for %s in %s" % (k, sorted(need - seen[k]))
    # the cases named by their row tails: one row; rp - 1, rp, rp + 1 rows; a last block of ONE row for every float4 C
    for Cc in sorted({c["C"] for c in R.cases("f4")}):
        Ps = [c["P"] for c in R.cases("f4", Cc)]
        rp = R.plan_from_library(lib, 1, Cc)["rp"]
        assert {1, rp - 1, rp, rp + 1} - {0} <= set(Ps), (Cc, rp, Ps)
        tails = [P for P in Ps if P > 1 and P % R.plan_from_library(lib, P, Cc)["rows_per_block"] == 1]
        assert tails, "C = %d: no case whose last row block is one row long" % Cc
    for Cc in sorted({c["C"] for c in R.cases("scalar")}):
        assert {1, 255, 256, 257} <= {c["P"] for c in R.cases("scalar", Cc)}, Cc
    assert {c["C"] for c in R.cases("f4")} == {4, 12, 64, 256, 260, 512, 4000}
    assert {c["C"] for c in R.cases("scalar")} == {1, 3, 5, 6, 8}
    assert all(c["P"] * c["C"] <= 1 << 22 for c in R.CASES)


def test_multi_tables_mix_the_geometries():
    from video_filler_amd import _lib
    lib = _lib.load()
    assert sorted(R.MULTI_TABLES) == [1, 2, 13] and all(len(t) == n for n, t in R.MULTI_TABLES.items())
    t = R.MULTI_TABLES[13]
    geo = [R.plan_from_library(lib, P, Cc) for P, Cc, _ in t]
    one = [g["gx"] * g["gy"] == 1 for g in geo]
    big = [g["gx"] == 512 for g in geo]
    assert one[0] and one[-1], "a one-block layer stands first and last"
    assert any(big[i - 1] and one[i] and big[i + 1] for i in range(1, len(t) - 1)), "a one-block layer between two 512-slab layers"
    assert {g["gx"] for g in geo} >= {1, 15, 49, 64, 65, 128, 129, 512} and {g["gy"] for g in geo} == {1, 2, 16}
    assert {g["cq"] for g in geo} == {1, 4, 16, 64}
    for n, tab in R.MULTI_TABLES.items():
        assert all(P * Cc <= 1 << 22 and Cc % 4 == 0 for P, Cc, _ in tab)
        assert {b for _, _, b in R.MULTI_TABLES[13]} == {0.0, 1.0, 0.5}
