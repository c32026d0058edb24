"""The three-plane products of every conv kernel BIT FOR BIT through the low planes (tests/planes3_cases.py: the operands, the
six-term reference, its mutants; tests/test_planes3_ref.py: why this test cannot pass vacuously).

Operands whose truncation split is hi = +-1, mid = +-2^-8 or 0, lo = +-2^-16 or 0, thinned so that every sum of |terms| stays below
2^23 units of 2^-16: fp32 accumulation is exact in any order, so whichever kernel, tile, split count or summation order served a
pass, its result equals hi.hi + hi.mid + mid.hi + hi.lo + lo.hi + mid.mid in every bit of every element.  THERE IS NO TOLERANCE IN
THIS FILE.  A mismatch names the wrong form of the rule (a dropped term, swapped planes, a rounded split ...) the device tensor
equals, where it equals one.  In the bf16 mode the same operands are held to the rounded-operand reference, ties to even.

The passes run through tests/test_gpu_nonsquare.py's Run: guarded NaN-filled outputs, guard tails, the route asserted from the
library's launch list, (case, mode, pass, route) printed — pytest -rP shows the table, and the module ends with the launch names
reached and the ones it leaves out."""
import pytest
import torch

import nonsquare_cases as NS
import planes3_cases as P3
from helpers import guarded, untouched, workspace
from test_gpu_nonsquare import Run, dev, g_act, in_mode      # noqa: F401  (in_mode is a fixture)

pytestmark = pytest.mark.gpu

REACHED = {}        # launch name -> the (case, mode, pass) that reached it
# in scope, not reached, and why
NOT_REACHED = {
    "igemm_128x128_kmajorB_* / igemm_128x64_kmajorB_*": "the largest tiles on the TRANSPOSED passes: as many blocks again in four parity "
                                                        "classes; their row-major forms are reached, and K-major weights on every other tile",
}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("launch names reached, %d:" % len(REACHED))
    for name in sorted(REACHED):
        print("    %-44s %d passes, e.g. %s" % (name, len(REACHED[name]), sorted(REACHED[name])[0]))
    for name, why in NOT_REACHED.items():
        print("not reached: %s — %s" % (name, why))


def note(names, what):
    for n in names:
        REACHED.setdefault(n, set()).add(what)


class Run3(Run):
    """Run on the planes3 operands: each pass takes the operands and the reference of its family"""

    def __init__(self, b, case, mode):
        self.b, self.c, self.mode, self.kind, self.tol = b, case, mode, "planes3", None
        self.routes = []

    def run(self):
        c = self.c
        for pname in P3.passes(c):
            self.family = P3.FAMILY[pname]
            self.d = {k: dev(self.b, v) for k, v in P3.operands(c)[self.family].items()}
            self.ref = P3.reference(c, self.family, rounded=(self.mode == 1))
            self._unsupported = False
            getattr(self, "p_" + pname.replace("_b0", "").replace("_b1", ""))(pname)
        for pname, names in self.routes:
            note(names, "%s mode %d %s" % (c.id, self.mode, pname))
        return self

    def same(self, got, key, what, tol=None):
        msg = NS.exact_mismatch(got, self.ref[key])
        if msg is None:
            return
        if self.mode == 3 and not key.startswith("gb_"):
            eq = P3.which_mutant(self.c, self.family, key, got)
            msg += "; the device tensor equals, bit for bit: %s" % (", ".join(eq) if eq else "no mutant of the six-term rule")
        assert False, "%s mode %d %s: %s" % (self.c.id, self.mode, what, msg)

    def launch(self, pname, fn, *bufs):
        ran = super().launch(pname, fn, *bufs)
        if ran and getattr(self.c, "exact", False):
            names, want = self.routes[-1][1], self.c.routes[pname]
            assert set(want) & set(names), "%s %s: launches %s, not %s" % (self.c.id, pname, names, want)
        return ran


TABLE = [pytest.param(c, m, id="%s-mode%d" % (c.id, m)) for c in P3.CASES if c in NS.CASES for m in c.modes if m in (3, 1)]


@pytest.mark.parametrize("case,mode", TABLE)
def test_table(case, mode, hipb, in_mode):
    """the non-square table's maps, so that both checks ride on one launch set: mode 3 against the six-term value, mode 1 against
    the rounded-operand product"""
    in_mode(mode)
    Run3(hipb, case, mode).run()


def extra(group):
    return [c for c in P3.EXTRA if c.group == group]


@pytest.mark.parametrize("split", [True, False], ids=["split-K", "one-range"])
@pytest.mark.parametrize("case", extra("klin") + extra("db"), ids=lambda c: c.id)
def test_igemm_forms(case, split, hipb, in_mode):
    """k_igemm's memory-order walk (KLIN) and its double-buffered schedule, each under split-K with the slab reduce and — the
    workspace taken away — in one K range"""
    in_mode(3)
    if split:
        r = Run3(hipb, case, 3).run()
    else:
        with workspace(hipb, 0):
            r = Run3(hipb, case, 3).run()
    for pname, names in r.routes:
        assert ("slab_reduce_igemm" in names) == split, "%s %s: %s" % (case.id, pname, names)
        if case.group == "klin":      # launch_igemm: 64 x 128 tile, row-major weights, 16-byte loads and more than one tap are the KLIN walk
            assert "igemm_64x128_rowB_v2_bf16x3" in names, names
        elif pname.startswith("fwd"):
            assert any(n.startswith("igemm_64x64_") and n.endswith("_v2_bf16x3_db") for n in names), names


@pytest.mark.parametrize("split", [True, False], ids=["split-K", "one-range"])
@pytest.mark.parametrize("case", extra("wgrad_splitk") + extra("pwgrad_splitk"), ids=lambda c: c.id)
def test_wgrad_split_k(case, split, hipb, in_mode):
    """k_wgrad and k_pwgrad_group over 16 K steps: two K ranges and their slab reduce (beta = 0 and 1 through the reduce), or — a
    workspace that holds the bias-gradient partials but not two slabs — one range (beta in the kernel's epilogue)"""
    in_mode(3)
    slab = 4 * case.Cout * 16 * case.Cin
    kernel, reduce = (("pwgrad_group_128x128x32", "slab_reduce_wgrad_group") if case.group == "pwgrad_splitk" else
                      ("wgrad_64x128_bf16x3", "slab_reduce_wgrad"))
    if split:
        r = Run3(hipb, case, 3).run()
    else:
        with workspace(hipb, slab - 1024):
            r = Run3(hipb, case, 3).run()
    assert r.routes
    for pname, names in r.routes:
        assert (reduce in names) == split and kernel in names, "%s: %s" % (pname, names)


@pytest.mark.parametrize("case", extra("tile128"), ids=lambda c: c.id)
def test_igemm_largest_tiles(case, hipb, in_mode):
    """the 128 x 128 and 128 x 64 tiles of k_igemm (single-buffered three-plane stages), by their whole launch names"""
    in_mode(3)
    Run3(hipb, case, 3).run()


@pytest.mark.parametrize("case", extra("pgemm"), ids=lambda c: c.id)
def test_pgemm_kernels(case, hipb, in_mode):
    """the planes GEMM's kernels the table's maps do not take, each by its whole launch name (Run3.launch)"""
    in_mode(3)
    Run3(hipb, case, 3).run()


# ---------------------------------------------------------------------------------------------------------------- groups
class Layer:
    """one weight gradient of a group: guarded outputs, the call, the comparison with the case's six-term reference"""

    def __init__(self, b, case, beta, planes):
        self.b, self.c, self.beta = b, case, beta
        o = P3.operands(case)["wg"]
        self.x, self.gy = dev(b, o["x"]), dev(b, o["gy"])
        self.gw, self.gwbuf = g_act(b, *case.w_shape)
        self.gbbuf = guarded(b, case.Cout)
        self.gb = self.gbbuf[:case.Cout]
        if beta:
            self.gw.copy_(dev(b, o["gw0"]))
            self.gb.copy_(o["gb0"].to(b.device))
        self.kw = dict(x_planes=b.planes_split(self.x), gy_planes=b.planes_split(self.gy)) if planes else {}

    def call(self):
        fn = self.b.deconv2d_bwd_weight if self.c.full else self.b.conv2d_bwd_weight
        fn(self.x, self.gy, self.gw, self.gb, self.c.k, self.c.s, self.c.p, float(self.beta), **self.kw)

    def check(self, what):
        c, ref = self.c, P3.reference(self.c, "wg")
        assert untouched(self.gwbuf, self.gw.numel()) and untouched(self.gbbuf, c.Cout), "%s %s: a kernel wrote past its output" % (c.id, what)
        for got, key in ((self.gw, "gw_b%d" % self.beta), (self.gb, "gb_b%d" % self.beta)):
            msg = NS.exact_mismatch(got, ref[key])
            if msg is not None and key.startswith("gw_"):
                eq = P3.which_mutant(c, "wg", key, got)
                msg += "; the device tensor equals, bit for bit: %s" % (", ".join(eq) if eq else "no mutant of the six-term rule")
            assert msg is None, "%s %s %s: %s" % (c.id, what, key, msg)


def table_case(group, B, H, W, Cin, Cout):
    c, = [c for c in P3.CASES if (c.group, c.B, c.H, c.W, c.Cin, c.Cout, c.full) == (group, B, H, W, Cin, Cout, False)]
    return c


def grouped(b, layers, what):
    b.prof_begin()
    try:
        b.wgrad_group_begin()
        for layer in layers:
            layer.call()
        b.wgrad_group_end()
    finally:
        names = sorted(b.prof_end())
    b.synchronize()
    for layer in layers:
        layer.check(what)
    note(names, what)
    print("(%s: %s, %s)" % (what, " + ".join(l.c.id for l in layers), "+".join(names)))
    return names


@pytest.mark.parametrize("beta", [0, 1])
def test_planes_weight_gradient_group(beta, hipb, in_mode):
    """vf_wgrad_group_begin / _end around a 128-row and a 64-row planes layer: ONE k_pwgrad_group launch with both tile forms"""
    in_mode(3)
    layers = [Layer(hipb, table_case("planes", 2, 16, 32, 64, 128), beta, True), Layer(hipb, table_case("planes", 2, 16, 32, 128, 64), beta, True)]
    names = grouped(hipb, layers, "planes group beta %d" % beta)
    assert "pwgrad_group_64+128x128x32" in names and not any(n.startswith("wgrad_") for n in names), names


@pytest.mark.parametrize("beta", [0, 1])
def test_fp32_fed_weight_gradient_group(beta, hipb, in_mode):
    """the same walk without planes: k_wgrad_group splits the fp32 operands inside the kernel, a 128-row and a 64-row layer"""
    in_mode(3)
    layers = [Layer(hipb, table_case("igemm_conv", 2, 8, 16, 64, 128), beta, False), Layer(hipb, table_case("planes", 2, 16, 32, 32, 64), beta, False)]
    names = grouped(hipb, layers, "fp32-fed group beta %d" % beta)
    assert any(n.startswith("wgrad_group_") and n.endswith("_bf16x3") for n in names), names
    assert not any(n.startswith(("pwgrad_", "wgrad_64", "wgrad_128")) for n in names), names


# ---------------------------------------------------------------------------------------------------------------- U^T V + Adam
@pytest.mark.parametrize("oc", P3.OUTERS, ids=lambda oc: oc.id)
def test_fused_adam_gradient(oc, hipb, in_mode):
    """vf_wgrad_adam_outer (and its gathered form: two ranks' operands side by side, the mean of their gradients) from 64 rows on:
    operands pre-split into planes in fragment order, six terms on the bf16 pipe — the stored gradient is U^T V's six-term value"""
    in_mode(3)
    b, o = hipb, P3.outer(oc)
    K, Nu, Ncols, n = oc.K, oc.Nu, oc.Ncols, oc.Nu * oc.Ncols
    assert b.lib.vf_wgrad_adam_outer_supported(K, Nu, Ncols) == 1
    gen = torch.Generator().manual_seed(5)
    x, m, v = (torch.randn(n, generator=gen).to(b.device), (0.1 * torch.randn(n, generator=gen)).to(b.device),
               (0.01 * torch.rand(n, generator=gen)).to(b.device))
    t = b.zeros(2, dtype=torch.int32)
    gbuf = guarded(b, n)
    b.adam_prep(2e-4, 0.5, 0.999, t)
    b.prof_begin()
    try:
        if oc.world == 1:
            b.wgrad_adam_outer(o["U"].to(b.device), o["V"].to(b.device), x, m, v, gbuf[:n], 0.5, 0.999, 1e-8, t)
        else:
            pad4 = lambda k: (k + 3) & ~3
            v_off = pad4(K * Nu)
            seg = v_off + pad4(K * Ncols) + 8
            host = torch.zeros(oc.world * seg)
            for r in range(oc.world):
                host[r * seg:r * seg + K * Nu] = o["U"][r * K:(r + 1) * K].reshape(-1)
                host[r * seg + v_off:r * seg + v_off + K * Ncols] = o["V"][r * K:(r + 1) * K].reshape(-1)
            b.wgrad_adam_outer_gathered(host.to(b.device), 0, v_off, oc.world, K, seg, Nu, Ncols, x, m, v, gbuf[:n], 0.5, 0.999, 1e-8, t)
    finally:
        names = sorted(b.prof_end())
    b.synchronize()
    note(names, oc.id)
    print("(%s, %s)" % (oc.id, "+".join(names)))
    assert "adam_fused_operand_planes" in names, names
    assert untouched(gbuf, n), "a kernel wrote past the stored gradient"
    got = gbuf[:n].view(Nu, Ncols)
    msg = NS.exact_mismatch(got, o["g"])
    if msg is not None:
        eq = P3.which_outer_mutant(oc, got)
        msg += "; the device tensor equals, bit for bit: %s" % (", ".join(eq) if eq else "no mutant of the six-term rule")
    assert msg is None, "%s: %s" % (oc.id, msg)
