"""The three-plane products (mode f32_3xbf16) pinned BIT FOR BIT through the low planes: operands, the six-term reference and its
mutants (CPU only: numpy and torch, nothing of the project linked).  tests/test_planes3_ref.py holds this file to its own premises;
tests/test_gpu_planes3.py runs it on the device.

The rule.  Every fp32 operand is split by TRUNCATION into three bf16 planes (top 16 bits, subtract, repeat: hi + mid + lo == v),
and a product a . b is the sum of exactly six cross terms: hi.hi, hi.mid, mid.hi, hi.lo, lo.hi and mid.mid.  The "int" operands of
tests/nonsquare_cases.py sit whole in the high plane, and the 2e-5 bar of every random run lies above a lost second-order term
(tests/test_planes3_ref.py::test_the_gap keeps the figures): neither sees which planes meet in which term.

The operands.  Elements are 0 or +-1, +-(1 + 2^-8), +-(1 + 2^-8 + 2^-16): hi = +-1, mid = +-2^-8 or 0, lo = +-2^-16 or 0 — taken
from a restatement of the split (split_trunc), never from this recipe (1 + 2^-16 alone would put 2^-16 into the MID plane).  Every
one of the six terms of every product is a multiple of u = 2^-16.  One operand of each pass is dense; the other is thinned so that
an output element sees about TARGET non-zero products, drawn afresh per pass family:

  fwd  forward (x, w)                          w thinned to TARGET / (taps per output element)
  tr   data-gradient and scatter (gy, w)       w thinned likewise for the transposed pass
  wg   weight gradient (x, gy)                 gy thinned to TARGET / (low-resolution pixels), and to TARGET_BIAS elements per
                                               channel at most: the bias gradient of the same call sums them all

While the sum of |terms| of an output element — bias, bias_t and the beta = 1 starting value included — stays below CAP = 2^23 u
= 128, every partial sum is an fp32 number WHATEVER THE ORDER (inside an MFMA, across the six, across K steps, split-K slabs and
their reduce, col2im): the device result equals the six-term value in every bit.  Slope 0.25, the (Leaky)ReLU masks and
beta . gw0 with integer gw0 are exact.  rounded=True is the bf16 mode on the same operands: 1 + 2^-8 is an exact tie and rounds to
even (1.0), 1 + 2^-8 + 2^-16 rounds up to 1 + 2^-7; products are multiples of 2^-14, exact below 2^10.

MUTANTS are wrong forms of the rule, each as a reference: a term dropped, a second-order term taken twice in place of another, the
mid and lo planes of one operand swapped, a lo plane zeroed, the split rounded to nearest.  The GPU test names the mutant a
mismatching device tensor equals.

Out of scope — no planes there, the products are formed in fp32: the BatchNorm by-product group, the generic conv,
conv_thin_in / deconv_thin_out forward, vf_smallm.hip and wgrad_smallk_f32; and product mode 0."""
import functools

import numpy as np
import torch

import nonsquare_cases as NS
from nonsquare_cases import Case

UNIT = 2.0 ** -16
CAP = 128.0             # 2^23 units: below it every partial sum of multiples of UNIT is an fp32 number
CAP_ROUNDED = 1024.0    # the bf16 mode: multiples of 2^-14
TARGET = 56             # non-zero products per output element (mean; the spread and the epilogue's terms stay under CAP)
TARGET_BIAS = 80        # non-zero gradOutput elements per channel: the bias gradient sums them all (a full-conv's over 4 P pixels)
MAGNITUDES = (1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -16)
SHARES = (0.2, 0.3, 0.5)        # of the non-zero elements: a lo plane in half, a mid plane in four fifths

SIX = ((1, 1, 1), (1, 1, 0), (1, 0, 0))       # coef[i][j] of plane i of the first operand times plane j of the second
FAMILY = {"fwd": "fwd", "fwd_act": "fwd", "fwd_planes": "fwd", "pconv_gather": "fwd",
          "bwd_data": "tr", "bwd_data_act": "tr", "pconv_scatter": "tr", "pconv_scatter_mask": "tr", "pconv_scatter_fwd": "tr",
          "bwd_weight_b0": "wg", "bwd_weight_b1": "wg", "pwgrad_b0": "wg", "pwgrad_b1": "wg"}
KEYS = {"fwd": ("fwd", "fwd_act", "fwd_relu", "fwd_lrelu"), "tr": ("bwd_data", "bwd_data_act", "scatter_fwd"),
        "wg": ("gw_b0", "gw_b1", "gb_b0", "gb_b1")}
PRODUCT_KEYS = {"fwd": ("fwd",), "tr": ("bwd_data",), "wg": ("gw_b0",)}      # the bare products (bias aside): what a mutant moves

# the passes of the table's groups that form plane products (thin_in: only its weight gradient, k_wgrad on 3-channel pixels)
IN_SCOPE = {"igemm_conv": NS.CONV_PASSES, "igemm_full": NS.FULL_PASSES, "thin_in": ("bwd_weight_b0",), "thin_in_grad": ("bwd_data",),
            "col2im": ("fwd", "fwd_act", "bwd_data", "bwd_data_act"), "planes": NS.PLANES_PASSES, "patch_gather": ("pconv_gather",),
            "patch_scatter": ("pconv_scatter", "pconv_scatter_mask", "pconv_scatter_fwd")}


def _extra():
    """cases the non-square table does not hold, each at the smallest shape its route's dispatch rule allows (launch_igemm and
    wg_plan in vf_conv.hip)"""
    T = []
    ig = lambda *ps: {p: ("igemm_",) for p in ps}
    # the KLIN bottleneck walk (64 x 128 tile, K in memory order): conv k4 s1 p0 from a 4 x 4 map onto 1 x 1, and the data-gradient
    # of the full-conv back; 16 rows — more than the 8 vf_smallm.hip takes.  (Their weight gradient is wgrad_smallk_f32's: fp32.)
    T.append(Case("klin", False, 16, 4, 4, 64, 128, (4, 1, 0), ("fwd", "fwd_act"), routes=ig("fwd", "fwd_act")))
    T.append(Case("klin", True, 16, 1, 1, 128, 64, (4, 1, 0), ("bwd_data",), routes=ig("bwd_data")))
    # the double-buffered 64 x 64 tile (mode 3, 16-byte loads, a grid of at most 512 blocks): 256 GEMM rows onto 128 channels
    T.append(Case("db", False, 2, 16, 32, 64, 128, passes=("fwd", "fwd_act", "bwd_data"), routes=ig("fwd", "fwd_act", "bwd_data")))
    # k_wgrad under split-K: 512 low-resolution pixels are 16 K steps, the fewest wg_plan splits
    T.append(Case("wgrad_splitk", False, 4, 16, 32, 32, 64, passes=("bwd_weight_b0", "bwd_weight_b1"),
                  routes={"bwd_weight_b0": ("wgrad_",), "bwd_weight_b1": ("wgrad_",)}))
    # ---- the planes GEMM's kernels beyond the table's (launch_pconv, vf_pgemm.hip), by their full launch names.  Conv layers Cin -> Cout
    # whose gather pass runs from the input map and whose scatter passes run from the low-resolution one:
    SC = ("pconv_scatter", "pconv_scatter_mask", "pconv_scatter_fwd")
    pg = lambda B, H, W, Cin, Cout, passes, gather, scatter: Case(
        "pgemm", False, B, H, W, Cin, Cout, passes=passes, routes=dict({"pconv_gather": (gather,)}, **{p: (scatter,) for p in SC}))
    # whole 8 x 8 and 4 x 4 low-resolution maps in one 128-row tile: the patch kernel's m1 / m2 forms, gather and transposed
    T.append(pg(2, 16, 16, 64, 64, ("pconv_gather",) + SC, "pconv_patchg_128x64_t16_m1", "pconv_patchg_128x64_t4_m1"))
    T.append(pg(8, 8, 8, 64, 64, ("pconv_gather",) + SC, "pconv_patchg_128x64_t16_m2", "pconv_patchg_128x64_t4_m2"))
    # a 16 x 4 low-resolution map is no patch kernel's: the two-stage LDS-DMA kernel on 128-row tiles (the table's 192-row maps take
    # its 64-row form)
    T.append(pg(2, 32, 8, 64, 64, ("pconv_gather",) + SC, "pconv_dma_128x64x64_t16", "pconv_dma_128x64x64_t4"))
    # ... and its one-stage form from 512 blocks: 32 row tiles x 4 column tiles x 4 parity classes from a 16 x 8 map
    T.append(pg(32, 32, 16, 256, 64, ("pconv_scatter",), None, "pconv_dma_128x64x64_t4_1stage"))
    # four parity classes per block of k_pconv_patch_tr from 512 tiles: 256 row tiles x 2 column slices (the table's maps take two)
    T.append(pg(32, 64, 64, 128, 64, ("pconv_scatter_mask",), None, "pconv_patch_128x64_t4_c4"))
    # ---- k_pwgrad_group under split-K: 512 low-resolution pixels again, whole 128-row tiles, planes at hand
    T.append(Case("pwgrad_splitk", False, 4, 16, 32, 64, 128, passes=("pwgrad_b0", "pwgrad_b1")))
    # ---- k_igemm's largest tiles, taken from 1024 blocks of their own (launch_igemm): 131072 GEMM rows onto 128 channels for
    # 128 x 128, 65536 for 128 x 64; the thinnest K the 16-byte loads allow (16 channels: 8 K steps)
    T.append(Case("tile128", False, 16, 128, 256, 16, 128, passes=("fwd",), routes={"fwd": ("igemm_128x128_rowB_v2_bf16x3",)}))
    T.append(Case("tile128", False, 8, 128, 256, 16, 128, passes=("fwd",), routes={"fwd": ("igemm_128x64_rowB_v2_bf16x3",)}))
    for c in T:
        c.exact = c.group in ("pgemm", "tile128")        # routes hold whole launch names, not prefixes
    return T


def cases():
    return [c for c in NS.CASES if c.group in IN_SCOPE] + EXTRA


def passes(case):
    return tuple(p for p in case.passes if p in IN_SCOPE.get(case.group, case.passes))


EXTRA = _extra()
CASES = cases()


# ---------------------------------------------------------------------------------------------------------------- the split
def _f32(a):
    return np.ascontiguousarray(a.detach().numpy() if isinstance(a, torch.Tensor) else a, np.float32)


def split_trunc(a):
    """vf_trunc16 three times: the top 16 bits of the residual, subtracted exactly; nothing is left after three"""
    r = _f32(a).copy()
    planes = []
    for _ in range(3):
        h = (r.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
        planes.append(h)
        r = r - h
    assert not r.any(), "a residual is left after three planes"
    return planes


def rne16(a):
    u = _f32(a).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def split_rne(a):
    """the WRONG split (a mutant): each plane rounded to nearest even"""
    r = _f32(a).copy()
    planes = []
    for _ in range(3):
        h = rne16(r)
        planes.append(h)
        r = r - h
    return planes


def split_round1(a):
    """the bf16 mode: one plane, rounded to nearest even"""
    return [rne16(a)]


# ---------------------------------------------------------------------------------------------------------------- operands
def taps(case, transposed):
    """products per output element, at most: the contraction length of the forward pass or of its transpose"""
    full = case.full != transposed
    c = case.Cout if transposed else case.Cin
    per = (-(-case.k // case.s)) ** 2 if full else case.k * case.k
    return c * per


def _values(g, shape, density):
    n = int(np.prod(shape))
    mag = torch.tensor(MAGNITUDES, dtype=torch.float32)[torch.multinomial(torch.tensor(SHARES), n, True, generator=g)]
    sign = torch.randint(0, 2, (n,), generator=g).float() * 2 - 1
    keep = (torch.rand(n, generator=g) < density).float()
    return (mag * sign * keep).view(shape)


@functools.lru_cache(maxsize=None)
def _operands(idx):
    c = CASES[idx]
    g = torch.Generator().manual_seed(7000 + 31 * idx)
    xs, ys = (c.B, c.Cin, c.H, c.W), (c.B, c.Cout, c.Ho, c.Wo)
    P = c.low_res()[2]
    ints = NS._ints
    return {"fwd": dict(x=_values(g, xs, 1.0), w=_values(g, c.w_shape, TARGET / taps(c, False)), bias=ints(g, (c.Cout,), -4, 4)),
            "tr": dict(gy=_values(g, ys, 1.0), w=_values(g, c.w_shape, TARGET / taps(c, True)), bias_t=ints(g, (c.Cin,), -4, 4),
                       xact=ints(g, xs, -3, 3, nonzero=True)),
            "wg": dict(x=_values(g, xs, 1.0), gy=_values(g, ys, min(TARGET / P, TARGET_BIAS / (c.B * c.Ho * c.Wo))), gw0=ints(g, c.w_shape, -8, 8), gb0=ints(g, (c.Cout,), -8, 8))}


def _large(case):
    """the few cases whose tensors run to millions of elements are formed afresh at every call, not kept for the session"""
    return case.B * max(case.Cin * case.H * case.W, case.Cout * case.Ho * case.Wo) > 1 << 20


def operands(case):
    """family -> float32 CPU tensors, logical NCHW; read-only"""
    return (_operands.__wrapped__ if _large(case) else _operands)(CASES.index(case))


# ---------------------------------------------------------------------------------------------------------------- reference
def _planes64(split, t):
    return [torch.from_numpy(v.astype(np.float64)) for v in split(t)]


class Rule:
    """a form of the product: how the operands are split, and coef[i][j] times (plane i of the first) . (plane j of the second)"""

    def __init__(self, coef=SIX, split=split_trunc):
        self.coef, self.split = coef, split

    def product(self, f, a, b, magnitudes=False):
        """sum of coef[i][j] f(a_i, b_j) in fp64, formed as sum_i f(a_i, sum_j coef[i][j] b_j): one evaluation of f per plane of the
        first operand (the six-term value: f(hi, w) + f(mid, w_hi + w_mid) + f(lo, w_hi)); magnitudes: of |a_i|, |b_j| instead"""
        A, Bp = _planes64(self.split, a), _planes64(self.split, b)
        if magnitudes:
            A, Bp = [v.abs() for v in A], [v.abs() for v in Bp]
        out = None
        for i, ai in enumerate(A):
            row = [(cf, Bp[j]) for j, cf in enumerate(self.coef[i][:len(Bp)]) if cf]
            if row:
                t = f(ai, sum(cf * bj for cf, bj in row))
                out = t if out is None else out + t
        return out


class Terms:
    """the products f(a_i, b_j) of single planes, each formed once: any rule on the same split is a sum of them (every one exact in
    fp64), so the whole mutant table costs eight evaluations of f, not sixty"""

    def __init__(self, f, a, b, split=split_trunc):
        self.f, self.A, self.B, self.T = f, _planes64(split, a), _planes64(split, b), {}

    def value(self, coef):
        out = None
        for i, row in enumerate(coef):
            for j, cf in enumerate(row):
                if cf:
                    if (i, j) not in self.T:
                        self.T[i, j] = self.f(self.A[i], self.B[j])
                    out = cf * self.T[i, j] if out is None else out + cf * self.T[i, j]
        return out


def slotted(slots_a=(0, 1, 2), slots_b=(0, 1, 2)):
    """the six terms with plane slots_a[i] of the first operand standing in slot i (None: zeros), likewise the second: as coef"""
    cf = [[0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            if SIX[i][j] and slots_a[i] is not None and slots_b[j] is not None:
                cf[slots_a[i]][slots_b[j]] += SIX[i][j]
    return tuple(tuple(r) for r in cf)


TRUNC6 = Rule()
ROUND1 = Rule(((1,),), split_round1)
EXACT = Rule(((1,),), lambda a: [_f32(a)])        # the unsplit fp32 operands: the product itself


def _mutants():
    names = {(0, 0): "hi.hi", (0, 1): "hi.mid", (1, 0): "mid.hi", (0, 2): "hi.lo", (2, 0): "lo.hi", (1, 1): "mid.mid"}
    with_ = lambda kv: tuple(tuple(kv.get((i, j), SIX[i][j]) for j in range(3)) for i in range(3))
    M = {}
    for ij, n in names.items():
        M["%s dropped" % n] = Rule(with_({ij: 0}))
    second = [(0, 2), (2, 0), (1, 1)]
    for twice in second:
        for lost in second:
            if twice != lost:
                M["%s twice in place of %s" % (names[twice], names[lost])] = Rule(with_({twice: 2, lost: 0}))
    M["mid and lo swapped in the first operand"] = Rule(slotted(slots_a=(0, 2, 1)))
    M["mid and lo swapped in the second operand"] = Rule(slotted(slots_b=(0, 2, 1)))
    M["lo zeroed in the first operand"] = Rule(slotted(slots_a=(0, 1, None)))
    M["lo zeroed in the second operand"] = Rule(slotted(slots_b=(0, 1, None)))
    M["lo zeroed in both operands"] = Rule(slotted((0, 1, None), (0, 1, None)))
    M["split rounded to nearest"] = Rule(split=split_rne)
    return M


MUTANTS = _mutants()
SECOND_ORDER_DROPS = ("hi.lo dropped", "lo.hi dropped", "mid.mid dropped")


def mutant_values(f, a, b):
    """name -> the product under that mutant (a generator: one tensor alive at a time beside the shared single-plane products)"""
    terms = {split_trunc: Terms(f, a, b), split_rne: Terms(f, a, b, split_rne)}
    for name, rule in MUTANTS.items():
        yield name, terms[rule.split].value(rule.coef)


def bilinear(case, family):
    """(f, name of the first operand, name of the second) of a pass family; f maps fp64 tensors to the fp64 product"""
    fwd, tr = NS.conv_ops(case)
    if family == "fwd":
        return (lambda x, w: fwd(x, w)), "x", "w"
    if family == "tr":
        return (lambda gy, w: tr(gy, w)), "gy", "w"
    return (lambda x, gy: NS.weight_grad(case, x, gy)), "x", "gy"


def epilogues(case, family, o, v, mag=None):
    """every tensor the passes of one family write, from the value v of the family's product; mag (the same product of the
    magnitudes) -> "abs": the largest sum of |terms| behind an element of any of them"""
    d = lambda t: t.to(torch.float64)
    r = {}
    if family == "fwd":
        b = d(o["bias"]).view(1, -1, 1, 1)
        y = v + b
        r.update(fwd=y, fwd_act=NS.act(y, case.act), fwd_relu=NS.act(y, "relu"), fwd_lrelu=NS.act(y, "lrelu"))
        if mag is not None:
            r["abs"] = float((mag + b.abs()).max())
    elif family == "tr":
        bt = d(o["bias_t"]).view(1, -1, 1, 1)
        r.update(bwd_data=v, bwd_data_act=torch.where(d(o["xact"]) > 0, v, NS.SLOPE * v), scatter_fwd=NS.act(v + bt, "relu"))
        if mag is not None:
            r["abs"] = float((mag + bt.abs()).max())
    else:
        gb = d(o["gy"]).sum((0, 2, 3))      # the bias gradient stays fp32 on the unsplit gradOutput in every mode
        r.update(gw_b0=v, gw_b1=v + d(o["gw0"]), gb_b0=gb, gb_b1=gb + d(o["gb0"]))
        if mag is not None:
            r["abs"] = max(float((mag + d(o["gw0"]).abs()).max()), float((d(o["gy"]).abs().sum((0, 2, 3)) + d(o["gb0"]).abs()).max()))
    return r


def family_passes(case, family, o, rule=TRUNC6):
    f, na, nb = bilinear(case, family)
    return epilogues(case, family, o, rule.product(f, o[na], o[nb]), rule.product(f, o[na], o[nb], magnitudes=True))


@functools.lru_cache(maxsize=None)
def _reference(idx, family, rounded):
    return family_passes(CASES[idx], family, operands(CASES[idx])[family], ROUND1 if rounded else TRUNC6)


def reference(case, family, rounded=False):
    """fp64, computed once per (case, family, mode) and shared; read-only"""
    return (_reference.__wrapped__ if _large(case) else _reference)(CASES.index(case), family, bool(rounded))


def which_mutant(case, family, key, got):
    """the names of the mutants whose value of `key` the tensor `got` equals bit for bit"""
    o = operands(case)[family]
    f, na, nb = bilinear(case, family)
    return [n for n, v in mutant_values(f, o[na], o[nb]) if NS.exact_mismatch(got, epilogues(case, family, o, v)[key]) is None]


# ---------------------------------------------------------------------------------------------------------------- U^T V
class Outer:
    """the bottleneck pair's fused weight gradient (vf_wgrad_adam_outer): g = (1 / world) sum over ranks of U_r^T V_r, U_r [K][Nu],
    V_r [K][Ncols]; K >= 64, K % 16 == 0 takes the operand planes.  The contraction runs over world * K: U dense, V thinned to
    about OUTER_TARGET products where it is longer; the scale 1 / world is a power of two"""

    def __init__(self, world, K, Nu, Ncols):
        self.world, self.K, self.Nu, self.Ncols = world, K, Nu, Ncols
        self.id = "outer-world%d-K%d-%dx%d" % (world, K, Nu, Ncols)

    def f(self, U, V):
        return (U.t() @ V) / self.world


OUTER_TARGET = 84
OUTERS = [Outer(1, 64, 64, 128), Outer(1, 80, 70, 384), Outer(2, 64, 128, 256)]


@functools.lru_cache(maxsize=None)
def _outer(idx):
    oc = OUTERS[idx]
    g = torch.Generator().manual_seed(9000 + idx)
    rows = oc.world * oc.K
    U, V = _values(g, (rows, oc.Nu), 1.0), _values(g, (rows, oc.Ncols), min(1.0, OUTER_TARGET / rows))
    ref = TRUNC6.product(oc.f, U, V)
    return dict(U=U, V=V, g=ref, abs=float(TRUNC6.product(oc.f, U, V, magnitudes=True).max()) * oc.world)


def outer(oc):
    """U, V (all ranks' rows, rank-major), the six-term gradient g, and the largest sum of |terms| before the scale"""
    return _outer(OUTERS.index(oc))


def which_outer_mutant(oc, got):
    o = outer(oc)
    return [n for n, v in mutant_values(oc.f, o["U"], o["V"]) if NS.exact_mismatch(got, v) is None]
