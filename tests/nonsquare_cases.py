"""Every conv route on NON-SQUARE maps: the case table, the operands and an fp64 reference (CPU only: numpy and torch, nothing of
the project linked).  tests/test_nonsquare_ref.py holds this file to its own premises; tests/test_gpu_nonsquare.py runs the
table on the device.

The kernels carry H and W separately (lgMh / lgMw, tiles_x / tiles_y, ilog2(Hi) / ilog2(Wi), Wo % 16 && Ho % 8); a row / column
decode that takes the wrong extent is invisible on a square map.  Two sets of operands per case:

  "int"   small integers: activations and gradOutput in {-3..3}, weights in {-2..2} x 0.25, bias in {-4..4}, the beta = 1
          starting values in {-8..8}, mask tensors in {-3..-1, 1..3} (no zero: the kink convention cannot matter), BatchNorm shifts
          in {-2..2}, slope 0.25.  Every operand has at most 8 significant bits: the three-plane split puts it whole into the high
          plane and rounding to bf16 leaves it unchanged.  Every product and partial sum is a multiple of 2^-4 far below 2^20: fp32
          accumulation is exact in ANY order (split-K and slab reduce included).  So the device result must equal the fp64 reference
          bit for bit, in every element, in the product modes 3, 1 and 0 alike — no tolerance.
  "rand"  randn, weights x 0.05: the suite's usual operands at the suite's usual bars.

A case is one LAYER on the input map (B, H, W) of that layer, with the passes its group runs.  The maps are the smallest that
reach each route, both orders of every non-square map (H < W and H > W) in every group; ONE_ORDER names the exceptions."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

SLOPE = 0.25
MODES = {3: "f32_3xbf16", 1: "bf16", 0: "f32"}
TOL = {3: 2e-5, 0: 2e-5, 1: 3e-5}      # the random run: test_gpu_conv_sweep.py / test_gpu_workspace.py; test_gpu_bf16.py (rounded operands)
TOL_BIAS_GRAD = 2e-5                   # the bias gradient stays fp32 in every mode (test_gpu_bf16.py)

CONV_PASSES = ("fwd", "fwd_act", "fwd_planes", "bwd_data", "bwd_data_act", "bwd_weight_b0", "bwd_weight_b1")
FULL_PASSES = ("fwd", "fwd_act", "bwd_data", "bwd_weight_b0", "bwd_weight_b1")
GENERIC_PASSES = ("fwd", "bwd_data", "bwd_weight_b0", "bwd_weight_b1")
PLANES_PASSES = ("pconv_gather", "pconv_scatter", "pconv_scatter_mask", "pconv_scatter_fwd", "pwgrad_b0", "pwgrad_b1")


class Case:
    """one layer: conv (weight [Cout][Cin][k][k]) or full-conv (weight [Cin][Cout][k][k]) on the input map B x H x W"""

    def __init__(self, group, full, B, H, W, Cin, Cout, geo=(4, 2, 1), passes=(), modes=(3,), routes=None, refused=None):
        self.group, self.full, self.B, self.H, self.W, self.Cin, self.Cout = group, full, B, H, W, Cin, Cout
        self.k, self.s, self.p = geo
        self.passes, self.modes = tuple(passes), tuple(modes)
        self.routes = dict(routes or {})        # pass -> prefixes, one of which a launch of that pass must carry
        self.refused = dict(refused or {})      # pass -> part of the message the library refuses it with, before any launch
        self.act = "relu" if full else "lrelu"  # the fused activation of "fwd_act"
        k, s, p = geo
        self.Ho, self.Wo = ((H - 1) * s - 2 * p + k, (W - 1) * s - 2 * p + k) if full else ((H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1)

    @property
    def id(self):
        return "%s-%s-B%d-%dx%d-%dto%d-k%ds%dp%d" % (self.group, "full" if self.full else "conv", self.B, self.H, self.W, self.Cin,
                                                    self.Cout, self.k, self.s, self.p)

    @property
    def w_shape(self):
        return (self.Cin, self.Cout, self.k, self.k) if self.full else (self.Cout, self.Cin, self.k, self.k)

    def low_res(self):
        """the low-resolution map of the layer (a conv's output, a full-conv's input) and the pixels on it"""
        h, w = (self.H, self.W) if self.full else (self.Ho, self.Wo)
        return h, w, self.B * h * w


def pwgrad_route(mode, c):
    """wg_plan (vf_conv.hip): a conv layer's planes-fed weight gradient is k_pwgrad_group's where its rows are whole 128-row
    tiles (or, in the three-plane mode, one tile of 64), its columns whole 64-channel steps and its pixels whole 32-deep K steps;
    every other shape stays on the fp32-fed kernel although planes are at hand"""
    _, _, P = c.low_res()
    takes = mode in (3, 1) and (c.Cout % 128 == 0 or (c.Cout == 64 and mode == 3)) and c.Cin % 64 == 0 and P % 32 == 0
    return ("pwgrad_group_",) if takes else ("wgrad_",)


def pconv_supported(mode, c, transposed):
    """vf_pconv_supported_in_mode for the gather pass of the conv layer c, or the transposed pass from its low-resolution map"""
    if mode not in (3, 1) or (c.k, c.s, c.p) != (4, 2, 1):
        return False
    Hl, Wl, M = c.low_res()
    ci, co = (c.Cout, c.Cin) if transposed else (c.Cin, c.Cout)
    pow2 = lambda v: v > 0 and v & (v - 1) == 0
    if ci % 32 or co < 32 or co % 4 or M <= 64 or not pow2(Hl) or not pow2(Wl):
        return False
    return mode == 3 or (ci % 64 == 0 and co % 64 == 0 and M % 64 == 0)


def _table():
    T = []
    IG = {"fwd": ("igemm_",), "fwd_act": ("igemm_",), "fwd_planes": ("igemm_",), "bwd_data": ("igemm_",), "bwd_data_act": ("igemm_",),
          "bwd_weight_b0": ("wgrad_",), "bwd_weight_b1": ("wgrad_",)}
    # ---- the implicit GEMM (k_igemm, k_wgrad) in all three product modes.  The transposed passes onto fewer than 32 channels
    # (full-conv 128 -> 4 and 64 -> 1 forward) take the column buffer: an inner k_igemm launch, then col2im4x4
    for B, H, W in ((2, 8, 16), (3, 16, 4)):
        for Cin, Cout in ((32, 33), (64, 128), (128, 4), (64, 1)):
            T.append(Case("igemm_conv", False, B, H, W, Cin, Cout, passes=CONV_PASSES, modes=(3, 1, 0), routes=IG))
            T.append(Case("igemm_full", True, B, H, W, Cin, Cout, passes=FULL_PASSES, modes=(3, 1, 0), routes=IG))
    # ---- thin input (k_conv_thin_in: 3 channels in, tiles of 8 x 8 outputs, a block per ROW of tiles)
    TI = {"fwd": ("conv_thin_in",), "fwd_planes": ("conv_thin_in_planes",), "bwd_weight_b0": ("wgrad_",)}
    for B, H, W in ((2, 16, 32), (2, 32, 16)):
        T.append(Case("thin_in", False, B, H, W, 3, 64, passes=("fwd", "fwd_planes", "bwd_weight_b0"), routes=TI))
    # the other 3-channel gather, a full-conv 64 -> 3's data-gradient (3 channels on 16 x 32 / 32 x 16): vf_internal_deconv2d_bwd_data
    # hands it to conv_like_fwd, so it is k_igemm's with scalar loads, not k_conv_thin_in's (which the rows above reach)
    for B, H, W in ((2, 8, 16), (2, 16, 8)):
        T.append(Case("thin_in_grad", True, B, H, W, 64, 3, passes=("bwd_data",), routes={"bwd_data": ("igemm_",)}))
    # ---- thin output (k_deconv_thin_out: 3 channels out, tiles_x / tiles_y of 8 x 8 low-resolution positions)
    for B, H, W in ((2, 8, 16), (2, 16, 8)):
        T.append(Case("thin_out", True, B, H, W, 64, 3, passes=("fwd", "fwd_act"),
                      routes={"fwd": ("deconv_thin_out",), "fwd_act": ("deconv_thin_out",)}))
    # ---- column buffer (transposed pass with N < 32: GEMM into columns, then k_col2im4x4 with ilog2(Hi), ilog2(Wi))
    for B, H, W in ((2, 8, 16), (3, 16, 4)):
        T.append(Case("col2im", True, B, H, W, 64, 16, passes=("fwd", "fwd_act"), routes={"fwd": ("col2im4x4",), "fwd_act": ("col2im4x4",)}))
        T.append(Case("col2im", False, B, H, W, 16, 64, passes=("bwd_data", "bwd_data_act"),
                      routes={"bwd_data": ("col2im4x4",), "bwd_data_act": ("col2im4x4",)}))
    # ---- generic (vf_conv_generic.hip), modes 3 and 0.  Its weight gradient stages Cout + k * k * Cin <= 1024 floats per pixel: the
    # 128 -> 4 layers are refused (a stated limit, checked before any launch); 32 -> 33 and 16 -> 32 reach gconv_bwd_weight
    GC = {"fwd": ("gconv_fwd",), "bwd_data": ("gconv_bwd_data",), "bwd_weight_b0": ("gconv_bwd_weight",), "bwd_weight_b1": ("gconv_bwd_weight",)}
    big = {"bwd_weight_b0": "exceeds the staging tile", "bwd_weight_b1": "exceeds the staging tile"}
    for B, H, W in ((2, 8, 16), (3, 16, 4)):
        for Cin, Cout in ((32, 33), (128, 4)):
            for geo in ((5, 2, 2), (4, 1, 0)):
                T.append(Case("generic", False, B, H, W, Cin, Cout, geo, GENERIC_PASSES, (3, 0), GC, big if Cin == 128 else None))
    for B, H, W in ((2, 6, 10), (2, 10, 6)):
        T.append(Case("generic_no_pow2", False, B, H, W, 16, 32, (3, 1, 1), GENERIC_PASSES, (3, 0), GC))
    # ---- planes GEMM (vf_pgemm.hip), modes 3 and 1.  64 -> 33 is not a planes shape (Cout % 4, Cin % 32 of the transposed pass): the
    # entry points refuse it, and its weight gradient, planes at hand, stays fp32-fed.  Mode 1 serves whole 64-wide tiles only
    for B, H, W in ((2, 16, 32), (3, 32, 8)):
        for Cin, Cout in ((32, 64), (64, 128), (128, 64), (64, 33)):
            T.append(Case("planes", False, B, H, W, Cin, Cout, passes=PLANES_PASSES, modes=(3, 1),
                          routes={"pconv_gather": ("pconv_",), "pconv_scatter": ("pconv_",), "pconv_scatter_mask": ("pconv_",),
                                  "pconv_scatter_fwd": ("pconv_",)}))
    # ---- patch kernels.  k_pconv_patch_g<0> wants Wo % 16 == 0 && Ho % 8 == 0 and whole 128-row tiles: 16 x 32 -> 8 x 16 is the
    # smallest; 32 x 16 -> 16 x 8 is NOT its shape (k_pconv_dma takes that), so the H > W order is 64 x 32
    for B, H, W in ((2, 16, 32), (1, 32, 64), (1, 64, 32)):
        T.append(Case("patch_gather", False, B, H, W, 64, 64, passes=("pconv_gather",), routes={"pconv_gather": ("pconv_patchg_128x64_t16_m0",)}))
    # k_pconv_patch_tr wants Wi % 16 == 0 && Hi % 8 == 0 on the LOW-RESOLUTION grid, whole 128-row tiles, one K range: grids 8 x 16,
    # 16 x 32 (the issue's) and 32 x 16 (the smallest H > W grid its rule allows; 16 x 8 is k_pconv_dma's).  The layer is the conv
    # 64 -> 64 whose data-gradient scatters from that grid: input maps 16 x 32, 32 x 64, 64 x 32
    PT = ("pconv_patch_128x64_t4_c",)
    for B, H, W in ((2, 16, 32), (1, 32, 64), (1, 64, 32)):
        T.append(Case("patch_scatter", False, B, H, W, 64, 64, passes=("pconv_scatter", "pconv_scatter_mask", "pconv_scatter_fwd"),
                      routes={"pconv_scatter": PT, "pconv_scatter_mask": PT, "pconv_scatter_fwd": PT}))
    # ---- BatchNorm by-products of the GEMM that produces the tensor (vf_bn_fuse_next_fwd / _bwd), groups 1
    for B, H, W in ((2, 16, 32), (3, 32, 8)):
        T.append(Case("bn", False, B, H, W, 64, 128, passes=("bn_fwd", "bn_bwd"), routes={"bn_fwd": ("igemm_",), "bn_bwd": ("igemm_",)}))
    return T


CASES = _table()
# groups whose table holds one order only, and why (tests/test_nonsquare_ref.py::test_table_coverage): none — where a kernel's rule
# forbids the swapped map (the patch kernels), the H > W order is the next map its rule allows
ONE_ORDER = {}

# the net chain (tests/test_gpu_nonsquare.py::test_net_chain): inputs, both orders
NET_INPUTS = [(2, 3, 32, 64), (3, 3, 64, 16)]
NET_TOL_OUT, NET_TOL_GRAD = 2e-5, 1e-4      # tests/test_gpu_net.py's bars


# ---------------------------------------------------------------------------------------------------------------- operands
def _ints(g, shape, lo, hi, nonzero=False):
    t = torch.randint(lo, hi + 1, shape, generator=g)
    if nonzero:
        t = torch.where(t == 0, torch.randint(0, 2, shape, generator=g) * 2 - 1, t)
    return t.to(torch.float32)


@functools.lru_cache(maxsize=None)
def _operands(idx, kind):
    c = CASES[idx]
    g = torch.Generator().manual_seed(1000 * (idx + 1) + (0 if kind == "int" else 1))
    xs, ys = (c.B, c.Cin, c.H, c.W), (c.B, c.Cout, c.Ho, c.Wo)
    if kind == "int":
        o = dict(x=_ints(g, xs, -3, 3), w=_ints(g, c.w_shape, -2, 2) * 0.25, bias=_ints(g, (c.Cout,), -4, 4), gy=_ints(g, ys, -3, 3),
                 gw0=_ints(g, c.w_shape, -8, 8), gb0=_ints(g, (c.Cout,), -8, 8), xact=_ints(g, xs, -3, 3, nonzero=True),
                 bias_t=_ints(g, (c.Cin,), -4, 4), shift=_ints(g, (c.Cout,), -2, 2), mean=_ints(g, (c.Cin,), -2, 2),
                 bn_x=_ints(g, xs, -3, 3), bn_yact=_ints(g, xs, -3, 3, nonzero=True))
    else:
        r = lambda shape, scale=1.0: torch.randn(shape, generator=g) * scale
        o = dict(x=r(xs), w=r(c.w_shape, 0.05), bias=r((c.Cout,), 0.1), gy=r(ys), gw0=r(c.w_shape), gb0=r((c.Cout,)), xact=r(xs),
                 bias_t=r((c.Cin,), 0.1), shift=r((c.Cout,), 0.1), mean=r((c.Cin,), 0.1), bn_x=r(xs), bn_yact=r(xs))
    return o


def operands(case, kind):
    """float32 CPU tensors, logical NCHW (the device holds 4-D ones channels-last); treat them as read-only"""
    return _operands(CASES.index(case), kind)


def bf16_round(t):
    """round-to-nearest-even to bf16, kept in float32: tests/test_gpu_bf16.py's rule"""
    a = t.detach().contiguous().numpy()
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return torch.from_numpy(u.astype(np.uint32).view(np.float32).reshape(a.shape))


# ---------------------------------------------------------------------------------------------------------------- reference
def act(y, name):
    if name == "lrelu":
        return torch.where(y > 0, y, SLOPE * y)
    if name == "relu":
        return torch.clamp(y, min=0)
    return y


def conv_ops(case, dtype=torch.float64):
    """(forward, its transpose) of the layer as functions of (input, weight, bias).  hw: the map the transpose lands on (a conv
    whose stride does not divide its padded map loses the last rows: conv_transpose2d alone cannot know the input's size)"""
    kw = dict(stride=case.s, padding=case.p)
    if case.full:
        return (lambda x, w, b=None: F.conv_transpose2d(x, w, b, **kw)), (lambda gy, w, b=None, hw=None: F.conv2d(gy, w, b, **kw))

    def tr(gy, w, b=None, hw=None):
        H, W = hw or (case.H, case.W)
        oph, opw = H - ((gy.shape[2] - 1) * case.s - 2 * case.p + case.k), W - ((gy.shape[3] - 1) * case.s - 2 * case.p + case.k)
        return F.conv_transpose2d(gy, w, b, output_padding=(oph, opw), **kw)
    return (lambda x, w, b=None: F.conv2d(x, w, b, **kw)), tr


def weight_grad(case, x, gy):
    """autograd on the forward call, as WLayer.ref in tests/test_gpu_workspace.py"""
    w = torch.zeros(case.w_shape, dtype=x.dtype, requires_grad=True)
    conv_ops(case)[0](x, w).backward(gy)
    return w.grad


def passes_of(case, o, dtype=torch.float64, rnd=None):
    """every tensor the case's passes write, evaluated in `dtype`.  rnd (the bf16 mode): applied to exactly the two operands the
    GEMM of each pass stages; bias, masks, the beta = 1 starting values and the bias gradient stay unrounded"""
    rnd = rnd or (lambda t: t)
    d = lambda t: t.to(dtype)
    fwd, tr = conv_ops(case, dtype)
    x, w, gy = d(o["x"]), d(o["w"]), d(o["gy"])
    xr, wr, gyr = d(rnd(o["x"])), d(rnd(o["w"])), d(rnd(o["gy"]))
    bias = d(o["bias"])
    r = {}
    y = fwd(xr, wr, bias)
    r["fwd"], r["fwd_act"], r["fwd_relu"], r["fwd_lrelu"] = y, act(y, case.act), act(y, "relu"), act(y, "lrelu")
    gx = tr(gyr, wr)
    r["bwd_data"] = gx
    r["bwd_data_act"] = torch.where(d(o["xact"]) > 0, gx, SLOPE * gx)
    r["scatter_fwd"] = act(tr(gyr, wr, d(o["bias_t"])), "relu")
    gw = weight_grad(case, xr, gyr)
    gb = gy.sum((0, 2, 3))
    r["gw_b0"], r["gb_b0"] = gw, gb
    r["gw_b1"], r["gb_b1"] = gw + d(o["gw0"]), gb + d(o["gb0"])
    # BatchNorm by-products: the forward's sums of (y - shift) and its square per channel; the data-gradient stored masked by the
    # derivative at bn_yact, its sums of g and g * (bn_x - mean) (BnFused.check_sums, tests/test_gpu_workspace.py)
    t = y - d(o["shift"]).view(1, -1, 1, 1)
    r["bn_fwd_sums"] = torch.stack([t.sum((0, 2, 3)), (t * t).sum((0, 2, 3))])
    g = torch.where(d(o["bn_yact"]) > 0, gx, SLOPE * gx)
    r["bn_bwd"] = g
    gxm = g * (d(o["bn_x"]) - d(o["mean"]).view(1, -1, 1, 1))
    r["bn_bwd_sums"] = torch.stack([g.sum((0, 2, 3)), gxm.sum((0, 2, 3))])
    # the largest per-channel sum of |terms| among the four: no partial sum, in any order, exceeds it
    r["bn_abs_sums"] = max(float(v.abs().sum((0, 2, 3)).max()) for v in (t, t * t, g, gxm))
    return r


@functools.lru_cache(maxsize=None)
def _reference(idx, kind, rounded):
    return passes_of(CASES[idx], _operands(idx, kind), torch.float64, bf16_round if rounded else None)


def reference(case, kind, rounded=False):
    """fp64, computed once per (case, operands, rounding) and shared; treat as read-only"""
    return _reference(CASES.index(case), kind, bool(rounded))


# ---------------------------------------------------------------------------------------------------------------- H / W mix-up
def reread(t):
    """the channels-last bytes of a logical B x C x H x W tensor read as a W x H map (logical B x C x W x H)"""
    B, Cc, H, W = t.shape
    return t.permute(0, 2, 3, 1).contiguous().view(B, W, H, Cc).permute(0, 3, 1, 2)


def swapped_passes(case, o):
    """forward, data-gradient and weight gradient as a kernel would form them that took H for W: operands' bytes read as W x H maps,
    the result's bytes read back as H' x W'"""
    d = lambda t: t.to(torch.float64)
    fwd, tr = conv_ops(case)
    x, gy, w = reread(d(o["x"])), reread(d(o["gy"])), d(o["w"])
    return {"fwd": reread(fwd(x, w, d(o["bias"]))), "bwd_data": reread(tr(gy, w, hw=(case.W, case.H))), "gw_b0": weight_grad(case, x, gy)}


# ---------------------------------------------------------------------------------------------------------------- comparison
def exact_mismatch(got, ref):
    """None if `got` (any float dtype, any device) equals the fp64 reference bit for bit in every element, else what differs.
    NaN — an element no launch wrote — never equals."""
    g = got.detach().to("cpu", torch.float64)
    if tuple(g.shape) != tuple(ref.shape):
        return "shape %s, reference %s" % (tuple(g.shape), tuple(ref.shape))
    if torch.equal(g, ref):
        return None
    bad = (g != ref) | torch.isnan(g)
    i = tuple(int(v) for v in bad.nonzero()[0])
    return "%d of %d elements differ (%d NaN); first at %s: got %r, reference %r" % (
        int(bad.sum()), g.numel(), int(torch.isnan(g).sum()), i, float(g[i]), float(ref[i]))


def rel_err(got, ref):
    """max-norm relative error; NaN fails every bar"""
    g = got.detach().to("cpu", torch.float64)
    return float((g - ref).abs().max() / ref.abs().max())


# ---------------------------------------------------------------------------------------------------------------- net chain
def torch_chain(params, eps=1e-5):
    """the chain of test_gpu_nonsquare.py::test_net_chain in torch float64: conv 3 -> 64, 64 -> 128 + BN, 128 -> 64 + BN, full-conv
    64 -> 128 + BN, 128 -> 32 + BN, 32 -> 3, Tanh; LeakyReLU(1.0) — the identity — in place of every (Leaky)ReLU; training-mode
    BatchNorm.  params: the float64 leaf tensors in module order (weight, bias per parametrised module).  Returns f(x)."""
    kinds = ["conv", "conv", "bn", "conv", "bn", "full", "bn", "full", "bn", "full"]

    def f(x):
        it = iter(params)
        for kind in kinds:
            w, b = next(it), next(it)
            if kind == "conv":
                x = F.conv2d(x, w, b, stride=2, padding=1)
            elif kind == "full":
                x = F.conv_transpose2d(x, w, b, stride=2, padding=1)
            else:
                x = F.batch_norm(x, None, None, w, b, True, 0.1, eps)
        return torch.tanh(x)
    return f
