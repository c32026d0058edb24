"""The conv passes under small workspaces, against fp64 on the CPU, with guard bands around every buffer a kernel writes.

The dispatchers pick their route partly from the context's workspace: launch_igemm (csrc/vf_conv.hip) and launch_pconv
(csrc/vf_pgemm.hip) clamp their split-K count to the slabs that fit; the BatchNorm statistics come from the GEMM epilogue or
from the split-K combine; a weight-gradient group is flushed in the middle of a walk when its slabs no longer fit; the thin-output
transposed pass takes its column buffer only with room to spare; the bottleneck GEMMs take the weight-streaming kernels only if
their slabs fit.  Production runs all of these sizes (1 GiB main context, 128 MB side contexts), so every case here runs at the
size hint and at sizes on both sides of each threshold, on a backend of its own whose workspace is re-pointed per run.

Every run checks:
  - the result against an fp64 evaluation of the same operation (the suite's bar: 2e-5 of the max-norm);
  - that nothing was written past the workspace, past the output tensor or past the BatchNorm partial rows (guard bands);
  - the split count the library reports through its profile (slab_reduce_* records 4 * out_elems * (ksplit + 1) bytes per
    launch) against the workspace it had: ksplit * slab <= workspace, never more splits for less room.
The split counts and routes each case reached are printed (pytest -rP shows them)."""
import pytest
import torch
import torch.nn.functional as F

from helpers import FILL64, TAIL32, WS_FILL, guarded, untouched, workspace  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = 2e-5           # against fp64, relative to the max-norm
# two split counts of one pass: the same products, K summed in another order.  At ksplit 1 one fp32 accumulator takes the whole
# K = 16 * 256 (or 16 * 384) products; against ksplit 32 (or 6) that moves the worst element by up to 2.7e-6 of the max-norm
# (measured on the 256 -> 512 forward and the 384-channel gather), so the bar is 4e-6: still five times inside the fp64 bar
AGREE = 4e-6
U = 2.0 ** -24       # unit roundoff of fp32
SLOPE = 0.2


# ---------------------------------------------------------------------------------------------------------------- harness
@pytest.fixture(scope="module")
def wb():
    """a backend of its own: the shared `hipb` serves the nn modules and the other tests and keeps its 1 GiB workspace"""
    from video_filler_amd.backend import HipBackend
    b = HipBackend(workspace_bytes=1 << 20)
    b.set_mfma_mode("f32_3xbf16")
    yield b
    b.synchronize()


@pytest.fixture(params=["f32_3xbf16", "f32"])
def mode(request, wb):
    wb.set_mfma_mode(request.param)
    try:
        yield request.param
    finally:
        wb.set_mfma_mode("f32_3xbf16")


def hint(b):
    return int(b.lib.vf_workspace_bytes_hint())


def g_act(b, B, Cc, H, W):
    """a guarded channels-last tensor (logical B x Cc x H x W) -> (tensor, backing buffer)"""
    n = B * Cc * H * W
    buf = guarded(b, n)
    return buf[:n].view(B, H, W, Cc).permute(0, 3, 1, 2), buf


def profiled(b, fn):
    b.prof_begin()
    try:
        fn()
    finally:
        prof = b.prof_end()
    return prof


def split_of(prof, kind, out_elems):
    """the split count of the ONE pass in `prof` (kind: igemm / pconv / wgrad); no slab reduce: 1"""
    hits = [e for n, e in prof.items() if n in ("slab_reduce_" + kind, "slab_reduce_%s_bnstats" % kind)]
    if not hits:
        return 1
    assert len(hits) == 1 and hits[0]["launches"] == 1, prof
    k = hits[0]["bytes"] / (4.0 * out_elems) - 1
    assert abs(k - round(k)) < 1e-6, (k, prof)
    return int(round(k))


def route_of(prof):
    return "+".join(sorted(n for n in prof if not n.startswith("slab_reduce")))


def _r(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def d_act(b, B, Cc, H, seed, scale=1.0):
    return _r((B, H, H, Cc), seed, scale).to(b.device).permute(0, 3, 1, 2)


def d_w(b, d0, d1, seed, scale=0.05, k=4):
    """a weight, logical [d0][d1][k][k], physical [d0][k][k][d1]"""
    return _r((d0, k, k, d1), seed, scale).to(b.device).permute(0, 3, 1, 2)


def f64(t):
    return t.detach().to("cpu", torch.float64)


def act64(y, act):
    if act == "lrelu":
        return torch.where(y > 0, y, SLOPE * y)
    if act == "relu":
        return torch.clamp(y, min=0)
    return y


def rel(got, ref):
    """max-norm relative error; NaN (a value no launch wrote) fails every bar"""
    return float((f64(got) - ref).abs().max() / ref.abs().max())


def igemm_nk(C, taps):
    """launch_igemm's K steps: with 16-byte loads of both operands (C % 16 == 0 here) the loop takes nq = taps * C / 16
    sixteen-wide chunks, two per step, nk = (nq + 1) / 2; otherwise K = taps * C is walked 32 at a time"""
    return (taps * (C // 16) + 1) // 2 if C % 16 == 0 else -(-taps * C // 32)


# ---------------------------------------------------------------------------------------------------------------- passes
class Pass:
    """one conv-like pass at one shape: its operands, its launch into a given output, its fp64 reference"""

    def __init__(self, b, kind, B, Cin, H, Cout, act=None, seed=0):
        self.b, self.kind, self.B, self.Cin, self.H, self.Cout = b, kind, B, Cin, H, Cout
        s = seed * 10
        if kind == "fwd":                          # conv Cin -> Cout on H x H, stride 2
            self.act = "lrelu" if act is None else act
            self.x = d_act(b, B, Cin, H, s + 1)
            self.w = d_w(b, Cout, Cin, s + 2)
            self.bias = _r((Cout,), s + 3, 0.1).to(b.device)
            self.out_shape = (B, Cout, H // 2, H // 2)
            self.gemm = ("igemm", Cin, 16)
        elif kind == "bwd_data":                   # its data gradient: gy (Cout, H/2) -> gx (Cin, H)
            self.act = "none"
            self.x = d_act(b, B, Cout, H // 2, s + 1)
            self.w = d_w(b, Cout, Cin, s + 2)
            self.bias = None
            self.out_shape = (B, Cin, H, H)
            self.gemm = ("igemm", Cout, 4)
        elif kind == "deconv_fwd":                 # full-conv Cin -> Cout, H -> 2H
            self.act = "relu" if act is None else act
            self.x = d_act(b, B, Cin, H, s + 1)
            self.w = d_w(b, Cin, Cout, s + 2)
            self.bias = _r((Cout,), s + 3, 0.1).to(b.device)
            self.out_shape = (B, Cout, 2 * H, 2 * H)
            self.gemm = ("igemm", Cin, 4)
        elif kind == "gather":                     # conv forward from planes
            self.act = "lrelu"
            self.x = d_act(b, B, Cin, H, s + 1)
            self.w = d_w(b, Cout, Cin, s + 2)
            self.bias = _r((Cout,), s + 3, 0.1).to(b.device)
            self.xp = b.planes_split(self.x)
            self.wp, _ = b.weight_planes(self.w, want_transposed=False)
            self.out_shape = (B, Cout, H // 2, H // 2)
            self.gemm = ("pconv", Cin, 16)
        elif kind == "scatter_data":               # conv data gradient from planes: gy (Cout, H/2) -> gx (Cin, H)
            self.act = "none"
            self.x = d_act(b, B, Cout, H // 2, s + 1)
            self.w = d_w(b, Cout, Cin, s + 2)
            self.bias = None
            self.xp = b.planes_split(self.x)
            _, self.wp = b.weight_planes(self.w)
            self.out_shape = (B, Cin, H, H)
            self.gemm = ("pconv", Cout, 4)
        elif kind == "scatter_fwd":                # full-conv forward from planes: x (Cin, H) -> y (Cout, 2H)
            self.act = "relu"
            self.x = d_act(b, B, Cin, H, s + 1)
            self.w = d_w(b, Cin, Cout, s + 2)      # full-conv weight [Cin][Cout]: the conv weight of Cout -> Cin read the other way
            self.bias = _r((Cout,), s + 3, 0.1).to(b.device)
            self.xp = b.planes_split(self.x)
            _, self.wp = b.weight_planes(self.w)
            self.out_shape = (B, Cout, 2 * H, 2 * H)
            self.gemm = ("pconv", Cin, 4)
        else:
            raise ValueError(kind)
        self.n_out = B * self.out_shape[1] * self.out_shape[2] * self.out_shape[3]
        self._ref = None

    @property
    def name(self):
        return "%s B=%d %d->%d %dx%d" % (self.kind, self.B, self.Cin, self.Cout, self.H, self.H)

    def launch(self, y, dmask=None):
        b, B, H = self.b, self.B, self.H
        if self.kind == "fwd":
            b.conv2d_fwd(self.x, self.w, self.bias, y, 4, 2, 1, self.act, SLOPE)
        elif self.kind == "bwd_data":
            if dmask is None:
                b.conv2d_bwd_data(self.x, self.w, y, 4, 2, 1)
            else:
                b.conv2d_bwd_data_act(self.x, self.w, y, dmask, "lrelu", SLOPE, 4, 2, 1)
        elif self.kind == "deconv_fwd":
            b.deconv2d_fwd(self.x, self.w, self.bias, y, 4, 2, 1, self.act, SLOPE)
        elif self.kind == "gather":
            b.pconv_gather(self.xp, self.wp, self.bias, y, B, H, H, self.Cin, self.Cout, self.act, SLOPE)
        elif self.kind == "scatter_data":
            b.pconv_scatter(self.xp, self.wp, None, y, B, H // 2, H // 2, self.Cout, self.Cin, dmask=dmask,
                            dact="lrelu" if dmask is not None else "none", dslope=SLOPE)
        else:
            b.pconv_scatter(self.xp, self.wp, self.bias, y, B, H, H, self.Cin, self.Cout, self.act, SLOPE)

    def ref(self):
        """fp64 on the CPU, without any derivative mask"""
        if self._ref is None:
            x, w = f64(self.x), f64(self.w)
            bias = None if self.bias is None else f64(self.bias)
            if self.kind in ("fwd", "gather"):
                r = F.conv2d(x, w, bias, stride=2, padding=1)
            else:
                r = F.conv_transpose2d(x, w, bias, stride=2, padding=1)
            self._ref = act64(r, self.act)
        return self._ref

    def run(self, ws, dmask=None):
        """one launch into a fresh guarded output with a fresh guarded workspace -> (output, ksplit, route)"""
        y, ybuf = g_act(self.b, *self.out_shape)
        with workspace(self.b, ws):
            prof = profiled(self.b, lambda: self.launch(y, dmask))
        assert untouched(ybuf, self.n_out), "%s: a kernel wrote past the output (workspace %d)" % (self.name, ws)
        return y, split_of(prof, self.gemm[0], self.n_out), route_of(prof)


def sweep(p, check_nchunks=False):
    """the pass at the hint (split count k0), then at j * slab and j * slab - 4 bytes for j = k0 .. 1, then at 0 bytes"""
    b = p.b
    slab = 4 * p.n_out
    ref = p.ref()
    runs = []

    def one(ws):
        y, k, route = p.run(ws)
        e = rel(y, ref)
        assert e <= TOL, "%s, workspace %d, ksplit %d (%s): error %.3e against fp64" % (p.name, ws, k, route, e)
        assert k == 1 or k * slab <= ws, "%s: ksplit %d needs %d bytes of slabs, the workspace has %d" % (p.name, k, k * slab, ws)
        if check_nchunks:
            nchunks = p.gemm[1] // (64 if p.gemm[1] % 64 == 0 else 32)
            assert nchunks % k == 0, "%s: ksplit %d does not divide the %d channel chunks" % (p.name, k, nchunks)
        runs.append((ws, k, route, y))

    one(hint(b))
    k0 = runs[0][1]
    for j in range(k0, 0, -1):
        one(j * slab)
        one(j * slab - 4)
    one(0)
    ks = [r[1] for r in runs]
    assert all(a >= c for a, c in zip(ks, ks[1:])), "%s: the split count rose as the workspace shrank: %s" % (p.name, ks)
    y0 = runs[0][3]
    for ws, k, route, y in runs[1:]:
        e = float((y - y0).abs().max() / y0.abs().max())
        assert e <= AGREE, "%s: ksplit %d (workspace %d) differs from ksplit %d by %.3e" % (p.name, k, ws, k0, e)
    print("%s [%s]: route %s; ksplit %s over workspaces %s" % (p.name, p.b.mfma_mode, runs[0][2], sorted(set(ks), reverse=True),
                                                          [r[0] for r in runs]))
    return runs


# ---------------------------------------------------------------------------------------------------------------- split-K
# netD / netG's deep 4x4 stride-2 layers at a small batch (256 -> 512 on 8 x 8, its data gradient, the 512 -> 256 full-conv)
# and netD's 12-channel first layer of the video nets (scalar loads: nk = 6, no split at any size)
IGEMM_CASES = [("fwd", 4, 256, 8, 512), ("bwd_data", 4, 256, 8, 512), ("deconv_fwd", 4, 512, 4, 256), ("fwd", 2, 12, 32, 64)]


@pytest.mark.parametrize("case", IGEMM_CASES, ids=lambda c: "%s-B%d-%dto%d-%dx%d" % (c[0], c[1], c[2], c[4], c[3], c[3]))
def test_igemm_split_k_sweep(case, mode, wb):
    kind, B, Cin, H, Cout = case
    p = Pass(wb, kind, B, Cin, H, Cout, seed=1)
    runs = sweep(p)
    nk = igemm_nk(*p.gemm[1:])
    ks = sorted(set(r[1] for r in runs))
    if nk >= 8 and runs[0][1] >= 3:
        # a split count that does not divide the K steps (the last split runs fewer steps than the others) must be among them:
        # 256 -> 512 forward nk = 128, the transposed passes over 512 channels nk = 64; j = 3 gives ksplit 3 for both
        assert any(nk % k for k in ks), "%s: every split count %s divides nk = %d" % (p.name, ks, nk)


# the planes kernels: channel chunks of 64; C = 384 -> 6 chunks, so the split counts 6, 3, 2, 1 are all reached
PCONV_CASES = [("gather", 8, 384, 8, 128), ("scatter_fwd", 8, 512, 4, 256), ("scatter_data", 8, 256, 8, 512)]


@pytest.mark.parametrize("case", PCONV_CASES, ids=lambda c: "%s-B%d-%dto%d-%dx%d" % (c[0], c[1], c[2], c[4], c[3], c[3]))
def test_pconv_split_k_sweep(case, wb):
    kind, B, Cin, H, Cout = case
    p = Pass(wb, kind, B, Cin, H, Cout, seed=2)
    runs = sweep(p, check_nchunks=True)
    if Cin == 384:
        assert {6, 3, 2, 1} <= set(r[1] for r in runs), [r[1] for r in runs]


# ---------------------------------------------------------------------------------------------------------------- BatchNorm sums
# mode 1: the conv forward a BatchNorm follows (128 -> 256 on 16 x 16); mode 2: the data gradient a BatchNorm + LeakyReLU sits on
# (256 <- 512 on 8 x 8), on k_igemm and on the planes kernels.  All three leave >= 4 partial rows per group on both routes.
BN_CASES = [(1, "fwd", 8, 128, 16, 256), (2, "bwd_data", 8, 256, 8, 512), (2, "scatter_data", 16, 256, 8, 512)]


class BnFused:
    def __init__(self, b, mode_, kind, B, Cin, H, Cout, groups):
        self.b, self.mode, self.groups = b, mode_, groups
        self.p = Pass(b, kind, B, Cin, H, Cout, act="none", seed=3)
        Bo, self.C, Ho, Wo = self.p.out_shape
        self.npix = Bo * Ho * Wo // groups
        if mode_ == 1:
            self.shift = _r((self.C,), 41, 0.1).to(b.device)
        else:
            self.x = d_act(b, Bo, self.C, Ho, 42)                                        # the BatchNorm input
            self.yact = d_act(b, Bo, self.C, Ho, 43)                                     # its activated output
            self.mean = _r((groups * self.C,), 44, 0.1).to(b.device)

    def run(self, ws, cap):
        """the pass with the attachment, `cap` partial rows per group -> (output, part buffer, rows per group, ksplit)"""
        b, C = self.b, self.C
        n = self.groups * cap * 2 * C
        part = guarded(b, n, torch.float64)
        y, ybuf = g_act(b, *self.p.out_shape)
        with workspace(b, ws):
            def go():
                if self.mode == 1:
                    b.bn_fuse_next_fwd(self.shift, part[:n], self.groups)
                else:
                    b.bn_fuse_next_bwd(self.x, self.yact, "lrelu", SLOPE, self.mean, part[:n], self.groups)
                self.p.launch(y)
            prof = profiled(b, go)
            R = b.bn_fuse_result()
        assert untouched(ybuf, self.p.n_out), "a kernel wrote past the output"
        assert untouched(part, n), "a kernel wrote past the partial-row buffer"
        return y, part, R, split_of(prof, self.p.gemm[0], self.p.n_out)

    def masked_ref(self):
        r = self.p.ref()
        if self.mode == 2:
            r = torch.where(f64(self.yact) > 0, r, SLOPE * r)
        return r

    def check_sums(self, y, part, R, what):
        """per group, the partial rows summed in fp64 against fp64 sums over the output the kernel stored.
        Bound: each partial row is a sum of fp32 terms formed with at most two roundings (v - shift, then its square; or
        x - mean, then the product) and accumulated in fp32 by a thread over at most the row's own n_row = npix / R elements
        before the block combines its threads in fp64.  First-order error of such a sum: (n_row + 2) * u * sum |term|, with
        u = 2^-24 — for these cases (n_row <= 128) under 8e-6 of sum |term| per channel, and for the sums of squares (every
        term positive) of the sum itself."""
        C, G = self.C, self.groups
        rows = f64(part[:G * R * 2 * C]).view(G, R, 2, C).sum(1)
        yv = f64(y).permute(0, 2, 3, 1).reshape(G, self.npix, C)
        n_row = self.npix / R
        for g in range(G):
            if self.mode == 1:
                d = yv[g] - f64(self.shift)
                terms = (d, d * d)
            else:
                xv = f64(self.x).permute(0, 2, 3, 1).reshape(G, self.npix, C)[g]
                terms = (yv[g], yv[g] * (xv - f64(self.mean)[g * C:(g + 1) * C]))
            for i, t in enumerate(terms):
                bound = (n_row + 2) * U * t.abs().sum(0) + 1e-30
                err = (rows[g, i] - t.sum(0)).abs()
                assert bool((err <= bound).all()), "%s: group %d sum %d off by %.2f times the bound" % (
                    what, g, i + 1, float((err / bound).max()))


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("case", BN_CASES, ids=lambda c: "mode%d-%s-B%d-%dto%d" % (c[0], c[1], c[2], c[3], c[5]))
def test_batchnorm_partials_against_fp64(case, groups, wb):
    mode_, kind, B, Cin, H, Cout = case
    f = BnFused(wb, mode_, kind, B, Cin, H, Cout, groups)
    slab = 4 * f.p.n_out
    want = f.masked_ref()
    plain = f.p.ref()
    seen = []
    for ws in (hint(wb), 3 * slab, 0):
        y, part, R, k = f.run(ws, 1024)
        what = "%s mode %d groups %d, workspace %d, ksplit %d" % (f.p.name, mode_, groups, ws, k)
        assert R >= 2, "%s: not fused (rows per group %d)" % (what, R)
        assert rel(y, want) <= TOL, what
        f.check_sums(y, part, R, what)
        assert untouched(part, groups * R * 2 * f.C), "%s: rows beyond groups * R were written" % what
        # the row cap at exactly R per group still fuses, R - 1 does not: then nothing is written and the output is unmasked
        y2, part2, R2, k2 = f.run(ws, R)
        assert (R2, k2) == (R, k), what
        f.check_sums(y2, part2, R2, what + " (cap R)")
        y3, part3, R3, k3 = f.run(ws, R - 1)
        assert R3 == 0 and k3 == k, "%s: cap R - 1 fused %d rows" % (what, R3)
        assert untouched(part3, 0), "%s: cap R - 1 wrote partial rows" % what
        assert rel(y3, plain) <= TOL, "%s: cap R - 1: the output is not the unmasked one" % what
        seen.append((ws, "slab reduce" if k > 1 else "epilogue", k, R))
    assert seen[0][2] > 1 and seen[-1][2] == 1, seen
    print("%s mode %d groups %d: (workspace, route, ksplit, rows per group) %s" % (f.p.name, mode_, groups, seen))


# ---------------------------------------------------------------------------------------------------------------- wgrad groups
class WLayer:
    """one weight gradient of a backward walk: conv (or full-conv) Cin -> Cout on H x H"""

    def __init__(self, b, name, full, B, Cin, H, Cout, beta, bias, planes=False, seed=0):
        self.b, self.name, self.full, self.beta, self.planes = b, name, full, beta, planes
        Ho = 2 * H if full else H // 2
        self.x = d_act(b, B, Cin, H, seed + 1)
        self.gy = d_act(b, B, Cout, Ho, seed + 2, 0.1)
        d0, d1 = (Cin, Cout) if full else (Cout, Cin)
        self.gw, self.gwbuf = g_act(b, d0, d1, 4, 4)
        self.gw0 = _r((d0, 4, 4, d1), seed + 3).permute(0, 3, 1, 2) if beta else None
        self.gb, self.gbbuf, self.gb0 = None, None, None
        if bias:
            self.gbbuf = guarded(b, Cout)
            self.gb = self.gbbuf[:Cout]
            self.gb0 = _r((Cout,), seed + 4) if beta else None
        self.total = d0 * 16 * d1
        self.kind = "wgrad"
        if planes:
            self.xp, self.gyp = b.planes_split(self.x), b.planes_split(self.gy)
        self._ref = None

    def reset(self):
        if self.gw0 is not None:
            self.gw.copy_(self.gw0.to(self.b.device))
        else:
            self.gw.fill_(float("nan"))
        if self.gb is not None:
            self.gb.copy_(self.gb0.to(self.b.device)) if self.gb0 is not None else self.gb.fill_(float("nan"))

    def launch(self):
        b = self.b
        kw = dict(x_planes=self.xp, gy_planes=self.gyp) if self.planes else {}
        fn = b.deconv2d_bwd_weight if self.full else b.conv2d_bwd_weight
        fn(self.x, self.gy, self.gw, self.gb, 4, 2, 1, float(self.beta), **kw)

    def ref(self):
        if self._ref is None:
            x, gy = f64(self.x), f64(self.gy)
            w = torch.zeros(self.gw.shape, dtype=torch.float64, requires_grad=True)
            out = (F.conv_transpose2d if self.full else F.conv2d)(x, w, None, stride=2, padding=1)
            out.backward(gy)
            gw = w.grad + (f64(self.gw0) * self.beta if self.gw0 is not None else 0)
            gb = None
            if self.gb is not None:
                gb = gy.sum((0, 2, 3)) + (self.gb0.double() * self.beta if self.gb0 is not None else 0)
            self._ref = (gw, gb)
        return self._ref

    def check(self, what):
        gw, gb = self.ref()
        assert untouched(self.gwbuf, self.gw.numel()), "%s: %s wrote past its weight gradient" % (what, self.name)
        assert rel(self.gw, gw) <= TOL, "%s: %s weight gradient %.3e" % (what, self.name, rel(self.gw, gw))
        if gb is not None:
            assert untouched(self.gbbuf, self.gb.numel()), "%s: %s wrote past its bias gradient" % (what, self.name)
            assert rel(self.gb, gb) <= TOL, "%s: %s bias gradient" % (what, self.name)


def _need(b, layer):
    """the slab bytes a recorded layer reserves (rounded to 256 as the recorder does), from its split count at the hint"""
    layer.reset()
    with workspace(b, hint(b)):
        prof = profiled(b, layer.launch)
    layer.check("alone at the hint")
    k = max(split_of(prof, "wgrad", layer.total), split_of(prof, "wgrad_group", layer.total))
    return k, ((k * layer.total * 4 + 255) // 256 * 256) if k > 1 else 0


def test_wgrad_group_under_pressure(wb):
    b = wb
    L1 = WLayer(b, "conv 64->128 32x32", False, 8, 64, 32, 128, 0, True, seed=10)
    L2 = WLayer(b, "full-conv 128->64 16x16", True, 8, 128, 16, 64, 1, True, seed=20)
    L3 = WLayer(b, "conv 128->256 16x16 (planes)", False, 8, 128, 16, 256, 1, True, planes=True, seed=30)
    TH = WLayer(b, "conv 3->64 64x64 (not recordable)", False, 2, 3, 64, 64, 0, True, seed=40)
    L4 = WLayer(b, "conv 64->128 64x64", False, 8, 64, 64, 128, 1, False, seed=50)
    need = {}
    for L in (L1, L2, L3, TH):
        need[L.name] = _need(b, L)
    n1, n2, n3, nt = (need[L.name][1] for L in (L1, L2, L3, TH))
    assert min(n1, n2, n3, nt) > 0, need
    print("slab bytes per layer at the hint:", need)

    # walk A: L1 and L2 fill the workspace, recording L3 flushes them mid-walk; the thin layer fits behind L3's slabs; a partial
    # end launches L3; L4 (whose split count the workspace clamps) is recorded after it and launched by the end
    wsA = n1 + n2 + n3 // 2
    assert n1 + n2 <= wsA < n1 + n2 + n3 and n3 + nt <= wsA
    for L in (L1, L2, L3, TH, L4):
        L.reset()
    counts = []
    with workspace(b, wsA, guard=8 << 20):
        def walk_a():
            b.wgrad_group_begin()
            for L in (L1, L2, L3):
                L.launch()
                counts.append(b.wgrad_group_count())
            TH.launch()
            counts.append(b.wgrad_group_count())
            b.wgrad_group_end_partial(b.wgrad_group_count())
            counts.append(b.wgrad_group_count())
            L4.launch()
            counts.append(b.wgrad_group_count())
            b.wgrad_group_end()
        prof = profiled(b, walk_a)
    assert counts == [1, 2, 1, 1, 0, 1], counts
    groups = {n: e["launches"] for n, e in prof.items() if n.startswith(("wgrad_group", "pwgrad_group"))}
    assert sum(groups.values()) >= 3 and any(n.startswith("pwgrad_group") for n in groups), groups
    for L in (L1, L2, L3, TH, L4):
        L.check("walk A")
    print("walk A, workspace %d: counts %s, group launches %s" % (wsA, counts, groups))

    # walk B: no room behind L1 and L2 for the thin layer's slabs: the group is launched first
    wsB = n1 + n2 + nt - 256
    assert wsB >= max(n1, n2, nt)
    for L in (L1, L2, TH):
        L.reset()
    counts = []
    with workspace(b, wsB, guard=8 << 20):
        def walk_b():
            b.wgrad_group_begin()
            for L in (L1, L2, TH):
                L.launch()
                counts.append(b.wgrad_group_count())
            b.wgrad_group_end()
        profiled(b, walk_b)
    assert counts == [1, 2, 0], counts
    for L in (L1, L2, TH):
        L.check("walk B")


def test_wgrad_group_longer_than_a_table(wb):
    """one walk that records more layers per kernel family than a descriptor table holds (16): 16 planes layers on the 128-row
    tile and a 17th on the 64-row form, 17 fp32-fed layers on each of the 128- and 64-row families.  Every layer is B = 2 on an
    8 x 8 map: one K step, so nothing splits.  Each layer has its own operands, so a descriptor in the wrong slot shows."""
    b = wb
    fams = {"planes": [WLayer(b, "planes conv 64->128 #%d" % i, False, 2, 64, 8, 128, i % 2, False, planes=True, seed=1000 + 10 * i)
                       for i in range(16)]}
    fams["planes"].append(WLayer(b, "planes conv 64->64 #16", False, 2, 64, 8, 64, 0, False, planes=True, seed=1160))
    fams["fp32_128"] = [WLayer(b, "conv 32->128 #%d" % i, False, 2, 32, 8, 128, i % 2, False, seed=2000 + 10 * i) for i in range(17)]
    fams["fp32_64"] = [WLayer(b, "conv 32->64 #%d" % i, False, 2, 32, 8, 64, i % 2, False, seed=3000 + 10 * i) for i in range(17)]
    walk = fams["planes"] + fams["fp32_128"] + fams["fp32_64"]
    for L in walk:
        L.reset()
    counts = []
    with workspace(b, hint(b)):
        def go():
            b.wgrad_group_begin()
            for L in walk:
                L.launch()
            counts.append(b.wgrad_group_count())
            b.wgrad_group_end()
            counts.append(b.wgrad_group_count())
        prof = profiled(b, go)
    assert counts == [len(walk), 0], counts
    for L in walk:
        L.check("one walk of %d layers" % len(walk))
    launches = {n: e["launches"] for n, e in prof.items()}
    print("launches:", launches)
    assert launches.get("pwgrad_group_128x128x32") == 1, launches      # the first table: no 64-row layer counted into its label
    assert launches.get("pwgrad_group_64x128x32") == 1, launches       # the 17th planes record, alone in the second table
    assert "pwgrad_group_64+128x128x32" not in launches, launches
    assert launches.get("wgrad_group_128x128_bf16x3") == 2, launches
    assert launches.get("wgrad_group_64x128_bf16x3") == 2, launches
    assert "slab_reduce_wgrad_group" not in launches and "slab_reduce_wgrad" not in launches, launches
    # alone, outside a group, a layer runs the same tile code over the same single K range: the same bits
    for fam, layers in fams.items():
        for i in (0, 15, 16):
            L = layers[i]
            grouped = L.gw.clone()
            L.reset()
            with workspace(b, hint(b)):
                L.launch()
            L.check("alone")
            assert torch.equal(L.gw, grouped), "%s: grouped and alone differ" % L.name


def test_wgrad_group_protocol(wb):
    """begin / end / abort / end_partial: what each leaves recorded, launched and open"""
    b = wb
    L = WLayer(b, "conv 32->128 8x8", False, 2, 32, 8, 128, 0, False, seed=4000)
    M = WLayer(b, "conv 32->64 8x8", False, 2, 32, 8, 64, 0, False, seed=4010)

    def all_nan(t):
        b.synchronize()
        return bool(torch.isnan(t).all())

    with workspace(b, hint(b)):
        with pytest.raises(RuntimeError, match="no group is open"):
            b.wgrad_group_end()
        # a walk abandoned before its end: the next begin drops its records, nothing of it is launched
        L.reset()
        b.wgrad_group_begin()
        L.launch()
        assert b.wgrad_group_count() == 1
        b.wgrad_group_begin()
        assert b.wgrad_group_count() == 0
        b.wgrad_group_end()
        assert all_nan(L.gw), "a record of the abandoned walk was launched"
        # abort: records dropped, group closed; the next launch runs at once
        b.wgrad_group_begin()
        L.launch()
        b.wgrad_group_abort()
        assert b.wgrad_group_count() == 0
        assert all_nan(L.gw), "abort launched a record"
        L.launch()
        L.check("ungrouped, after an abort")
        with pytest.raises(RuntimeError, match="no group is open"):
            b.wgrad_group_end()
        # a partial end of at least everything recorded: all launched, the group stays open and takes further records
        L.reset()
        M.reset()
        b.wgrad_group_begin()
        L.launch()
        b.wgrad_group_end_partial(5)
        assert b.wgrad_group_count() == 0
        L.check("launched by end_partial")
        M.launch()
        assert b.wgrad_group_count() == 1 and all_nan(M.gw)
        b.wgrad_group_end()
        M.check("recorded after end_partial")
        L.check("after the end")


# ---------------------------------------------------------------------------------------------------------------- routes
def test_thin_output_column_buffer_threshold(wb):
    """the transposed passes with 4 < N < 32 outputs take the column buffer + col2im4x4 only if col_bytes + 32 MB fit: the video
    netG's last layer (64 -> 12 full-conv, 32 -> 64) and, with the derivative mask, netD's 12-channel first layer's data
    gradient"""
    b = wb
    B, C, H, N = 2, 64, 32, 12
    col = B * H * H * 16 * N * 4
    thr = col + (32 << 20)
    cases = [Pass(b, "deconv_fwd", B, C, H, N, act="relu", seed=5), Pass(b, "bwd_data", B, N, 2 * H, C, seed=6)]
    for p in cases:
        for dm in ((None,) if p.kind == "deconv_fwd" else (None, "mask")):
            dmask = want = None
            want = p.ref()
            if dm:
                dmask = d_act(b, *p.out_shape[:3], 7)
                want = torch.where(f64(dmask) > 0, want, SLOPE * want)
            got = {}
            for ws in (thr, thr - 4):
                y, k, route = p.run(ws, dmask)
                assert rel(y, want) <= TOL, "%s at %d (%s)" % (p.name, ws, route)
                got[ws] = (route, k)
            assert "col2im4x4" in got[thr][0] and "col2im4x4" not in got[thr - 4][0], got
            print("%s%s: %s" % (p.name, " + dmask" if dm else "", got))


def test_bottleneck_weight_streaming_threshold(wb):
    """the bottleneck pair at B = 2 (512 x 4 x 4 <-> 4000): smallm_rowdot / smallm_axpy if their ksplit * M * N floats of slabs
    fit, else a tile"""
    b = wb
    B, C, Z = 2, 512, 4000
    x = d_act(b, B, C, 4, 60)
    w = d_w(b, Z, C, 61, 0.02)
    bias = _r((Z,), 62, 0.1).to(b.device)
    z = d_act(b, B, Z, 1, 63)
    bias2 = _r((C,), 64, 0.1).to(b.device)
    ref_f = act64(F.conv2d(f64(x), f64(w), f64(bias)), "lrelu")
    ref_t = act64(F.conv_transpose2d(f64(z), f64(w), f64(bias2)), "relu")
    forms = [("smallm_rowdot", (B, Z, 1, 1), lambda y: b.conv2d_fwd(x, w, bias, y, 4, 1, 0, "lrelu", SLOPE), ref_f),
             ("smallm_axpy", (B, C, 4, 4), lambda y: b.deconv2d_fwd(z, w, bias2, y, 4, 1, 0, "relu", SLOPE), ref_t)]
    for kname, shape, launch, ref in forms:
        n = shape[0] * shape[1] * shape[2] * shape[3]
        res = []
        for ws in [hint(b)] + ([None] * 2):
            if ws is None:
                ws = res[0][1] * 4 * n - (0 if len(res) == 1 else 4)
            y, ybuf = g_act(b, *shape)
            with workspace(b, ws):
                prof = profiled(b, lambda: launch(y))
            assert untouched(ybuf, n)
            k = split_of(prof, "igemm", n)
            assert rel(y, ref) <= TOL, (kname, ws, route_of(prof))
            res.append((route_of(prof), k, ws))
        assert kname in res[0][0] and res[0][1] >= 2, res
        assert kname in res[1][0] and res[1][1] == res[0][1], res
        assert kname not in res[2][0] and "igemm" in res[2][0], res
        assert res[2][1] == 1 or res[2][1] * 4 * n <= res[2][2], res
        print("%s: (route, ksplit, workspace) %s" % (kname, res))


def test_generic_weight_gradient_slabs(wb):
    """the option branches' 5 x 5 stride-2 conv (vf_conv_generic.hip): its weight gradient takes as many partial-sum slabs as fit,
    down to one; below one it refuses.  (The bias gradient's partials need more than one slab here: only the runs at the hint
    take it.)"""
    b = wb
    B, Cin, H, Cout, k = 3, 3, 32, 64, 5
    x = d_act(b, B, Cin, H, 70)
    gy = d_act(b, B, Cout, H // 2, 71)
    xr, gyr = f64(x), f64(gy)
    w = torch.zeros((Cout, Cin, k, k), dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, w, None, stride=2, padding=2).backward(gyr)
    want_w, want_b = w.grad, gyr.sum((0, 2, 3))
    per_slab = Cout * k * k * Cin * 4
    for ws in (hint(b), 4 * per_slab, per_slab, 0, per_slab - 4, hint(b)):
        gw, gwbuf = g_act(b, Cout, Cin, k, k)
        gbbuf = guarded(b, Cout)
        gb = gbbuf[:Cout] if ws == hint(b) else None
        with workspace(b, ws):
            if ws < per_slab:
                with pytest.raises(RuntimeError):
                    b.conv2d_bwd_weight(x, gy, gw, gb, k, 2, 2, 0.0)
                continue
            b.conv2d_bwd_weight(x, gy, gw, gb, k, 2, 2, 0.0)
        assert untouched(gwbuf, gw.numel()) and untouched(gbbuf, Cout)
        assert rel(gw, want_w) <= TOL, ws
        if gb is not None:
            assert rel(gb, want_b) <= TOL


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_partials_refuse_a_small_workspace(wb):
    """BatchNorm statistics and conv bias-gradient partials need a workspace: below their minimum they raise; the same context
    then gives the fp64 answer with room"""
    b = wb
    B, Cc, H = 4, 64, 8
    x = d_act(b, B, Cc, H, 80)
    gamma, beta = (1 + _r((Cc,), 81, 0.1)).to(b.device), _r((Cc,), 82, 0.1).to(b.device)
    xr = f64(x)
    mean = xr.mean((0, 2, 3), keepdim=True)
    var = xr.var((0, 2, 3), unbiased=False, keepdim=True)
    want_y = (xr - mean) / torch.sqrt(var + 1e-5) * f64(gamma).view(1, -1, 1, 1) + f64(beta).view(1, -1, 1, 1)

    def bn_fwd(y):
        rm, rv = b.zeros(Cc), b.zeros(Cc) + 1
        sm, si, su = b.zeros(Cc), b.zeros(Cc), b.zeros(2 * Cc, dtype=torch.float64)
        b.bn_train_fwd_groups(x, y, gamma, beta, rm, rv, sm, si, su, 1, 0.1, 1e-5)
        return sm, si, su

    gy = d_act(b, B, Cc, H, 83)
    w = d_w(b, Cc, 32, 84)
    xin = d_act(b, B, 32, 2 * H, 85)
    want_gb = f64(gy).sum((0, 2, 3))
    for ws in (0, 64):
        with workspace(b, ws):
            y, _ = g_act(b, B, Cc, H, H)
            with pytest.raises(RuntimeError):
                bn_fwd(y)
            gw, _ = g_act(b, Cc, 32, 4, 4)
            with pytest.raises(RuntimeError):
                b.conv2d_bwd_weight(xin, gy, gw, b.zeros(Cc), 4, 2, 1, 0.0)
    with workspace(b, hint(b)):
        y, ybuf = g_act(b, B, Cc, H, H)
        sm, si, su = bn_fwd(y)
        gbbuf = guarded(b, Cc)
        gw, _ = g_act(b, Cc, 32, 4, 4)
        b.conv2d_bwd_weight(xin, gy, gw, gbbuf[:Cc], 4, 2, 1, 0.0)
    assert untouched(ybuf, y.numel()) and untouched(gbbuf, Cc)
    assert rel(y, want_y) <= TOL
    assert rel(gbbuf[:Cc], want_gb) <= TOL


# ---------------------------------------------------------------------------------------------------------------- one-shot
@pytest.mark.parametrize("refused", ["conv_B0", "pconv_shape"])
def test_refused_call_drops_the_batchnorm_attachment(refused, wb):
    """vf_bn_fuse_next_bwd, then a conv call the library refuses, then a valid data-gradient pass whose output has the
    attachment's shape and whose `part` has room: that pass must not take the attachment (its output stays unmasked, `part`
    untouched, bn_fuse_result() 0).  A stale attachment would store the output masked by another tensor's derivative."""
    b = wb
    f = BnFused(b, 2, "bwd_data", 8, 256, 8, 512, 1)
    n = 1024 * 2 * f.C
    part = guarded(b, n, torch.float64)
    y, ybuf = g_act(b, *f.p.out_shape)
    with workspace(b, hint(b)):
        b.bn_fuse_next_bwd(f.x, f.yact, "lrelu", SLOPE, f.mean, part[:n], 1)
        with pytest.raises(RuntimeError):
            if refused == "conv_B0":
                b.conv2d_bwd_data(f.p.x[:0], f.p.w, y[:0], 4, 2, 1)
            else:
                xp = b.planes_split(b.zeros(4 * 8 * 8 * 48))
                b.pconv_gather(xp, b.planes_split(b.zeros(64 * 16 * 48)), None, b.zeros(4 * 4 * 4 * 64), 4, 8, 8, 48, 64)
        f.p.launch(y)
        R = b.bn_fuse_result()
    assert untouched(ybuf, f.p.n_out)
    assert untouched(part, 0), "the pass after the refused call wrote BatchNorm partial rows"
    assert R == 0, "the pass after the refused call took the attachment (%d rows)" % R
    assert rel(y, f.p.ref()) <= TOL, "the pass after the refused call stored a masked output"
