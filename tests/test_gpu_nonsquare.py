"""Every conv route of the C-ABI on NON-SQUARE maps (tests/nonsquare_cases.py: the table, the operands, the fp64 reference;
tests/test_nonsquare_ref.py: why this test cannot pass vacuously).

Per case and product mode, two runs of every pass of the case:
  int    integer-valued operands: the device result equals the fp64 reference BIT FOR BIT, in every element, whichever kernel,
         split count or summation order served the pass — no tolerance;
  rand   randn operands against fp64 at the suite's own bars (2e-5 of the max-norm; 3e-5 in the bf16 mode against the
         rounded-operand reference).
Every tensor a pass writes is a guarded buffer (NaN body: an element no launch wrote fails the comparison; guard tail: a write past
the end fails), and every pass asserts from the library's launch list the route its group is named after.  (case, mode, pass,
route) is printed: pytest -rP shows the table reached.  A pass the library refuses (a stated limit of the generic weight gradient;
shapes the planes GEMM does not serve) is asserted to be refused before anything is written."""
import pytest
import torch

import nonsquare_cases as NS
from helpers import guarded, untouched

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
WORST = {}      # (group, mode) -> (worst random-run error / its bar, error, bar, where)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (group, mode), (ratio, e, bar, where) in sorted(WORST.items()):
        print("worst random-run error, group %s mode %s: %.3e against %.1e (%.2f of the bar) at %s" % (group, mode, e, bar, ratio, where))


@pytest.fixture()
def in_mode(hipb):
    prev = hipb.mfma_mode

    def set_mode(mode):
        hipb.set_mfma_mode(NS.MODES[mode])
    yield set_mode
    hipb.set_mfma_mode(prev)


def dev(b, t):
    """CPU float32 -> device; 4-D tensors logical NCHW / physical NHWC"""
    t = t.to(b.device)
    if t.dim() == 4:
        t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return t


def g_act(b, B, Cc, H, W):
    """a guarded channels-last tensor (logical B x Cc x H x W) -> (tensor, backing buffer)"""
    n = B * Cc * H * W
    buf = guarded(b, n)
    return buf[:n].view(B, H, W, Cc).permute(0, 3, 1, 2), buf


def nan_planes(b, n):
    return torch.full((3, n), float("nan"), dtype=torch.bfloat16, device=b.device)


class Run:
    """the passes of one case in one mode with one set of operands"""

    def __init__(self, b, case, mode, kind):
        self.b, self.c, self.mode, self.kind = b, case, mode, kind
        o = NS.operands(case, kind)
        self.d = {k: dev(b, v) for k, v in o.items()}
        self.ref = NS.reference(case, kind, rounded=(mode == 1))
        self.tol = None if kind == "int" else NS.TOL[mode]
        self.routes = []

    # ---- checks
    def same(self, got, key, what, tol=None):
        ref = self.ref[key]
        if self.tol is None:
            msg = NS.exact_mismatch(got, ref)
            assert msg is None, "%s mode %d %s: %s" % (self.c.id, self.mode, what, msg)
            return
        bar = tol or self.tol
        e = NS.rel_err(got, ref)
        k = (self.c.group, self.mode)
        if not e <= WORST.get(k, (0.0,))[0] * bar:
            WORST[k] = (e / bar, e, bar, "%s %s" % (self.c.id, what))
        print("    %s mode %d %s: %.3e of the max-norm (bar %.1e)" % (self.c.id, self.mode, what, e, bar))
        assert e <= bar, "%s mode %d %s: error %.3e against fp64, bar %.1e" % (self.c.id, self.mode, what, e, bar)

    def launch(self, pname, fn, *bufs):
        """fn() under the profile; its route; the guard tails of the buffers it wrote"""
        b, c = self.b, self.c
        if pname in c.refused or getattr(self, "_unsupported", False):
            msg = c.refused.get(pname, "unsupported shape")
            with pytest.raises(RuntimeError, match=msg):
                fn()
            b.synchronize()
            for buf, n in bufs:
                assert bool(torch.isnan(buf[:n].float()).all()) and untouched(buf, n), "%s %s: a refused call wrote" % (c.id, pname)
            print("(%s, mode %d, %s, REFUSED: %s)" % (c.id, self.mode, pname, msg))
            return False
        b.prof_begin()
        try:
            fn()
        finally:
            prof = b.prof_end()
        b.synchronize()
        for buf, n in bufs:
            assert untouched(buf, n), "%s mode %d %s: a kernel wrote past its output" % (c.id, self.mode, pname)
        names = sorted(prof)
        want = NS.pwgrad_route(self.mode, c) if pname.startswith("pwgrad") else c.routes[pname]
        assert any(n.startswith(p) for n in names for p in want), "%s mode %d %s: launches %s, none of %s" % (c.id, self.mode, pname, names, want)
        self.routes.append((pname, names))
        if self.tol is None:
            print("(%s, mode %d, %s, %s)" % (c.id, self.mode, pname, "+".join(names)))
        return True

    # ---- passes
    def run(self):
        for pname in self.c.passes:
            self._unsupported = False
            getattr(self, "p_" + pname.replace("_b0", "").replace("_b1", ""))(pname)

    def _fns(self):
        b = self.b
        return ((b.deconv2d_fwd, b.deconv2d_bwd_data, b.deconv2d_bwd_weight) if self.c.full else
                (b.conv2d_fwd, b.conv2d_bwd_data, b.conv2d_bwd_weight))

    def _geo(self):
        return self.c.k, self.c.s, self.c.p

    def p_fwd(self, pname, act="none", key="fwd"):
        c, d = self.c, self.d
        y, ybuf = g_act(self.b, c.B, c.Cout, c.Ho, c.Wo)
        if self.launch(pname, lambda: self._fns()[0](d["x"], d["w"], d["bias"], y, *self._geo(), act, NS.SLOPE), (ybuf, y.numel())):
            self.same(y, key, pname)

    def p_fwd_act(self, pname):
        self.p_fwd(pname, self.c.act, "fwd_act")

    def p_fwd_planes(self, pname):
        c, d, b = self.c, self.d, self.b
        y, ybuf = g_act(b, c.B, c.Cout, c.Ho, c.Wo)
        n = y.numel()
        yp = nan_planes(b, n)
        self.launch(pname, lambda: b.conv2d_fwd_planes(d["x"], d["w"], d["bias"], y, yp, *self._geo(), "relu", 0.0), (ybuf, n))
        self.same(y, "fwd_relu", pname)
        flat = ybuf[:n]
        if self.mode == 1:      # one plane: y rounded to bf16
            assert torch.equal(yp[0].float().cpu(), NS.bf16_round(flat.cpu())), "%s %s: the plane is not bf16(y)" % (c.id, pname)
        else:                   # three planes: an exact split
            assert torch.equal(yp.double().sum(0), flat.double()), "%s %s: the planes do not sum to y" % (c.id, pname)

    def p_bwd_data(self, pname):
        c, d = self.c, self.d
        gx, gxbuf = g_act(self.b, c.B, c.Cin, c.H, c.W)
        if self.launch(pname, lambda: self._fns()[1](d["gy"], d["w"], gx, *self._geo()), (gxbuf, gx.numel())):
            self.same(gx, "bwd_data", pname)

    def p_bwd_data_act(self, pname):
        c, d = self.c, self.d
        gx, gxbuf = g_act(self.b, c.B, c.Cin, c.H, c.W)
        self.launch(pname, lambda: self.b.conv2d_bwd_data_act(d["gy"], d["w"], gx, d["xact"], "lrelu", NS.SLOPE, *self._geo()), (gxbuf, gx.numel()))
        self.same(gx, "bwd_data_act", pname)

    def p_bwd_weight(self, pname, planes=False):
        c, d, b = self.c, self.d, self.b
        beta = int(pname[-1])
        gw, gwbuf = g_act(b, *c.w_shape)
        gbbuf = guarded(b, c.Cout)
        gb = gbbuf[:c.Cout]
        if beta and pname not in c.refused:
            gw.copy_(d["gw0"])
            gb.copy_(d["gb0"])
        kw = dict(x_planes=b.planes_split(d["x"]), gy_planes=b.planes_split(d["gy"])) if planes else {}
        if self.launch(pname, lambda: self._fns()[2](d["x"], d["gy"], gw, gb, *self._geo(), float(beta), **kw),
                       (gwbuf, gw.numel()), (gbbuf, c.Cout)):
            self.same(gw, "gw_b%d" % beta, pname + " gradWeight")
            self.same(gb, "gb_b%d" % beta, pname + " gradBias", NS.TOL_BIAS_GRAD)

    def p_pwgrad(self, pname):
        self.p_bwd_weight(pname, planes=True)

    # the planes passes of a conv layer: gather x -> y; scatter gy (low-resolution map) -> gx, plain, with the derivative mask, and
    # as the forward of the full-conv Cout -> Cin that shares the weight's layout (bias + ReLU)
    def _planes(self, transposed):
        b, c, d = self.b, self.c, self.d
        self._unsupported = not NS.pconv_supported(self.mode, c, transposed)
        co, ci = (c.Cin, c.Cout) if transposed else (c.Cout, c.Cin)
        geo = (c.B, c.Ho, c.Wo) if transposed else (c.B, c.H, c.W)
        assert bool(b.lib.vf_pconv_supported_in_mode(self.mode, *geo, ci, co, 4, 2, 1, int(transposed))) != self._unsupported, c.id
        nat, tr = b.weight_planes(d["w"])
        return b.planes_split(d["gy" if transposed else "x"]), (tr if transposed else nat)

    def p_pconv_gather(self, pname):
        c, d, b = self.c, self.d, self.b
        xp, wp = self._planes(False)
        y, ybuf = g_act(b, c.B, c.Cout, c.Ho, c.Wo)
        if self.launch(pname, lambda: b.pconv_gather(xp, wp, d["bias"], y, c.B, c.H, c.W, c.Cin, c.Cout, "lrelu", NS.SLOPE), (ybuf, y.numel())):
            self.same(y, "fwd_lrelu", pname)

    def p_pconv_scatter(self, pname, key="bwd_data", **kw):
        c, d, b = self.c, self.d, self.b
        gp, wp = self._planes(True)
        gx, gxbuf = g_act(b, c.B, c.Cin, c.H, c.W)
        args = kw.pop("args", (None,))
        if self.launch(pname, lambda: b.pconv_scatter(gp, wp, args[0], gx, c.B, c.Ho, c.Wo, c.Cout, c.Cin, *args[1:], **kw), (gxbuf, gx.numel())):
            self.same(gx, key, pname)

    def p_pconv_scatter_mask(self, pname):
        self.p_pconv_scatter(pname, "bwd_data_act", dmask=self.d["xact"], dact="lrelu", dslope=NS.SLOPE)

    def p_pconv_scatter_fwd(self, pname):
        self.p_pconv_scatter(pname, "scatter_fwd", args=(self.d["bias_t"], "relu", 0.0))

    # BatchNorm statistics as by-products: partial rows [R][2][C] in fp64
    def _sums(self, pname, part, R, C, stored, terms_of, key):
        assert R >= 2, "%s %s: the by-product did not run (rows per group %d)" % (self.c.id, pname, R)
        assert untouched(part, R * 2 * C), "%s %s: rows beyond R were written" % (self.c.id, pname)
        rows = part[:R * 2 * C].cpu().view(R, 2, C).sum(0)
        if self.tol is None:
            msg = NS.exact_mismatch(rows, self.ref[key])
            assert msg is None, "%s %s sums: %s" % (self.c.id, pname, msg)
            return
        # BnFused.check_sums (tests/test_gpu_workspace.py): against fp64 sums over the output the kernel stored, each partial row an
        # fp32 sum of at most n_row terms formed with two roundings: (n_row + 2) * u * sum |term|
        sv = stored.detach().to("cpu", torch.float64)
        n_row = sv.numel() / C / R
        for i, t in enumerate(terms_of(sv)):
            bound = (n_row + 2) * U * t.abs().sum((0, 2, 3)) + 1e-30
            err = (rows[i] - t.sum((0, 2, 3))).abs()
            assert bool((err <= bound).all()), "%s %s: sum %d off by %.2f times the bound" % (self.c.id, pname, i + 1, float((err / bound).max()))

    def p_bn_fwd(self, pname):
        c, d, b = self.c, self.d, self.b
        n = 1024 * 2 * c.Cout
        part = guarded(b, n, torch.float64)
        y, ybuf = g_act(b, c.B, c.Cout, c.Ho, c.Wo)
        res = {}

        def go():
            b.bn_fuse_next_fwd(d["shift"], part[:n], 1)
            b.conv2d_fwd(d["x"], d["w"], d["bias"], y, *self._geo())
            res["R"] = b.bn_fuse_result()
        self.launch(pname, go, (ybuf, y.numel()), (part, n))
        self.same(y, "fwd", pname)
        shift = NS.operands(c, self.kind)["shift"].double().view(1, -1, 1, 1)
        self._sums(pname, part, res["R"], c.Cout, y, lambda v: (v - shift, (v - shift) ** 2), "bn_fwd_sums")
        print("(%s, mode %d, %s, rows per group %d)" % (c.id, self.mode, pname, res["R"]))

    def p_bn_bwd(self, pname):
        c, d, b = self.c, self.d, self.b
        n = 1024 * 2 * c.Cin
        part = guarded(b, n, torch.float64)
        gx, gxbuf = g_act(b, c.B, c.Cin, c.H, c.W)
        res = {}

        def go():
            b.bn_fuse_next_bwd(d["bn_x"], d["bn_yact"], "lrelu", NS.SLOPE, d["mean"], part[:n], 1)
            b.conv2d_bwd_data(d["gy"], d["w"], gx, *self._geo())
            res["R"] = b.bn_fuse_result()
        self.launch(pname, go, (gxbuf, gx.numel()), (part, n))
        self.same(gx, "bn_bwd", pname)
        o = NS.operands(c, self.kind)
        xm = o["bn_x"].double() - o["mean"].double().view(1, -1, 1, 1)
        self._sums(pname, part, res["R"], c.Cin, gx, lambda v: (v, v * xm), "bn_bwd_sums")
        print("(%s, mode %d, %s, rows per group %d)" % (c.id, self.mode, pname, res["R"]))


PARAMS = [pytest.param(c, m, id="%s-mode%d" % (c.id, m)) for c in NS.CASES for m in c.modes]


@pytest.mark.parametrize("kind", ["int", "rand"])
@pytest.mark.parametrize("case,mode", PARAMS)
def test_nonsquare(case, mode, kind, hipb, in_mode):
    in_mode(mode)
    Run(hipb, case, mode, kind).run()


# ---------------------------------------------------------------------------------------------------------------- net chain
def _chain(nn):
    BN = nn.SpatialBatchNormalization
    conv = lambda i, o: nn.SpatialConvolution(i, o, 4, 4, 2, 2, 1, 1)
    full = lambda i, o: nn.SpatialFullConvolution(i, o, 4, 4, 2, 2, 1, 1)
    smooth = lambda: nn.LeakyReLU(1.0, True)
    return [conv(3, 64), smooth(), conv(64, 128), BN(128), smooth(), conv(128, 64), BN(64), smooth(), full(64, 128), BN(128), smooth(),
            full(128, 32), BN(32), smooth(), full(32, 3), nn.Tanh()]


@pytest.mark.parametrize("gate", ["dropped", "shipped"])
@pytest.mark.parametrize("shape", NS.NET_INPUTS, ids=lambda s: "B%d-%dx%d" % (s[0], s[2], s[3]))
def test_net_chain(shape, gate, hipb):
    """an encoder-decoder through the library's net object (vf_net, cnet.CNet) on a non-square input, with the planes gate dropped
    (every pass of >= 1 GEMM row that the planes kernels serve takes them) and as shipped; the smooth form of tests/test_gpu_net.py:
    LeakyReLU(1.0) in place of every (Leaky)ReLU, so no element sits near a kink; fp64 torch with autograd is the reference"""
    from video_filler_amd import _lib, nn
    from video_filler_amd.cnet import CNet, adopt_if_chain
    old = (nn._PCONV_MIN_GFLOP, nn._PCONV_MIN_ROWS)
    nn._PCONV_MIN_GFLOP, nn._PCONV_MIN_ROWS = (0.0, 0) if gate == "dropped" else (nn.PCONV_MIN_GFLOP_SHIPPED, 1024)
    try:
        seq = nn.Sequential(True, True)
        for m in _chain(nn):
            seq.add(m)
        net = adopt_if_chain(seq)
        assert isinstance(net, CNet)
        net.getParameters()
        g = torch.Generator().manual_seed(77 + shape[3])
        segs = net._flat[2]
        host = [torch.randn(tuple(getattr(m, name).shape), generator=g) * 0.05 + (1.0 if "BatchNorm" in m.type_name() and name == "weight" else 0.0)
                for m, name, _, _, _ in segs]
        net.load_reference_flat(torch.cat([t.reshape(-1) for t in host]).to(hipb.device))
        x, gy = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
        net.zeroGradParameters()
        hipb.prof_begin()
        try:
            y = net.forward(dev(hipb, x))
            gx = net.backward(dev(hipb, x), dev(hipb, gy))
        finally:
            prof = hipb.prof_end()
        hipb.synchronize()
        eps = {m.eps for m in net.leaves() if isinstance(m, nn.SpatialBatchNormalization)}
        assert len(eps) == 1
        params = [t.double().requires_grad_() for t in host]
        xr = x.double().requires_grad_()
        yr = NS.torch_chain(params, eps.pop())(xr)
        yr.backward(gy.double())
        print("(net chain %s, gate %s, launches %s)" % (shape, gate, "+".join(sorted(prof))))
        e = NS.rel_err(y, yr.detach())
        print("    output %.3e (bar %.1e)" % (e, NS.NET_TOL_OUT))
        assert e <= NS.NET_TOL_OUT, e
        e = NS.rel_err(gx, xr.grad)
        print("    gradInput %.3e (bar %.1e)" % (e, NS.NET_TOL_GRAD))
        assert e <= NS.NET_TOL_GRAD, e
        # tests/test_gpu_net.py's bar: a module's two tensors share one scale — the bias of a convolution in front of a BatchNorm has
        # a TRUE gradient of 0 (the fp64 reference leaves 1e-17 there), so its error is measured against the module's weight gradient
        scale = {}
        for (m, _, _, _, _), p in zip(segs, params):
            scale[id(m)] = max(scale.get(id(m), 0.0), float(p.grad.abs().max()))
        for (m, name, gname, _, _), p in zip(segs, params):
            e = float((getattr(m, gname).detach().to("cpu", torch.float64) - p.grad).abs().max()) / scale[id(m)]
            print("    %s.%s %s %.3e" % (m.type_name(), gname, tuple(p.shape), e))
            assert e <= NS.NET_TOL_GRAD, (m.type_name(), gname, e)
        if gate == "dropped":
            assert any(n.startswith("pconv_") for n in prof), sorted(prof)
    finally:
        nn._PCONV_MIN_GFLOP, nn._PCONV_MIN_ROWS = old
        _lib.check(hipb.lib.vf_net_set_planes_gate(float(old[0]), int(old[1])))
