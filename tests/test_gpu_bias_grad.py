"""Conv bias gradients on their own, against tests/bias_grad_ref.py: the single-tensor route (vf_internal_colsum -> k_colsum4 / k_colsum1 ->
k_reduce_partials<2>, reached through a vf_conv2d_bwd_weight call with gb != NULL) and the whole-walk route (HipBackend.bias_grad_multi ->
k_colsum4_multi -> k_reduce_bias_multi), at the (P, C) cases of bias_grad_ref.CASES / MULTI_TABLES (tests/test_bias_grad_ref.py checks on
the CPU that each case reaches the block geometry it is there for).

Every case runs on a backend of the test's own whose workspace lies inside a guard band (helpers.workspace, guards on both sides); every
gradBias is a slice of a guarded buffer with guard words in front of and behind it.  Checks, both routes:
  - exact inputs (integers; see bias_grad_ref) with beta in {0, 1} (the tables also 0.5 on even gb0): the result is the integer sum, bit
    for bit; with beta = 0 the gradBias is pre-filled with NaN and must come out finite;
  - random inputs (mean 1): within the derived bound of the float64 reference, per element;
  - the same call twice: the same bits (the kernels sum in a fixed order);
  - the profile names the launch that was meant (bias_grad / bias_grad_multi).
And: plans built under one workspace must not write into it after the context was pointed at another (HipBackend.bias_grad_multi's plan
cache, vf_net's bias_grad_flush)."""
import numpy as np
import pytest
import torch

import bias_grad_ref as R
from helpers import TAIL32, WS_FILL, guarded, set_workspace, untouched, workspace

pytestmark = pytest.mark.gpu

WS = 4 << 20                     # the workspace of every case: the largest partials here take 2.7 MB (the 13-layer table)
FRONT = 1 << 16                  # guard bytes in front of it
GB_FRONT = 64                    # guard words in front of a gradBias


@pytest.fixture(scope="module")
def wb():
    """a backend of its own: the shared `hipb` serves the nn modules and the other tests and keeps its workspace"""
    from video_filler_amd.backend import HipBackend
    b = HipBackend(workspace_bytes=1 << 20)
    yield b
    b.synchronize()


def profiled(b, fn):
    b.prof_begin()
    try:
        fn()
    finally:
        prof = b.prof_end()
    return prof


class Out:
    """a gradBias of C floats between guard words"""

    def __init__(self, b, C):
        self.C = C
        self.buf = guarded(b, GB_FRONT + C)
        self.buf[:GB_FRONT].view(torch.int32).fill_(TAIL32)
        self.gb = self.buf[GB_FRONT:GB_FRONT + C]

    def set(self, gb0):
        """gb0 None: NaN (a beta = 0 call must not read it)"""
        if gb0 is None:
            self.gb.fill_(float("nan"))
        else:
            self.gb.copy_(torch.from_numpy(gb0).to(self.gb.device))

    def get(self, what):
        assert untouched(self.buf, 0, GB_FRONT) and untouched(self.buf, GB_FRONT + self.C), "%s: written outside the gradBias" % what
        return self.gb.cpu().numpy().copy()


def upload(b, g, misalign=False):
    """[P][C] numpy -> flat device tensor, 16-byte aligned; misalign: one float past a 16-byte boundary"""
    n = g.size
    buf = torch.empty(n + 4, dtype=torch.float32, device=b.device)
    t = buf[1:1 + n] if misalign else buf[:n]
    t.copy_(torch.from_numpy(g.reshape(-1)).to(b.device))
    assert t.data_ptr() % 16 == (4 if misalign else 0)
    return t


class SingleCall:
    """the cheapest vf_conv2d_bwd_weight with a bias gradient over [P][C]: a 1 x 1 convolution of ONE input channel on a 1 x H x W map
    (vf_conv_generic.hip; any H x W, hence any P); for C = 4000, beyond that kernel's staging tile, the bottleneck convolution (4 x 4,
    stride 1) of 16 channels on a 4 x 4 map with batch P.  Both end in vf_internal_colsum(gy, gb, P, C, beta)."""

    def __init__(self, b, P, C):
        self.b, self.P, self.C = b, P, C
        if C <= 1000:
            H = max(d for d in range(1, 65) if P % d == 0)
            self.x = torch.zeros((1, H, P // H, 1), device=b.device).permute(0, 3, 1, 2)
            self.gw = torch.empty((C, 1, 1, 1), device=b.device).permute(0, 3, 1, 2)
            self.geom = (1, 1, 0)
        else:
            self.x = torch.zeros((P, 4, 4, 16), device=b.device).permute(0, 3, 1, 2)
            self.gw = torch.empty((C, 4, 4, 16), device=b.device).permute(0, 3, 1, 2)
            self.geom = (4, 1, 0)

    def __call__(self, g, out, beta):
        """g: flat device tensor of P * C floats (only its address is passed on)"""
        prof = profiled(self.b, lambda: self.b.conv2d_bwd_weight(self.x, g, self.gw, out.gb, *self.geom, float(beta)))
        e = prof.get("bias_grad")
        assert e is not None and e["launches"] == 1 and e["bytes"] == 4.0 * self.P * self.C, prof
        assert "bias_grad_multi" not in prof, prof


def check_exact(got, want, what):
    assert np.isfinite(got).all(), "%s: not finite" % what
    bad = np.flatnonzero(got.astype(np.float64) != want)
    assert bad.size == 0, "%s: %d of %d columns differ from the integer sum, first column %d: got %r want %r" % (
        what, bad.size, want.size, bad[0], got[bad[0]], want[bad[0]])


def check_bound(got, g, gb0, beta, n_t, what):
    ref, bnd = R.ref64(g, gb0, beta), R.bound(g, gb0, beta, n_t)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / bnd).max())
    print("%s: worst error %.3f of the bound (n_t = %d)" % (what, worst, n_t))
    assert np.isfinite(got).all() and (err <= bnd).all(), "%s: %.3f times the bound at column %d" % (what, worst, int((err / bnd).argmax()))


def n_t_of(b, case):
    if case["route"] == "f4":
        return R.rows_per_thread("f4", R.plan_from_library(b.lib, case["P"], case["C"]))
    return R.rows_per_thread("scalar", R.scalar_geom(case["P"], case["C"]))


# ---------------------------------------------------------------------------------------------------------------- single route
SINGLE = [("f4", Cc) for Cc in (4, 12, 64, 256, 260, 512, 4000)] + [("scalar", Cc) for Cc in (1, 3, 5, 6, 8)]


@pytest.mark.parametrize("route,Cc", SINGLE, ids=lambda v: str(v))
def test_single_route(route, Cc, wb):
    b = wb
    out = Out(b, Cc)
    mis = route == "scalar" and Cc % 4 == 0
    gb0_e, gb0_r = R.exact_gb0(Cc, 5), R.random_gb0(Cc, 11)
    for case in R.cases(route, Cc):
        P, what = case["P"], case["id"]
        call = SingleCall(b, P, Cc)
        g_e, g_r = R.exact_g(P, Cc, 5), R.random_g(P, Cc, 11)
        d_e, d_r = upload(b, g_e, mis), upload(b, g_r, mis)
        with workspace(b, WS, front=FRONT):
            out.set(None)
            call(d_e, out, 0.0)
            check_exact(out.get(what), R.ref64(g_e, gb0_e, 0.0), what + " exact beta 0 over NaN")
            out.set(gb0_e)
            call(d_e, out, 1.0)
            check_exact(out.get(what), R.ref64(g_e, gb0_e, 1.0), what + " exact beta 1")
            n_t = n_t_of(b, case)
            res = []
            for beta in (0.0, 0.5, 0.5):
                out.set(gb0_r if beta else None)
                call(d_r, out, beta)
                res.append(out.get(what))
                check_bound(res[-1], g_r, gb0_r, beta, n_t, "%s random beta %g" % (what, beta))
            assert res[1].tobytes() == res[2].tobytes(), "%s: the same call twice gave different bits" % what


@pytest.mark.parametrize("P,Cc", [(261889, 1), (87041, 3)], ids=lambda v: str(v))
def test_scalar_route_leaves_the_restated_slabs(P, Cc, wb):
    """bias_grad_ref.scalar_geom restates vf_internal_colsum's slab arithmetic for k_colsum1; this pins it: after one call (the profile
    names it, with 4 * P * C bytes) the workspace holds exactly nslab partial rows of C doubles — the ones the emulation forms from the
    exact inputs, slab by slab, which fixes the rows per slab and with them the slab count — and nothing behind them.  (The weight
    gradient's own slabs, 1024 * C floats here, start at the same address and are written first: with 1024 partial rows they lie
    under them and the extent is checked to the byte, with 341 they reach 4 KB further and the extent is checked behind those.)"""
    b = wb
    geo = R.scalar_geom(P, Cc)
    assert geo["nslab"] in (1024, 341)
    under = 1024 * Cc * 4
    assert (under <= geo["nslab"] * Cc * 8) == (geo["nslab"] == 1024)
    g = R.exact_g(P, Cc, 5)
    d = upload(b, g)
    out = Out(b, Cc)
    out.set(None)
    with workspace(b, WS, front=FRONT) as buf:
        SingleCall(b, P, Cc)(d, out, 0.0)
        b.synchronize()
        ws = buf[FRONT:FRONT + WS].cpu().numpy()
    nb = geo["nslab"] * Cc * 8
    assert (ws[max(nb, under):] == WS_FILL).all(), "written behind %d partial rows: the library takes more slabs than the restatement" % geo["nslab"]
    part = ws[:nb].view(np.float64).reshape(geo["nslab"], Cc)
    assert (part == R.partials_scalar(g, geo)).all(), "the partial rows are not the restated slabs' sums"
    check_exact(out.get("slabs"), R.ref64(g, None, 0.0), "P %d C %d" % (P, Cc))


# ---------------------------------------------------------------------------------------------------------------- multi route
class Table:
    def __init__(self, b, layers):
        self.b, self.layers = b, layers
        self.outs = [Out(b, Cc) for _, Cc, _ in layers]
        self.geo = [R.plan_from_library(b.lib, P, Cc) for P, Cc, _ in layers]
        self.off = [0]
        for (P, Cc, _), ge in zip(layers, self.geo):
            self.off.append(self.off[-1] + (ge["gx"] * Cc * 8 + 255) // 256 * 256)

    def data(self, exact):
        gs = [(R.exact_g if exact else R.random_g)(P, Cc, 100 + i) for i, (P, Cc, _) in enumerate(self.layers)]
        gb0 = [(R.exact_gb0 if exact else R.random_gb0)(Cc, 100 + i) for i, (_, Cc, _) in enumerate(self.layers)]
        dev = [upload(self.b, g).view(1, g.shape[0], 1, g.shape[1]).permute(0, 3, 1, 2) for g in gs]
        return gs, gb0, dev

    def run(self, dev, gb0):
        for o, v, (_, _, beta) in zip(self.outs, gb0, self.layers):
            o.set(v if beta else None)
        items = [(d, o.gb, beta) for d, o, (_, _, beta) in zip(dev, self.outs, self.layers)]
        prof = profiled(self.b, lambda: self.b.bias_grad_multi(items))
        assert set(prof) == {"bias_grad_multi"} and prof["bias_grad_multi"]["launches"] == 1, prof
        return [o.get("layer %d" % i) for i, o in enumerate(self.outs)]


@pytest.mark.parametrize("n", sorted(R.MULTI_TABLES))
def test_multi_route(n, wb):
    b = wb
    layers = R.MULTI_TABLES[n]
    T = Table(b, layers)
    assert T.off[-1] <= WS
    # exact: every layer's integer sums, its partial rows at its 256-byte-rounded offset, nothing between or behind them
    gs, gb0, dev = T.data(True)
    with workspace(b, WS, front=FRONT) as buf:
        got = T.run(dev, gb0)
        b.synchronize()
        ws = buf[FRONT:FRONT + WS].cpu().numpy()
    for i, (P, Cc, beta) in enumerate(layers):
        what = "table of %d, layer %d (P %d, C %d, beta %g)" % (n, i, P, Cc, beta)
        check_exact(got[i], R.ref64(gs[i], gb0[i], beta), what)
        nb = T.geo[i]["gx"] * Cc * 8
        part = ws[T.off[i]:T.off[i] + nb].view(np.float64).reshape(T.geo[i]["gx"], Cc)
        assert (part == R.partials_f4(gs[i], T.geo[i])).all(), "%s: its partial rows are not at workspace offset %d" % (what, T.off[i])
        assert (ws[T.off[i] + nb:T.off[i + 1]] == WS_FILL).all(), "%s: written behind its partial rows" % what
    assert (ws[T.off[-1]:] == WS_FILL).all(), "table of %d: written behind the last layer's partial rows" % n
    # random: the bound, and the same bits from the same call (the second and third run take the cached plan)
    gs, gb0, dev = T.data(False)
    with workspace(b, WS, front=FRONT):
        got = T.run(dev, gb0)
        again = T.run(dev, gb0)
    for i, (P, Cc, beta) in enumerate(layers):
        what = "table of %d, layer %d (P %d, C %d, beta %g)" % (n, i, P, Cc, beta)
        check_bound(got[i], gs[i], gb0[i], beta, R.rows_per_thread("f4", T.geo[i]), what)
        assert got[i].tobytes() == again[i].tobytes(), "%s: the same call twice gave different bits" % what


# ---------------------------------------------------------------------------------------------------------------- re-pointed workspace
OTHER_FILL = 0x5A


def _two_workspaces(b, nbytes, run, reset):
    """run() under workspace A; fill A with a pattern; point the context at workspace B (A stays referenced here: a stale pointer writes
    into live memory, never into freed memory); reset(); run() again -> (first result, second result, A intact)"""
    A = torch.full((nbytes,), WS_FILL, dtype=torch.uint8, device=b.device)
    Bw = torch.full((nbytes,), WS_FILL, dtype=torch.uint8, device=b.device)
    old = b.workspace
    try:
        set_workspace(b, A.data_ptr(), nbytes)
        b.workspace = A
        reset()
        first = run()
        b.synchronize()
        torch.cuda.synchronize()
        A.fill_(OTHER_FILL)
        torch.cuda.synchronize()
        set_workspace(b, Bw.data_ptr(), nbytes)
        b.workspace = Bw
        reset()
        second = run()
        b.synchronize()
        torch.cuda.synchronize()
        intact = bool((A == OTHER_FILL).all())
    finally:
        b.synchronize()
        b.workspace = old
        set_workspace(b, old.data_ptr(), old.numel())
    return first, second, intact


def test_backend_plans_follow_a_repointed_workspace(wb):
    """HipBackend.bias_grad_multi keeps its descriptor tables, which hold the address of the partial rows: the same items under another
    workspace must put their partial rows there"""
    b = wb
    T = Table(b, [(257, 256, 0.0), (897, 12, 1.0)])
    gs, gb0, dev = T.data(True)
    first, second, intact = _two_workspaces(b, WS, lambda: T.run(dev, gb0), lambda: None)
    for i, (P, Cc, beta) in enumerate(T.layers):
        check_exact(first[i], R.ref64(gs[i], gb0[i], beta), "first workspace, layer %d" % i)
        assert first[i].tobytes() == second[i].tobytes(), "layer %d: another result under the second workspace" % i
    assert intact, "the second call wrote into the FIRST workspace: its plan kept the old address"


def test_vf_net_plans_follow_a_repointed_workspace(hipb):
    """the same through vf_net (cnet.CNet; bias_grad_flush in csrc/vf_net.hip): a small net of three convolutions, forward and backward
    under one workspace, then under another.  (No BatchNorm: its training forward is not bit-repeatable, the running mean moves.)"""
    from video_filler_amd import nn
    from video_filler_amd.cnet import CNet, adopt_if_chain
    from video_filler_amd.trainers import weights_init
    conv = lambda i, o: nn.SpatialConvolution(i, o, 4, 4, 2, 2, 1, 1)
    seq = nn.Sequential().add(conv(3, 8)).add(nn.LeakyReLU(0.2, True)).add(conv(8, 16)).add(nn.LeakyReLU(0.2, True)).add(conv(16, 32))
    weights_init(seq, torch.Generator().manual_seed(3))
    net = adopt_if_chain(seq)
    assert isinstance(net, CNet)
    _, gflat = net.getParameters()
    gen = torch.Generator().manual_seed(4)
    x = (torch.rand((2, 3, 32, 32), generator=gen) * 2 - 1).to(hipb.device)
    gy = torch.randn((2, 32, 4, 4), generator=gen).to(hipb.device)
    bias = [(o, n) for m, name, gname, o, n in net._flat[2] if name == "bias"]
    assert [n for _, n in bias] == [8, 16, 32]

    def run():
        net.forward(x)
        prof = profiled(hipb, lambda: net.backward(x, gy))
        assert prof.get("bias_grad_multi", {}).get("launches") == 1 and "bias_grad" not in prof, prof
        hipb.synchronize()
        return [gflat[o:o + n].cpu().numpy().copy() for o, n in bias]

    net.forward(x)       # (creates the library's net object: zeroGradParameters reaches it from here on, so both runs take beta = 0)
    first, second, intact = _two_workspaces(hipb, 64 << 20, run, net.zeroGradParameters)
    want = gy.double().sum((0, 2, 3)).cpu().numpy()
    assert np.abs(first[2] - want).max() <= 1e-5 * np.abs(want).max()
    for i in range(3):
        assert np.isfinite(first[i]).all() and first[i].tobytes() == second[i].tobytes(), "bias %d: another result under the second workspace" % i
    assert intact, "the second backward wrote into the FIRST workspace: a plan kept the old address"
