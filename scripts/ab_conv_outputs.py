"""Same answers from two builds of the library, byte for byte (whether those answers are RIGHT on non-square maps is
tests/test_gpu_nonsquare.py's business: exact and fp64 checks of every route): every conv pass of the C-ABI on
NON-SQUARE maps with Cin != Cout, the bottleneck and head geometries, the generic path, the planes passes, pending BatchNorm
requests, vf_net with the planes gate dropped, weight-gradient groups under small workspaces and with every route in one walk
— raw output bytes, and the messages of the calls that are refused; and, per case of tests/route_cases.py (`pass_routes`), the
profiler's launch list beside the output: the patch-fed planes kernels are bit-identical to k_pconv_dma by design, so equal bytes
alone do not show that the same kernel ran.

    VF_HIP_LIB=/path/to/other/libvf_hip.so python scripts/ab_conv_outputs.py dump a.npz      # one fresh process per build
    python scripts/ab_conv_outputs.py dump b.npz                                             # the in-tree build
    python scripts/ab_conv_outputs.py compare a.npz b.npz [result.json]                      # byte for byte; exit 1 on a mismatch
    VF_HIP_LIB=/path/to/parent/libvf_hip.so python scripts/ab_conv_outputs.py record-routes  # tests/golden/conv_routes.json

The criterion is equality between the builds, not correctness: a shape one build refuses or gets wrong must be refused or wrong
identically by the other (the tool of a refactoring of the host code: profiles/README.md, "One conv geometry type")."""
import contextlib
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MAPS = [(2, 8, 16), (3, 16, 4)]                                        # (B, H, W): both orders of a non-square map, two batches
CHANNELS = [(3, 64), (32, 33), (64, 128), (128, 4), (64, 1), (128, 64)]     # Cin != Cout
PLANES_MAPS = [(2, 16, 32), (3, 32, 8)]                                # large enough for vf_pconv_* (more than 64 GEMM rows)


class Dump:
    def __init__(self, hipb):
        self.B = hipb
        self.out = {}
        self.seed = 0

    def rand(self, *shape, scale=1.0):
        """seeded values; 4-D tensors are logical NCHW / physical NHWC, as every activation and weight of the library"""
        self.seed += 1
        g = torch.Generator().manual_seed(self.seed)
        t = (torch.randn(shape, generator=g) * scale).to(self.B.device)
        if t.dim() == 4:
            t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        return t

    def zeros(self, *shape):
        t = torch.zeros(shape, device=self.B.device)
        if t.dim() == 4:
            t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        return t

    def planes(self, n):
        return torch.zeros((3, n), dtype=torch.bfloat16, device=self.B.device)

    def keep(self, name, *tensors):
        assert name not in self.out, name
        torch.cuda.synchronize()
        self.out[name] = np.concatenate([t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy() if torch.is_tensor(t)
                                         else np.frombuffer(np.asarray(t).tobytes(), np.uint8) for t in tensors] or [np.zeros(0, np.uint8)])

    def run(self, name, fn, *tensors):
        """fn() is one or more C-ABI calls that write `tensors`; a refusal is recorded by its message"""
        try:
            fn()
        except RuntimeError as e:
            assert name not in self.out, name
            self.out["refused:" + name] = np.frombuffer(str(e).encode(), np.uint8)
            return False
        self.keep(name, *tensors)
        return True


def conv_passes(d, tag, B, H, W, Cin, Cout, k, s, p, full):
    """every pass of one layer: forward (plain, fused activation, with planes), data-gradient (plain, with the activation mask),
    weight gradient with beta 0 and 1, from fp32 operands and from planes"""
    hb = d.B
    Ho, Wo = ((H - 1) * s - 2 * p + k, (W - 1) * s - 2 * p + k) if full else ((H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1)
    x = d.rand(B, Cin, H, W)
    w = d.rand(*((Cin, Cout, k, k) if full else (Cout, Cin, k, k)), scale=0.05)
    bias = d.rand(Cout, scale=0.1)
    gy = d.rand(B, Cout, Ho, Wo)
    fwd, bwd_d, bwd_w = ((hb.deconv2d_fwd, hb.deconv2d_bwd_data, hb.deconv2d_bwd_weight) if full else
                         (hb.conv2d_fwd, hb.conv2d_bwd_data, hb.conv2d_bwd_weight))
    y = d.zeros(B, Cout, Ho, Wo)
    d.run(tag + "/fwd", lambda: fwd(x, w, bias, y, k, s, p), y)
    d.run(tag + "/fwd_lrelu", lambda: fwd(x, w, bias, y, k, s, p, "lrelu", 0.2), y)
    if not full:
        yp = d.planes(y.numel())
        d.run(tag + "/fwd_planes", lambda: hb.conv2d_fwd_planes(x, w, bias, y, yp, k, s, p, "relu", 0.0), y, yp)
    gx = d.zeros(B, Cin, H, W)
    d.run(tag + "/bwd_data", lambda: bwd_d(gy, w, gx, k, s, p), gx)
    if not full:
        xact = torch.where(x > 0, x, 0.2 * x)
        d.run(tag + "/bwd_data_act", lambda: hb.conv2d_bwd_data_act(gy, w, gx, xact, "lrelu", 0.2, k, s, p), gx)
    xp, gp = d.planes(x.numel()), d.planes(gy.numel())
    split = d.run(tag + "/planes_split", lambda: (hb.planes_split(x, xp), hb.planes_split(gy, gp)), xp, gp)
    for with_planes in ([False, True] if split else [False]):
        gw, gb = d.rand(*w.shape), d.rand(Cout)
        for beta in (1.0, 0.0):
            d.run("%s/bwd_weight%s_beta%d" % (tag, "_planes" if with_planes else "", beta),
                  lambda: bwd_w(x, gy, gw, gb, k, s, p, beta, xp if with_planes else None, gp if with_planes else None), gw, gb)


def planes_passes(d, tag, B, H, W, Cin, Cout):
    """vf_pconv_gather / vf_pconv_scatter of one conv layer (4x4 stride 2 pad 1): forward, and the data-gradient with its mask"""
    hb = d.B
    x, gy = d.rand(B, Cin, H, W), d.rand(B, Cout, H // 2, W // 2)
    w = d.rand(Cout, Cin, 4, 4, scale=0.05)
    bias = d.rand(Cout, scale=0.1)
    xp, gp, wn, wt = d.planes(x.numel()), d.planes(gy.numel()), d.planes(w.numel()), d.planes(w.numel())
    d.run(tag + "/operand_planes", lambda: (hb.planes_split(x, xp), hb.planes_split(gy, gp), hb.weight_planes(w, wn, wt)), xp, gp, wn, wt)
    y, gx = d.zeros(B, Cout, H // 2, W // 2), d.zeros(B, Cin, H, W)
    d.run(tag + "/gather", lambda: hb.pconv_gather(xp, wn, bias, y, B, H, W, Cin, Cout, "lrelu", 0.2), y)
    xact = torch.where(x > 0, x, 0.2 * x)
    d.run(tag + "/scatter", lambda: hb.pconv_scatter(gp, wt, None, gx, B, H // 2, W // 2, Cout, Cin), gx)
    d.run(tag + "/scatter_mask", lambda: hb.pconv_scatter(gp, wt, None, gx, B, H // 2, W // 2, Cout, Cin, dmask=xact, dact="lrelu", dslope=0.2), gx)
    d.run(tag + "/scatter_bias_and_mask", lambda: hb.pconv_scatter(gp, wt, bias[:Cin] if Cin <= Cout else None, gx, B, H // 2, W // 2, Cout, Cin,
                                                                   dmask=xact, dact="lrelu", dslope=0.2), gx)


def pending_bn(d, tag, B, H, W, Cin, Cout):
    """a vf_bn_fuse_next_fwd request in front of a forward, a _bwd request in front of a data-gradient: the partial sums they leave"""
    hb = d.B
    x, gy = d.rand(B, Cin, H, W), d.rand(B, Cout, H // 2, W // 2)
    w = d.rand(Cout, Cin, 4, 4, scale=0.05)
    y, gx = d.zeros(B, Cout, H // 2, W // 2), d.zeros(B, Cin, H, W)
    part_f = torch.zeros(64 * 2 * Cout, dtype=torch.float64, device=hb.device)
    part_b = torch.zeros(64 * 2 * Cin, dtype=torch.float64, device=hb.device)
    rows = torch.zeros(2, dtype=torch.int32)
    shift, save_mean, xbn = d.rand(Cout, scale=0.1), d.rand(Cin, scale=0.1), d.rand(B, Cin, H, W)
    yact = torch.where(xbn > 0, xbn, 0.2 * xbn)

    def fwd():
        hb.bn_fuse_next_fwd(shift, part_f, 1)
        hb.conv2d_fwd(x, w, None, y, 4, 2, 1)
        rows[0] = hb.bn_fuse_result()
    d.run(tag + "/fwd", fwd, y, part_f, rows)

    def bwd():
        hb.bn_fuse_next_bwd(xbn, yact, "lrelu", 0.2, save_mean, part_b, 1)
        hb.conv2d_bwd_data(gy, w, gx, 4, 2, 1)
        rows[1] = hb.bn_fuse_result()
    d.run(tag + "/bwd_data", bwd, gx, part_b, rows)


def net_passes(d, tag, mods, shape):
    """a chain hosted by vf_net (cnet.CNet): output, gradInput and every parameter gradient of one forward + backward"""
    from video_filler_amd import nn
    from video_filler_amd.cnet import CNet, adopt_if_chain
    seq = nn.Sequential(True, True)
    for m in mods(nn):
        seq.add(m)
    net = adopt_if_chain(seq)
    assert isinstance(net, CNet)
    flat, gflat = net.getParameters()
    d.seed += 1
    flat.copy_((torch.randn(flat.shape, generator=torch.Generator().manual_seed(d.seed)) * 0.05).to(flat.device))
    x = d.rand(*shape)
    net.zeroGradParameters()

    def go():
        y = net.forward(x)
        gy = d.rand(*y.shape)
        gx = net.backward(x, gy)
        go.res = (y, gx, gflat)
    if d.run(tag, go):
        d.keep(tag + "/tensors", *go.res)


def conv(nn, cin, cout, s2=True):
    return nn.SpatialConvolution(cin, cout, 4, 4, 2, 2, 1, 1) if s2 else nn.SpatialConvolution(cin, cout, 4, 4, 1, 1, 0, 0)


def full(nn, cin, cout, s2=True):
    return nn.SpatialFullConvolution(cin, cout, 4, 4, 2, 2, 1, 1) if s2 else nn.SpatialFullConvolution(cin, cout, 4, 4, 1, 1, 0, 0)


def encoder_decoder(nn):
    BN = nn.SpatialBatchNormalization
    return [conv(nn, 3, 64), nn.LeakyReLU(0.2, True), conv(nn, 64, 128), BN(128), nn.LeakyReLU(0.2, True), conv(nn, 128, 64), BN(64),
            nn.LeakyReLU(0.2, True), full(nn, 64, 128), BN(128), nn.ReLU(True), full(nn, 128, 32), BN(32), nn.ReLU(True), full(nn, 32, 3),
            nn.Tanh()]


def head(nn):      # netD's end: ... -> 4x4 map -> the 512 -> 1 conv with its Sigmoid fused
    return [conv(nn, 3, 64), nn.LeakyReLU(0.2, True), conv(nn, 64, 512), nn.SpatialBatchNormalization(512), nn.LeakyReLU(0.2, True),
            conv(nn, 512, 1, s2=False), nn.Sigmoid()]


def bottleneck(nn):      # netG's middle: 4x4 -> 1x1 -> 4x4
    BN = nn.SpatialBatchNormalization
    return [conv(nn, 32, 64), BN(64), nn.LeakyReLU(0.2, True), conv(nn, 64, 100, s2=False), BN(100), nn.LeakyReLU(0.2, True),
            full(nn, 100, 64, s2=False), BN(64), nn.ReLU(True), full(nn, 64, 32), nn.Tanh()]


def refusals(d):
    """calls that are refused before anything is launched (one small buffer stands for every pointer)"""
    hb = d.B
    t = d.zeros(4096)
    lib, ctx, p = hb.lib, hb.ctx, C.c_void_p(t.data_ptr())

    def call(name, fn, *args):
        def f():
            from video_filler_amd import _lib
            _lib.check(getattr(lib, fn)(ctx, *args))
        d.run("refusal/" + name, f, t)
    call("conv_fwd_batch_0", "vf_conv2d_fwd", p, p, p, p, 0, 8, 16, 32, 64, 4, 2, 1, 0, 0.0)
    call("conv_fwd_weight_too_large", "vf_conv2d_fwd", p, p, p, p, 2, 8, 16, 16384, 16384, 4, 2, 1, 0, 0.0)
    call("conv_fwd_operand_2gib", "vf_conv2d_fwd", p, p, p, p, 1, 1024, 1024, 512, 64, 4, 2, 1, 0, 0.0)
    call("conv_bwd_data_operand_2gib", "vf_conv2d_bwd_data", p, p, p, 1, 2048, 2048, 64, 512, 4, 2, 1)
    call("conv_bwd_weight_operand_2gib", "vf_conv2d_bwd_weight", p, p, p, p, 1, 1024, 2048, 256, 64, 4, 2, 1, 0.0)
    call("conv_fwd_stride1_map_2x4", "vf_conv2d_fwd", p, p, p, p, 2, 2, 4, 32, 64, 4, 1, 0, 0, 0.0)
    call("gconv_fwd_kernel_larger_than_input", "vf_conv2d_fwd", p, p, p, p, 2, 2, 3, 32, 64, 7, 1, 0, 0, 0.0)
    call("gconv_bwd_data_kernel_larger_than_input", "vf_conv2d_bwd_data", p, p, p, 2, 3, 2, 32, 64, 7, 1, 0)
    call("gconv_bwd_weight_bad_sizes", "vf_conv2d_bwd_weight", p, p, p, p, 2, 8, 16, 0, 64, 5, 2, 2, 0.0)
    call("conv_bwd_data_act_stride1", "vf_conv2d_bwd_data_act", p, p, p, p, 1, 0.2, 2, 4, 4, 32, 64, 4, 1, 0)
    call("conv_bwd_data_act_tanh", "vf_conv2d_bwd_data_act", p, p, p, p, 3, 0.0, 2, 8, 16, 32, 64, 4, 2, 1)
    call("conv_bwd_data_act_k5", "vf_conv2d_bwd_data_act", p, p, p, p, 1, 0.2, 2, 8, 16, 32, 64, 5, 2, 2)
    call("conv_fwd_planes_null", "vf_conv2d_fwd_planes", p, p, p, p, None, 2, 8, 16, 32, 64, 4, 2, 1, 0, 0.0)
    call("deconv_fwd_k3", "vf_deconv2d_fwd", p, p, p, p, 2, 8, 16, 32, 64, 3, 2, 1, 0, 0.0)
    call("deconv_fwd_pad0", "vf_deconv2d_fwd", p, p, p, p, 2, 8, 16, 32, 64, 4, 2, 0, 0, 0.0)
    call("deconv_fwd_map_6x8", "vf_deconv2d_fwd", p, p, p, p, 2, 6, 8, 32, 64, 4, 2, 1, 0, 0.0)
    call("deconv_fwd_stride1_map_2x1", "vf_deconv2d_fwd", p, p, p, p, 2, 2, 1, 32, 64, 4, 1, 0, 0, 0.0)
    call("deconv_bwd_data_k5", "vf_deconv2d_bwd_data", p, p, p, 2, 8, 16, 32, 64, 5, 2, 2)
    call("deconv_bwd_data_map_8x12", "vf_deconv2d_bwd_data", p, p, p, 2, 8, 12, 32, 64, 4, 2, 1)
    call("deconv_bwd_weight_stride3", "vf_deconv2d_bwd_weight", p, p, p, p, 2, 8, 16, 32, 64, 4, 3, 1, 0.0)
    call("deconv_bwd_weight_map_3x4", "vf_deconv2d_bwd_weight", p, p, p, p, 2, 3, 4, 32, 64, 4, 2, 1, 0.0)
    call("pconv_gather_48_channels", "vf_pconv_gather", p, p, p, p, 4, 8, 16, 48, 64, 0, 0.0)
    call("pconv_gather_few_rows", "vf_pconv_gather", p, p, p, p, 1, 8, 16, 64, 64, 0, 0.0)
    call("pconv_scatter_thin_output", "vf_pconv_scatter", p, p, p, p, 2, 16, 8, 64, 3, 0, 0.0, None, 0, 0.0)
    call("pconv_scatter_bias_and_mask", "vf_pconv_scatter", p, p, p, p, 2, 16, 8, 64, 32, 0, 0.0, p, 1, 0.2)
    # a refused call takes the pending BatchNorm request with it
    def pending():
        from video_filler_amd import _lib
        _lib.check(lib.vf_bn_fuse_next_fwd(ctx, p, p, 64, 1))
        rc = lib.vf_conv2d_fwd(ctx, p, p, p, p, 0, 8, 16, 32, 64, 4, 2, 1, 0, 0.0)
        rows = C.c_int(-1)
        _lib.check(lib.vf_bn_fuse_result(ctx, C.byref(rows)))
        d.out["refusal/pending_request_result"] = np.frombuffer(np.asarray([rc, rows.value], np.int32).tobytes(), np.uint8)
    pending()


def truth_tables(d):
    """vf_conv_is_fast, vf_pconv_supported and vf_pconv_supported_in_mode over a grid of geometries (host code only)"""
    lib = d.B.lib
    sizes = [0, 1, 2, 3, 4, 6, 8, 16]
    geo = [(4, 2, 1), (4, 1, 0), (5, 2, 2), (4, 2, 0)]
    fast = [lib.vf_conv_is_fast(h, w, k, s, p) for h in sizes + [-4] for w in sizes + [-4] for k, s, p in geo]
    sup = []
    for b in (1, 2, 3, 64):
        for h in sizes:
            for w in sizes:
                for cin in (3, 32, 48, 64):
                    for cout in (3, 4, 32, 64):
                        for k, s, p in geo:
                            for tr in (0, 1):
                                sup.append(lib.vf_pconv_supported(b, h, w, cin, cout, k, s, p, tr))
                                sup += [lib.vf_pconv_supported_in_mode(m, b, h, w, cin, cout, k, s, p, tr) for m in (0, 1, 3)]
    d.out["truth/conv_is_fast"] = np.asarray(fast, np.uint8)
    d.out["truth/pconv_supported"] = np.asarray(sup, np.uint8)


class WgLayer:
    """one weight gradient of a backward walk (4x4 taps): its operands, optionally their planes, gw and gb"""

    def __init__(self, d, full, B, Cin, H, Cout, beta, bias, planes=False, stride=2):
        hb = d.B
        pad = 1 if stride == 2 else 0
        Ho = ((H - 1) * stride - 2 * pad + 4) if full else ((H + 2 * pad - 4) // stride + 1)
        self.x, self.gy = d.rand(B, Cin, H, H), d.rand(B, Cout, Ho, Ho, scale=0.1)
        self.gw = d.rand(*((Cin, Cout, 4, 4) if full else (Cout, Cin, 4, 4)))
        self.gb = d.rand(Cout) if bias else None
        self.gw0, self.gb0 = self.gw.clone(), None if self.gb is None else self.gb.clone()
        self.xp = self.gp = None
        if planes:
            self.xp, self.gp = hb.planes_split(self.x), hb.planes_split(self.gy)
        fn = hb.deconv2d_bwd_weight if full else hb.conv2d_bwd_weight
        self.launch = lambda: fn(self.x, self.gy, self.gw, self.gb, 4, stride, pad, float(beta), self.xp, self.gp)
        self.total = self.gw.numel()

    def reset(self):
        self.gw.copy_(self.gw0)
        if self.gb is not None:
            self.gb.copy_(self.gb0)

    def tensors(self):
        return [self.gw] + ([] if self.gb is None else [self.gb])

    def slab_need(self, hb):
        """the slab bytes this layer reserves when recorded (256-byte rounding), from the split count its profile shows"""
        self.reset()
        hb.prof_begin()
        try:
            self.launch()
        finally:
            prof = hb.prof_end()
        k = max([int(round(e["bytes"] / (4.0 * self.total) - 1)) for n, e in prof.items() if n in ("slab_reduce_wgrad", "slab_reduce_wgrad_group")] or [1])
        return ((k * self.total * 4 + 255) // 256 * 256) if k > 1 else 0


@contextlib.contextmanager
def small_workspace(hb, nbytes):
    from video_filler_amd import _lib
    buf = torch.zeros(max(nbytes, 256), dtype=torch.uint8, device=hb.device)
    old = hb.workspace
    _lib.check(hb.lib.vf_ctx_set_workspace(hb.ctx, C.c_void_p(buf.data_ptr()), nbytes))
    hb.workspace = buf[:nbytes]
    hb.__dict__.pop("_colsum_plans", None)
    try:
        yield
    finally:
        hb.synchronize()
        hb.workspace = old
        hb.__dict__.pop("_colsum_plans", None)
        _lib.check(hb.lib.vf_ctx_set_workspace(hb.ctx, C.c_void_p(old.data_ptr()), old.numel()))


def wgrad_groups(d):
    """vf_wgrad_group_*: the two walks of tests/test_gpu_workspace.py::test_wgrad_group_under_pressure with their small workspaces
    (a flush in the middle of a walk, a single launch behind recorded slabs, a partial end), and in every product mode one walk
    that holds every route: planes on the 128- and the 64-row tile, the bottleneck pair at a batch the small-K kernel takes and at
    one it declines (there they ride with the planes layers), fp32-fed layers of both tile heights and a thin one launched singly"""
    hb = d.B
    hb.set_mfma_mode("f32_3xbf16")
    L1 = WgLayer(d, False, 8, 64, 32, 128, 0, True)
    L2 = WgLayer(d, True, 8, 128, 16, 64, 1, True)
    L3 = WgLayer(d, False, 8, 128, 16, 256, 1, True, planes=True)
    TH = WgLayer(d, False, 2, 3, 64, 64, 0, True)
    L4 = WgLayer(d, False, 8, 64, 64, 128, 1, False)
    n1, n2, n3, nt = (L.slab_need(hb) for L in (L1, L2, L3, TH))
    d.out["wgrad_groups/slab_needs"] = np.frombuffer(np.asarray([n1, n2, n3, nt], np.int64).tobytes(), np.uint8)

    def walk(name, ws, layers, steps):
        counts = []

        def go():
            for L in layers:
                L.reset()
            with small_workspace(hb, ws):
                try:
                    steps(counts)
                except RuntimeError:
                    hb.wgrad_group_abort()
                    raise
        if d.run(name, go, *[t for L in layers for t in L.tensors()]):
            d.out[name + "/counts"] = np.frombuffer(np.asarray(counts, np.int32).tobytes(), np.uint8)

    def walk_a(counts):
        hb.wgrad_group_begin()
        for L in (L1, L2, L3, TH):
            L.launch()
            counts.append(hb.wgrad_group_count())
        hb.wgrad_group_end_partial(hb.wgrad_group_count())
        counts.append(hb.wgrad_group_count())
        L4.launch()
        counts.append(hb.wgrad_group_count())
        hb.wgrad_group_end()

    def walk_b(counts):
        hb.wgrad_group_begin()
        for L in (L1, L2, TH):
            L.launch()
            counts.append(hb.wgrad_group_count())
        hb.wgrad_group_end()
    walk("wgrad_groups/pressure_walk_a", n1 + n2 + n3 // 2, (L1, L2, L3, TH, L4), walk_a)
    walk("wgrad_groups/pressure_walk_b", n1 + n2 + nt - 256, (L1, L2, TH), walk_b)

    for mode in ("f32_3xbf16", "bf16", "f32"):
        hb.set_mfma_mode(mode)
        mixed = [WgLayer(d, False, 8, 64, 32, 128, 1, True, planes=True),             # planes, 128-row tile
                 WgLayer(d, False, 8, 64, 32, 64, 0, True, planes=True),              # planes, 64-row tile (three-plane mode)
                 WgLayer(d, False, 8, 128, 4, 128, 0, True, stride=1),                # bottleneck 4x4 -> 1x1, K = 8
                 WgLayer(d, True, 8, 128, 1, 128, 1, True, stride=1),                 # bottleneck 1x1 -> 4x4
                 WgLayer(d, False, 40, 128, 4, 128, 1, False, stride=1),              # the pair at K = 40: not the small-K kernel's
                 WgLayer(d, True, 40, 128, 1, 128, 0, False, stride=1),
                 WgLayer(d, True, 8, 128, 16, 64, 0, True),                           # fp32-fed, 128-row family
                 WgLayer(d, False, 8, 32, 32, 64, 1, False),                          # fp32-fed, 64-row family
                 WgLayer(d, False, 2, 3, 64, 64, 0, True)]                            # thin: launched singly while the group is open

        def walk_mixed(counts):
            hb.wgrad_group_begin()
            for L in mixed:
                L.launch()
                counts.append(hb.wgrad_group_count())
            hb.wgrad_group_end()
        walk("wgrad_groups/%s/mixed_walk" % mode, hb.workspace.numel(), mixed, walk_mixed)
        walk("wgrad_groups/%s/mixed_walk_64MB" % mode, 64 << 20, mixed, walk_mixed)
    hb.set_mfma_mode("f32_3xbf16")


def pass_routes(d):
    """every case of tests/route_cases.py: what the pass wrote, and its launch list (name, launches, flops, bytes) as JSON text"""
    import route_cases as RC
    for c in RC.CASES:
        res = {}

        def go():
            res["rec"], res["written"] = RC.run_case(d.B, c)
        if d.run("pass_routes/" + c["id"], go):
            d.keep("pass_routes/%s/tensors" % c["id"], *res["written"])
            d.out["pass_routes/%s/launches" % c["id"]] = np.frombuffer(json.dumps(res["rec"], sort_keys=True).encode(), np.uint8)


def record_routes():
    """tests/golden/conv_routes.json: per case the enumerators it stands for and the launch list of THIS process's library — the
    parent commit's, through VF_HIP_LIB, when the table is recorded for a change of the plan functions"""
    import route_cases as RC
    from video_filler_amd import _lib
    from video_filler_amd.backend import HipBackend
    hb = HipBackend(workspace_bytes=1 << 20)
    cases, wrong = {}, []
    for c in RC.CASES:
        rec, _ = RC.run_case(hb, c)
        try:
            RC.check_routes(c, rec)
        except AssertionError as e:      # the case list is wrong about this library: say so for every case, then fail
            wrong.append(str(e))
        cases[c["id"]] = {"routes": c["routes"], "launches": rec}
    with open(RC.GOLDEN, "w") as fh:
        json.dump({"cases": cases}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%s: %d cases, library %s" % (RC.GOLDEN, len(cases), _lib.lib_path()))
    if wrong:
        sys.exit("\n".join(wrong))


def dump(path):
    from video_filler_amd import _lib, nn
    from video_filler_amd.backend import get_backend
    hb = get_backend()
    d = Dump(hb)
    truth_tables(d)
    refusals(d)
    for mode in ("f32_3xbf16", "bf16"):      # product modes 3 and 1
        hb.set_mfma_mode(mode)
        for (B, H, W) in MAPS:
            for i, (Cin, Cout) in enumerate(CHANNELS):
                tag = "%s/B%d_%dx%d_%d_%d" % (mode, B, H, W, Cin, Cout)
                conv_passes(d, tag + "/conv_s2", B, H, W, Cin, Cout, 4, 2, 1, False)
                conv_passes(d, tag + "/full_s2", B, H, W, Cin, Cout, 4, 2, 1, True)
                if i % 2 == (B & 1):      # the generic path (k = 5 stride 2 pad 2; 4x4 stride 1 on a map that is not 4x4): half the list each
                    conv_passes(d, tag + "/generic_k5", B, H, W, Cin, Cout, 5, 2, 2, False)
                    conv_passes(d, tag + "/generic_k4_s1", B, H, W, Cin, Cout, 4, 1, 0, False)
            for (Cin, Cout) in CHANNELS:      # the bottleneck both ways (4x4 -> 1x1, 1x1 -> 4x4) and, with Cout = 1, the head's geometry
                conv_passes(d, "%s/B%d_bottleneck_%d_%d/conv_s1" % (mode, B, Cin, Cout), B, 4, 4, Cin, Cout, 4, 1, 0, False)
                conv_passes(d, "%s/B%d_bottleneck_%d_%d/full_s1" % (mode, B, Cin, Cout), B, 1, 1, Cin, Cout, 4, 1, 0, True)
        for (B, H, W) in PLANES_MAPS:
            for (Cin, Cout) in [(32, 64), (64, 128), (128, 64), (64, 33)]:
                planes_passes(d, "%s/B%d_%dx%d_%d_%d/pconv" % (mode, B, H, W, Cin, Cout), B, H, W, Cin, Cout)
            pending_bn(d, "%s/B%d_%dx%d/pending_bn_64_128" % (mode, B, H, W), B, H, W, 64, 128)
            pending_bn(d, "%s/B%d_%dx%d/pending_bn_32_64" % (mode, B, H, W), B, H, W, 32, 64)
        for gate, gname in (((0.0, 0), "gate_dropped"), ((3.0, 1024), "gate_shipped")):
            nn._PCONV_MIN_GFLOP, nn._PCONV_MIN_ROWS = gate      # (cnet.CNet hands them to vf_net_set_planes_gate)
            _lib.check(hb.lib.vf_net_set_planes_gate(*gate))
            net_passes(d, "%s/%s/net_encoder_decoder_B2_32x64" % (mode, gname), encoder_decoder, (2, 3, 32, 64))
            net_passes(d, "%s/%s/net_encoder_decoder_B3_64x16" % (mode, gname), encoder_decoder, (3, 3, 64, 16))
            net_passes(d, "%s/%s/net_head_B2" % (mode, gname), head, (2, 3, 16, 16))
            net_passes(d, "%s/%s/net_head_B3" % (mode, gname), head, (3, 3, 16, 16))
            net_passes(d, "%s/%s/net_bottleneck_B3" % (mode, gname), bottleneck, (3, 32, 8, 8))
    wgrad_groups(d)
    pass_routes(d)
    np.savez(path, **d.out)
    n = sum(1 for k in d.out if k.startswith("refused:"))
    print("%s: %d records (%d refused), %d bytes, library %s" % (path, len(d.out), n, sum(v.size for v in d.out.values()), _lib.lib_path()))


def compare(pa, pb, out_json=None):
    a, b = np.load(pa), np.load(pb)
    ka, kb = set(a.files), set(b.files)
    mism = sorted(ka ^ kb)
    nbytes = 0
    for k in sorted(ka & kb):
        va, vb = a[k], b[k]
        nbytes += va.size
        if va.shape != vb.shape or not np.array_equal(va, vb):
            mism.append(k)
            if k.startswith("refused:"):
                print("%s:\n  %s\n  %s" % (k, va.tobytes().decode(errors="replace"), vb.tobytes().decode(errors="replace")))
    refused = sorted(k for k in ka & kb if k.startswith("refused:"))
    res = {"a": pa, "b": pb, "records": len(ka & kb), "refused_identically": len([k for k in refused if k not in mism]),
           "bytes_compared": int(nbytes), "mismatches": len(mism), "mismatching_records": mism,
           "refusal_messages": {k[len("refused:"):]: a[k].tobytes().decode(errors="replace") for k in refused}}
    print(json.dumps({k: v for k, v in res.items() if k != "refusal_messages"}))
    if out_json:
        with open(out_json, "w") as fh:
            json.dump(res, fh, indent=1)
    return 1 if mism else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) >= 2 and sys.argv[1] == "record-routes":
        record_routes()
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else None))
    else:
        sys.exit(__doc__)
