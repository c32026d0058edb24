"""Shared helpers for the parity tests: layout conversion between the oracle's NCHW numpy arrays and the
backend's channels-last device tensors, and error metrics."""
import contextlib

import numpy as np
import torch


def to_dev(a, backend):
    """NCHW numpy (or 1-D) -> device tensor; 4-D tensors become logical NCHW / physical NHWC."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    t = t.to(backend.device)
    if t.dim() == 4:
        t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return t


def to_np(t):
    return t.detach().cpu().contiguous().numpy()


def rel_err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def assert_close(a, b, tol, what=""):
    e = rel_err(a, b)
    assert e <= tol, "%s: max-norm relative error %.3e > %.1e" % (what, e, tol)


class FastRng:
    """Stand-in for numpy's Generator in `weights_init` at FULL net sizes (hundreds of millions of parameters): float32
    ziggurat draws instead of float64 ones.  `normal(mu, sd, shape)` is the only call weights_init makes; the value
    stream is `mu + sd * standard_normal(float32)` evaluated in float32, so any side that consumes the same shapes in the
    same order (the oracle's weights_init; `fast_init_flat` below for the HIP nets) holds bit-identical weights."""

    def __init__(self, seed):
        self.g = np.random.default_rng(seed)

    def normal(self, mu, sd, shape):
        z = self.g.standard_normal(shape, dtype=np.float32)
        z *= np.float32(sd)
        z += np.float32(mu)
        return z


def fast_init_flat(net, rng):
    """The reference-order parameter vector `weights_init(net, rng)` would leave in the oracle's twin of the
    HIP net `net` (after getParameters()): convolution weights N(0, 0.02), BatchNorm gains N(1, 0.02), every bias 0 — the
    draws consumed module by module in the same order (train.lua:58-67)."""
    parts = []
    for m, name, gname, o, n in net._flat[2]:
        if name == "bias":
            parts.append(np.zeros(n, np.float32))
        elif "BatchNormalization" in m.type_name():
            parts.append(rng.normal(1.0, 0.02, (n,)))
        else:
            parts.append(rng.normal(0.0, 0.02, (n,)))
    return np.concatenate(parts)


class KinkSync:
    """Pins the derivative choice of every (Leaky)ReLU in a HIP training iteration to the oracle's.

    LeakyReLU/ReLU derivatives jump at 0 and are evaluated from the activated output.  Two correct fp32
    implementations differ by ~1e-7 in a pre-activation, so an element that sits that close to the kink can take slope 1
    on one side and 0.2 (or 0) on the other, which moves whole gradient tensors by up to 1e-2 of their norm although
    nothing is wrong.  With this helper the oracle runs first and records every activated tensor; during the HIP run
    (nn.Sequential.act_hook) every element whose ORACLE value is within `delta` (relative to that tensor's max) of 0 is
    overwritten with the oracle's value — a perturbation of at most `delta` on a handful of elements — so both sides
    take the same branch everywhere and the gradients can be held to the fp32 bar (1e-4) on the real nets too.
    An element further from 0 than `delta` whose sign differs is a real forward error and still fails the test."""

    def __init__(self, oracle_mod, pairs, delta=1e-5):
        """pairs: [(oracle net, hip net)] built by the same recipe (leaf order identical)."""
        self.O = oracle_mod
        self.delta = delta
        self.map = {}
        for rnet, hnet in pairs:
            ra = [m for m in self._oleaves(rnet) if type(m).__name__ in ("LeakyReLU", "ReLU")]
            ha = [m for m in hnet.leaves() if getattr(m, "act", None) in ("lrelu", "relu")]
            assert len(ra) == len(ha), (len(ra), len(ha))
            for a, b in zip(ra, ha):
                self.map[id(b)] = a
        self.rec = {}
        self.pos = {}
        self.touched = 0
        self.checked = 0
        self.calls = 0
        self.edited_calls = 0
        # The band |oracle value| < delta * max holds ~1e-4 .. 1.5e-3 of a net's activations (measured over the suite: a LeakyReLU
        # output maps pre-activations in (-5 delta, delta) into it; narrow test nets have the heavier tails), and nearly all of
        # them differ from the oracle in the last bit, so that is also the share the pin rewrites.  Two guards keep the pin from
        # hiding a forward error: every rewritten element must already agree with the oracle to `near_tol` of the tensor's max
        # (checked in __call__), and the rewritten share stays below `max_touched_frac`.
        self.max_touched_frac = 3e-3
        self.near_tol = 1e-4
        self.worst_near = 0.0

    def _oleaves(self, m):
        if hasattr(m, "modules"):
            out = []
            for c in m.modules:
                out += self._oleaves(c)
            return out
        return [m]

    def oracle_step(self, fn):
        """run fn() (the oracle's iteration) while recording its activations, pass by pass"""
        self.O.Module.act_trace = []
        try:
            out = fn()
        finally:
            trace, self.O.Module.act_trace = self.O.Module.act_trace, None
        self.rec, self.pos = {}, {}
        for m, y in trace:
            self.rec.setdefault(id(m), []).append(y)
        return out

    def __call__(self, a, y):                 # nn.Sequential.act_hook; returns True iff it edited `y`
        ra = self.map.get(id(a))
        if ra is None:
            return False
        passes = self.rec[id(ra)]
        k = self.pos.get(id(ra), 0)
        ref = passes[k]
        used = 1
        if y.shape[0] != ref.shape[0]:        # netD's real and fake passes run as one batch of 2B on the HIP side
            ref = np.concatenate([passes[k], passes[k + 1]], axis=0)
            used = 2
        self.pos[id(ra)] = k + used
        assert tuple(y.shape) == ref.shape, (tuple(y.shape), ref.shape)
        r = torch.from_numpy(ref).to(y.device)
        scale = max(1.0, float(np.abs(ref).max()))
        near = r.abs() < self.delta * scale
        n_edit = int((near & (r != y)).sum().item())
        if n_edit:
            # what is about to be rewritten must already BE the oracle's value to the forward tolerance: a forward error that
            # only shows on elements near 0 would otherwise be overwritten silently
            worst = float((y - r).abs()[near].max().item())
            self.worst_near = max(self.worst_near, worst / scale)
            assert worst <= self.near_tol * scale, "KinkSync: an element within the kink band differs from the oracle by %.3e (> %g of the tensor's max %.3e): forward error near 0" % (worst, self.near_tol, scale)
        self.touched += n_edit
        self.checked += y.numel()
        self.calls += 1
        if n_edit:
            y.copy_(torch.where(near, r, y))
        self.edited_calls += 1 if n_edit else 0
        return n_edit > 0

    def hip_step(self, fn):
        import video_filler_amd.nn as hnn
        hnn.Sequential.act_hook = self
        t0, c0 = self.touched, self.checked
        try:
            out = fn()
        finally:
            hnn.Sequential.act_hook = None
        # every recorded pass must have been consumed: a HIP-side (Leaky)ReLU the hook never saw would go unpinned
        for rid, passes in self.rec.items():
            assert self.pos.get(rid, 0) == len(passes), "an oracle activation pass was not consumed by the HIP run (%d of %d)" % (
                self.pos.get(rid, 0), len(passes))
        # the pin is the band's population (see __init__): beyond max_touched_frac the forward pass is wrong near 0
        touched, checked = self.touched - t0, self.checked - c0
        assert checked > 0, "the hook was never called: nothing was pinned"
        assert touched <= max(self.max_touched_frac * checked, 8), "KinkSync rewrote %d of %d activations (> %g): forward error near 0" % (
            touched, checked, self.max_touched_frac)
        try:        # evidence for DESIGN.md 6: what the pin looked at, rewrote, and how far the rewritten values were off
            import json
            import os
            os.makedirs("gpurun_out", exist_ok=True)
            with open(os.path.join("gpurun_out", "kinksync_stats.jsonl"), "a") as fh:
                fh.write(json.dumps(dict(test=os.environ.get("PYTEST_CURRENT_TEST", ""), touched=touched, checked=checked,
                                         frac=touched / checked, worst_near=self.worst_near)) + "\n")
        except OSError:
            pass
        return out


def attach_world1_comm(hipb):
    """a one-rank RCCL communicator on the session's HIP backend (vf_comm_init), created once"""
    if hipb.comm is None:
        hipb.init_comm(1, 0, hipb.comm_unique_id())
    return hipb


def to_internal(net, vec_ref):
    """reference-order flat vector -> this net's padded channels-last flat layout."""
    flat = torch.zeros_like(net._flat[0])
    off = 0
    for m, name, gname, o, n in net._flat[2]:
        t = getattr(m, name)
        seg = torch.from_numpy(vec_ref[off:off + n].copy()).to(flat.device)
        if t.dim() == 4:
            seg = seg.reshape(t.shape).permute(0, 2, 3, 1).reshape(-1)
        flat[o:o + n] = seg
        off += n
    return flat


def from_internal(net, flat):
    parts = []
    for m, name, gname, o, n in net._flat[2]:
        t = getattr(m, name)
        seg = flat[o:o + n]
        if t.dim() == 4:
            d0, d1, kH, kW = t.shape
            seg = seg.view(d0, kH, kW, d1).permute(0, 3, 1, 2).contiguous().reshape(-1)
        parts.append(seg)
    return to_np(torch.cat(parts))


def grads_reference_order(tr, net, gref):
    """net.reference_flat(grads=True) as numpy.  The slices of netG's gradient vector that step() does not write
    (trainer.fused_adam_ranges(): the bottleneck pair's weight gradients are formed and consumed inside the Adam kernel,
    optim.adam_update_fused) are read back from Adam's first moment after a FIRST update (m = (1 - beta1) g, m having started
    at zero); after later updates they are taken from the oracle's vector `gref`, and what vouches for them is the comparison
    of the parameters and of Adam's m and v, which those tests make."""
    ranges = tr.fused_adam_ranges() if net is tr.netG and hasattr(tr, "fused_adam_ranges") else []
    if not ranges:
        return to_np(net.reference_flat(grads=True))
    flat = net._flat[1].clone()
    st = tr.optimStateG
    if int(st["t_dev"][0].item()) == 1:
        # after the first update m = (1 - beta1) g exactly (m started at zero): the gradient the kernel consumed, read back
        for lo, hi in ranges:
            flat[lo:hi] = st["m"][lo:hi] / (1.0 - st.get("beta1", 0.9))
    else:
        want = to_internal(net, np.asarray(gref, np.float32))
        for lo, hi in ranges:
            flat[lo:hi] = want[lo:hi]
    return from_internal(net, flat)


# ---- guarded device buffers (tests/test_gpu_workspace.py, tests/test_gpu_elementwise.py)
TAIL32 = 0x7FA5A5A5              # float32 guard words: a NaN payload no kernel computes
FILL64 = 0x7FF5A5A5A5A5A5A5      # float64 words of the BatchNorm partial buffers (body and tail): also a NaN payload


def guarded(b, n, dtype=torch.float32, pad=4096):
    """a flat buffer of n elements and a pad-element guard tail.  float32: body NaN; float64 (BatchNorm partials): body and
    tail FILL64, so that rows no launch wrote can be told apart"""
    buf = torch.empty(n + pad, dtype=dtype, device=b.device)
    if dtype == torch.float32:
        buf[:n].fill_(float("nan"))
        buf[n:].view(torch.int32).fill_(TAIL32)
    else:
        buf.view(torch.int64).fill_(FILL64)
    return buf


def untouched(buf, lo, hi=None):
    seg = buf[lo:hi]
    if buf.dtype == torch.float32:
        return bool((seg.view(torch.int32) == TAIL32).all())
    return bool((seg.view(torch.int64) == FILL64).all())


# ---- a context's workspace inside a guard band (tests/test_gpu_workspace.py, tests/test_gpu_bias_grad.py)
WS_FILL = 0xA5                   # workspace guard bytes


def set_workspace(b, ptr, nbytes):
    import ctypes as C
    from video_filler_amd import _lib
    _lib.check(b.lib.vf_ctx_set_workspace(b.ctx, C.c_void_p(ptr), nbytes))


@contextlib.contextmanager
def workspace(b, nbytes, guard=1 << 20, front=0):
    """point b's context at `nbytes` of a fresh buffer followed by `guard` bytes of a fixed pattern (and, front > 0, behind `front`
    such bytes); on exit the guards must be byte-identical.  b.workspace follows (bias_grad_multi sizes its partials from it; its
    plans and vf_net's follow the workspace by themselves).  Yields the whole buffer: the workspace is buf[front:front + nbytes]."""
    buf = torch.full((front + nbytes + guard,), WS_FILL, dtype=torch.uint8, device=b.device)
    old = b.workspace
    set_workspace(b, buf.data_ptr() + front, nbytes)
    b.workspace = buf[front:front + nbytes]
    try:
        yield buf
    finally:
        b.synchronize()
        intact = bool((buf[front + nbytes:] == WS_FILL).all()) and bool((buf[:front] == WS_FILL).all())
        b.workspace = old
        set_workspace(b, old.data_ptr(), old.numel())
    assert intact, "a kernel wrote outside a %d-byte workspace" % nbytes
