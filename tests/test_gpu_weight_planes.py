"""The weight-plane kernels of csrc/vf_pgemm.hip, plane by plane: k_weight_planes (vf_weight_planes, one weight) and
k_weight_planes_multi (vf_weight_planes_multi, every weight of a net in one launch: its own LDS tile, 8-byte stores where d0 and d1 are
multiples of 4, a scalar path where they are not, and a block -> (weight, tile, tap) decode).

Reference: vf_trunc16 (three times) and vf_rne16 of csrc/vf_device.h restated on integers in numpy.  Plane q of the exact split is the top
16 bits of the running residual, and the residual loses exactly those bits: r - float(top16(r)) is exact in fp32, so numpy's float32
subtraction IS the kernel's.  The one-plane mode rounds to nearest-even: (u + 0x7FFF + ((u >> 16) & 1)) >> 16.
Both images are compared as uint16 patterns: native [3][d0][16][d1] and transposed [3][d1][16][d0], with guard words around every plane
buffer.  Values: Gaussians * 0.05, +0 and -0, and magnitudes spread over 2^-100 .. 2^100 (the range include/vf_hip.h documents: every
residual stays a normal number)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64), (96, 40), (36, 100), (3, 64), (64, 3), (1, 512), (33, 130), (4000, 64), (27, 6)]
# one launch for all nine: a small weight first, last and in between (a handful of blocks beside the 4000 x 64 weight's 4000)
ALL_NINE = [(3, 64), (4000, 64), (27, 6), (64, 64), (96, 40), (1, 512), (36, 100), (33, 130), (64, 3)]
TABLES = {1: [(33, 130)], 2: [(96, 40), (27, 6)], 9: ALL_NINE}
GUARD = 4096                     # uint16 guard words on either side of a plane buffer (a multiple of 4: the planes stay 8-byte aligned)
FILL = 0x7FA5                    # a bf16 NaN: no plane of a finite weight holds it


# ---------------------------------------------------------------------------------------------------------------- reference
def trunc3(w):
    """vf_trunc16 three times: float32 [n] -> uint16 [3][n]"""
    r = w.astype(np.float32).copy()
    out = np.empty((3, r.size), np.uint16)
    for q in range(3):
        u = r.view(np.uint32)
        out[q] = (u >> np.uint32(16)).astype(np.uint16)
        r = r - (u & np.uint32(0xFFFF0000)).view(np.float32)
        assert r.dtype == np.float32
    assert (r == 0).all()        # three planes take every bit: the documented range
    return out


def rne16(w):
    u = w.astype(np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def weight_values(d0, d1, seed):
    """physical [d0][16][d1] float32"""
    rng = np.random.default_rng(seed)
    n = d0 * 16 * d1
    w = (rng.standard_normal(n) * 0.05).astype(np.float32)
    idx = np.arange(3, n, 7)
    w[idx] = np.ldexp((1 + rng.random(idx.size)) * rng.choice([-1.0, 1.0], idx.size), rng.integers(-100, 101, idx.size)).astype(np.float32)
    w[0], w[1], w[-1], w[n // 2] = 0.0, -0.0, -0.0, 0.0
    return w.reshape(d0, 16, d1)


def images(w, fn):
    """planes of the native image [q][d0][16][d1] and of the transposed one [q][d1][16][d0], flat uint16 [q * n]"""
    nat = fn(w.reshape(-1))
    tr = fn(np.ascontiguousarray(w.transpose(2, 1, 0)).reshape(-1))
    return nat.reshape(-1), tr.reshape(-1)


@functools.lru_cache(maxsize=None)
def reference(d0, d1, seed=0):
    w = weight_values(d0, d1, 1000 * d0 + d1 + seed)
    w.setflags(write=False)
    return w, images(w, trunc3), images(w, rne16)


def test_restatement_splits_exactly():
    """the reference itself: hi + mid + lo == w without rounding, hi is the top half of w, every plane below carries at most 8 significant
    bits of the residual; round-to-nearest-even on the three tie cases"""
    w = weight_values(33, 130, 1).reshape(-1)
    p = trunc3(w)
    f = (p.astype(np.uint32) << np.uint32(16)).view(np.float32)
    s = (f[0] + f[1]) + f[2]
    assert s.dtype == np.float32 and (s == w).all()                 # (as values: -0 splits into -0, +0, +0, whose sum is +0)
    assert (p[0] == (w.view(np.uint32) >> np.uint32(16))).all()
    assert (np.abs(f[1]) <= np.abs(f[0]) * 2.0 ** -7).all() and (np.abs(f[2]) <= np.abs(f[0]) * 2.0 ** -15).all()
    ties = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x80000000], np.uint32).view(np.float32)
    assert list(rne16(ties)) == [0x3F80, 0x3F82, 0x3F81, 0x3F80, 0x8000]


# ---------------------------------------------------------------------------------------------------------------- harness
@pytest.fixture(scope="module")
def wb():
    """a backend of its own: the product mode is switched here, the shared `hipb` keeps its own"""
    from video_filler_amd.backend import HipBackend
    b = HipBackend(workspace_bytes=1 << 20)
    b.set_mfma_mode("f32_3xbf16")
    yield b
    b.synchronize()


class Weight:
    """a weight on the device with guarded buffers for both images"""

    def __init__(self, b, d0, d1):
        self.b, self.d0, self.d1, self.n = b, d0, d1, d0 * 16 * d1
        self.w_np, self.split, self.rounded = reference(d0, d1)
        self.w = torch.from_numpy(self.w_np.copy()).to(b.device).view(d0, 4, 4, d1).permute(0, 3, 1, 2)      # logical [d0][d1][4][4]
        self.bufs = [torch.empty(2 * GUARD + 3 * self.n, dtype=torch.int16, device=b.device) for _ in range(2)]
        self.nat, self.tr = (buf[GUARD:GUARD + 3 * self.n] for buf in self.bufs)
        assert self.nat.data_ptr() % 8 == 0 and self.tr.data_ptr() % 8 == 0
        self.refill()

    def refill(self):
        for buf in self.bufs:
            buf.fill_(FILL)

    def check(self, want, planes, what, transposed=True):
        """want: (native, transposed) flat uint16 of `planes` planes; the planes beyond and the guards keep their fill.
        transposed=False: the call was given no transposed image, that buffer keeps its fill throughout"""
        self.b.synchronize()
        for name, buf, ref in (("native", self.bufs[0], want[0]), ("transposed", self.bufs[1], want[1])):
            got = buf.cpu().numpy().view(np.uint16)
            assert (got[:GUARD] == FILL).all() and (got[GUARD + 3 * self.n:] == FILL).all(), "%s: %s guard words written" % (what, name)
            body = got[GUARD:GUARD + 3 * self.n]
            if name == "transposed" and not transposed:
                assert (body == FILL).all(), "%s: the transposed buffer was written" % what
                continue
            assert (body[planes * self.n:] == FILL).all(), "%s: %s planes beyond the first %d written" % (what, name, planes)
            bad = np.flatnonzero(body[:planes * self.n] != ref[:planes * self.n])
            assert bad.size == 0, "%s (%d x %d): %s image differs in %d of %d words, first at plane %d element %d: got %04x want %04x" % (
                what, self.d0, self.d1, name, bad.size, planes * self.n, bad[0] // self.n, bad[0] % self.n, body[bad[0]], ref[bad[0]])


def run_multi(b, ws):
    plan = b.weight_planes_multi([(W.w, W.nat, W.tr) for W in ws])
    b.prof_begin()
    try:
        b.weight_planes_run(plan)
    finally:
        prof = b.prof_end()
    assert set(prof) == {"weight_planes_multi"} and prof["weight_planes_multi"]["launches"] == 1, prof
    return plan


# ---------------------------------------------------------------------------------------------------------------- mode 3
@pytest.mark.parametrize("d0,d1", SHAPES, ids=lambda v: str(v))
def test_single_exact_split(d0, d1, wb):
    W = Weight(wb, d0, d1)
    wb.weight_planes(W.w, W.nat, W.tr)
    W.check(W.split, 3, "vf_weight_planes")
    # without the transposed image: the native one alone, the other buffer untouched
    W.refill()
    wb.weight_planes(W.w, W.nat, None, want_transposed=False)
    W.check(W.split, 3, "vf_weight_planes, native only", transposed=False)


@pytest.mark.parametrize("n", sorted(TABLES))
def test_multi_exact_split(n, wb):
    ws = [Weight(wb, d0, d1) for d0, d1 in TABLES[n]]
    run_multi(wb, ws)
    for i, W in enumerate(ws):
        W.check(W.split, 3, "vf_weight_planes_multi, table of %d, weight %d" % (n, i))


# ---------------------------------------------------------------------------------------------------------------- mode 1
@pytest.fixture
def bf16_mode(wb):
    wb.set_mfma_mode("bf16")
    try:
        yield wb
    finally:
        wb.set_mfma_mode("f32_3xbf16")


def test_single_rounded_plane(bf16_mode):
    b = bf16_mode
    for d0, d1 in SHAPES:
        W = Weight(b, d0, d1)
        b.weight_planes(W.w, W.nat, W.tr)
        W.check(W.rounded, 1, "vf_weight_planes, one rounded plane")


def test_multi_rounded_plane(bf16_mode):
    b = bf16_mode
    ws = [Weight(b, d0, d1) for d0, d1 in ALL_NINE]
    run_multi(b, ws)
    for i, W in enumerate(ws):
        W.check(W.rounded, 1, "vf_weight_planes_multi, one rounded plane, weight %d" % i)


# ---------------------------------------------------------------------------------------------------------------- plan reuse
def test_kept_plan_follows_the_weights(wb):
    """the nets build their table once and run it after every Adam step: the planes must be those of the weights as they are NOW"""
    ws = [Weight(wb, d0, d1) for d0, d1 in TABLES[2] + [(64, 64)]]
    plan = run_multi(wb, ws)
    for W in ws:
        W.check(W.split, 3, "first run")
    for W in ws:
        new, split, _ = reference(W.d0, W.d1, seed=77)
        assert new.tobytes() != W.w_np.tobytes()
        W.w.permute(0, 2, 3, 1).copy_(torch.from_numpy(new.copy()).to(wb.device).view(W.d0, 4, 4, W.d1))      # in place: same address
        W.split = split
    wb.weight_planes_run(plan)
    for W in ws:
        W.check(W.split, 3, "kept plan, weights edited in place")
