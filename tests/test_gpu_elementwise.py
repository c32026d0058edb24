"""vf_core.hip's byte kernels against float64, element by element: the pointwise modules, the criteria, the layout transposes,
vf_zero_segments and Adam, at scalar tails, beyond the 2048-block grid cap, on unaligned views, in place and at n = 0.

How a case is judged
  * Every output is a slice of a buffer filled with a NaN payload (helpers.TAIL32); after the call the words in front of and
    behind the slice must still be the payload (`Guard.check`).
  * EXACT inputs: small integers / powers of two, position coded (a hash of the flat NCHW index), chosen so that every fp32
    intermediate is exact.  Elementwise results must then be bit-identical to the float64 reference rounded to fp32, and a loss
    must equal integer_sum / n: exactly where n is a power of two, else to 1e-12 relative (one fp64 rounding per block and per
    atomic add; a dropped or duplicated element moves the loss by >= 1/n >= 2.8e-8 relative at the largest n used here).
  * RANDOM inputs: |got - ref64| <= k * U * S + FLT_MIN per element, U = 2^-24, S = the sum of the absolute values of the terms the
    op adds, k = the number of fp32 roundings of the op without contraction (a fused multiply-add only removes one).  The
    derivation stands next to each bound function below.  FLT_MIN allows a flushed denormal.
    tests/test_elementwise_bounds.py checks on the CPU that fp32 arithmetic in the kernel's statement order (separate and fused)
    stays inside these bounds on the inputs generated here, and that the exact inputs are exact.
  * tanhf / expf are the one measured figure, see TRANSCENDENTAL_ULPS.

Importing this module does not touch the device (the CPU companion imports the generators and the bounds)."""
import functools
import math

import numpy as np
import pytest
import torch

from helpers import FILL64, TAIL32, to_dev, to_np

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FLT_MIN = float(np.finfo(np.float32).tiny)
SWEEP = 1 << 21                  # floats one sweep of the capped 2048-block grid covers at four floats per thread
PAD = 1024                       # guard floats on either side (a multiple of 4: the slice's alignment is the offset asked for)
SLOPE = 0.2
F32 = np.float32

# The one bound that cannot be derived: the device's tanhf(x) and 1.f / (1.f + expf(-x)).  ROCm's accuracy table for the HIP math
# API is not part of the installed toolkit, so the figure is MEASURED, not taken from the kernel under test: a stand-alone HIP program
# that links nothing of this project evaluated both expressions over act_inputs(n, seed) for every (n, seed) this module uses, and
# their negations (50 741 350 values), and the largest error against float64, in ulps of the float64 value at fp32 precision, was
#     tanhf                      1.3962 ulp  (at x = -0.6352141)
#     1.f / (1.f + expf(-x))     2.2009 ulp  (at x = -1.9709661), over results in fp32's normal range; below it (x <= -88) the device
#                                returns 0 or a denormal and the FLT_MIN floor of every bound here applies
# (MI355X, ROCm 7.2 hipcc -O3 -ffp-contract=off, 2026-10-16).  The bound is twice the figure, rounded up to whole ulps.
MEASURED_ULPS = {"tanh": 1.3962, "sigmoid": 2.2009}
TRANSCENDENTAL_ULPS = {k: int(math.ceil(2 * v)) for k, v in MEASURED_ULPS.items()}      # tanh 3, sigmoid 5


# ------------------------------------------------------------------------------------------------------------- generators
@functools.lru_cache(maxsize=6)
def _hash_ints(n, seed, lo, hi):
    with np.errstate(over="ignore"):
        h = (np.arange(n, dtype=np.uint64) + np.uint64(seed * 0x632BE5AB + 1)) * np.uint64(0x9E3779B97F4A7C15)
        h ^= h >> np.uint64(29)
        h *= np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(32)
    return (lo + (h % np.uint64(hi - lo + 1)).astype(np.int64)).astype(np.int64)


def hash_ints(n, seed, lo, hi):
    """position-coded integers in [lo, hi]: splitmix64 of (flat index + seed)"""
    return _hash_ints(n, seed, lo, hi).copy()


@functools.lru_cache(maxsize=6)
def _normal(n, seed):
    return np.random.default_rng(seed).standard_normal(n, dtype=F32)


def normal(n, seed, scale=1.0):
    return (_normal(n, seed) * F32(scale)).astype(F32)


ACT_EDGES = np.array([0.0, -0.0, FLT_MIN, -FLT_MIN, 1e-30, -1e-30, 20, -20, 88, -88, 89, -89, 100, -100, 1e30, -1e30], F32)


def act_inputs(n, seed):
    """normal data (sd 3: tanh and sigmoid over their whole curved range) with the edge values planted at hashed places"""
    x = normal(n, seed, 3.0)
    pos = hash_ints(len(ACT_EDGES), seed + 17, 0, max(n - 1, 0))
    if n >= 4 * len(ACT_EDGES):
        x[pos] = ACT_EDGES
    else:
        x[:min(n, len(ACT_EDGES))] = ACT_EDGES[:n]
    return x


def ulp32(ref):
    """one unit in the last place of fp32 at |ref| (float64 array)"""
    a = np.maximum(np.abs(ref), FLT_MIN)
    return np.ldexp(1.0, np.floor(np.log2(a)).astype(np.int64) - 23)


# ------------------------------------------------------------------------------------------------------- pointwise: the ops
# name -> inputs (read-only operands in the kernel's a, b, c order), whether `out` is read (in place), scalars (random, exact)
PW = {
    "act_fwd_lrelu": dict(ins=1, rw=False), "act_fwd_relu": dict(ins=1, rw=False), "act_fwd_tanh": dict(ins=1, rw=False),
    "act_fwd_sigmoid": dict(ins=1, rw=False),
    "act_bwd_lrelu": dict(ins=2, rw=False), "act_bwd_relu": dict(ins=2, rw=False), "act_bwd_tanh": dict(ins=2, rw=False),
    "act_bwd_sigmoid": dict(ins=2, rw=False),
    "axpby": dict(ins=1, rw=True, f=(0.25, -1.5), fx=(0.5, -2.0)),
    "cmul": dict(ins=1, rw=True),
    "scale_shift": dict(ins=0, rw=True, f=(0.95, 0.05), fx=(0.5, 0.25)),
    "compose": dict(ins=3, rw=False),
    "mse_bwd": dict(ins=2, rw=False),
}
PW_SIZES = [1, 3, 4, 5, 1021, 1024, 1027, 65536, 65539, SWEEP, SWEEP + 7, 3 * SWEEP + 1029, 12582912]
COMPOSE_MASKS = np.array([0.0, 1.0, -0.0, 0.5, 1e-40], F32)


def pw_inputs(op, n, seed, exact):
    """-> (list of read-only inputs, initial value of `out` or None, (f0, f1))"""
    spec = PW[op]
    f = spec.get("fx" if exact else "f", (0.0, 0.0))
    if op.startswith("act_fwd"):
        ins = [hash_ints(n, seed, -8, 8).astype(F32) * F32(0.25)] if exact else [act_inputs(n, seed)]
    elif op.startswith("act_bwd"):
        act = op[8:]
        if exact:      # y in {-1, -.5, 0, .5, 1}: 1 - y*y, (1 - y)*y, g*0.25 exact; lrelu slope -> 0.25 (the call passes it)
            ins = [hash_ints(n, seed, -2, 2).astype(F32) * F32(0.5), hash_ints(n, seed + 1, -16, 16).astype(F32)]
        else:
            y = normal(n, seed, 1.0)
            if act == "tanh":
                y = np.tanh(y).astype(F32)
            elif act == "sigmoid":
                y = (1 / (1 + np.exp(-y.astype(np.float64)))).astype(F32)
            if n >= 8:
                y[hash_ints(4, seed + 5, 0, n - 1)] = np.array([0.0, -0.0, 1.0, -1.0], F32)
            ins = [y, normal(n, seed + 1, 1.0)]
    elif op == "compose":
        m = COMPOSE_MASKS[hash_ints(n, seed + 2, 0, len(COMPOSE_MASKS) - 1)]
        ins = [hash_ints(n, seed, 1, 1 << 20).astype(F32), -hash_ints(n, seed + 1, 1, 1 << 20).astype(F32), m]
    elif op == "mse_bwd":
        if exact:
            x = hash_ints(n, seed, -4, 4)
            ins = [x.astype(F32), (x - hash_ints(n, seed + 1, -2, 2)).astype(F32)]
        else:
            ins = [normal(n, seed), normal(n, seed + 1)]
    elif spec["ins"] == 1:
        ins = [hash_ints(n, seed, -64, 64).astype(F32) * F32(0.125)] if exact else [normal(n, seed)]
    else:
        ins = []
    out0 = None
    if spec["rw"]:
        out0 = hash_ints(n, seed + 9, -64, 64).astype(F32) * F32(0.25) if exact else normal(n, seed + 9)
    return ins, out0, (float(F32(f[0])), float(F32(f[1])))


def pw_slope(exact):
    return 0.25 if exact else SLOPE


def pw_ref64(op, ins, out0, f, n, slope):
    """the op on the fp32 inputs widened to float64"""
    a = [v.astype(np.float64) for v in ins]
    o = None if out0 is None else out0.astype(np.float64)
    s = float(F32(slope))
    if op == "act_fwd_lrelu":
        return np.where(a[0] > 0, a[0], a[0] * s)
    if op == "act_fwd_relu":
        return np.where(a[0] > 0, a[0], 0.0)
    if op == "act_fwd_tanh":
        return np.tanh(a[0])
    if op == "act_fwd_sigmoid":
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(-a[0]))
    if op == "act_bwd_lrelu":
        return np.where(a[0] > 0, a[1], a[1] * s)
    if op == "act_bwd_relu":
        return np.where(a[0] > 0, a[1], 0.0)
    if op == "act_bwd_tanh":
        return a[1] * (1.0 - a[0] * a[0])
    if op == "act_bwd_sigmoid":
        return a[1] * (1.0 - a[0]) * a[0]
    if op == "axpby":
        return f[0] * a[0] + f[1] * o
    if op == "cmul":
        return o * a[0]
    if op == "scale_shift":
        return o * f[0] + f[1]
    if op == "compose":
        # maskedSelect / maskedCopy take a ByteTensor of 0 / 1; the project's mask is a float tensor of 0.0 / 1.0 and the header
        # defines every other value by IEEE `mask != 0`: -0.0 selects `real`, 0.5 and a denormal select `fake`
        return np.where(a[2] != 0, a[1], a[0])
    if op == "mse_bwd":
        return (2.0 / n) * (a[0] - a[1])
    raise KeyError(op)


def pw_bound(op, ins, out0, f, n):
    """per-element k * U * S (None: bit-exact against fp32 numpy, i.e. against ref64 rounded once)

      relu, lrelu (fwd and bwd), cmul, compose: a select or ONE correctly rounded multiply -> bit-exact
      axpby        f0*a, f1*o, the sum: 3 roundings, S = |f0 a| + |f1 o|                                  k = 3
      scale_shift  o*f0, the sum: 2 roundings, S = |o f0| + |f1|                                          k = 2
      mse_bwd      (float)n, 2.f / it, a - b, the product: 4 roundings; a - b is one rounding of the exact difference,
                   so S = (2/n) |a - b|                                                                   k = 4
      act_bwd tanh     y*y, 1 - it, g * it: 3 roundings, S = |g| (1 + y^2)                                k = 3
      act_bwd sigmoid  1 - y, g * it, * y: 3 roundings, S = |g| (|y| + y^2)                               k = 3"""
    a = [np.abs(v.astype(np.float64)) for v in ins]
    o = None if out0 is None else np.abs(out0.astype(np.float64))
    if op == "axpby":
        return 3 * U * (abs(f[0]) * a[0] + abs(f[1]) * o)
    if op == "scale_shift":
        return 2 * U * (o * abs(f[0]) + abs(f[1]))
    if op == "mse_bwd":
        return 4 * U * (2.0 / n) * np.abs(ins[0].astype(np.float64) - ins[1].astype(np.float64))
    if op == "act_bwd_tanh":
        return 3 * U * a[1] * (1 + a[0] * a[0])
    if op == "act_bwd_sigmoid":
        return 3 * U * a[1] * (a[0] + a[0] * a[0])
    return None


def pw_exact_is_bitwise(op, n):
    """on the exact inputs every op is bit-exact, mse_bwd where 2/n is a power of two"""
    return op != "mse_bwd" or (n & (n - 1)) == 0


# ---------------------------------------------------------------------------------------------------------- criteria: bounds
def mse_inputs(n, seed, exact):
    if exact:
        x = hash_ints(n, seed, -4, 4)
        return x.astype(F32), (x - hash_ints(n, seed + 1, -2, 2)).astype(F32)
    return normal(n, seed), normal(n, seed + 1)


def sum64(v):
    return float(np.sum(v, dtype=np.float64))


def mse_ref(x, t):
    d = x.astype(np.float64) - t.astype(np.float64)
    return sum64(d * d) / x.size


MSE_FWD_REL = (64 + 3) * U + 1e-12
"""k_mse_fwd: d = x - t (1 rounding, squared: 2 U), d*d (1): 3 U on each square; a thread adds at most 16 float4 = 64 non-negative
squares (plus, in the tail sweep, at most one more after at most 15 float4) into an fp32 partial sum before it folds it into fp64:
at most 64 additions of relative error U each on a sum of non-negative terms -> (64 + 3) U relative; the fp64 reduction 1e-12."""
RECON_LOSS_REL = 3 * U + 1e-12
"""k_recon_grad_mix*: every fp32 square goes straight into fp64: 3 U as above, fp64 reduction 1e-12"""
F64_REL = 1e-12


def recon_weights(B, C, H, form, band, seed):
    """(mask or None, W) on the LOGICAL NCHW tensor, from (row, column): W = c0 + c1 * mask, or c0 inside the band / c0 + c1 on it"""
    if form == "mask":
        m = (hash_ints(B * C * H * H, seed + 3, 0, 2) > 0).astype(F32).reshape(B, C, H, H)
        return m, m
    if form == "band":
        row = np.arange(H)[:, None] * np.ones(H, np.int64)[None, :]
        col = row.T
        inside = (row >= band) & (row < H - band) & (col >= band) & (col < H - band)
        border = np.broadcast_to((~inside).astype(F32), (B, C, H, H)).copy()
        return None, border
    return None, np.zeros((B, C, H, H), F32)


def recon_inputs(B, C, H, seed, exact):
    n = B * C * H * H
    if exact:
        x = hash_ints(n, seed, -4, 4)
        t = x - hash_ints(n, seed + 1, -2, 2)
        g = hash_ints(n, seed + 2, -8, 8).astype(F32) * F32(0.25)
        sc = (0.5, 0.5, 2.0)
        x, t = x.astype(F32), t.astype(F32)
    else:
        x, t, g = normal(n, seed), normal(n, seed + 1), normal(n, seed + 2)
        sc = (float(F32(1 - 0.999)), float(F32(0.999 * 0.05 + 0.5)), float(F32(0.999 * 0.95)))
    shp = (B, C, H, H)
    return g.reshape(shp), x.reshape(shp), t.reshape(shp), sc


def recon_ref(g, x, t, wsel, sc):
    alpha, c0, c1 = sc
    n = x.size
    d = x.astype(np.float64) - t.astype(np.float64)
    w = c0 + c1 * wsel.astype(np.float64)
    return alpha * g.astype(np.float64) + (2.0 / n) * d * w, sum64(d * d) / n


def recon_bound(g, x, t, wsel, sc):
    """out = alpha*g + ((2/n) * d) * w:  (float)n (exact below 2^24, else 1) and 2.f / it (1), d = x - t (1, of the exact difference),
    their product (1), w = c0 + c1*m (2; relative to |c0| + |c1 m|), the product with w (1): 7 roundings on
    T = (2/n)|d|(|c0| + |c1 m|); alpha*g (1) on A = |alpha g|; the final sum (1) on A + T   ->   k = 8 on S = A + T"""
    alpha, c0, c1 = sc
    n = x.size
    d = np.abs(x.astype(np.float64) - t.astype(np.float64))
    return 8 * U * (abs(alpha) * np.abs(g.astype(np.float64)) + (2.0 / n) * d * (abs(c0) + abs(c1) * np.abs(wsel.astype(np.float64))))


def gdl_crops(X):
    """per (b, c) plane, i1 = X[0:H-1, :], j1 = X[1:H, :], i2 = X[:, 0:W-1], j2 = X[:, 1:W], each FLATTENED row-major;
    element k of i2 (j2) pairs with element k of i1 (j1) although the crops have different shapes"""
    B, C, H, W = X.shape
    fl = lambda v: np.ascontiguousarray(v).reshape(B, C, -1)
    return fl(X[:, :, :H - 1, :]), fl(X[:, :, 1:, :]), fl(X[:, :, :, :W - 1]), fl(X[:, :, :, 1:])


def gdl_terms(yh, y):
    """the fp32 differences the criterion forms (one correctly rounded subtraction each: numpy's fp32 and the device agree bit
    for bit, and a sign test on them is exact) -> |Y_2 - Y_1|, Yh_2 - Yh_1 for the i and the j pairing, as float64"""
    i1, j1, i2, j2 = gdl_crops(y)
    hi1, hj1, hi2, hj2 = gdl_crops(yh)
    f = lambda v: v.astype(np.float64)
    return f(np.abs(i2 - i1)), f(hi2 - hi1), f(np.abs(j2 - j1)), f(hj2 - hj1)


def gdl_fwd_ref(yh, y):
    """-> (loss, bound).  loss = mean|t12| + mean|t34| over the exact differences of the fp32 inputs.  Bound: t1 = |a - b| (1
    rounding), t2 likewise, |t1 - t2| (1): the error of one term is at most U (t1 + t2 + |t1 - t2|) (1 + U): k = 1 on
    S = mean(t1 + t2 + |t1 - t2|) (+ the j pairing), with 0.1 % for the second order; fp64 reduction 1e-12"""
    i1, j1, i2, j2 = [v.astype(np.float64) for v in gdl_crops(y)]
    hi1, hj1, hi2, hj2 = [v.astype(np.float64) for v in gdl_crops(yh)]
    t1, t2, t3, t4 = np.abs(i2 - i1), np.abs(hi2 - hi1), np.abs(j2 - j1), np.abs(hj2 - hj1)
    cnt = t1.size
    loss = (sum64(np.abs(t1 - t2)) + sum64(np.abs(t3 - t4))) / cnt
    S = (sum64(t1 + t2 + np.abs(t1 - t2)) + sum64(t3 + t4 + np.abs(t3 - t4))) / cnt
    return loss, 1.001 * U * S + 1e-12 * loss


def gdl_bwd_counts(yh, y):
    """the gradient as an integer multiple of 1 / count per element, by SCATTER (gdl_criterion.lua:47-53 through the crops):
    pairing k hands s = -sign_ge0(t12[k]) * sign_ge0(Yh_2[k] - Yh_1[k]) to its `2` element and -s to its `1` element
    (THNN Abs / AbsCriterion: derivative +1 at 0)"""
    B, C, H, W = y.shape
    a12, d12, a34, d34 = gdl_terms(yh, y)
    sg = lambda v: np.where(v >= 0, 1, -1).astype(np.int64)
    s12 = -sg((a12.astype(F32) - np.abs(d12).astype(F32))) * sg(d12)
    s34 = -sg((a34.astype(F32) - np.abs(d34).astype(F32))) * sg(d34)
    K = np.zeros((B, C, H, W), np.int64)
    K[:, :, :, :W - 1] += s12.reshape(B, C, H, W - 1)
    K[:, :, :H - 1, :] -= s12.reshape(B, C, H - 1, W)
    K[:, :, :, 1:] += s34.reshape(B, C, H, W - 1)
    K[:, :, 1:, :] -= s34.reshape(B, C, H - 1, W)
    return K


def bce_inputs(n, seed):
    p = np.random.default_rng(seed).random(n, dtype=F32)
    edges = np.array([0.0, 1.0, 1e-9, 1e-12, 1 - 2.0 ** -24], F32)
    k = min(n, len(edges))
    p[hash_ints(k, seed, 0, n - 1) if n >= 64 else np.arange(k)] = edges[:k]
    return p


def bce_ref(p, label):
    """nn.BCECriterion with its 1e-12 epsilon, float64 (the device computes in float64 too) -> loss, sum of |terms| / n, gradient"""
    x, t, n = p.astype(np.float64), float(F32(label)), p.size
    terms = np.log(x + 1e-12) * t + np.log(1.0 - x + 1e-12) * (1.0 - t)
    g = -(1.0 / n) * (t - x) / ((1.0 - x + 1e-12) * (x + 1e-12))
    return -sum64(terms) / n, sum64(np.abs(terms)) / n, g


# --------------------------------------------------------------------------------------------------------------------- Adam
ADAM_SIZES = [4, 1023, 10007, SWEEP, SWEEP + 1031, 5 * SWEEP + 1]
ADAM_BETAS = [(0.5, 0.999), (0.9, 0.999)]
ADAM_LR, ADAM_EPS = 0.002, 1e-8
ADAM_PLANT = np.array([0.0, 1e-30, -1e-30, 1e-10, -1e-10, 1e3, -1e3], F32)


def adam_grad(n, seed):
    g = normal(n, seed, 1e-3)
    reps = max(1, min(8, n // (4 * len(ADAM_PLANT))))
    k = min(n, reps * len(ADAM_PLANT))
    pos = hash_ints(k, seed + 1, 0, n - 1) if n >= 64 else np.arange(k)
    g[pos] = np.tile(ADAM_PLANT, reps)[:k]
    return g


def adam_step_size(t, beta1, beta2, lr=ADAM_LR):
    return lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)


def adam_ref(x, g, m, v, t, beta1, beta2, lr=ADAM_LR, eps=ADAM_EPS):
    """optim.adam's update in float64 from the fp32 state -> (x, m, v) and their per-element bounds.

    vf_adam_upd, statement by statement (b1 = (float)beta1, omb1 = (float)(1 - beta1), ... each ONE rounding of the double):
      mi = mv * b1                  2 roundings (b1, the product) on A = |beta1 m|
      mi = mi + omb1 * gv           3 (omb1, the product, the sum)          -> m: k = 5 on S_m = |beta1 m| + |(1 - beta1) g|
      vi = vv * b2                  2
      vi = vi + (omb2 * gv) * gv    4 (omb2, two products, the sum)         -> v: k = 6 on S_v = beta2 v + (1 - beta2) g^2
      d = sqrtf(vi)                 correctly rounded: 1; vi carries dv = 6 U S_v + FLT_MIN (g^2 may underflow), and
                                    sqrt(v + dv) - sqrt(v) <= min(dv / (2 sqrt v), sqrt dv)
      d = d + eps                   2 (the rounding of (float)eps, the sum)  -> dd = dsqrt + U sqrt(v) + 2 U d
      xv = xv - (step * mi) / d     step is the fp32 rounding of the double k_adam_prep forms (1), the product (1), the quotient
                                    (1), the difference (1):
                                    dq = step (dm + FLT_MIN) / d + |q| (3 U + dd / d),   dx = dq + U (|x| + |q|) + FLT_MIN"""
    x64, g64, m64, v64 = [a.astype(np.float64) for a in (x, g, m, v)]
    step = adam_step_size(t, beta1, beta2, lr)
    mr = beta1 * m64 + (1 - beta1) * g64
    vr = beta2 * v64 + (1 - beta2) * g64 * g64
    sq = np.sqrt(vr)
    d = sq + eps
    q = step * mr / d
    xr = x64 - q
    dm = 5 * U * (np.abs(beta1 * m64) + np.abs((1 - beta1) * g64)) + FLT_MIN
    dv = 6 * U * vr + FLT_MIN
    with np.errstate(divide="ignore", invalid="ignore"):
        dsq = np.minimum(np.where(sq > 0, dv / (2 * sq), np.inf), np.sqrt(dv))
    dd = dsq + U * sq + 2 * U * d
    dq = step * (dm + FLT_MIN) / d + np.abs(q) * (3 * U + dd / d)
    dx = dq + U * (np.abs(x64) + np.abs(q)) + FLT_MIN
    return (xr, mr, vr), (dx, dm, dv)


# ------------------------------------------------------------------------------------------------------------ device harness
class Guard:
    """n elements at `off` elements past a 16-byte boundary inside a buffer filled with the NaN payload, PAD words either side"""

    def __init__(self, b, n, off=0, init=None, dtype=torch.float32):
        self.n, self.lo, self.dtype = n, PAD + off, dtype
        self.buf = torch.empty(2 * PAD + off + n, dtype=dtype, device=b.device)
        self.fill()
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[self.lo:self.lo + n]
        if init is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(init).reshape(-1)))

    def words(self, t):
        if self.dtype == torch.float64:
            return t.view(torch.int64), FILL64
        return (t.view(torch.int32) if self.dtype == torch.float32 else t), TAIL32 if self.dtype == torch.float32 else 0xA5

    def fill(self):
        w, pat = self.words(self.buf)
        w.fill_(pat)

    def check(self, what="", body_untouched=False):
        torch.cuda.synchronize()
        for name, seg in (("in front of", self.buf[:self.lo]), ("behind", self.buf[self.lo + self.n:])) + (
                (("inside (the call was refused or a no-op)", self.view),) if body_untouched else ()):
            w, pat = self.words(seg)
            bad = torch.nonzero(w != pat).flatten()
            assert bad.numel() == 0, "%s: %d guard words %s the output were overwritten (first at %d)" % (
                what, bad.numel(), name, int(bad[0]))

    def get(self):
        return to_np(self.view).copy()


def dview(b, a, off=0):
    """a read-only operand on the device at `off` floats past a 16-byte boundary"""
    a = np.ascontiguousarray(a).reshape(-1)
    buf = torch.empty(a.size + off + 4, dtype=torch.from_numpy(a[:0]).dtype, device=b.device)
    v = buf[off:off + a.size]
    v.copy_(torch.from_numpy(a))
    return v


def loss_slot(b):
    return Guard(b, 1, off=0, dtype=torch.float64)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def assert_bitwise(got, want32, what):
    bad = np.flatnonzero(bits(got) != bits(want32))
    assert bad.size == 0, "%s: %d of %d elements differ bitwise; first at %d: got %r, want %r" % (
        what, bad.size, got.size, bad[0], got.flat[bad[0]], want32.flat[bad[0]])


def assert_within(got, ref64, bound, what):
    err = np.abs(got.astype(np.float64) - ref64)
    bad = np.flatnonzero(~(err <= bound + FLT_MIN))
    assert bad.size == 0, "%s: %d of %d elements beyond the bound; first at %d: got %r, fp64 %r, |err| %.3e > %.3e" % (
        what, bad.size, got.size, bad[0], got.flat[bad[0]], ref64.flat[bad[0]], err.flat[bad[0]], bound.flat[bad[0]] + FLT_MIN)


def assert_loss(got, ref, rel, n, exact, what):
    print("%s: loss %.17g, reference %.17g, relative difference %.3e" % (what, got, ref, abs(got - ref) / max(abs(ref), 1e-300)))
    if exact and (n & (n - 1)) == 0:
        assert got == ref, "%s: loss %.17g != %.17g on exact inputs (n a power of two)" % (what, got, ref)
    else:
        tol = (1e-12 if exact else rel) * abs(ref)
        assert abs(got - ref) <= tol, "%s: loss %.17g, reference %.17g: |diff| %.3e > %.3e" % (what, got, ref, abs(got - ref), tol)


def last_error(b):
    return b.lib.vf_last_error().decode()


def pw_call(b, op, views, out, n, f, slope):
    """through the backend's wrappers where they take n from the output (views are flat)"""
    if op.startswith("act_fwd"):
        b.act_fwd(views[0], out, op[8:], slope)
    elif op.startswith("act_bwd"):
        b.act_bwd(views[0], views[1], out, op[8:], slope)
    elif op == "axpby":
        b.axpby(f[0], views[0], f[1], out)
    elif op == "cmul":
        b.cmul(views[0], out)
    elif op == "scale_shift":
        b.scale_shift(out, f[0], f[1])
    elif op == "compose":
        b.masked_compose(out, views[0], views[1], views[2])
    elif op == "mse_bwd":
        b.mse_bwd(views[0], views[1], out)


def pw_judge(op, got, ins, out0, f, n, exact, what):
    slope = pw_slope(exact)
    ref = pw_ref64(op, ins, out0, f, n, slope)
    assert not np.isnan(got).any(), "%s: NaN in the output" % what
    bound = pw_bound(op, ins, out0, f, n)
    if op in ("act_fwd_tanh", "act_fwd_sigmoid"):
        ulps = TRANSCENDENTAL_ULPS[op[8:]]
        assert_within(got, ref, ulps * ulp32(ref), what)
        return
    if exact and not pw_exact_is_bitwise(op, n):
        assert_within(got, ref, bound, what)
    elif bound is None or exact:
        assert_bitwise(got, ref.astype(F32), what)
    else:
        assert_within(got, ref, bound, what)


def offset_combos(nops, n):
    """operand offsets (floats past a 16-byte boundary), output last.  Every combination at n in {5, 1027, 65536}; elsewhere each
    operand alone by 1, 2, 3 and all of them together by 1, 2, 3"""
    import itertools
    if n in (5, 1027, 65536):
        return [c for c in itertools.product(range(4), repeat=nops) if any(c)]
    out = []
    for o in (1, 2, 3):
        out += [tuple(o if j == i else 0 for j in range(nops)) for i in range(nops)]
        if nops > 1:
            out.append((o,) * nops)
    return out


# ------------------------------------------------------------------------------------------------------- pointwise: the tests
# (tanhf / expf have no exact inputs: the random kind judges them.)  Ordered so that the ops of one size share its generated inputs
PW_CASES = [(op, n, kind) for n in PW_SIZES for kind in ("exact", "random") for op in PW
            if not (kind == "exact" and op in ("act_fwd_tanh", "act_fwd_sigmoid"))]


@pytest.mark.parametrize("op,n,kind", PW_CASES, ids=["pw_%s-n%d-%s" % c for c in PW_CASES])
def test_pointwise_aligned(op, n, kind, hipb):
    exact = kind == "exact"
    ins, out0, f = pw_inputs(op, n, 1000 + n % 997, exact)
    out = Guard(hipb, n, 0, out0)
    pw_call(hipb, op, [dview(hipb, a) for a in ins], out.view, n, f, pw_slope(exact))
    out.check(op)
    pw_judge(op, out.get(), ins, out0, f, n, exact, "%s n=%d %s" % (op, n, kind))


PW_UNALIGNED = [(op, n) for n in PW_SIZES if n <= 65536 for op in PW]


@pytest.mark.parametrize("op,n", PW_UNALIGNED, ids=["pw_%s-n%d-unaligned" % c for c in PW_UNALIGNED])
def test_pointwise_unaligned_views(op, n, hipb):
    """the vec = 0 route: any operand (the output alone, one input alone, ...) 1, 2 or 3 floats off a 16-byte boundary"""
    ins, out0, f = pw_inputs(op, n, 2000 + n % 997, False)
    for combo in offset_combos(len(ins) + 1, n):
        out = Guard(hipb, n, combo[-1], out0)
        pw_call(hipb, op, [dview(hipb, a, o) for a, o in zip(ins, combo)], out.view, n, f, SLOPE)
        what = "%s n=%d offsets(inputs..., out)=%r" % (op, n, combo)
        out.check(what)
        pw_judge(op, out.get(), ins, out0, f, n, False, what)


@pytest.mark.parametrize("off", [1, 2, 3], ids=lambda o: "off%d" % o)
@pytest.mark.parametrize("op", list(PW), ids=lambda o: "pw_" + o)
def test_pointwise_refuses_large_unaligned(op, off, hipb):
    from video_filler_amd._lib import VfError
    n = 65537
    ins, out0, f = pw_inputs(op, n, 7, False)
    nops = len(ins) + 1
    for which in range(nops):
        offs = [off if j == which else 0 for j in range(nops)]
        out = Guard(hipb, n, offs[-1])
        with pytest.raises(VfError):
            pw_call(hipb, op, [dview(hipb, a, o) for a, o in zip(ins, offs)], out.view, n, f, SLOPE)
        assert "aligned" in last_error(hipb), last_error(hipb)
        out.check("%s refused, offsets %r" % (op, offs), body_untouched=True)


@pytest.mark.parametrize("n,off", [(SWEEP + 7, 0), (1027, 1)], ids=["n2097159-aligned", "n1027-off1"])
@pytest.mark.parametrize("act", ["lrelu", "relu", "tanh", "sigmoid"])
def test_act_bwd_in_place_equals_out_of_place(act, n, off, hipb):
    """nn.py's in-place activations hand the incoming gradient as gy AND gx"""
    ins, _, f = pw_inputs("act_bwd_" + act, n, 31, False)
    y = dview(hipb, ins[0], off)
    out = Guard(hipb, n, off)
    hipb.act_bwd(y, dview(hipb, ins[1], off), out.view, act, SLOPE)
    out.check()
    inpl = Guard(hipb, n, off, ins[1])
    hipb.act_bwd(y, inpl.view, inpl.view, act, SLOPE)
    inpl.check("in place")
    assert_bitwise(inpl.get(), out.get(), "act_bwd %s in place against out of place" % act)
    fw = Guard(hipb, n, off, ins[1])
    ref = Guard(hipb, n, off)
    hipb.act_fwd(dview(hipb, ins[1], off), ref.view, act, SLOPE)
    hipb.act_fwd(fw.view, fw.view, act, SLOPE)
    fw.check("act_fwd in place")
    assert_bitwise(fw.get(), ref.get(), "act_fwd %s in place against out of place" % act)


@pytest.mark.parametrize("n", [1027, SWEEP + 7], ids=lambda n: "n%d" % n)
def test_activation_edges(n, hipb):
    """finite everywhere, tanh odd and exactly +-1 where float64's tanh is +-1, sigmoid(x) + sigmoid(-x) = 1 within both bounds"""
    x = act_inputs(n, 5)
    x = np.concatenate([x, -x])
    res = {}
    for act in ("tanh", "sigmoid"):
        out = Guard(hipb, x.size)
        hipb.act_fwd(dview(hipb, x), out.view, act, 0.0)
        out.check(act)
        res[act] = out.get()
        assert np.isfinite(res[act]).all(), act
    th, sg = res["tanh"], res["sigmoid"]
    assert_bitwise(th[n:], -th[:n], "tanh(-x) == -tanh(x)")
    one = np.abs(np.tanh(x.astype(np.float64))) == 1.0
    assert one.any() and (np.abs(th[one]) == 1.0).all() and (np.sign(th[one]) == np.sign(x[one])).all()
    ref = pw_ref64("act_fwd_sigmoid", [x], None, None, x.size, 0.0)
    tol = TRANSCENDENTAL_ULPS["sigmoid"] * (ulp32(ref[:n]) + ulp32(ref[n:])) + 2 * FLT_MIN
    assert (np.abs(sg[:n].astype(np.float64) + sg[n:] - 1.0) <= tol).all()
    assert ((sg >= 0) & (sg <= 1)).all()


# --------------------------------------------------------------------------------------------------------------- recon_grad_mix
RECON_SHAPES = [(64, 3, 64), (16, 48, 128), (3, 3, 48), (2, 3, 10), (1, 3, 9), (2, 5, 12), (1, 1, 2), (5, 12, 32)]


def recon_forms(H):
    bands = sorted({b for b in (1, 4, H // 2) if 1 <= b <= H // 2})
    return [("mask", 0)] + [("band", b) for b in bands] + [("none", 0)]


def recon_route(n, offs):
    """vf_recon_grad_mix's dispatch rule: the float4 kernel iff n % 4 == 0, n < 2^31 and every operand is 16-byte aligned"""
    return "recon_grad_mix" if n % 4 == 0 and not any(offs) else "recon_grad_mix_scalar"


RECON_CASES = [(s, form, band, unal) for s in RECON_SHAPES for form, band in recon_forms(s[2])
               for unal in ["aligned", "dfdg+1", "x+1"] + (["mask+1"] if form == "mask" else [])
               if unal == "aligned" or (form, band) == ("mask", 0) or ((form, band) == ("band", 1) and s[0] * s[1] * s[2] * s[2] < 1 << 20)]


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("shape,form,band,unal", RECON_CASES,
                         ids=["recon-B%dC%dH%d-%s%s-%s" % (s + (f, b if f == "band" else "", u)) for s, f, b, u in RECON_CASES])
def test_recon_grad_mix(shape, form, band, unal, kind, hipb):
    B, C, H = shape
    exact = kind == "exact"
    g, x, t, sc = recon_inputs(B, C, H, 77 + H, exact)
    mask, wsel = recon_weights(B, C, H, form, band, 77 + H)
    n = x.size
    offs = dict(dfdg=0, x=0, mask=0)
    if unal != "aligned":
        offs[unal[:-2]] = 1
    nhwc = lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1))
    as4 = lambda v: v.view(B, H, H, C).permute(0, 3, 1, 2)
    dg = Guard(hipb, n, offs["dfdg"], nhwc(g))
    dx, dt = as4(dview(hipb, nhwc(x), offs["x"])), as4(dview(hipb, nhwc(t)))
    dm = None if mask is None else as4(dview(hipb, nhwc(mask), offs["mask"]))
    slot = loss_slot(hipb)
    hipb.prof_begin()
    try:
        hipb.recon_grad_mix(as4(dg.view), dx, dt, dm, sc[0], sc[1], sc[2], band, slot.view)
    finally:
        prof = hipb.prof_end()
    dg.check("df_dg")
    slot.check("loss")
    want_route = recon_route(n, offs.values())
    assert list(prof) == [want_route] and prof[want_route]["launches"] == 1, (prof, want_route)
    got = dg.get().reshape(B, H, H, C).transpose(0, 3, 1, 2)
    ref, loss = recon_ref(g, x, t, wsel, sc)
    what = "recon %r %s%s %s %s" % (shape, form, band or "", unal, kind)
    if exact and (n & (n - 1)) == 0:
        assert_bitwise(got, ref.astype(F32), what)
    else:
        assert_within(got, ref, recon_bound(g, x, t, wsel, sc), what)
    assert_loss(float(slot.get()[0]), loss, RECON_LOSS_REL, n, exact, what)


def test_recon_grad_mix_refuses_a_band_on_non_square_maps(hipb):
    from helpers import to_dev as td
    x = np.zeros((1, 3, 8, 12), F32)
    dg = Guard(hipb, x.size)
    slot = loss_slot(hipb)
    with pytest.raises(ValueError):
        hipb.recon_grad_mix(dg.view.view(1, 8, 12, 3).permute(0, 3, 1, 2), td(x, hipb), td(x, hipb), None, 0.5, 1.0, 1.0, 2, slot.view)
    dg.check(body_untouched=True)
    slot.check(body_untouched=True)


# -------------------------------------------------------------------------------------------------------------- MSE / masked MSE
MSE_SIZES = [1, 3, 4, 1027, 1 << 23, 12582912, (1 << 25) + 3 * SWEEP + 7]


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("n", MSE_SIZES, ids=lambda n: "n%d" % n)
def test_mse_fwd_bwd(n, kind, hipb, oracle):
    exact = kind == "exact"
    x, t = mse_inputs(n, 300 + n % 991, exact)
    dx, dt = dview(hipb, x), dview(hipb, t)
    slot = loss_slot(hipb)
    hipb.mse_fwd(dx, dt, slot.view)
    slot.check("mse_fwd")
    ref = mse_ref(x, t)
    what = "mse_fwd n=%d %s" % (n, kind)
    assert_loss(float(slot.get()[0]), ref, MSE_FWD_REL, n, exact, what)
    if n <= 1 << 23:
        orc = oracle.MSECriterion().forward(x, t)
        assert abs(orc - ref) <= 1e-8 * abs(ref) + 1e-300, (orc, ref)      # a sequential float64 sum of n terms
    gx = Guard(hipb, n)
    hipb.mse_bwd(dx, dt, gx.view)
    gx.check("mse_bwd")
    pw_judge("mse_bwd", gx.get(), [x, t], None, (0, 0), n, exact, "mse_bwd n=%d %s" % (n, kind))


@pytest.mark.parametrize("n", [1, 5, 1027, 65536], ids=lambda n: "n%d" % n)
@pytest.mark.parametrize("offs", [(1, 0), (0, 2), (3, 3)], ids=lambda o: "off%d%d" % o)
def test_mse_fwd_unaligned_views_take_the_scalar_route(n, offs, hipb):
    for exact in (True, False):
        x, t = mse_inputs(n, 41, exact)
        slot = loss_slot(hipb)
        hipb.mse_fwd(dview(hipb, x, offs[0]), dview(hipb, t, offs[1]), slot.view)
        slot.check()
        assert_loss(float(slot.get()[0]), mse_ref(x, t), MSE_FWD_REL, n, exact, "mse_fwd n=%d offsets %r" % (n, offs))


def test_mse_fwd_refuses_large_unaligned(hipb):
    from video_filler_amd._lib import VfError
    x, t = mse_inputs(65537, 3, True)
    slot = loss_slot(hipb)
    with pytest.raises(VfError):
        hipb.mse_fwd(dview(hipb, x, 1), dview(hipb, t), slot.view)
    assert "aligned" in last_error(hipb)
    slot.check(body_untouched=True)


# every w x mask at the small sizes; at grid_for(n, 8)'s cap (2^22) and beyond it the two ends of the cross product
MMSE_CASES = [(n, w, mk, kind) for n in (1, 3, 4, 1027, 1 << 22, (1 << 22) + 3 * SWEEP + 7) for w in (0.05, 0.25, 1.0)
              for mk in ("all0", "all1", "rand") for kind in ("exact", "random")
              if n < 1 << 22 or (w, mk) in ((0.05, "rand"), (1.0, "all1"), (0.25, "all0"))]


@pytest.mark.parametrize("n,w,maskkind,kind", MMSE_CASES, ids=["mmse-n%d-w%g-%s-%s" % c for c in MMSE_CASES])
def test_masked_mse(n, w, maskkind, kind, hipb, oracle):
    """everything is float64 on the device: the loss to 1e-12 relative, the gradient to ONE rounding of the float64 value"""
    exact = kind == "exact"
    x, t = mse_inputs(n, 500 + n % 977, exact)
    m = {"all0": np.zeros(n, np.uint8), "all1": np.ones(n, np.uint8)}.get(maskkind)
    if m is None:
        m = (hash_ints(n, 9, 0, 1)).astype(np.uint8)
    w32 = float(F32(w))
    wm = (1.0 - w32) * m + w32
    d = x.astype(np.float64) - t.astype(np.float64)
    ref = sum64(wm * d * d) / n
    gref = (1.0 / n) * wm * 2.0 * d
    dx, dt, dm = dview(hipb, x), dview(hipb, t), dview(hipb, m)
    slot = loss_slot(hipb)
    hipb.masked_mse_fwd(dx, dt, dm, w, slot.view)
    slot.check()
    got = float(slot.get()[0])
    assert abs(got - ref) <= F64_REL * abs(ref), (got, ref)
    gx = Guard(hipb, n)
    hipb.masked_mse_bwd(dx, dt, dm, w, gx.view)
    gx.check()
    assert_within(gx.get(), gref, 1.0001 * U * np.abs(gref), "masked_mse_bwd n=%d w=%g %s" % (n, w, maskkind))
    if n <= 1 << 22:
        crit = oracle.MaskedMSECriterion(w)
        crit.setMask(m)
        assert abs(crit.forward(x, t) - ref) <= 1e-9 * abs(ref) + 1e-300
        assert_within(crit.backward(x, t), gref, 4 * U * np.abs(gref), "oracle masked_mse_bwd")


# ----------------------------------------------------------------------------------------------------------------------- GDL
GDL_BWD_ABS_U = 7      # see test_gdl
GDL_SHAPES = [(1, 1, 2), (2, 3, 3), (2, 3, 8), (4, 12, 32), (3, 5, 17), (2, 48, 128), (8, 48, 128)]


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("shape", GDL_SHAPES, ids=lambda s: "gdl-B%dC%dH%d" % s)
def test_gdl(shape, kind, hipb, oracle):
    B, C, H = shape
    n = B * C * H * H
    exact = kind == "exact"
    if exact:      # integers in [-2, 2]: most d and t12 are ties
        yh, y = [hash_ints(n, 60 + k, -2, 2).astype(F32).reshape(B, C, H, H) for k in (0, 1)]
    else:
        yh, y = [normal(n, 60 + k).reshape(B, C, H, H) for k in (0, 1)]
    dyh, dy = to_dev(yh, hipb), to_dev(y, hipb)
    slot = loss_slot(hipb)
    hipb.gdl_fwd(dyh, dy, slot.view)
    slot.check()
    got = float(slot.get()[0])
    ref, bound = gdl_fwd_ref(yh, y)
    what = "gdl %r %s" % (shape, kind)
    print("%s: loss %.17g reference %.17g" % (what, got, ref))
    assert abs(got - ref) <= (1e-12 * abs(ref) if exact else bound), (what, got, ref, bound)
    orc = oracle.GDLCriterion(1).forward(yh, y)
    assert abs(orc - ref) <= (1e-9 * abs(ref) if exact else 4 * bound + 1e-9 * abs(ref)), (orc, ref)
    # backward: the kernel adds up to four terms +-norm, norm = (float)(1 / count), one after the other in fp32.  The partial sums are
    # j * norm with |j| <= 4, and only j = +-3 is not a power-of-two multiple of norm: a sum that passes through it is rounded there
    # (<= 3 U norm) and once more by the add that follows (<= 4 U norm).  So |got - K norm| <= 7 U norm for every element, and an
    # element with |K| <= 1 never passes +-3 (0, 1, 2, 1 at most) and is bit-exact.  A wrong sign moves an element by 2 norm.
    g = Guard(hipb, n)
    hipb.gdl_bwd(dyh, dy, g.view.view(B, H, H, C).permute(0, 3, 1, 2))
    g.check("gdl_bwd")
    gg = g.get().reshape(B, H, H, C).transpose(0, 3, 1, 2)
    K = gdl_bwd_counts(yh, y)
    norm = float(F32(1.0 / (B * C * (H - 1) * H)))
    want = K.astype(np.float64) * norm
    small = np.abs(K) <= 1
    assert_bitwise(gg[small], want[small].astype(F32), what + " bwd (|K| <= 1)")
    assert_within(gg, want, np.full(want.shape, GDL_BWD_ABS_U * U * norm), what + " bwd")
    og = oracle.GDLCriterion(1).backward(yh, y)
    assert_within(og, want, 4 * U * np.abs(want) + 4 * U * norm, what + " bwd (oracle)")


def test_gdl_refuses_non_square_maps(hipb):
    from video_filler_amd._lib import VfError
    x = to_dev(np.zeros((1, 2, 4, 6), F32), hipb)
    slot = loss_slot(hipb)
    g = Guard(hipb, x.numel())
    with pytest.raises(VfError):
        hipb.gdl_fwd(x, x, slot.view)
    with pytest.raises(VfError):
        hipb.gdl_bwd(x, x, g.view.view(1, 4, 6, 2).permute(0, 3, 1, 2))
    slot.check(body_untouched=True)
    g.check(body_untouched=True)


# ----------------------------------------------------------------------------------------------------------------------- BCE
@pytest.mark.parametrize("labels", [(0.0, 1.0), (1.0, 0.0), (0.9, 0.1)], ids=lambda l: "labels%g_%g" % l)
@pytest.mark.parametrize("n", [1, 2, 37, 64, 255, 256, 257, 1000], ids=lambda n: "n%d" % n)
def test_bce(n, labels, hipb, oracle):
    """loss: |got - ref| <= 1e-12 * mean|terms| (float64 on both sides, the terms computed identically; only log's last place and
    the order of the sum differ); gradient: one rounding of the float64 value to fp32"""
    p = np.concatenate([bce_inputs(n, 80), bce_inputs(n, 81)])
    dp = dview(hipb, p)
    two = Guard(hipb, 2 * n)
    l0, l1 = loss_slot(hipb), loss_slot(hipb)
    hipb.bce_fwd_bwd(dp, labels[0], labels[1], n, 2, l0.view, l1.view, two.view)
    two.check("bce_fwd_bwd")
    for grp, (label, slot2) in enumerate(zip(labels, (l0, l1))):
        pg = p[grp * n:(grp + 1) * n]
        ref, cond, gref = bce_ref(pg, label)
        what = "bce n=%d group %d label %g" % (n, grp, label)
        slot = loss_slot(hipb)
        hipb.bce_fwd(dp[grp * n:(grp + 1) * n], label, slot.view)
        slot.check(what)
        slot2.check(what)
        got = float(slot.get()[0])
        assert abs(got - ref) <= 1e-12 * cond, (what, got, ref)
        assert float(slot2.get()[0]) == got, what + ": the one-launch loss differs from vf_bce_fwd's"
        gx = Guard(hipb, n)
        hipb.bce_bwd(dp[grp * n:(grp + 1) * n], label, gx.view)
        gx.check(what)
        assert_within(gx.get(), gref, 1.0001 * U * np.abs(gref), what + " gradient")
        assert_bitwise(two.get()[grp * n:(grp + 1) * n], gx.get(), what + ": one-launch gradient against vf_bce_bwd")
        one = Guard(hipb, n)
        s1 = loss_slot(hipb)
        hipb.bce_fwd_bwd(dp[grp * n:(grp + 1) * n], label, 0.0, n, 1, s1.view, None, one.view)
        one.check(what)
        s1.check(what)
        assert float(s1.get()[0]) == got
        assert_bitwise(one.get(), gx.get(), what + ": one-group launch")
        if label in (0.0, 1.0):
            t = np.full(n, label, F32)
            assert abs(oracle.BCECriterion().forward(pg, t) - ref) <= 1e-9 * max(1.0, cond)
            assert_within(oracle.BCECriterion().backward(pg, t), gref, 4 * U * np.abs(gref), what + " (oracle)")


# ---------------------------------------------------------------------------------------------------------------------- Adam
def _adam_state(n, seed):
    x = normal(n, seed)
    m = normal(n, seed + 1, 1e-3)
    v = (normal(n, seed + 2, 1e-3) ** 2).astype(F32)
    g0 = adam_grad(n, seed + 3)
    zero = g0 == 0
    m[zero] = 0
    v[zero] = 0
    return x, m, v


def _adam_check(got, before, g, t, b1, b2, what):
    (xr, mr, vr), (dx, dm, dv) = adam_ref(*before[:1], g, *before[1:], t, b1, b2)
    for name, a, r, bd in (("m", got[1], mr, dm), ("v", got[2], vr, dv), ("x", got[0], xr, dx)):
        assert_within(a, r, bd, "%s step %d: %s" % (what, t, name))
    still = (g == 0) & (before[1] == 0) & (before[2] == 0)
    assert_bitwise(got[0][still], before[0][still], what + ": x where g = m = v = 0")


# vf_adam_step at every size; vf_adam_prep + vf_adam_apply (the same kernel behind another entry point) at a tail and beyond the cap
ADAM_CASES = [(n, b, "step") for n in ADAM_SIZES for b in ADAM_BETAS] + [(n, b, "prep_apply") for n in (1023, SWEEP + 1031) for b in ADAM_BETAS]


@pytest.mark.parametrize("n,betas,form", ADAM_CASES, ids=["adam-n%d-b%g_%g-%s" % (n, b[0], b[1], f) for n, b, f in ADAM_CASES])
def test_adam(n, betas, form, hipb, oracle):
    """five steps; before each one the float64 reference restarts from the device's fp32 (x, m, v): the one-step bound of adam_ref
    holds at every step"""
    b1, b2 = betas
    x, m, v = _adam_state(n, 90)
    G = [Guard(hipb, n, 0, a) for a in (x, m, v)]
    t_dev = torch.zeros(2, dtype=torch.int32, device=hipb.device)
    ostate, ox = None, None
    for t in range(1, 6):
        g = adam_grad(n, 90 + 3) if t == 1 else adam_grad(n, 200 + t)
        before = [a.get() for a in G]
        dg = dview(hipb, g)
        if form == "step":
            hipb.adam_step(G[0].view, dg, G[1].view, G[2].view, ADAM_LR, b1, b2, ADAM_EPS, t_dev)
        else:
            hipb.adam_prep(ADAM_LR, b1, b2, t_dev)
            hipb.adam_apply(G[0].view, dg, G[1].view, G[2].view, b1, b2, ADAM_EPS, t_dev)
        for a in G:
            a.check("adam n=%d" % n)
        td = t_dev.cpu().numpy()
        assert td[0] == t
        assert td[1:].view(F32)[0] == F32(adam_step_size(t, b1, b2)), "t_dev[1] is not the fp32 rounding of the step size"
        got = [a.get() for a in G]
        _adam_check(got, before, g, t, b1, b2, "adam n=%d betas %r" % (n, betas))
        if n <= SWEEP:      # the oracle's optim.adam from the same state, one step
            st = {"learningRate": ADAM_LR, "beta1": b1, "beta2": b2, "t": t - 1, "m": before[1].copy(), "v": before[2].copy(),
                  "denom": np.zeros(n, F32)}
            xo = before[0].copy()
            oracle.adam(lambda _x: (0.0, g), xo, st)
            (xr, mr, vr), (dx, dm, dv) = adam_ref(before[0], g, before[1], before[2], t, b1, b2)
            assert_within(xo, xr, 2 * dx, "oracle adam x")


def test_adam_ranges(hipb):
    """ranges that together cross the cap, one of a single float4, two that touch; every float between them bitwise untouched"""
    n = 2 * SWEEP + 8192
    ranges = [(0, 4), (64, 64 + SWEEP), (SWEEP + 4096, SWEEP + 4096 + 1028), (SWEEP + 4096 + 1028, SWEEP + 4096 + 2048),
              (SWEEP + 8192, n - 1024)]
    b1, b2 = 0.9, 0.999
    x, m, v = _adam_state(n, 120)
    g = adam_grad(n, 123)
    G = [Guard(hipb, n, 0, a) for a in (x, m, v)]
    t_dev = torch.zeros(2, dtype=torch.int32, device=hipb.device)
    hipb.adam_prep(ADAM_LR, b1, b2, t_dev)
    hipb.adam_apply_ranges(G[0].view, dview(hipb, g), G[1].view, G[2].view, ranges, b1, b2, ADAM_EPS, t_dev)
    for a in G:
        a.check("adam ranges")
    got = [a.get() for a in G]
    inside = np.zeros(n, bool)
    for lo, hi in ranges:
        inside[lo:hi] = True
    for name, a, a0 in zip("xmv", got, (x, m, v)):
        assert_bitwise(a[~inside], a0[~inside], "adam ranges: %s between the ranges" % name)
    sel = lambda arrs: [a[inside] for a in arrs]
    _adam_check(sel(got), sel([x, m, v]), g[inside], 1, b1, b2, "adam ranges")
    assert (got[1][inside] != m[inside]).sum() >= 0.9 * inside.sum(), "the ranges were not updated"


@pytest.mark.parametrize("which", range(4), ids=["x", "g", "m", "v"])
def test_adam_refuses_unaligned_operands(which, hipb):
    from video_filler_amd._lib import VfError
    n = 1024
    offs = [1 if j == which else 0 for j in range(4)]
    x, m, v = _adam_state(n, 5)
    G = [Guard(hipb, n, o, a) for o, a in zip((offs[0], offs[2], offs[3]), (x, m, v))]
    t_dev = torch.zeros(2, dtype=torch.int32, device=hipb.device)
    hipb.adam_prep(ADAM_LR, 0.5, 0.999, t_dev)
    dg = dview(hipb, adam_grad(n, 6), offs[1])
    for call in (lambda: hipb.adam_apply(G[0].view, dg, G[1].view, G[2].view, 0.5, 0.999, ADAM_EPS, t_dev),
                 lambda: hipb.adam_apply_ranges(G[0].view, dg, G[1].view, G[2].view, [(0, 512)], 0.5, 0.999, ADAM_EPS, t_dev)):
        with pytest.raises(VfError):
            call()
        assert "aligned" in last_error(hipb)
    for a, a0 in zip(G, (x, m, v)):
        a.check()
        assert_bitwise(a.get(), a0, "refused Adam call")


# ------------------------------------------------------------------------------------------------- transposes, zero_segments
@pytest.mark.parametrize("B", [1, 3], ids=lambda v: "B%d" % v)
@pytest.mark.parametrize("HW", [(1, 1), (4, 4), (33, 31), (32, 32), (25, 41)], ids=lambda s: "HW%d" % (s[0] * s[1]))
@pytest.mark.parametrize("C", [1, 3, 31, 32, 33, 100], ids=lambda v: "C%d" % v)
def test_transposes(C, HW, B, hipb):
    H, W = HW
    n = B * C * H * W
    x = np.arange(n, dtype=np.int64).astype(F32).reshape(B, C, H, W) + F32(0.5)      # position coded, exact below 2^24
    src = dview(hipb, x)
    nhwc = Guard(hipb, n)
    hipb._c("vf_nchw_to_nhwc", src.data_ptr(), nhwc.view.data_ptr(), B, C, H, W)
    nhwc.check("nchw_to_nhwc")
    assert_bitwise(nhwc.get().reshape(B, H, W, C), x.transpose(0, 2, 3, 1), "nchw_to_nhwc")
    back = Guard(hipb, n)
    hipb._c("vf_nhwc_to_nchw", nhwc.view.data_ptr(), back.view.data_ptr(), B, C, H, W)
    back.check("nhwc_to_nchw")
    assert_bitwise(back.get().reshape(B, C, H, W), x, "round trip")
    y = x + F32(1)
    ynhwc = dview(hipb, y.transpose(0, 2, 3, 1))
    back.fill()
    hipb._c("vf_nhwc_to_nchw", ynhwc.data_ptr(), back.view.data_ptr(), B, C, H, W)
    back.check()
    assert_bitwise(back.get().reshape(B, C, H, W), y, "nhwc_to_nchw")


ZERO_LENS = [0, 1, 255, 256, 257, 1000003]


@pytest.mark.parametrize("layout", ["adjacent", "separated"])
def test_zero_segments(layout, hipb):
    gap = 0 if layout == "adjacent" else 5
    offs, o = [], 3
    for ln in ZERO_LENS:
        offs.append(o)
        o += ln + gap
    n = o + 7
    base0 = np.arange(n, dtype=np.int64).astype(F32) + F32(1)
    base = Guard(hipb, n, 0, base0)
    dev = lambda v: torch.tensor(v, dtype=torch.int64, device=hipb.device)
    hipb.zero_segments(base.view, dev(offs), dev(ZERO_LENS))
    base.check("zero_segments")
    want = base0.copy()
    for of, ln in zip(offs, ZERO_LENS):
        want[of:of + ln] = 0
    assert_bitwise(base.get(), want, "zero_segments " + layout)
    hipb.zero_segments(base.view, dev([]), dev([]))
    base.check()
    assert_bitwise(base.get(), want, "nseg = 0")


# --------------------------------------------------------------------------------------------------------------------- n = 0
def test_empty_operands_are_a_no_op(hipb):
    """include/vf_hip.h: n <= 0 launches nothing and writes nothing, on every entry point of vf_core.hip"""
    b = hipb
    out = Guard(b, 16)
    e = out.view[:0]
    slot, slot1 = loss_slot(b), loss_slot(b)
    one = dview(b, np.ones(16, F32))
    z = one[:0]
    e4 = out.view[:0].view(0, 1, 1, 1)
    z4 = z.view(0, 1, 1, 1)
    t_dev = torch.zeros(2, dtype=torch.int32, device=b.device)
    b.adam_prep(ADAM_LR, 0.5, 0.999, t_dev)
    calls = [lambda: b.act_fwd(z, e, "tanh"), lambda: b.act_bwd(z, z, e, "lrelu", 0.2), lambda: b.axpby(1.0, z, 1.0, e),
             lambda: b.cmul(z, e), lambda: b.scale_shift(e, 2.0, 1.0), lambda: b.masked_compose(e, z, z, z),
             lambda: b.mse_bwd(z, z, e), lambda: b.mse_fwd(z, z, slot.view), lambda: b.bce_fwd(z, 1.0, slot.view),
             lambda: b.bce_bwd(z, 1.0, e), lambda: b.bce_fwd_bwd(z, 1.0, 0.0, 0, 2, slot.view, slot1.view, e),
             lambda: b.recon_grad_mix(e4, z4, z4, None, 0.5, 1.0, 1.0, 0, slot.view),
             lambda: b.masked_mse_fwd(z, z, z.view(torch.uint8)[:0], 0.05, slot.view),
             lambda: b.masked_mse_bwd(z, z, z.view(torch.uint8)[:0], 0.05, e),
             lambda: b.gdl_fwd(one[:2].view(2, 1, 1, 1), one[:2].view(2, 1, 1, 1), slot.view),
             lambda: b.gdl_bwd(one[:2].view(2, 1, 1, 1), one[:2].view(2, 1, 1, 1), out.view[:2].view(2, 1, 1, 1)),
             lambda: b.adam_apply(e, z, e, e, 0.5, 0.999, ADAM_EPS, t_dev),
             lambda: b._c("vf_nchw_to_nhwc", one.data_ptr(), out.view.data_ptr(), 0, 3, 4, 4),
             lambda: b._c("vf_nhwc_to_nchw", one.data_ptr(), out.view.data_ptr(), 2, 0, 4, 4)]
    for i, call in enumerate(calls):
        call()
        out.check("call %d" % i, body_untouched=True)
        slot.check("call %d" % i, body_untouched=True)
        slot1.check("call %d" % i, body_untouched=True)
