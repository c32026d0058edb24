"""What a conv gradBias must be: gb[c] = beta * gb0[c] + sum_p g[p][c] over a row-major [P][C] gradOutput, as csrc/vf_bn.hip forms it
(single tensor: vf_internal_colsum -> k_colsum4 / k_colsum1 -> k_reduce_partials<2>; a whole backward walk: vf_bias_grad_multi ->
k_colsum4_multi -> k_reduce_bias_multi).  No device: tests/test_bias_grad_ref.py checks this file on the CPU, tests/test_gpu_bias_grad.py
holds the kernels to it.

  generators   exact_g / exact_gb0: position-hashed integers, g in [-8, 8], gb0 EVEN in [-8, 8] (so beta = 0.5 stays exact too).  Every
               case here has P <= 2^18, so every fp32 partial sum and every total is an integer below 2^21 + 8 < 2^24: exact in fp32,
               whatever the order.  A dropped, duplicated or misrouted row or block changes an integer.
               random_g / random_gb0: Gaussians with mean 1, sd 1 — the mean keeps the error of the partial sums from cancelling.
  ref64        the float64 column sums plus beta * gb0 in float64.
  bound        derived below, nothing in it is measured.
  emulate      the kernels' summation order in numpy: fp32 per thread, then fp64 in the kernels' fixed order, then the fp32 epilogue
               (both as written and contracted to one fused multiply-add).
  CASES / MULTI_TABLES  the (P, C, route) cases both test files walk, with the geometry each one is there to reach.

Bound, per column c, for one call.  U = 2^-24, S_c = sum_p |g[p][c]|, n_t = the rows ONE thread adds in fp32.
  * A thread's fp32 running sum over n_t terms makes n_t - 1 rounded additions (the first lands on +0): its error is at most
    (n_t - 1) U times the sum of the absolute values it added, to first order; over all threads of all blocks (n_t - 1) U S_c.
  * The threads of a block, the blocks of a column: added in DOUBLE (LDS walk / tree, k_reduce_partials or k_reduce_bias_multi).  At most
    256 + 1024 double additions on sums bounded by S_c: below 1280 * 2^-53 S_c < 2^-42 S_c.
  * The epilogue gb = fl(fl(beta * gb0) + fl32(t)): fl32(t) costs U |t| <= U S_c, the product U |beta gb0|, the addition
    U (|beta gb0| + |t|) (1 + 2U); contracted to one fused multiply-add it is the same without the product's rounding.
    Together at most 2 U S_c + 2 U |beta gb0| to first order.
  Sum: (n_t + 1) U S_c + 2 U |beta gb0| + second-order terms; those are below U S_c + U |beta gb0| for every n_t here
  (n_t^2 U^2 < U needs n_t < 4096; the table's largest is 1024).  Hence
      |got - ref| <= (n_t + 2) U S_c + 3 U |beta gb0_c| + FLT_MIN
  with FLT_MIN for a denormal result the device flushes.
  n_t = rows_per_block / (256 / cq) on the float4 kernels (a thread walks rows r0 + ty, r0 + ty + rp, ...), ceil(rows_per_block / 256)
  in k_colsum1 (threads along the rows)."""
import ctypes

import numpy as np

import bn_ref

F32 = np.float32
U = 2.0 ** -24
FLT_MIN = float(np.finfo(np.float32).tiny)


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------- generators
def _hash(n, seed):
    """splitmix64 of (flat index + seed)"""
    with np.errstate(over="ignore"):
        h = (np.arange(n, dtype=np.uint64) + np.uint64(seed * 0x632BE5AB + 1)) * np.uint64(0x9E3779B97F4A7C15)
        h ^= h >> np.uint64(29)
        h *= np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(32)
    return h


def exact_g(P, C, seed):
    """[P][C] float32 integers in [-8, 8], position coded"""
    return ((_hash(P * C, seed) % np.uint64(17)).astype(np.int64) - 8).astype(F32).reshape(P, C)


def exact_gb0(C, seed):
    """[C] float32 EVEN integers in [-8, 8]: beta * gb0 is an integer for beta in {0, 1, 0.5}"""
    return (2 * ((_hash(C, seed + 7919) % np.uint64(9)).astype(np.int64) - 4)).astype(F32)


def random_g(P, C, seed):
    return (np.random.default_rng(seed).standard_normal((P, C), dtype=F32) + F32(1)).astype(F32)


def random_gb0(C, seed):
    return (np.random.default_rng(seed + 7919).standard_normal(C, dtype=F32) + F32(1)).astype(F32)


# ------------------------------------------------------------------------------------------------------------- reference and bound
def ref64(g, gb0, beta):
    t = np.asarray(g, np.float64).sum(0)
    if beta != 0:       # beta == 0: gb0 is not read (it may hold NaN)
        t = t + float(F32(beta)) * np.asarray(gb0, np.float64)
    return t


def bound(g, gb0, beta, n_t):
    S = np.abs(np.asarray(g, np.float64)).sum(0)
    carry = np.abs(float(F32(beta)) * np.asarray(gb0, np.float64)) if beta != 0 else 0.0
    return (n_t + 2) * U * S + 3 * U * carry + FLT_MIN


# ------------------------------------------------------------------------------------------------------------- geometry
def f4_geom(P, C):
    """vf_bias_grad_plan restated (bn_geom at one block per 32 KB, 128 .. 512 blocks) -> dict(cq, rp, gy, gx, rows_per_block).  The
    CPU test asks the library for the same figures; this restatement only feeds the emulation."""
    return bn_ref.bn_geom(P, C, bn_ref.bn_stat_blocks(P, C, 32768))


def plan_from_library(lib, P, C):
    """vf_bias_grad_plan itself (host-only) -> dict(cq, rp, gy, gx, rows_per_block)"""
    v = [ctypes.c_int() for _ in range(4)]
    rc = lib.vf_bias_grad_plan(P, C, *[ctypes.byref(x) for x in v])
    assert rc == 0, lib.vf_last_error()
    cq, rpb, gx, gy = [x.value for x in v]
    return dict(cq=cq, rp=256 // cq, gy=gy, gx=gx, rows_per_block=rpb)


def scalar_geom(P, C):
    """vf_internal_colsum's slab arithmetic for the k_colsum1 route, restated (tests/test_gpu_bias_grad.py pins it on the device:
    the partial rows one case leaves in its workspace) -> dict(nslab, rows_per_block)"""
    rpb = max(256, cdiv(P, max(1, 1024 // C)))
    return dict(nslab=cdiv(P, rpb), rows_per_block=rpb)


def rows_per_thread(route, geo):
    return geo["rows_per_block"] // geo["rp"] if route == "f4" else cdiv(geo["rows_per_block"], 256)


# ------------------------------------------------------------------------------------------------------------- emulation
def partials_f4(g, geo):
    """k_colsum4 / k_colsum4_multi: [gx][C] float64"""
    P, C = g.shape
    return bn_ref._partials([np.asarray(g, F32)], P, C, geo)[:, 0]


def partials_scalar(g, geo):
    """k_colsum1: thread t of slab s adds rows r0 + t, r0 + t + 256, ... in fp32; the 256 threads meet in a double tree
    (offsets 128, 64, ... 1) -> [nslab][C] float64"""
    P, C = g.shape
    ns, rpb = geo["nslab"], geo["rows_per_block"]
    K = cdiv(rpb, 256)
    pad = np.zeros((ns, K * 256, C), F32)      # a row past the slab's end adds +0: the value the thread keeps
    for s in range(ns):
        rows = g[s * rpb:min(P, (s + 1) * rpb)]
        pad[s, :len(rows)] = rows
    pad = pad.reshape(ns, K, 256, C)
    acc = np.zeros((ns, 256, C), F32)
    for k in range(K):
        acc = acc + pad[:, k]
    red = acc.astype(np.float64)
    o = 128
    while o > 0:
        red = red[:, :o] + red[:, o:2 * o]
        o >>= 1
    return red[:, 0]


def total_single(part):
    """k_reduce_partials' column_total"""
    return bn_ref._column_total(part)


def total_multi(part):
    """k_reduce_bias_multi: lane l of a column's wave adds partial rows l, l + 128, ... into s0 and l + 64, l + 192, ... into s1 while
    both exist, the rest into s0; t = s0 + s1; then the shuffle tree (offsets 32 .. 1), lane 0 keeps the total"""
    gx, ncol = part.shape
    t = np.zeros((64, ncol))
    for lane in range(64):
        s0, s1 = np.zeros(ncol), np.zeros(ncol)
        k = lane
        while k + 64 < gx:
            s0 = s0 + part[k]
            s1 = s1 + part[k + 64]
            k += 128
        while k < gx:
            s0 = s0 + part[k]
            k += 64
        t[lane] = s0 + s1
    off = 32
    while off > 0:
        t = t[:off] + t[off:2 * off]
        off >>= 1
    return t[0]


def epilogue(t, gb0, beta, fused):
    """gb = (beta != 0 ? beta * gb : 0) + (float)t in fp32; fused: the product and the sum contracted to one fused multiply-add"""
    tf = t.astype(F32)
    if beta == 0:
        return (F32(0) + tf).astype(F32)
    b, g0 = F32(beta), np.asarray(gb0, F32)
    if fused:      # the exact product (a float64 holds it) plus tf, rounded once.  The float64 sum is exact to 2^-53: it decides no tie here
        return (b.astype(np.float64) * g0.astype(np.float64) + tf.astype(np.float64)).astype(F32)
    return ((b * g0).astype(F32) + tf).astype(F32)


def emulate(g, gb0, beta, route, stage2, fused=False):
    """route 'f4' | 'scalar'; stage2 'single' | 'multi' (the multi kernels have no scalar route) -> float32 [C]"""
    P, C = g.shape
    if route == "f4":
        part = partials_f4(g, f4_geom(P, C))
    else:
        assert stage2 == "single"
        part = partials_scalar(g, scalar_geom(P, C))
    t = total_single(part) if stage2 == "single" else total_multi(part)
    return epilogue(t, gb0, beta, fused)


# ------------------------------------------------------------------------------------------------------------- cases
def _case(P, C, route="f4", **reach):
    return dict(P=P, C=C, route=route, reach=reach, id="%s-C%d-P%d" % (route, C, P))


# Float4 route.  rp = 256 / cq row lanes per block; for small P a block takes rp rows, so P in {1, rp - 1, rp, rp + 1} are: one row, a
# short only block, a whole block, a second block of ONE row.  `reach` names the geometry a case exists for (checked against the
# library on the CPU: retune bn_geom and the case that lost its geometry fails by name).
CASES = [
    # C = 4: one float4 column, 256 row lanes
    _case(1, 4, cq=1, gy=1, gx=1), _case(255, 4), _case(256, 4, gx=1), _case(257, 4, gx=2),
    # C = 12: three live float4 columns of four (one idle column lane), 64 row lanes
    _case(1, 12, cq=4, gy=1, gx=1), _case(63, 12), _case(64, 12), _case(65, 12, gx=2), _case(897, 12, gx=15),
    # C = 64: 16 columns, 16 row lanes
    _case(1, 64, cq=16, gy=1, gx=1), _case(15, 64), _case(16, 64), _case(17, 64, gx=2), _case(256, 64, gx=16), _case(257, 64, gx=17),
    _case(65536, 64, gx=512),
    # C = 256: 64 columns, 4 row lanes
    _case(1, 256, cq=64, gy=1, gx=1), _case(3, 256), _case(4, 256), _case(5, 256, gx=2), _case(192, 256, gx=48), _case(193, 256, gx=49),
    _case(256, 256, gx=64), _case(257, 256, gx=65), _case(512, 256, gx=128), _case(4128, 256, gx=129), _case(16384, 256, gx=512),
    # C = 260: two column chunks, ONE live float4 column in the second
    _case(1, 260, cq=64, gy=2, gx=1), _case(3, 260), _case(4, 260), _case(5, 260, gx=2), _case(253, 260, gy=2, gx=64),
    # C = 512: two full column chunks
    _case(1, 512, cq=64, gy=2, gx=1), _case(3, 512), _case(4, 512), _case(5, 512, gx=2), _case(2080, 512, gy=2, gx=65),
    # C = 4000 (nBottleneck): 16 column chunks, the last with 40 of 64 columns
    _case(1, 4000, cq=64, gy=16, gx=1), _case(3, 4000), _case(4, 4000), _case(5, 4000, gx=2), _case(33, 4000, gy=16), _case(1048, 4000, gy=16),
    # Scalar route (C % 4 != 0, or a misaligned g): nslab slabs of at least 256 rows, at most max(1, 1024 / C) of them.
    # 513 and 1024 slabs (k_reduce_partials' second pass of 512 rows) need C = 1.
    _case(1, 1, "scalar", nslab=1), _case(255, 1, "scalar"), _case(256, 1, "scalar", nslab=1), _case(257, 1, "scalar", nslab=2),
    _case(130817, 1, "scalar", nslab=512), _case(131073, 1, "scalar", nslab=513), _case(261889, 1, "scalar", nslab=1024),
    _case(1, 3, "scalar", nslab=1), _case(255, 3, "scalar"), _case(256, 3, "scalar"), _case(257, 3, "scalar", nslab=2),
    _case(87041, 3, "scalar", nslab=341),
    _case(1, 5, "scalar"), _case(255, 5, "scalar"), _case(256, 5, "scalar"), _case(257, 5, "scalar", nslab=2),
    _case(1, 6, "scalar"), _case(255, 6, "scalar"), _case(256, 6, "scalar"), _case(257, 6, "scalar", nslab=2),
    # C = 8 with g one float past a 16-byte boundary: the alignment test sends it to k_colsum1
    _case(1, 8, "scalar"), _case(255, 8, "scalar"), _case(256, 8, "scalar"), _case(257, 8, "scalar", nslab=2), _case(32769, 8, "scalar", nslab=128),
]

REQUIRED_F4 = dict(cq={1, 4, 16, 64}, gy={1, 2, 16}, gx={1, 15, 16, 17, 48, 49, 64, 65, 128, 129, 512})
REQUIRED_SCALAR = dict(nslab={1, 2, 341, 512, 513, 1024})

# vf_bias_grad_multi: tables of (P, C, beta).  A one-block layer stands first, last, and between the two 512-slab layers; the rest mix
# the float4 geometries above (gx 15, 49, 64, 65, 128, 129; gy 1, 2, 16); beta cycles through 0, 1, 0.5.
MULTI_TABLES = {
    1: [(4128, 256, 1.0)],
    2: [(257, 256, 0.0), (1, 4, 0.5)],
    13: [(1, 4, 0.0), (65536, 64, 1.0), (2, 12, 0.5), (16384, 256, 0.0), (4128, 256, 1.0), (257, 256, 0.5), (512, 256, 0.0),
         (256, 256, 1.0), (193, 260, 0.5), (2080, 512, 0.0), (33, 4000, 1.0), (897, 12, 0.5), (5, 64, 1.0)],
}


def cases(route=None, C=None):
    return [c for c in CASES if (route is None or c["route"] == route) and (C is None or c["C"] == C)]
