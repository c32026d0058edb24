"""References for the BatchNorm kernels of vf_bn.hip: numpy only, nothing of the project is linked.

Layout: activations are row-major [groups * npix][C] float32 (the NHWC rows the kernels walk); a batch group g owns rows
[g * npix, (g + 1) * npix).  Per-group statistics are [groups][C], per-channel values [C].

  ref64      THNN BatchNormalization (train forward, backward, evaluate forward) evaluated in float64 from the fp32 inputs: two
             passes over the data, no shift, nothing rounded to fp32 on the way.
  emulate32  the kernels' arithmetic restated step by step (k_bn_stats, k_reduce_partials / k_bn_finalize, k_bn_apply,
             k_bn_eval_coeff, k_bn_bwd_stats, k_bn_bwd_apply): the shift subtracted in fp32, every thread's fp32 partial sums over
             exactly the rows r0 + ty, r0 + ty + rp, ... that bn_geom / bn_stat_blocks give it, the doubles afterwards in the
             kernels' order (the rp row lanes of a block, then k_reduce_partials' four running sums per slab lane and its 16 slab
             lanes), and a cast to float wherever the kernels cast.  The geometry functions are restated from the .hip source
             (`bn_geom`, `bn_stat_blocks` below), so this is the route "restate the geometry", not "worst grouping".  The library
             is built with -ffp-contract=off: every fp32 multiply and add rounds on its own, as numpy's float32 does.
  bounds     forward-error bounds of the device outputs against ref64, per element or per channel, derived below.

Derivation of `bounds`.  u = 2^-24 is the unit roundoff of fp32.  Everything on the right-hand sides is a float64 quantity of
ref64's (or an input).  Per channel and group: n rows, s the shift (the running mean before the call, the same for every
group), mean, var = m2 / n, d = mean - s, kappa = d^2 / var, K the rows a thread sums in fp32 (rows_per_block / rp of the
statistics launch, Kb for the backward statistics), A1 = sum |x - s|, A2 = sum (x - s)^2 = n var (1 + kappa).
A factor SLACK = 1.01 on every rounding term covers the second-order terms and the float64 roundings of the partials (each
2^-53 against 2^-24); it is valid while K u < 2^-8, which `bounds` asserts.

  q1 = sum fl(x - s): one rounding per term and at most K - 1 more in the thread's running sum:   |dq1| <= K u A1
  save_mean = fl(s + q1 / n):                       B_mean = u (|mean| + K A1 / n)
      (u times |mean| plus rows_per_thread times the mean |x - s|)
  q2 = sum fl(fl(x - s)^2): three roundings per term, K - 1 in the running sum, all terms >= 0:   |dq2| <= (K + 2) u A2
  m2 = q2 - q1^2 / n:                               D n = |dm2| <= (K + 2) u A2 + 2 |d| K u A1
      Relative to m2 = n var this is (K + 2) u (1 + kappa) + 2 K u sqrt(kappa) A1 / (n sigma): the conditioning term.  With
      A1 <= n sigma sqrt(1 + kappa) it is at most (3 K + 2) u (1 + kappa): for kappa <= 1 a few K u, i.e. tight; it grows
      linearly in kappa.  The clamp m2 < 0 -> 0 only moves the value towards the true one.  n = 1: the kernels set m2 = 0.
  save_invstd = fl(1 / sqrt(m2' / n + eps)) with |m2' - m2| <= D n and m2' >= 0:  not linearised (D can exceed var):
      w = var + eps, lo = 1 / sqrt(w + D), hi = 1 / sqrt(max(w - D, eps)),
                                                    B_invstd = max(hi - is, is - lo) + u hi,      is_up = is + B_invstd
      For D << w this is D / (2 w) relative: save_invstd may leave 1e-5 relative once (3 K + 2) u (1 + kappa) / 2 reaches 1e-5,
      kappa ~ 110 / K (K = 8 on the nets' tensors up to 16 MB: |mean - s| ~ 3.7 sigma; K = 64 at 128 MB: 1.3 sigma).
  running_mean <- fl(m mean' + (1 - m) running_mean), group after group:
                                                    B_rm = m B_mean + (1 - m) B_rm(previous group) + u |running_mean|
  running_var likewise with m2' / (n - 1):          B_rv = m D n / (n - 1) + (1 - m) B_rv(previous) + u |running_var|
  y = act(fl(fl(fl(fl(x - mean') is') gamma) + beta)), a = |x - mean| + B_mean:
      B_y = |gamma| (is_up B_mean + |x - mean| B_invstd) + u (4 |gamma| a is_up + |beta|)  [+ u (|y| + B_y) for LeakyReLU's
      multiply].  An element whose sign differs between device and reference stays inside: for slopes in [0, 1] the activation
      is a contraction.  Evaluate mode: mean' = running_mean exactly, B_invstd = u is.
  backward, g = gy masked from y_act (LeakyReLU: one rounding, L = 1, else L = 0), G1 = sum |g|:
      sum' :      B_sum = (Kb - 1 + L) u G1
      dotp' = sum fl(g fl(x - mean')):              B_dot = B_mean |sum| + (Kb + 2 + L) u sum |g| (|x - mean| + B_mean)
      gbeta = fl(pbeta gbeta0) + sum_groups fl(sum'), 1 + 2 G roundings of values no larger than
      M = |pbeta gbeta0| + sum_groups (|sum| + B_sum):                  B_gbeta = sum_groups B_sum + (1 + 2 G) u M
      ggamma likewise with fl(dotp' is'), M = |pbeta ggamma0| + sum_groups (|dotp| + B_dot) is_up:
                                                    B_ggamma = sum_groups (B_dot is_up + |dotp| B_invstd) + (1 + 2 G) u M
      gm = fl(sum' / n):                            B_gm = B_sum / n + u (|sum| + B_sum) / n
      kk = fl(dotp' is'^2 / n), k_up = (|dotp| + B_dot) is_up^2 / n:
                                                    B_k = (B_dot is_up^2 + |dotp| B_invstd (is + is_up)) / n + u k_up
      p = g - gm - (x - mean) k in four fp32 operations:
          B_p = L u |g| + B_gm + B_mean k_up + |x - mean| B_k + u (2 |g| + 2 (|gm| + B_gm) + 3 a k_up)
      gx = fl(fl(p' is') gamma):                    B_gx = |gamma| (B_p is_up + |p| B_invstd) + 2 u |gamma| (|p| + B_p) is_up
"""
import numpy as np

F32 = np.float32
U = 2.0 ** -24
SLACK = 1.01


# ------------------------------------------------------------------------------------------------ geometry (vf_bn.hip, restated)
def cdiv(a, b):
    return -(-a // b)


def bn_geom(npix, C, target_blocks=2048):
    """BnGeom bn_geom(npix, C, target_blocks) -> dict(cq, rp, gy, gx, rows_per_block)"""
    C4 = C // 4
    cq = 1
    while cq < C4 and cq < 64:
        cq <<= 1
    rp = 256 // cq
    gy = cdiv(C4, cq)
    gx_target = max(1, target_blocks // gy)
    rpb = max(rp, cdiv(npix, gx_target))
    rpb = cdiv(rpb, rp) * rp
    return dict(cq=cq, rp=rp, gy=gy, gx=cdiv(npix, rpb), rows_per_block=rpb)


def bn_stat_blocks(npix, C, bytes_per_block):
    return min(512, max(128, npix * C * 4 // bytes_per_block))


def stats_geom(npix, C, backward=False):
    """the geometry of k_bn_stats (32 KB per block) / k_bn_bwd_stats (16 KB per block)"""
    return bn_geom(npix, C, bn_stat_blocks(npix, C, 16384 if backward else 32768))


def rows_per_thread(g):
    return g["rows_per_block"] // g["rp"]


# ------------------------------------------------------------------------------------------------ shared pieces
def _act64(v, act, slope):
    if act == "lrelu":
        return np.where(v > 0, v, v * slope)
    if act == "relu":
        return np.where(v > 0, v, 0.0)
    return v


def _mask(g, y_act, act, slope):
    """vf_act_grad from the ACTIVATED value, in g's own precision"""
    if act == "lrelu":
        return np.where(y_act > 0, g, g * g.dtype.type(slope))
    if act == "relu":
        return np.where(y_act > 0, g, g.dtype.type(0))
    return g


def _vec(v, C, fill, dtype):
    return np.full(C, fill, dtype) if v is None else np.asarray(v, dtype)


# ------------------------------------------------------------------------------------------------ ref64
def ref64(x, groups, rm, rv, gamma=None, beta=None, momentum=0.1, eps=1e-5, act="none", slope=0.2, gy=None, y_act=None,
          gg0=None, gb0=None, pbeta=1.0, evaluate=False):
    """x [groups * npix][C] fp32; rm, rv the running statistics BEFORE the call; gamma / beta None = absent.  momentum, eps,
    slope and pbeta are the fp32 numbers the C-ABI receives.  gy given: the backward pass as well, the activation derivative
    taken from y_act (default: this function's own y) and the parameter gradients accumulated onto pbeta * (gg0, gb0).
    evaluate=True: the evaluate-mode forward from (rm, rv) alone.  Returns a dict of float64 arrays; the keys without an
    underscore are the module's outputs, the others the per-channel quantities `bounds` is written in."""
    x = np.asarray(x, np.float64)
    N, C = x.shape
    n = N // groups
    assert n * groups == N
    ga, be = _vec(gamma, C, 1.0, np.float64), _vec(beta, C, 0.0, np.float64)
    mom, eps, slope, pbeta = float(F32(momentum)), float(F32(eps)), float(F32(slope)), float(F32(pbeta))
    rm, rv = np.asarray(rm, np.float64).copy(), np.asarray(rv, np.float64).copy()
    if evaluate:
        istd = 1.0 / np.sqrt(rv + eps)
        return dict(y=_act64(((x - rm) * istd) * ga + be, act, slope), _invstd=istd)
    xg = x.reshape(groups, n, C)
    mean = xg.sum(1) / n
    dev = xg - mean[:, None]
    m2 = (dev * dev).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        istd = 1.0 / np.sqrt(m2 / n + eps)
        for g in range(groups):
            rm = mom * mean[g] + (1 - mom) * rm
            rv = mom * (m2[g] / (n - 1.0)) + (1 - mom) * rv
    y = _act64((dev * istd[:, None]) * ga + be, act, slope).reshape(N, C)
    out = dict(save_mean=mean, save_invstd=istd, running_mean=rm, running_var=rv, y=y, _m2=m2, _dev=dev)
    if gy is not None:
        ya = y if y_act is None else np.asarray(y_act, np.float64)
        g = _mask(np.asarray(gy, np.float64), ya, act, slope).reshape(groups, n, C)
        s, dotp = g.sum(1), (g * dev).sum(1)
        k = dotp * istd * istd / n
        p = g - (s / n)[:, None] - dev * k[:, None]
        out.update(gx=(p * istd[:, None] * ga).reshape(N, C), _g=g, _sum=s, _dotp=dotp, _p=p,
                   ggamma=pbeta * _vec(gg0, C, 0.0, np.float64) + (dotp * istd).sum(0),
                   gbeta=pbeta * _vec(gb0, C, 0.0, np.float64) + s.sum(0))
    return out


# ------------------------------------------------------------------------------------------------ emulate32
def _partials(terms, npix, C, geo):
    """every block's partial row: per term, each thread's fp32 running sum over its rows r0 + ty, r0 + ty + rp, ... and the rp
    row lanes of a column added in double, lane 0 first -> [gx][len(terms)][C] float64"""
    gx, rp, rpb = geo["gx"], geo["rp"], geo["rows_per_block"]
    K = rpb // rp
    out = np.zeros((gx, len(terms), C))
    for i, t in enumerate(terms):
        assert t.dtype == F32
        pad = np.zeros((gx * rpb, C), F32)          # a row past npix adds +0 to a sum: the value the kernel keeps
        pad[:npix] = t
        pad = pad.reshape(gx, K, rp, C)
        s = np.zeros((gx, rp, C), F32)
        for k in range(K):
            s = s + pad[:, k]
        a = np.zeros((gx, C))
        for j in range(rp):
            a = a + s[:, j].astype(np.float64)
        out[:, i] = a
    return out


def _column_total(part):
    """k_reduce_partials' column_total: part [nslab][ncol] float64 -> [ncol], in the kernel's order"""
    nslab, ncol = part.shape
    red = np.zeros((16, ncol))
    for ry in range(16):
        s = [np.zeros(ncol) for _ in range(4)]
        for base in range(0, nslab, 512):
            for g in range(8):
                k0 = base + ry + 64 * g
                if k0 + 48 < nslab:
                    for j in range(4):
                        s[j] = s[j] + part[k0 + 16 * j]
                else:
                    for j in range(4):
                        if k0 + 16 * j < nslab:
                            s[0] = s[0] + part[k0 + 16 * j]
        red[ry] = (s[0] + s[1]) + (s[2] + s[3])
    t = np.zeros(ncol)
    for j in range(16):
        t = t + red[j]
    return t


def _act32(v, act, slope):
    if act == "lrelu":
        return np.where(v > 0, v, v * F32(slope))
    if act == "relu":
        return np.where(v > 0, v, F32(0))
    return v


def _apply32(x, mu, istd, ga, be, act, slope):
    v = ((x - mu) * istd) * ga + be                 # all float32: four roundings
    assert v.dtype == F32
    return _act32(v, act, slope)


def emulate32(x, groups, rm, rv, gamma=None, beta=None, momentum=0.1, eps=1e-5, act="none", slope=0.2, gy=None, y_act=None,
              gg0=None, gb0=None, pbeta=1.0, evaluate=False, skip_last_row=False):
    """the same arguments and keys as ref64 (outputs fp32, `sums` float64 [groups][2C] as the device buffer holds them after
    the last launch).  skip_last_row=True leaves the last row of every block's row range out of the forward statistics: the
    off-by-one the CPU suite must see `bounds` reject."""
    x = np.asarray(x, F32)
    N, C = x.shape
    n = N // groups
    ga, be = _vec(gamma, C, 1.0, F32), _vec(beta, C, 0.0, F32)
    mom, epsd = float(F32(momentum)), float(F32(eps))
    rm, rv = np.asarray(rm, F32).copy(), np.asarray(rv, F32).copy()
    if evaluate:
        istd = (1.0 / np.sqrt(rv.astype(np.float64) + epsd)).astype(F32)
        return dict(y=_apply32(x, rm, istd, ga, be, act, slope))
    geo = stats_geom(n, C)
    shift = rm.copy()
    mean32, istd32 = np.zeros((groups, C), F32), np.zeros((groups, C), F32)
    sums, m2_raw = np.zeros((groups, 2 * C)), np.zeros((groups, C))
    with np.errstate(divide="ignore", invalid="ignore"):
        for g in range(groups):
            v = x[g * n:(g + 1) * n] - shift
            if skip_last_row:
                v = v.copy()
                v[np.minimum(np.arange(1, geo["gx"] + 1) * geo["rows_per_block"], n) - 1] = 0
            part = _partials([v, v * v], n, C, geo)
            q = _column_total(part.reshape(geo["gx"], 2 * C))
            sums[g] = q
            q1, q2 = q[:C], q[C:]
            nd = float(n)
            mean = shift.astype(np.float64) + q1 / nd
            m2 = q2 - q1 * q1 / nd if n > 1 else np.zeros(C)
            m2_raw[g] = m2
            m2 = np.where(m2 < 0, 0.0, m2)
            istd32[g] = (1.0 / np.sqrt(m2 / nd + epsd)).astype(F32)
            mean32[g] = mean.astype(F32)
            rm = (mom * mean + (1.0 - mom) * rm.astype(np.float64)).astype(F32)
            rv = (mom * (m2 / (nd - 1.0)) + (1.0 - mom) * rv.astype(np.float64)).astype(F32)
    y = np.concatenate([_apply32(x[g * n:(g + 1) * n], mean32[g], istd32[g], ga, be, act, slope) for g in range(groups)])
    out = dict(save_mean=mean32, save_invstd=istd32, running_mean=rm, running_var=rv, y=y, sums=sums, _m2_raw=m2_raw)
    if gy is None:
        return out
    gy = np.asarray(gy, F32)
    ya = y if y_act is None else np.asarray(y_act, F32)
    geo = stats_geom(n, C, backward=True)
    gx = np.zeros((N, C), F32)
    pb = F32(pbeta)
    gg = pb * _vec(gg0, C, 0.0, F32) if pb != 0 else np.zeros(C, F32)
    gb = pb * _vec(gb0, C, 0.0, F32) if pb != 0 else np.zeros(C, F32)
    sums = np.zeros((groups, 2 * C))
    for g in range(groups):
        sl = slice(g * n, (g + 1) * n)
        gm_ = _mask(gy[sl], ya[sl], act, slope)
        xm = x[sl] - mean32[g]
        part = _partials([gm_, gm_ * xm], n, C, geo)
        sums[g] = _column_total(part.reshape(geo["gx"], 2 * C))
    for g in range(groups):                          # k_bn_bwd_apply: the parameter gradients in group order ...
        s, dp = sums[g, :C], sums[g, C:]
        gg = gg + (dp * istd32[g].astype(np.float64)).astype(F32)
        gb = gb + s.astype(F32)
    for g in range(groups):                          # ... and the input gradient
        sl = slice(g * n, (g + 1) * n)
        s, dp = sums[g, :C], sums[g, C:]
        isd = istd32[g].astype(np.float64)
        kk = (dp * isd * isd / float(n)).astype(F32)
        gmean = (s / float(n)).astype(F32)
        gm_ = _mask(gy[sl], ya[sl], act, slope)
        o = (gm_ - gmean - (x[sl] - mean32[g]) * kk) * istd32[g] * ga
        assert o.dtype == F32
        gx[sl] = o
    assert gg.dtype == F32 and gb.dtype == F32
    out.update(gx=gx, ggamma=gg, gbeta=gb, sums=sums)
    return out


# ------------------------------------------------------------------------------------------------ bounds
def kappa(x, groups, rm):
    """(mean - s)^2 / var per group and channel (inf for a constant channel away from s, 0 for one at s)"""
    r = ref64(x, groups, rm, np.ones_like(rm))
    n = x.shape[0] // groups
    d2 = (r["save_mean"] - np.asarray(rm, np.float64)) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d2 == 0, 0.0, d2 / (r["_m2"] / n))


def bounds(x, groups, rm, rv, gamma=None, beta=None, momentum=0.1, eps=1e-5, act="none", slope=0.2, gy=None, y_act=None,
           gg0=None, gb0=None, pbeta=1.0, evaluate=False):
    """the bound of every output of ref64 (same arguments, same keys), see the module docstring"""
    r = ref64(x, groups, rm, rv, gamma, beta, momentum, eps, act, slope, gy, y_act, gg0, gb0, pbeta, evaluate)
    x = np.asarray(x, np.float64)
    N, C = x.shape
    n = N // groups
    u = U * SLACK
    ga, be = np.abs(_vec(gamma, C, 1.0, np.float64)), np.abs(_vec(beta, C, 0.0, np.float64))
    mom, epsd, pb = float(F32(momentum)), float(F32(eps)), float(F32(pbeta))
    L = 1 if act == "lrelu" else 0
    s0 = np.asarray(rm, np.float64)

    def y_bound(adev, istd, is_up, b_mean, b_is, yref):
        a = adev + b_mean
        b = ga * (is_up * b_mean + adev * b_is) + u * (4 * ga * a * is_up + be)
        return b + u * (np.abs(yref) + b) if L else b

    if evaluate:
        istd = r["_invstd"]
        return dict(y=y_bound(np.abs(x - s0), istd, istd * (1 + u), 0.0, u * istd, r["y"]))
    K = rows_per_thread(stats_geom(n, C))
    Kb = rows_per_thread(stats_geom(n, C, backward=True))
    assert max(K, Kb) * U < 2.0 ** -8
    mean, istd, m2, dev = r["save_mean"], r["save_invstd"], r["_m2"], r["_dev"]
    xs = (x - s0).reshape(groups, n, C)
    A1, A2 = np.abs(xs).sum(1), (xs * xs).sum(1)
    b_mean = u * (np.abs(mean) + K * A1 / n)
    D = (u * ((K + 2) * A2 + 2 * np.abs(mean - s0) * K * A1) / n) if n > 1 else np.zeros((groups, C))
    w = m2 / n + epsd
    hi = 1.0 / np.sqrt(np.maximum(w - D, epsd))
    b_is = np.maximum(hi - istd, istd - 1.0 / np.sqrt(w + D)) + u * hi
    is_up = istd + b_is
    b_rm, b_rv = np.zeros(C), np.zeros(C)
    rmr, rvr = s0.copy(), np.asarray(rv, np.float64).copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        for g in range(groups):
            rmr = mom * mean[g] + (1 - mom) * rmr
            rvr = mom * (m2[g] / (n - 1.0)) + (1 - mom) * rvr
            b_rm = mom * b_mean[g] + (1 - mom) * b_rm + u * (np.abs(rmr) + b_rm)
            b_rv = mom * D[g] * n / (n - 1.0) + (1 - mom) * b_rv + u * (np.abs(rvr) + b_rv)
    adev = np.abs(dev)
    out = dict(save_mean=b_mean, save_invstd=b_is, running_mean=b_rm, running_var=b_rv,
               y=y_bound(adev, istd[:, None], is_up[:, None], b_mean[:, None], b_is[:, None],
                         r["y"].reshape(groups, n, C)).reshape(N, C))
    if gy is None:
        return out
    g, s, dotp, p = np.abs(r["_g"]), np.abs(r["_sum"]), np.abs(r["_dotp"]), np.abs(r["_p"])
    b_sum = (Kb - 1 + L) * u * g.sum(1)
    a = adev + b_mean[:, None]
    b_dot = b_mean * s + (Kb + 2 + L) * u * (g * a).sum(1)
    nr = 1 + 2 * groups
    Mb = np.abs(pb * _vec(gb0, C, 0.0, np.float64)) + (s + b_sum).sum(0)
    Mg = np.abs(pb * _vec(gg0, C, 0.0, np.float64)) + ((dotp + b_dot) * is_up).sum(0)
    b_gm = b_sum / n + u * (s + b_sum) / n
    k_up = (dotp + b_dot) * is_up * is_up / n
    b_k = (b_dot * is_up * is_up + dotp * b_is * (istd + is_up)) / n + u * k_up
    gmean = s / n
    b_p = (L * u * g + b_gm[:, None] + (b_mean * k_up)[:, None] + adev * b_k[:, None]
           + u * (2 * g + 2 * (gmean + b_gm)[:, None] + 3 * a * k_up[:, None]))
    b_gx = ga * (b_p * is_up[:, None] + p * b_is[:, None]) + 2 * u * ga * (p + b_p) * is_up[:, None]
    out.update(gx=b_gx.reshape(N, C), gbeta=b_sum.sum(0) + nr * u * Mb,
               ggamma=(b_dot * is_up + dotp * b_is).sum(0) + nr * u * Mg)
    return out


def outside(got, ref, bound):
    """indices (flat) at which `got` leaves `bound` around `ref`.  Where the reference is not finite (running_var of a single
    row: 0 / 0) the value must be the same non-finite one."""
    got, ref, bound = [np.asarray(v, np.float64) for v in (got, ref, bound)]
    fin = np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        ok = np.where(fin, np.abs(got - ref) <= bound, (np.isnan(ref) & np.isnan(got)) | (got == ref))
    return np.flatnonzero(~ok.ravel())


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the finite reference values with a positive bound (0 / 0 counts as 0)"""
    got, ref, bound = [np.asarray(v, np.float64).ravel() for v in (got, ref, bound)]
    fin = np.isfinite(ref) & np.isfinite(bound)
    err = np.abs(got[fin] - ref[fin])
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound[fin])
    return float(q.max()) if q.size else 0.0
