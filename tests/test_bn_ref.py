"""CPU companion of tests/test_gpu_bn.py: the bounds that file holds the BatchNorm kernels to are proven here without a GPU.

  * bn_ref.ref64 agrees with the oracle's SpatialBatchNormalization (THNN's loops in double) on test_batchnorm's cases;
  * bn_ref.emulate32, the kernels' arithmetic restated in numpy with the launches' own geometry, lies inside bn_ref.bounds on
    every case of the GPU module, train forward, backward and evaluate forward;
  * each bound can fail: a save_invstd off by 1e-4 relative, a ggamma formed with the neighbouring group's invstd and
    statistics that leave out the last row of each block's row range are all rejected;
  * the geometry figures quoted beside the GPU cases (cq, rp, gy, rows per block and per thread) are what the restated
    bn_geom / bn_stat_blocks give.

Largest |emulation - ref64| / bound over all cases of the GPU module, per output (measured here with numpy's float32
arithmetic; test_emulation_inside_bounds prints the figures per case):

    save_mean 0.94   save_invstd 0.70   running_mean 0.89   running_var 0.80   y 0.93   y (evaluate) 0.86
    gx 0.74          ggamma 0.93        gbeta 0.52

The bounds are worst-case sums of |rounding errors|.  The largest shares come from the one-row cases (c4000-n1, c260-n1), where
a bound is two or three roundings and the error one or two of them; the case with 16 rows per thread shows the other end
(save_mean 0.04, save_invstd 0.08, y 0.14, gx 0.20): there the errors add like a random walk while the bound adds their
magnitudes.  On the conditioning tensor the share of save_invstd is 0.69 with the shift at the mean (the constant channel: the
one rounding of 1 / sqrt(eps)) and 0.48 with the shift at 0."""
import numpy as np
import pytest

import bn_ref as R
import test_gpu_bn as G

ALL = G.CASES + G.COND_CASES
_cache = {}


def evaluated(c):
    """(inputs, emulation, ref64, bounds) of a case, computed once and shared read-only"""
    if c["name"] not in _cache:
        t = G.make_inputs(c)
        e = R.emulate32(t["x"], **G.ref_args(c, t))
        kw = G.ref_args(c, t, y_act=e["y"])
        for v in t.values():
            if v is not None:
                v.setflags(write=False)
        _cache[c["name"]] = (t, e, R.ref64(t["x"], **kw), R.bounds(t["x"], **kw))
    return _cache[c["name"]]


@pytest.mark.parametrize("shape", [(4, 64, 8, 8), (2, 128, 16, 16), (8, 100, 1, 1), (3, 260, 4, 4), (16, 4000, 1, 1)])
@pytest.mark.parametrize("act", ["none", "lrelu", "relu"])
def test_ref64_agrees_with_the_oracle(shape, act, oracle):
    """test_batchnorm's inputs (tests/test_gpu_ops.py).  The oracle stores fp32 and keeps invstd as a float: each output within
    a few fp32 roundings of ref64, relative to the value itself (y, gx: to the row's largest term)."""
    B, C, H, W = shape
    rng = np.random.default_rng(C * 7 + H)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    ref = oracle.SpatialBatchNormalization(C)
    ref.weight[...] = 1 + 0.1 * f(C)
    ref.bias[...] = 0.1 * f(C)
    ref.running_mean[...] = 0.3 * f(C)
    ref.running_var[...] = 1 + 0.2 * np.abs(f(C))
    rm0, rv0 = ref.running_mean.copy(), ref.running_var.copy()
    x = (f(*shape) * 1.7 + 0.8).astype(np.float32)
    y = ref.forward(x).copy()
    ya = np.where(y > 0, y, np.float32(0.2) * y) if act == "lrelu" else np.maximum(y, 0) if act == "relu" else y
    gy = f(*shape)
    g_eff = np.where(ya > 0, gy, np.float32(0.2) * gy) if act == "lrelu" else np.where(ya > 0, gy, 0).astype(np.float32) if act == "relu" else gy
    ref.gradWeight[...] = f(C)
    ref.gradBias[...] = f(C)
    gw0, gb0 = ref.gradWeight.copy(), ref.gradBias.copy()
    ref.backward(x, g_eff)
    rows = lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1)).reshape(-1, C)
    r = R.ref64(rows(x), 1, rm0, rv0, ref.weight, ref.bias, 0.1, 1e-5, act, 0.2, gy=rows(gy), y_act=rows(ya), gg0=gw0, gb0=gb0)
    u = R.U

    def close(got, want, scale, k, what):
        err = np.abs(np.asarray(got, np.float64) - want)
        assert (err <= k * u * scale).all(), "%s: %.2f of %d u" % (what, float((err / (u * scale + 1e-300)).max()), k)

    close(ref.save_mean, r["save_mean"][0], np.abs(r["save_mean"][0]), 1, "save_mean")
    close(ref.save_std, r["save_invstd"][0], r["save_invstd"][0], 1, "save_invstd")
    # the oracle forms (1 - momentum) and its product with the old running value in fp32: two more roundings of that term
    close(ref.running_mean, r["running_mean"], np.abs(r["running_mean"]) + 2 * np.abs(rm0), 1, "running_mean")
    close(ref.running_var, r["running_var"], r["running_var"] + 2 * rv0, 1, "running_var")
    dev = np.abs(r["_dev"][0]) * r["save_invstd"][0] * np.abs(ref.weight)
    close(rows(ya), r["y"], 4 * dev + np.abs(r["y"]) + np.abs(ref.bias), 1, "y")
    # the oracle's backward starts from its fp32 save_mean / save_invstd: their roundings reach every term
    g, p = np.abs(r["_g"][0]), np.abs(r["_p"][0])
    kterm = np.abs(r["_dev"][0] * r["_dotp"][0]) * r["save_invstd"][0] ** 2 / (B * H * W)
    mterm = np.abs(r["save_mean"][0] * r["_dotp"][0]) * r["save_invstd"][0] ** 2 / (B * H * W)
    close(rows(ref.gradInput), r["gx"], (p + g + kterm + mterm + np.abs(r["_sum"][0]) / (B * H * W)) * r["save_invstd"][0] * np.abs(ref.weight), 8, "gx")
    gabs = (g * (np.abs(r["_dev"][0]) + np.abs(r["save_mean"][0]))).sum(0) * r["save_invstd"][0]
    close(ref.gradWeight, r["ggamma"], np.abs(gw0) + gabs, 4, "ggamma")
    close(ref.gradBias, r["gbeta"], np.abs(gb0) + np.abs(r["_sum"][0]) + np.abs(r["gbeta"]) + g.sum(0), 1, "gbeta")   # g.sum: the fp32 gy * slope
    ref.train = False
    ye = rows(ref.forward(x))
    ye = np.where(ye > 0, ye, np.float32(0.2) * ye) if act == "lrelu" else np.maximum(ye, 0) if act == "relu" else ye
    re = R.ref64(rows(x), 1, ref.running_mean, ref.running_var, ref.weight, ref.bias, 0.1, 1e-5, act, 0.2, evaluate=True)
    close(ye, re["y"], 4 * np.abs(rows(x) - ref.running_mean) * re["_invstd"] * np.abs(ref.weight) + np.abs(re["y"]) + np.abs(ref.bias), 1, "eval y")


WORST = {}


@pytest.mark.parametrize("c", ALL, ids=G.ids(ALL))
def test_emulation_inside_bounds(c):
    t, e, r, b = evaluated(c)
    ratios = G.check(c, e, r, b, G.TRAIN_KEYS, "emulated train")
    kw = G.ref_args(c, t, backward=False)
    ee = R.emulate32(t["x"], evaluate=True, **kw)
    ratios["y_eval"] = G.check(c, ee, R.ref64(t["x"], evaluate=True, **kw), R.bounds(t["x"], evaluate=True, **kw), ["y"], "emulated evaluate")["y"]
    for k, v in ratios.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print("%s worst |err| / bound: %s" % (c["name"], ", ".join("%s %.3f" % kv for kv in ratios.items())))
    print("so far: %s" % ", ".join("%s %.2f" % kv for kv in WORST.items()))
    assert all(v <= 1.0 for v in ratios.values())
    n = c["B"] * c["H"] * c["W"] // c["groups"]
    if n == 1:
        assert np.isnan(r["running_var"]).all() and np.isnan(e["running_var"]).all()


def test_one_invstd_off_by_1e_4_is_rejected():
    hits = 0
    for c in G.CASES:
        t, e, r, b = evaluated(c)
        if c["B"] * c["H"] * c["W"] // c["groups"] < 2:
            continue
        bad = r["save_invstd"].copy()
        bad[-1, c["C"] // 2] *= 1 + 1e-4
        out = R.outside(bad, r["save_invstd"], b["save_invstd"])
        assert out.size <= 1
        hits += out.size
    assert hits >= 20, "a save_invstd 1e-4 off passes on nearly every case: the bound is not a bound (%d rejections)" % hits


def test_ggamma_with_the_neighbouring_groups_invstd_is_rejected():
    seen = 0
    for c in G.CASES:
        if c["groups"] < 2 or c["B"] * c["H"] * c["W"] // c["groups"] < 2:
            continue
        t, e, r, b = evaluated(c)
        istd = np.roll(r["save_invstd"], 1, axis=0)                      # every group takes its neighbour's
        pb = float(np.float32(c["pbeta"]))
        bad = pb * t["gg0"].astype(np.float64) + (r["_dotp"] * istd).sum(0)
        out = R.outside(bad, r["ggamma"], b["ggamma"])
        assert out.size >= 0.9 * c["C"], "%s: ggamma with the wrong group's invstd passes on %d of %d channels" % (c["name"], c["C"] - out.size, c["C"])
        seen += 1
    assert seen >= 4


def test_statistics_without_a_blocks_last_row_are_rejected():
    """emulate32(skip_last_row=True) leaves row r1 - 1 of every statistics block out of the sums (n unchanged): save_mean or
    save_invstd must leave the bound on every case with more than one row, on most channels"""
    seen = 0
    for c in G.CASES:
        n = c["B"] * c["H"] * c["W"] // c["groups"]
        if n < 2 or n > 1000:
            continue
        t, e, r, b = evaluated(c)
        s = R.emulate32(t["x"], skip_last_row=True, **G.ref_args(c, t, backward=False))
        out = np.union1d(R.outside(s["save_mean"], r["save_mean"], b["save_mean"]),
                         R.outside(s["save_invstd"], r["save_invstd"], b["save_invstd"]))
        assert out.size >= 0.9 * c["groups"] * c["C"], "%s: a dropped row passes on %d of %d channels" % (
            c["name"], c["groups"] * c["C"] - out.size, c["groups"] * c["C"])
        seen += 1
    assert seen >= 20


def test_geometry_of_the_cases():
    """the figures quoted in tests/test_gpu_bn.py's case comments"""
    want = {4: (1, 256, 1), 8: (2, 128, 1), 100: (32, 8, 1), 252: (64, 4, 1), 260: (64, 4, 2), 512: (64, 4, 2), 4000: (64, 4, 16)}
    for C, (cq, rp, gy) in want.items():
        g = R.bn_geom(1, C)
        assert (g["cq"], g["rp"], g["gy"]) == (cq, rp, gy), (C, g)
    per_c = {}
    for c in ALL:
        n = c["B"] * c["H"] * c["W"] // c["groups"]
        assert n * c["groups"] == c["B"] * c["H"] * c["W"] and n * c["C"] * 4 <= 8 << 20
        fw, bw, ap = R.stats_geom(n, c["C"]), R.stats_geom(n, c["C"], True), R.bn_geom(n, c["C"])
        tag = [k for k in ("rpb12", "rpb8") if k in c["name"]]
        if tag:
            rpb = int(tag[0][3:])
            assert fw["rows_per_block"] == rpb and bw["rows_per_block"] == rpb and n % rpb in (1, rpb - 1), (c["name"], fw)
        elif c["data"] == "easy" and "k16" not in c["name"]:
            assert fw["rows_per_block"] == fw["rp"] == bw["rows_per_block"], (c["name"], fw)
        if "k16" not in c["name"] and c["data"] == "easy":
            assert ap["rows_per_block"] == ap["rp"]
        per_c.setdefault(c["C"], set()).add(n)
    rp8, rp260 = 128, 4
    assert {1, 2, rp8 - 1, rp8, rp8 + 1, 2 * rp8 + 1} <= per_c[8]
    assert {1, 2, rp260 - 1, rp260, rp260 + 1, 2 * rp260 + 1, 517, 527} <= per_c[260]
    assert set(per_c) >= {4, 8, 100, 252, 260, 512, 4000}
    g = R.stats_geom(12289, 20)
    assert (g["cq"], g["rp"], g["rows_per_block"], g["gx"]) == (8, 32, 128, 97) and 12289 == 96 * 128 + 1
    k16 = [c for c in G.CASES if "k16" in c["name"]][0]
    n = k16["B"] * k16["H"] * k16["W"]
    assert R.rows_per_thread(R.stats_geom(n, 260)) == 16 and R.rows_per_thread(R.stats_geom(n, 260, True)) == 8


def test_most_rows_per_thread():
    """rows a thread sums in fp32, K = rows_per_block / rp, over every channel count up to 8192 at the largest npix that keeps
    the tensor within 8 MB (and a few below): 16, reached at C = 260.  With full chunks it is 8; beyond 16 MB it grows with the
    tensor (the kernel header used to say "<= 64 rows": true up to 128 MB only)."""
    best = (0, None)
    for C in range(4, 8193, 4):
        top = (8 << 20) // (4 * C)
        for n in {top, top - 1, top * 15 // 16, top * 3 // 4, top // 2 + 1}:
            for bw in (False, True):
                best = max(best, (R.rows_per_thread(R.stats_geom(n, C, bw)), (C, n, bw)))
    assert best[0] == 16 and best[1][0] in (260, 272), best        # C/4 = 65 .. 68: a second chunk nearly empty
    assert R.rows_per_thread(R.stats_geom((16 << 20) // (4 * 64), 64)) == 8
    assert R.rows_per_thread(R.stats_geom((16 << 20) // (4 * 64), 64, True)) == 8
    assert R.rows_per_thread(R.stats_geom((128 << 20) // (4 * 64), 64)) == 64
    assert R.rows_per_thread(R.stats_geom((256 << 20) // (4 * 64), 64)) == 128


def test_conditioning_tensor_is_what_it_says():
    for c in G.COND_CASES:
        t, e, r, b = evaluated(c)
        k = R.kappa(t["x"], 1, t["rm"])[0]
        sd = np.sqrt(r["_m2"][0] / t["x"].shape[0])
        for i, ratio in enumerate(G.COND_RATIOS):
            for j, std in enumerate(G.COND_STDS):
                ch = 3 * i + j
                assert abs(sd[ch] / std - 1) < 0.05
                if c["shift"] == "zero":
                    assert abs(np.sqrt(k[ch]) - ratio) <= 0.05 * ratio + 0.05, (ch, k[ch], ratio)
                else:
                    assert k[ch] < 1e-6
        assert r["_m2"][0, G.COND_CONST] == 0 and e["save_invstd"][0, G.COND_CONST] == np.float32(1 / np.sqrt(np.float64(np.float32(G.EPS))))
        if c["shift"] == "zero":
            # the clamp: the fp32 sums leave m2 < 0 on the alternating channel, and the bound there reaches 1 / sqrt(eps)
            assert e["_m2_raw"][0, G.COND_ALT] < 0 and e["save_invstd"][0, G.COND_ALT] == e["save_invstd"][0, G.COND_CONST]
            assert k[G.COND_ALT] > 1e12
            # the bound grows with kappa and is tight below 1: under 2e-6 relative there, past 1e-5 from kappa = 1e4 on
            rel = b["save_invstd"][0] / r["save_invstd"][0]
            assert (rel[:6] < 2e-6).all() and (rel[9:18] > 1e-5).all() and (np.diff(rel[1:18:3]) > 0).all(), rel
