"""CPU companion of tests/test_gpu_elementwise.py: the bounds that file holds the HIP kernels to are claims about fp32 arithmetic,
so they are checked here without a GPU.  For every random-input family the op is evaluated in fp32 numpy in the kernel's
statement order, once with separate multiplies and adds and once with the multiply-add fused (formed in float64, rounded once),
on the GPU test's own inputs, and both must stay inside the GPU test's bound.  The "exact" inputs must be exact: the fp32
evaluation equals the float64 one bit for bit and the integer sums stay below 2^24 per fp32 partial sum.  A failure on the GPU is
then the kernel's, not the bound's.  Large sizes are not needed for this: the generators are per-element."""
import numpy as np
import pytest

import test_gpu_elementwise as E

F32, U, FLT_MIN = E.F32, E.U, E.FLT_MIN
SIZES = [1, 5, 1027, 65539, E.SWEEP + 7]


def r(v):
    """round a float64 array to fp32 (kept as float64)"""
    return np.asarray(v, np.float64).astype(F32).astype(np.float64)


def inside(got, ref, bound, what):
    err = np.abs(got - ref)
    bad = np.flatnonzero(~(err <= bound + FLT_MIN))
    assert bad.size == 0, "%s: fp32 arithmetic leaves the bound at %d: |err| %.3e > %.3e" % (what, bad[0], err[bad[0]], bound[bad[0]])


def pw_eval32(op, ins, out0, f, n, fused):
    a = [v.astype(np.float64) for v in ins]
    o = None if out0 is None else out0.astype(np.float64)
    if op == "axpby":
        return r(f[0] * a[0] + r(f[1] * o)) if fused else r(r(f[0] * a[0]) + r(f[1] * o))
    if op == "scale_shift":
        return r(o * f[0] + f[1]) if fused else r(r(o * f[0]) + f[1])
    if op == "mse_bwd":
        return r(r(2.0 / r(n)) * r(a[0] - a[1]))
    if op == "act_bwd_tanh":
        return r(a[1] * (r(1.0 - a[0] * a[0]) if fused else r(1.0 - r(a[0] * a[0]))))
    if op == "act_bwd_sigmoid":
        return r(r(a[1] * r(1.0 - a[0])) * a[0])
    return r(E.pw_ref64(op, ins, out0, f, n, E.SLOPE))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op", [o for o in E.PW if o not in ("act_fwd_tanh", "act_fwd_sigmoid")])
def test_pointwise_bounds_hold_in_fp32(op, n):
    ins, out0, f = E.pw_inputs(op, n, 1000 + n % 997, False)
    ref = E.pw_ref64(op, ins, out0, f, n, E.SLOPE)
    bound = E.pw_bound(op, ins, out0, f, n)
    for fused in (False, True):
        got = pw_eval32(op, ins, out0, f, n, fused)
        if bound is None:
            assert (got.astype(F32).view(np.int32) == ref.astype(F32).view(np.int32)).all(), op
        else:
            inside(got, ref, bound, "%s n=%d fused=%s" % (op, n, fused))


@pytest.mark.parametrize("n", SIZES + [1024, 65536])
@pytest.mark.parametrize("op", [o for o in E.PW if o not in ("act_fwd_tanh", "act_fwd_sigmoid")])
def test_pointwise_exact_inputs_are_exact(op, n):
    ins, out0, f = E.pw_inputs(op, n, 1000 + n % 997, True)
    slope = E.pw_slope(True)
    ref = E.pw_ref64(op, ins, out0, f, n, slope)
    if not E.pw_exact_is_bitwise(op, n):
        return
    assert (r(ref) == ref).all(), "%s: the exact result is not an fp32 number" % op
    if op in ("axpby", "scale_shift", "mse_bwd", "act_bwd_tanh", "act_bwd_sigmoid"):
        for fused in (False, True):
            assert (pw_eval32(op, ins, out0, f, n, fused) == ref).all(), (op, fused)


def recon_eval32(g, x, t, wsel, sc, masked, fused):
    alpha, c0, c1 = sc
    n = x.size
    g, x, t, m = [v.astype(np.float64) for v in (g, x, t, wsel)]
    ton = r(2.0 / r(n))
    d = r(x - t)
    if masked:
        w = r(c0 + c1 * m) if fused else r(c0 + r(c1 * m))
    else:
        w = np.where(m != 0, r(c0 + c1), c0)
    term = r(r(ton * d) * w)
    return r(alpha * g + term) if fused else r(r(alpha * g) + term)


@pytest.mark.parametrize("shape", [(3, 3, 48), (2, 3, 10), (1, 3, 9), (1, 1, 2), (5, 12, 32)])
@pytest.mark.parametrize("form,band", [("mask", 0), ("band", 1), ("band", 4), ("none", 0)])
def test_recon_bounds_hold_in_fp32(shape, form, band):
    B, C, H = shape
    if band > H // 2:
        band = H // 2
    g, x, t, sc = E.recon_inputs(B, C, H, 77 + H, False)
    _, wsel = E.recon_weights(B, C, H, form, band, 77 + H)
    ref, loss = E.recon_ref(g, x, t, wsel, sc)
    bound = E.recon_bound(g, x, t, wsel, sc)
    for fused in (False, True):
        inside(recon_eval32(g, x, t, wsel, sc, form == "mask", fused).ravel(), ref.ravel(), bound.ravel(), "recon %r %s" % (shape, form))
    # the loss: every fp32 square into float64
    d = r(x.astype(np.float64) - t)
    assert abs(E.sum64(r(d * d)) / x.size - loss) <= E.RECON_LOSS_REL * loss
    # exact inputs: integers, and the elementwise result exact where n is a power of two
    g, x, t, sc = E.recon_inputs(B, C, H, 77 + H, True)
    ref, loss = E.recon_ref(g, x, t, wsel, sc)
    d = x.astype(np.float64) - t
    assert (d == np.round(d)).all() and np.abs(d).max() <= 2 and E.sum64(d * d) < 2.0 ** 53
    if (x.size & (x.size - 1)) == 0:
        for fused in (False, True):
            assert (recon_eval32(g, x, t, wsel, sc, form == "mask", fused) == ref).all()


def mse_partials32(x, t, chunk):
    """k_mse_fwd's arithmetic with the worst grouping a thread can see: `chunk` consecutive squares summed in fp32 one after the
    other, the partial sums in float64"""
    d = r(x.astype(np.float64) - t.astype(np.float64))
    sq = r(d * d)
    pad = (-sq.size) % chunk
    sq = np.concatenate([sq, np.zeros(pad)]).reshape(-1, chunk)
    s = np.zeros(sq.shape[0])
    for j in range(chunk):
        s = r(s + sq[:, j])
    return E.sum64(s), float(sq.sum(axis=1).max())


@pytest.mark.parametrize("n", [1, 3, 1027, 65539, E.SWEEP + 7])
def test_mse_loss_bound_holds_in_fp32(n):
    x, t = E.mse_inputs(n, 300 + n % 991, False)
    ref = E.mse_ref(x, t)
    for chunk in (4, 64, 65):
        got, _ = mse_partials32(x, t, chunk)
        assert abs(got / n - ref) <= E.MSE_FWD_REL * ref, (n, chunk)
    x, t = E.mse_inputs(n, 300 + n % 991, True)
    got, biggest = mse_partials32(x, t, 65)
    assert biggest < 2.0 ** 24 and got == E.mse_ref(x, t) * n or abs(got - E.mse_ref(x, t) * n) <= 1e-9
    d = x.astype(np.float64) - t
    assert (d == np.round(d)).all() and got == E.sum64(d * d)


@pytest.mark.parametrize("shape", [(1, 1, 2), (2, 3, 3), (2, 3, 8), (3, 5, 17)])
def test_gdl_bound_holds_in_fp32(shape):
    B, C, H = shape
    n = B * C * H * H
    yh, y = [E.normal(n, 60 + k).reshape(B, C, H, H) for k in (0, 1)]
    ref, bound = E.gdl_fwd_ref(yh, y)
    a12, d12, a34, d34 = E.gdl_terms(yh, y)          # already the fp32 differences
    got = (E.sum64(np.abs(r(a12 - np.abs(d12)))) + E.sum64(np.abs(r(a34 - np.abs(d34))))) / a12.size
    assert abs(got - ref) <= bound
    yh, y = [E.hash_ints(n, 60 + k, -2, 2).astype(F32).reshape(B, C, H, H) for k in (0, 1)]
    a12, d12, a34, d34 = E.gdl_terms(yh, y)
    ties = (d12 == 0).mean() + (a12 == np.abs(d12)).mean()
    assert ties > 0.3, "the exact GDL inputs are meant to be mostly ties"
    K = E.gdl_bwd_counts(yh, y)
    assert np.abs(K).max() <= 4 and K.sum() == 0


@pytest.mark.parametrize("shape", E.GDL_SHAPES)
def test_gdl_backward_sum_of_up_to_four_terms(shape):
    """every order of up to four +-norm terms summed in fp32: within GDL_BWD_ABS_U * U * norm of K * norm, bit-exact for |K| <= 1"""
    import itertools
    B, C, H = shape
    norm = float(F32(1.0 / (B * C * (H - 1) * H)))
    for seq in itertools.product((-1, 0, 1), repeat=4):
        acc = 0.0
        for sgn in seq:
            acc = float(r(acc + sgn * norm))
        K = sum(seq)
        assert abs(acc - K * norm) <= E.GDL_BWD_ABS_U * U * norm, (seq, acc)
        if abs(K) <= 1:
            assert acc == float(r(K * norm)), (seq, acc)


def adam_eval32(x, g, m, v, t, b1, b2, fused):
    """vf_adam_upd's eight statements"""
    x, g, m, v = [a.astype(np.float64) for a in (x, g, m, v)]
    fb1, fo1, fb2, fo2, eps = r(b1), r(1.0 - b1), r(b2), r(1.0 - b2), r(E.ADAM_EPS)
    step = r(E.adam_step_size(t, b1, b2))
    mi = r(m * fb1)
    mi = r(mi + fo1 * g) if fused else r(mi + r(fo1 * g))
    vi = r(v * fb2)
    og = r(fo2 * g)
    vi = r(vi + og * g) if fused else r(vi + r(og * g))
    d = r(r(np.sqrt(vi)) + eps)
    xo = r(x - r(r(step * mi) / d))
    return xo, mi, vi


@pytest.mark.parametrize("betas", E.ADAM_BETAS)
@pytest.mark.parametrize("n", [4, 1023, 10007, 65539])
def test_adam_bounds_hold_in_fp32(n, betas):
    b1, b2 = betas
    x, m, v = E._adam_state(n, 90)
    for t in range(1, 6):
        g = E.adam_grad(n, 90 + 3) if t == 1 else E.adam_grad(n, 200 + t)
        assert all((g == p).any() for p in E.ADAM_PLANT[:min(n, 7)]), "the planted gradients are missing"
        refs, bounds = E.adam_ref(x, g, m, v, t, b1, b2)
        outs = None
        for fused in (False, True):
            outs = adam_eval32(x, g, m, v, t, b1, b2, fused)
            for name, got, ref, bd in zip("xmv", outs, refs, bounds):
                inside(got, ref, bd, "adam %s n=%d t=%d fused=%s" % (name, n, t, fused))
        # flush-to-zero variant of the smallest intermediates: what the FLT_MIN floors are for
        x, m, v = [a.astype(F32) for a in outs]


def test_bce_reference_and_edges():
    for n in (1, 2, 37, 257):
        p = E.bce_inputs(n, 80)
        assert ((p >= 0) & (p <= 1)).all()
        for label in (0.0, 1.0, 0.9):
            loss, cond, g = E.bce_ref(p, label)
            assert np.isfinite(loss) and np.isfinite(g).all() and np.abs(g).max() < 3e38 and cond >= abs(loss) * (1 - 1e-12)


def test_helpers_and_case_tables():
    assert E.ulp32(np.array([1.0, 1.5, 0.75, 0.0]))[:3].tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -24]
    a, b = E.hash_ints(1000, 3, -2, 2), E.hash_ints(1000, 4, -2, 2)
    assert a.min() == -2 and a.max() == 2 and (a != b).any() and (a[:-1] != a[1:]).mean() > 0.5
    assert E.recon_route(12, [0, 0, 0]) == "recon_grad_mix" and E.recon_route(27, [0, 0, 0]) == "recon_grad_mix_scalar"
    assert E.recon_route(12, [0, 1, 0]) == "recon_grad_mix_scalar"
    x = E.act_inputs(E.SWEEP, 5)
    assert all((x == e).any() for e in E.ACT_EDGES if e != 0)
    assert all(isinstance(u, int) and u >= 1 for u in E.TRANSCENDENTAL_ULPS.values())
    for n in (5, 1027, 4):
        combos = E.offset_combos(2, n)
        assert (0, 1) in combos and (1, 0) in combos and (3, 3) in combos and (0, 0) not in combos
