"""The rule of the overlapped, blended inference windows (tests/window_blend_ref.py) held to hand-computed
cases, and inference.window_origins / window_weights held to the rule.  No GPU."""
import numpy as np
import pytest

import video_filler_amd  # noqa: F401
import window_blend_ref as R
import window_cases as K
from helpers import rel_err
from video_filler_amd import inference

ORIGINS = [
    # n, size, stride, origins
    (8, 8, 8, [0]),                       # n == size: one window
    (8, 8, 5, [0]),
    (18, 8, 5, [0, 5, 10]),               # n - size a multiple of the stride: no clamped window
    (24, 8, 8, [0, 8, 16]),               # stride == size
    (19, 8, 5, [0, 5, 10, 11]),           # clamped last window, triple cover at 11-12
    (21, 8, 5, [0, 5, 10, 13]),
    (20, 8, 4, [0, 4, 8, 12]),            # 2 stride == size
    (21, 8, 4, [0, 4, 8, 12, 13]),
    (9, 8, 8, [0, 1]),                    # stride == size and a clamped window
    (6, 3, 2, [0, 2, 3]),
    (5, 1, 1, [0, 1, 2, 3, 4]),           # L = 1
]
REFUSALS = [(7, 8, 8, "n"), (8, 8, 0, "stride"), (8, 8, 9, "stride"), (20, 8, 3, "stride"), (8, 8, -1, "stride")]
AXES = [(n, size, stride) for size in (1, 2, 3, 8, 128) for stride in range((size + 1) // 2, size + 1)
        for n in (size, size + 1, size + stride - 1, size + stride, size + 2 * stride + 1, 3 * size + 5)]


@pytest.mark.parametrize("fn", [R.origins, inference.window_origins], ids=["rule", "inference"])
def test_origins_table_and_refusals(fn):
    for n, size, stride, want in ORIGINS:
        assert list(fn(n, size, stride)) == want, (n, size, stride)
    for n, size, stride, name in REFUSALS:
        with pytest.raises(ValueError, match=r"\b%s=" % name):
            fn(n, size, stride)


def test_inference_plan_equals_the_rule_on_a_sweep():
    for n, size, stride in AXES:
        assert inference.window_origins(n, size, stride) == R.origins(n, size, stride)
        assert inference.window_weights(size, stride) == R.weights(size, stride).tolist()
    for size, stride in ((8, 0), (8, 9), (8, 3)):
        with pytest.raises(ValueError, match="stride="):
            inference.window_weights(size, stride)


def test_weights_and_covers():
    """every sample covered with a positive weight sum; r + 1 between regular neighbours; at most 3 covers per axis"""
    assert R.weights(8, 5).tolist() == [1, 2, 3, 4, 4, 3, 2, 1]
    assert R.weights(8, 8).tolist() == [1] * 8
    assert R.weights(8, 4).tolist() == [1, 2, 3, 4, 4, 3, 2, 1]
    assert R.weights(3, 2).tolist() == [1, 2, 1]
    for n, size, stride in AXES:
        o = R.origins(n, size, stride)
        assert o[0] == 0 and o[-1] == n - size and o == sorted(set(o))
        s, c = R.axis_weight_sum(n, size, stride)
        assert s.min() >= 1 and c.min() >= 1 and c.max() <= 3, (n, size, stride)
        r = size - stride
        regular = [i for i in o if i % stride == 0 and i // stride < len(o)]
        only_regular = np.zeros(n, bool)                     # samples no clamped window touches
        only_regular[:] = True
        if o[-1] % stride != 0:
            only_regular[o[-1]:] = False
        for a, b in zip(regular, regular[1:]):
            both = np.arange(b, a + size)
            both = both[only_regular[both]]
            assert np.all(s[both] == r + 1), (n, size, stride)
        if r == 0 and o[-1] % stride == 0:
            assert np.all(s == 1) and np.all(c == 1)


def test_weight_sums_are_exact_in_float32():
    """the largest sum of weights stays far below 2^24 for fineSize 128 at the deepest overlap, also with temporal overlap"""
    worst = 0
    for L, stride_t in ((1, 1), (2, 1), (4, 2), (16, 8)):
        p = R.Plan(3 * L + 1, 128 * 2 + 37, 128 * 2 + 1, L, 128, 64, stride_t)
        worst = max(worst, int(p.weight_sum().max()))
        assert p.weight_sum().min() >= 1
    assert worst < 1 << 24 and worst <= 27 * 65 * 65 * 9
    with pytest.raises(ValueError, match="stride_t="):
        R.Plan(1200, 128, 128, 600, 128, 64, 300)


@pytest.mark.parametrize("name", sorted(K.GEOMETRIES))
def test_reference_blend_does_not_depend_on_the_chunking(name):
    g = K.GEOMETRIES[name]
    plan = R.Plan(g["F"], g["H"], g["W"], g["L"], g["fs"], g["stride"], g["stride_t"])
    tiles = np.random.default_rng(3).uniform(-1, 1, (plan.NW, g["L"] * g["nc"], g["fs"], g["fs"])).astype(np.float32)
    want = R.blend(tiles, plan, g["nc"], None)
    for chunk in (1, 3):
        assert np.array_equal(R.blend(tiles, plan, g["nc"], chunk), want)
    if g["stride"] == g["fs"] and g["stride_t"] == g["L"] and g["H"] % g["fs"] == 0 and g["W"] % g["fs"] == 0:
        back = R.gather(want.astype(np.float32), plan)       # one cover of weight 1: the tile's value exactly
        assert np.array_equal(back, tiles)


def _ramp_x(size, stride, n, delta, c0):
    """a constant frame through the fake net tile -> tile + delta x_local, blended: (row of the output, its float64 value from
    the weights, the rounding allowance)"""
    plan = R.Plan(1, size, n, 1, size, stride, 1)
    frames = np.full((1, 1, size, n), c0, np.float32)
    ramp = (np.float32(delta) * np.arange(size, dtype=np.float32))[None, None, None, :]
    tiles = R.gather(frames, plan) + ramp
    out = R.blend(tiles, plan, 1)[0, 0]
    assert np.array_equal(out, np.broadcast_to(out[0], out.shape))       # the y taper cancels: one window in y
    w = R.weights(size, stride).astype(np.float64)
    num, den = np.zeros(n), np.zeros(n)
    for o in plan.ox:
        num[o:o + size] += w * (np.float64(c0) + np.float64(np.float32(delta)) * np.arange(size))
        den[o:o + size] += w
    # at most 3 covers: 3 products, 3 sums and a quotient, each within 2^-24 of a value <= |c0| + delta (size - 1), plus the float32
    # ramp and tile values themselves (one rounding each): 9 roundings
    allow = 9 * 2.0 ** -24 * (abs(c0) + delta * (size - 1))
    return out[0].astype(np.float64), num / den, allow


def test_overlap_removes_the_seam_in_x():
    """stride == size: the output steps by delta (size - 1) at every window border.  With overlap r and stride s the step between
    adjacent columns is delta |r - s + 1| / (r + 1) from the first column of an overlap to the column after its last, re-derived
    here from the weights: two regular neighbours at local coordinates l and l - s weigh size - l and l - s + 1, which sum to
    r + 1, so the blended ramp is [(size - l) l + (l - s + 1)(l - s)] / (r + 1), whose difference in l is (r - s + 1) / (r + 1)."""
    size, delta, c0 = 128, 2.0 ** -9, 0.25
    got, want, allow = _ramp_x(size, size, 4 * size, delta, c0)
    assert np.abs(got - want).max() <= allow
    steps = np.diff(got)
    borders = np.arange(size, 4 * size, size) - 1
    assert np.all(np.abs(np.abs(steps[borders]) - delta * (size - 1)) <= 2 * allow)
    stride, r = 96, 32
    n = 3 * stride + size
    got, want, allow = _ramp_x(size, stride, n, delta, c0)
    assert np.abs(got - want).max() <= allow
    steps = np.abs(np.diff(got))
    inside = np.zeros(n - 1, bool)
    for o in range(stride, n - size + 1, stride):
        inside[o - 1:o + r] = True                       # from the column before an overlap to its last column
    bound = delta * abs(r - stride + 1) / (r + 1)
    assert abs(bound / delta - 63 / 33) < 1e-12
    assert np.all(np.abs(steps[inside] - bound) <= 2 * allow)
    assert np.all(np.abs(steps[~inside] - delta) <= 2 * allow)
    assert steps.max() <= bound + 2 * allow < delta * (size - 1) / 60


def test_overlap_removes_the_jump_in_t():
    """the same along t: a net that adds delta * (frame's place in its group) to a constant clip"""
    L, fs, delta, c0 = 4, 8, 2.0 ** -6, -0.5

    def run(F, stride_t):
        plan = R.Plan(F, fs, fs, L, fs, fs, stride_t)
        frames = np.full((F, 1, fs, fs), c0, np.float32)
        off = (np.float32(delta) * np.arange(L, dtype=np.float32))[None, :, None, None]
        out = R.blend(R.gather(frames, plan) + off, plan, 1)
        assert np.array_equal(out, np.broadcast_to(out[:, :, :1, :1], out.shape))
        w = R.weights(L, stride_t).astype(np.float64)
        num, den = np.zeros(F), np.zeros(F)
        for o in plan.ot:
            num[o:o + L] += w * (c0 + delta * np.arange(L))
            den[o:o + L] += w
        allow = 9 * 2.0 ** -24 * (abs(c0) + delta * (L - 1))
        got = out[:, 0, 0, 0].astype(np.float64)
        assert np.abs(got - num / den).max() <= allow
        return np.diff(got), allow

    steps, allow = run(12, 4)
    assert np.all(np.abs(np.abs(steps[[3, 7]]) - delta * (L - 1)) <= 2 * allow)
    stride_t, r = 2, 2
    steps, allow = run(10, stride_t)
    bound = delta * abs(r - stride_t + 1) / (r + 1)                      # delta / 3 instead of 3 delta
    assert np.abs(steps).max() <= max(bound, delta) + 2 * allow
    inside = np.zeros(9, bool)
    for o in range(stride_t, 10 - L + 1, stride_t):
        inside[o - 1:o + r] = True
    assert np.all(np.abs(np.abs(steps[inside]) - bound) <= 2 * allow)


def fake_case(seed=11):
    g = K.GEOMETRIES["triple"]
    frames, mask = K.clip(g, seed)
    net = K.fake_net_host(K.position_map(g["L"] * g["nc"], g["fs"]))
    return g, frames, mask, net


def test_mutants_of_the_rule_move_the_result():
    """uniform weights, the last clamped window dropped, the y and x origin tables swapped, channel-to-frame mapping by k % L: each
    moves the fake-net result of the device test by at least 100 times the tolerance of the real-generator comparison (which
    checks its own case the same way), so those comparisons can tell the rule from its neighbours."""
    g, frames, mask, net = fake_case()
    args = (net, frames, mask, g["L"], g["fs"], g["stride"], g["stride_t"])
    want = R.inpaint(*args)
    for chunk in (1, 3):
        for a, b in zip(R.inpaint(*args, chunk=chunk), want):
            assert np.array_equal(a, b)
    keep = np.broadcast_to(mask[None] == 0, want[1].shape)
    assert np.array_equal(want[1][keep], want[2][keep]) and not np.array_equal(want[1], want[2])
    for mutant in R.MUTANTS:
        got = R.inpaint(*args, mutant=mutant)
        assert rel_err(got[0], want[0]) >= 100 * K.NET_TOL, mutant
        assert rel_err(got[1], want[1]) >= 100 * K.NET_TOL, mutant
