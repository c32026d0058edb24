"""tests/display_ref.py (the host restatement of image.toDisplayTensor / image.minmax and of test.lua's tail, DESIGN.md
5.4) held to hand-computed cases, so that the file the device kernels are compared with is not only checked against
itself; and the argument checks of inference.display_tensor, which run on the host before any backend exists."""
import numpy as np
import pytest

import display_ref as R

F = np.float32


def pack(values):
    return np.array(values, F).reshape(-1, 1, 1, 1)


def test_three_single_pixel_images_on_a_two_wide_grid():
    g = R.to_display_tensor(pack([2, 4, 3]), 0, 2)
    assert g.dtype == F and g.shape == (1, 2, 2)
    # filled with 4; minmax over the grid: (v - 2) / 2
    assert np.array_equal(g[0], np.array([[0, 1], [0.5, 1]], F))


def test_padding_puts_the_images_at_offset_one():
    g = R.to_display_tensor(pack([2, 4, 3]), 2, 2)
    assert g.shape == (1, 6, 6)
    want = np.ones((6, 6), F)
    want[1, 1], want[1, 4], want[4, 1] = 0, 1, 0.5
    assert np.array_equal(g[0], want)


def test_constant_and_zero_tensors():
    c = np.full((2, 3, 2, 2), 0.75, F)
    assert np.array_equal(R.to_display_tensor(c), np.zeros((3, 2, 4), F))          # shifted to 0, divisor 0: not divided
    z = np.zeros((2, 1, 2, 2), F)
    assert np.array_equal(R.to_display_tensor(z), np.zeros((1, 2, 4), F))
    assert np.array_equal(R.minmax(z), z)


def test_given_bounds_with_and_without_saturate():
    x = pack([0, 1, 2, 3, 4, 0.5])
    on = R.to_display_tensor(x, 0, 6, min=0, max=2)
    assert np.array_equal(on[0, 0], np.array([0, 0.5, 1, 1, 1, 0.25], F))
    off = R.to_display_tensor(x, 0, 6, min=0, max=2, saturate=False)
    assert np.array_equal(off[0, 0], np.array([0, 0.5, 1, 1.5, 2, 0.25], F))
    # neither bound given: saturate is dropped, but the inferred range maps into [0,1] anyway
    assert np.array_equal(R.to_display_tensor(x, 0, 6)[0, 0], np.array([0, 0.25, 0.5, 0.75, 1, 0.125], F))
    # values below a given min are clamped to 0 only when saturate holds
    assert np.array_equal(R.to_display_tensor(x, 0, 6, min=1, max=3)[0, 0], np.array([0, 0, 0.5, 1, 1, 0], F))
    assert np.array_equal(R.to_display_tensor(x, 0, 6, min=1, max=3, saturate=False)[0, 0], np.array([-0.5, 0, 0.5, 1, 1.5, -0.25], F))


def test_symmetric_range():
    g = R.to_display_tensor(pack([-1, 3, 0, 1.5]), 0, 4, symmetric=True)
    want = np.array([(v + F(3)) / F(6) for v in np.array([-1, 3, 0, 1.5], F)], F)     # fmin = 3: (v + 3) / 6
    assert np.array_equal(g[0, 0], want)
    assert g[0, 0, 1] == 1 and g[0, 0, 2] == 0.5


# The two ways a divisor is formed from a lower bound that is no float32 (min = 0.1), on a tensor whose maximum is 0.125:
#   max absent    d = max of the shifted tensor = fl32(0.125 + fl32(-0.1))   = 0.024999999  (0x3CCCCCCC)
#   max = 0.125   d = (float)(0.125 - 0.1) in double, cast once              = 0.025        (0x3CCCCCCD)
# found by a search over tmax = k / 16 with numpy; the values are committed here.
LASTBIT = dict(values=[0.105, 0.11, 0.12, 0.125], min=0.1, tmax=0.125, d_inferred=0x3CCCCCCC, d_given=0x3CCCCCCD)


def test_the_two_divisor_forms_differ_in_the_last_bit():
    c = LASTBIT
    x = pack(c["values"])
    d1 = F(F(c["tmax"]) + F(-c["min"]))
    d2 = F(float(c["tmax"]) - c["min"])
    assert d1.view(np.uint32) == c["d_inferred"] and d2.view(np.uint32) == c["d_given"]
    a = R.to_display_tensor(x, 0, 4, min=c["min"], saturate=False)[0, 0]
    b = R.to_display_tensor(x, 0, 4, min=c["min"], max=c["tmax"], saturate=False)[0, 0]
    shifted = x.reshape(-1) + F(-c["min"])
    assert np.array_equal(a, shifted / d1) and np.array_equal(b, shifted / d2)
    assert a[3] == F(1) and b[3] == np.nextafter(F(1), F(0))                        # the top value: 1 against 1 - 2^-24
    assert not np.array_equal(a, b)


def test_scaleeach_scales_every_image_by_its_own_range():
    x = np.zeros((3, 1, 1, 2), F)
    x[0, 0, 0], x[1, 0, 0], x[2, 0, 0] = (0, 10), (-1, 1), (5, 6)
    g = R.to_display_tensor(x, 0, 2, scaleeach=True)
    assert g.shape == (1, 2, 4)
    # every image becomes (0, 1); the empty cell holds the maximum of the SCALED pack, 1; nothing is scaled again
    assert np.array_equal(g[0], np.array([[0, 1, 0, 1], [0, 1, 1, 1]], F))
    # with bounds the images are not stretched to 1: the fill is the largest scaled value, 10 / 20
    g = R.to_display_tensor(x, 2, 3, scaleeach=True, min=0, max=20)
    assert g.shape == (1, 3, 12) and g[0, 0, 0] == F(0.5) and g[0, 1, 2] == F(0.5) and g[0, 1, 5] == 0 and g[0, 1, 10] == F(0.3)
    whole = R.to_display_tensor(x, 0, 2)
    assert np.array_equal(whole[0], (np.array([[0, 10, -1, 1], [5, 6, 10, 10]], F) + F(1)) / F(11))


def test_argument_checks_run_before_any_backend_is_created():
    """No GPU is needed (and none may be asked for) to refuse these."""
    from video_filler_amd import inference
    ok = np.zeros((2, 3, 4, 4), F)
    with pytest.raises(ValueError, match="padding"):
        inference.display_tensor(ok, padding=1)
    with pytest.raises(ValueError, match="padding"):
        inference.display_tensor(ok, padding=-2)
    with pytest.raises(ValueError, match=r"\(2, 2, 4, 4\)"):
        inference.display_tensor(np.zeros((2, 2, 4, 4), F))
    with pytest.raises(ValueError, match=r"\(5, 4, 4\)"):
        inference.display_tensor(np.zeros((5, 4, 4), F))                            # a K x h x w channel grid
    with pytest.raises(ValueError, match=r"\(4, 4\)"):
        inference.display_tensor(np.zeros((4, 4), F))
    with pytest.raises(ValueError, match="table"):
        inference.display_tensor([np.zeros((3, 4, 4), F)] * 2)
    with pytest.raises(ValueError, match="nrow"):
        inference.display_tensor(ok, nrow=0)
    for bad in (dict(padding=1), dict(padding=-2)):
        with pytest.raises(ValueError, match="padding"):
            R.to_display_tensor(ok, **bad)
    with pytest.raises(ValueError):
        R.to_display_tensor(np.zeros((2, 2, 4, 4), F))


@pytest.mark.parametrize("ov", [0, 1])
def test_center_finish_reference(ov):
    rng = np.random.default_rng(4 + ov)
    B, C, fs = 2, 3, 8
    ctx = rng.uniform(-1, 1, (B, C, fs, fs)).astype(F)
    pred = rng.uniform(-1, 1, (B, C, fs // 2, fs // 2)).astype(F)
    pretty, pasted, predm = R.center_finish(ctx, pred, ov)
    assert pretty.shape == (2 * B, C, fs, fs) and pretty.dtype == F
    lo, hi = 2 + ov, 6 - ov
    hole = np.zeros((fs, fs), bool)
    hole[lo:hi, lo:hi] = True
    half = lambda v: (v + F(1)) * F(0.5)                                             # noqa: E731
    for i in range(B):
        assert np.all(pretty[2 * i][:, hole] == 1)
        assert np.array_equal(pretty[2 * i][:, ~hole], half(ctx[i])[:, ~hole])
        assert np.array_equal(pretty[2 * i + 1][:, ~hole], half(ctx[i])[:, ~hole])
        assert np.array_equal(pretty[2 * i + 1][:, lo:hi, lo:hi], half(pred[i])[:, ov:4 - ov, ov:4 - ov])
    assert np.array_equal(pasted, pretty[1::2]) and np.array_equal(predm, half(pred))


def test_center_finish_refuses_an_empty_hole():
    with pytest.raises(ValueError, match="overlapPred=2"):
        R.center_finish(np.zeros((1, 3, 8, 8), F), np.zeros((1, 3, 4, 4), F), 2)
    with pytest.raises(ValueError, match="fineSize=6"):
        R.center_finish(np.zeros((1, 3, 6, 6), F), np.zeros((1, 3, 3, 3), F), 0)


def test_workspace_query_needs_no_gpu_and_refuses_what_the_call_refuses():
    """vf_display_workspace_bytes (host only): 8 bytes per (min, max) partial — one per slice of at least 8192 elements, at most
    256 (8 per image with scaleeach) — and nothing when the extremes are not needed."""
    import ctypes as C
    from video_filler_amd import _lib
    lib = _lib.load()

    def q(*a):
        n = C.c_size_t(12345)
        rc = lib.vf_display_workspace_bytes(*a, C.byref(n))
        return rc, n.value
    # N, C, h, w, padding, nrow, scaleeach, has_min, has_max
    assert q(6, 3, 64, 64, 0, 6, 0, 0, 0) == (0, 9 * 8)
    assert q(6, 3, 64, 64, 0, 6, 1, 0, 0) == (0, 6 * 2 * 8)
    assert q(6, 3, 64, 64, 0, 6, 0, 1, 1) == (0, 0)              # both bounds, nothing to fill
    assert q(6, 3, 64, 64, 2, 6, 0, 1, 1) == (0, 9 * 8)          # the padding holds the scaled maximum
    assert q(6, 3, 64, 64, 0, 4, 0, 1, 1) == (0, 9 * 8)          # so do the two empty cells
    assert q(4096, 3, 128, 128, 0, 64, 0, 0, 0) == (0, 256 * 8)
    rc, _ = q(6, 3, 64, 64, 3, 6, 0, 0, 0)
    assert rc != 0 and b"padding=3" in lib.vf_last_error()
    rc, _ = q(6, 2, 64, 64, 0, 6, 0, 0, 0)
    assert rc != 0 and b"6 x 2 x 64 x 64" in lib.vf_last_error()
