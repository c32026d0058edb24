"""Overlapped, blended inference windows on the device (vf_windows_gather / _accumulate / _finish and
inference.WindowedInpainter) against tests/window_blend_ref.py, bit for bit wherever the net is exact."""
import numpy as np
import pytest
import torch

import window_blend_ref as R
import window_cases as K
from helpers import rel_err, to_dev, to_np

pytestmark = pytest.mark.gpu


def _geo(g):
    return (g["L"], g["fs"], g["stride"], g["stride_t"])


def _plan(g):
    return R.Plan(g["F"], g["H"], g["W"], g["L"], g["fs"], g["stride"], g["stride_t"])


@pytest.mark.parametrize("chunk", K.CHUNKS, ids=["chunk1", "chunk3", "all"])
@pytest.mark.parametrize("name", sorted(K.GEOMETRIES))
def test_kernels_equal_the_rule_bit_for_bit(name, chunk, hipb):
    """gather, accumulate in chunks, finish (plain and with the paste and the mapping) on random tiles"""
    from video_filler_amd.backend import nhwc_empty
    g = K.GEOMETRIES[name]
    plan, geo = _plan(g), _geo(g)
    frames, mask = K.clip(g, 5)
    rng = np.random.default_rng(6)
    tiles = rng.uniform(-1, 1, (plan.NW, g["L"] * g["nc"], g["fs"], g["fs"])).astype(np.float32)
    f_d, m_d, t_d = hipb.from_host(torch.from_numpy(frames)), hipb.from_host(torch.from_numpy(mask)), to_dev(tiles, hipb)
    chunk = plan.NW if chunk is None else chunk
    want_windows = R.gather(frames, plan)
    acc = hipb.zeros(*frames.shape)
    for w0 in range(0, plan.NW, chunk):
        nw = min(chunk, plan.NW - w0)
        got = nhwc_empty(nw, g["L"] * g["nc"], g["fs"], g["fs"], hipb.device)
        got.fill_(float("nan"))
        hipb.windows_gather(f_d, got, geo, w0)
        np.testing.assert_array_equal(to_np(got), want_windows[w0:w0 + nw])
        hipb.windows_accumulate(t_d[w0:w0 + nw], acc, geo, w0)
    want = R.blend(tiles, plan, g["nc"])
    out = hipb.empty(*frames.shape)
    hipb.windows_finish(acc, geo, out)
    np.testing.assert_array_equal(to_np(out), want)
    if name == "tiles":                                   # one cover of weight 1: the accumulator IS the tile layout
        np.testing.assert_array_equal(R.gather(to_np(acc), plan), tiles)
    out, inp, full = (torch.full_like(acc, float("nan")) for _ in range(3))
    hipb.windows_finish(acc, geo, out, f_d, m_d, inp, full)
    for got, ref in zip((out, inp, full), R.finish(want, frames, mask)):
        np.testing.assert_array_equal(to_np(got), ref)


def test_refusals_name_the_argument_and_launch_nothing(hipb):
    from video_filler_amd import _lib
    from video_filler_amd.backend import _ptr, nhwc_empty
    g = K.GEOMETRIES["triple"]
    L, fs, nc = g["L"], g["fs"], g["nc"]
    frames = hipb.zeros(g["F"], nc, g["H"], g["W"])
    tiles = nhwc_empty(2, L * nc, fs, fs, hipb.device)
    tiles.fill_(7.0)
    acc = torch.full_like(frames, 3.0)
    out = torch.full_like(frames, 5.0)
    bad = [((L, fs, 0, 1), "stride="), ((L, fs, fs + 1, 1), "stride="), ((L, fs, 3, 1), "stride="), ((L, fs, 5, 0), "stride_t="),
           ((L, fs, 5, 3), "stride_t=")]
    for geo, word in bad:
        for call in (lambda: hipb.windows_gather(frames, tiles, geo, 0), lambda: hipb.windows_accumulate(tiles, acc, geo, 0),
                     lambda: hipb.windows_finish(acc, geo, out)):
            with pytest.raises(_lib.VfError, match=word):
                call()
    ok = (L, fs, 5, 1)
    small = hipb.zeros(g["F"], nc, fs - 1, g["W"])
    with pytest.raises(_lib.VfError, match="H="):
        hipb.windows_gather(small, tiles, ok, 0)
    with pytest.raises(_lib.VfError, match="W="):
        hipb.windows_accumulate(tiles, torch.full((g["F"], nc, g["H"], fs - 1), 3.0, device=hipb.device), ok, 0)
    with pytest.raises(_lib.VfError, match="F="):
        hipb.windows_finish(torch.full((1, nc, g["H"], g["W"]), 3.0, device=hipb.device), ok, out[:1].contiguous())
    NW = _plan(g).NW
    for w0 in (-1, NW - 1, NW):
        with pytest.raises(_lib.VfError, match="w0="):
            hipb.windows_gather(frames, tiles, ok, w0)
        with pytest.raises(_lib.VfError, match="w0="):
            hipb.windows_accumulate(tiles, acc, ok, w0)
    with pytest.raises(_lib.VfError, match="go together"):      # frames without mask, inpaint and full
        hipb._c("vf_windows_finish", _ptr(acc), _ptr(frames), None, _ptr(out), None, None, g["F"], nc, g["H"], g["W"], *ok)
    hipb.synchronize()
    assert bool((tiles == 7.0).all()) and bool((acc == 3.0).all()) and bool((out == 5.0).all())


class FakeNet:
    """-flip_x(row) + a fixed position map: a negation, a flip and one correctly rounded addition (tests/window_cases.py)"""

    def __init__(self, pos, device):
        self.pos = torch.from_numpy(pos).to(device)[None]
        self.evaluated = False

    def evaluate(self):
        self.evaluated = True

    def forward(self, x):
        assert self.evaluated
        return (-x.flip(-1)) + self.pos


@pytest.mark.parametrize("max_tiles", [1, 3, 64])
def test_driver_with_an_exact_fake_net_equals_the_rule(max_tiles, hipb):
    from video_filler_amd.inference import WindowedInpainter
    g = K.GEOMETRIES["triple"]
    frames, mask = K.clip(g, 11)
    pos = K.position_map(g["L"] * g["nc"], g["fs"])
    want = R.inpaint(K.fake_net_host(pos), frames, mask, g["L"], g["fs"], g["stride"], g["stride_t"])
    run = WindowedInpainter(FakeNet(pos, hipb.device), g["L"], g["fs"], g["nc"], g["stride"], g["stride_t"], max_tiles)
    got = run(torch.from_numpy(frames), torch.from_numpy(mask))
    for a, b in zip(got, want):
        assert tuple(a.shape) == frames.shape
        np.testing.assert_array_equal(to_np(a), b)


def test_driver_refuses_before_it_touches_the_net(hipb):
    from video_filler_amd.inference import WindowedInpainter
    net = FakeNet(K.position_map(3, 8), hipb.device)
    for kw, word in ((dict(stride=3), "stride="), (dict(stride=9), "stride="), (dict(stride_t=2), "stride_t="), (dict(max_tiles=0), "max_tiles=")):
        with pytest.raises(ValueError, match=word):
            WindowedInpainter(net, 1, 8, 3, **{"stride": 5, **kw})
    run = WindowedInpainter(net, 1, 8, 3, 5)
    with pytest.raises(ValueError, match="H="):
        run(torch.zeros(2, 3, 7, 9), torch.zeros(3, 7, 9, dtype=torch.uint8))
    with pytest.raises(ValueError, match="mask"):
        run(torch.zeros(2, 3, 8, 9), torch.zeros(3, 8, 9))


@pytest.fixture(scope="module")
def nets(oracle, hipb):
    """(oracle generator, device generator) of 6 -> 6 channels: inputLen = 2, nc = 3"""
    from test_gpu_pipeline import _small_netG
    return _small_netG(oracle, hipb, 6, 6, 5)


def test_driver_with_a_real_generator_matches_the_rule_over_the_oracle_forwards(nets, hipb):
    """F = 3 frames of 160 x 224, stride 96, stride_t 1: 2 x 2 x 2 windows of 2 frames x 128 x 128"""
    from video_filler_amd.inference import WindowedInpainter
    ref, net = nets
    g = dict(F=3, nc=3, H=160, W=224, L=2, fs=128, stride=96, stride_t=1)
    frames, mask = K.clip(g, 23)
    plan = _plan(g)
    assert (plan.NT, plan.NY, plan.NX) == (2, 2, 2)
    # (a copy of every result: the oracle's modules hand out their own output buffer)
    tiles = np.concatenate([np.array(ref.forward(w[None].copy()), np.float32) for w in R.gather(frames, plan)])
    want = R.finish(R.blend(tiles, plan, g["nc"]), frames, mask)
    # the comparison below can tell the rule from its neighbours: each mutant moves the result by 100 tolerances
    for mutant in R.MUTANTS:
        assert rel_err(R.blend(tiles, plan, g["nc"], mutant=mutant), R.blend(tiles, plan, g["nc"])) >= 100 * K.NET_TOL, mutant
    run = WindowedInpainter(net, g["L"], g["fs"], g["nc"], g["stride"], g["stride_t"])
    out, inp, full = run(torch.from_numpy(frames), torch.from_numpy(mask))
    assert tuple(out.shape) == frames.shape
    assert rel_err(to_np(out), want[0]) < K.NET_TOL
    assert rel_err(to_np(inp), want[1]) < K.NET_TOL
    np.testing.assert_array_equal(to_np(full), want[2])
    keep = np.broadcast_to(mask[None] == 0, frames.shape)
    np.testing.assert_array_equal(to_np(inp)[keep], want[2][keep])


def test_driver_without_overlap_equals_the_tile_loop_where_it_does_not_flip(nets, hipb):
    """stride == fineSize, stride_t == inputLen on a 256 x 512 clip: the bits of WholeImageInpainter on the bottom row and the
    fourth tile of the top row (the tiles its vertical-flip rule leaves alone) — the paste and the [0,1] mapping included"""
    from video_filler_amd.inference import WholeImageInpainter, WindowedInpainter
    _, net = nets
    g = dict(F=4, nc=3, H=256, W=512)
    frames, mask = K.clip(g, 29)
    whole = WholeImageInpainter(net, g["F"], 2, 128, 3)(torch.from_numpy(frames).reshape(-1, 256, 512), torch.from_numpy(mask))
    whole = [to_np(t) for t in whole]
    got = [to_np(t) for t in WindowedInpainter(net, 2, 128, 3, stride=128)(torch.from_numpy(frames), torch.from_numpy(mask))]
    for a, b in zip(got, whole):
        np.testing.assert_array_equal(a[:, :, 128:, :], b[:, :, 128:, :])
        np.testing.assert_array_equal(a[:, :, :128, 384:], b[:, :, :128, 384:])
    np.testing.assert_array_equal(got[2], whole[2])
    assert not np.array_equal(got[0][:, :, :128, :384], whole[0][:, :, :128, :384])     # the flipped tiles do differ
