"""Cases shared by tests/test_window_blend_ref.py (host) and tests/test_gpu_windows.py (device): small geometries of the
window plan (the kernels are generic in fineSize), and a fake net made of single exact or correctly rounded operations,
so that host and device agree on its output bit for bit."""
import numpy as np

# name -> dict(F, nc, H, W, L, fs, stride, stride_t)
GEOMETRIES = {
    # no overlap: the accumulator equals the tile layout
    "tiles": dict(F=2, nc=3, H=16, W=24, L=1, fs=8, stride=8, stride_t=1),
    # clamped windows and triple covers in y and x (19: 0, 5, 10, 11; 21: 0, 5, 10, 13), double covers in t (5 frames, L = 2,
    # stride 1: 0, 1, 2, 3)
    "triple": dict(F=5, nc=3, H=19, W=21, L=2, fs=8, stride=5, stride_t=1),
    # an axis with a single window (H = fs), a clamped t (6 frames of L = 3 at stride 2: 0, 2, 3), nc = 1
    "single": dict(F=6, nc=1, H=4, W=7, L=3, fs=4, stride=2, stride_t=2),
}
CHUNKS = (1, 3, None)          # None: all windows at once

# the tolerance of the real-generator comparison (the bar of test_whole_image_inpainting_matches_the_tile_loop); a mutant of the
# rule must move a result by 100 times that
NET_TOL = 5e-5


def clip(geo, seed):
    """(frames F x nc x H x W in [-1,1], mask nc x H x W uint8 with a hole that crosses window borders)"""
    rng = np.random.default_rng(seed)
    frames = rng.uniform(-1, 1, (geo["F"], geo["nc"], geo["H"], geo["W"])).astype(np.float32)
    mask = np.zeros((geo["nc"], geo["H"], geo["W"]), np.uint8)
    mask[:, geo["H"] // 4:geo["H"] - 1, 1:(3 * geo["W"]) // 4] = 1
    return frames, mask


def position_map(channels, fs, seed=7):
    return np.random.default_rng(seed).uniform(-1, 1, (channels, fs, fs)).astype(np.float32)


def fake_net_host(pos):
    """rows n x C x fs x fs -> -flip_x(row) + pos: a negation and a flip (exact) and one float32 addition"""
    return lambda tiles: (-tiles[..., ::-1]) + pos[None]
