"""Overlapped, blended windows (inference.WindowedInpainter) against the tile loop they generalise
(inference.WholeImageInpainter), on test_vid_wholeim.lua's default clip: 120 frames of 360 x 480 through the full-size
generator (nef = ngf = 64, nBottleneck 4000), for inputLen 1 and 2.
  whole     WholeImageInpainter on the clip zero-padded to 384 x 512 (the -1 the script feeds the net): the yardstick, run in
            slices of 40 frames (the whole clip's 1440 tiles in one batch exceed what the planes kernels address);
  windowed  WindowedInpainter on the 360 x 480 frames at stride 128, 96 and 64, and for inputLen 2 also at stride_t = 1.
Over `--rounds` alternating rounds (median and min-max of every figure): wall time of one call, ending in a device
synchronise; from one more, profiled call per variant the three window kernels' time (vf_prof scopes) and their share of
that call; and two effect figures on the results:
  seam     mean |step| between adjacent columns / rows of outImages across the borders of the un-overlapped plan (multiples
           of 128) over the mean |step| everywhere else;
  flicker  inputLen 2: mean |out[t] - out[t-1]| across group borders (t a multiple of inputLen) over the same within groups.
The generator is untrained: convolution weights N(0, 2 / taps per output) so that its output depends on its input (the
pipeline tests widen theirs for the same reason); times do not depend on the weights, the effect figures describe this net.
last_chunk: one forward at the driver's chunk size and at the size of its last, shorter chunk, alternating and repeated — what
a change of batch size costs the net's plan.
Not a gate; evidence only.  Usage: python scripts/bench_windows.py [--rounds 5] [--frames 120] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, PH, PW, FS, NC = 360, 480, 384, 512, 128, 3
KERNELS = ("windows_gather", "windows_accumulate", "windows_finish")
SLICE = 40          # frames per call of the yardstick


def stats(v):
    return dict(median=round(float(np.median(v)), 3), min=round(float(np.min(v)), 3), max=round(float(np.max(v)), 3))


def workload(n, rng):
    """smooth frames drifting over time with a little noise, in [-1,1], a blob-shaped hole filled with the script's grey"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    t = np.arange(n, dtype=np.float32).reshape(n, 1, 1, 1)
    ph = np.arange(NC, dtype=np.float32).reshape(1, NC, 1, 1)
    frames = 0.8 * np.sin(yy / 23 + t / 5 + ph) * np.cos(xx / 31 - t / 7) + 0.05 * rng.standard_normal((n, NC, H, W))
    mask = np.broadcast_to(((yy - 170) / 90) ** 2 + ((xx - 250) / 130) ** 2 < 1, (NC, H, W)).astype(np.uint8)
    frames = np.where(mask[None] != 0, 2 * 110.0 / 255.0 - 1, frames)
    return np.clip(frames, -1, 1).astype(np.float32), np.ascontiguousarray(mask)


def generator(L, seed):
    import torch
    from video_filler_amd.trainers import build_netG
    net = build_netG(NC * L, NC * L, 64, 64, 4000, True)
    net.getParameters()
    rng = np.random.default_rng(seed)
    parts = []
    for m, name, _, _, n in net._flat[2]:
        t = getattr(m, name)
        if name == "bias":
            parts.append(np.zeros(n, np.float32))
        elif t.dim() == 4:
            # the taps that meet in one output: Cin k^2 for a convolution, Cin (k / stride)^2 for a full convolution on a map,
            # Cin for the one on the 1 x 1 bottleneck
            taps = m.nInputPlane * ((m.kW // m.dW) ** 2 if m._is_full and m.dW > 1 else 1 if m._is_full else m.kW ** 2)
            parts.append(rng.standard_normal(n, dtype=np.float32) * np.float32(np.sqrt(2.0 / taps)))
        else:
            parts.append(np.ones(n, np.float32))
    net.load_reference_flat(torch.from_numpy(np.concatenate(parts)).to(net._flat[0].device))
    net.evaluate()
    return net


def seam(out):
    """out: F x nc x 360 x 480 device tensor -> (mean |step| at the 128-borders) / (mean |step| elsewhere), columns and rows pooled"""
    import torch
    dx = (out[..., :, 1:] - out[..., :, :-1]).abs().mean(dim=(0, 1, 2)).double()
    dy = (out[..., 1:, :] - out[..., :-1, :]).abs().mean(dim=(0, 1, 3)).double()
    bx = torch.zeros(W - 1, dtype=torch.bool, device=out.device)
    by = torch.zeros(H - 1, dtype=torch.bool, device=out.device)
    bx[FS - 1::FS] = True
    by[FS - 1::FS] = True
    border = torch.cat([dx[bx], dy[by]]).mean().item()
    other = torch.cat([dx[~bx], dy[~by]]).mean().item()
    return dict(border=round(border, 6), elsewhere=round(other, 6), ratio=round(border / other, 3))


def flicker(out, L):
    d = (out[1:] - out[:-1]).abs().mean(dim=(1, 2, 3)).double().cpu().numpy()
    t = np.arange(1, out.shape[0])
    at, within = float(d[t % L == 0].mean()), float(d[t % L != 0].mean())
    return dict(group_border=round(at, 6), within_group=round(within, 6), ratio=round(at / within, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import video_filler_amd  # noqa: F401
    from video_filler_amd import inference
    from video_filler_amd.backend import get_backend, nhwc_empty

    B = get_backend()
    F = args.frames
    frames, mask = workload(F, np.random.default_rng(0))
    fd, md = torch.from_numpy(frames).cuda(), torch.from_numpy(mask).cuda()
    padded = torch.full((F, NC, PH, PW), -1.0, device=fd.device)        # zero padding after mul(2):add(-1)
    padded[:, :, :H, :W] = fd
    padmask = torch.zeros((NC, PH, PW), dtype=torch.uint8, device=fd.device)
    padmask[:, :H, :W] = md
    res = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, clip="%d frames of %d x %d x %d" % (F, NC, H, W),
               whole_slice_frames=min(SLICE, F), nets={})
    for L in (1, 2):
        net = generator(L, 1)
        # all 12 * 120 / L tiles in one batch is more than the planes kernels address (2 GiB per operand): the yardstick runs the
        # clip in slices of SLICE frames, which changes no tile; its three results per slice are not joined inside the timing
        S = min(SLICE, F)
        assert F % S == 0 and S % L == 0
        whole = inference.WholeImageInpainter(net, S, L, FS, NC)

        def whole_sliced(whole=whole, S=S):
            parts = [whole(padded[f0:f0 + S].view(S * NC, PH, PW), padmask) for f0 in range(0, F, S)]
            return [[p[i] for p in parts] for i in range(3)]
        variants = {"whole_384x512": whole_sliced}
        windows = {"whole_384x512": (PH // FS) * (PW // FS) * (F // L)}
        for stride, st in [(128, L), (96, L), (64, L)] + ([(96, 1)] if L > 1 else []):
            run = inference.WindowedInpainter(net, L, FS, NC, stride, st)
            ot, oy, ox = run.plan(F, H, W)
            name = "windowed_stride%d_t%d" % (stride, st)
            variants[name] = lambda run=run: run(fd, md)
            windows[name] = len(ot) * len(oy) * len(ox)
        r = {}
        for name, fn in variants.items():                                # warm: code load, the nets' plans at both chunk sizes
            out = fn()[0]
            out = torch.cat(out) if isinstance(out, list) else out
            torch.cuda.synchronize()
            r[name] = dict(windows=windows[name], out_std=round(float(out.std().item()), 4), seam=seam(out[:, :, :H, :W]))
            if L > 1:
                r[name]["flicker"] = flicker(out[:, :, :H, :W], L)
            del out
        t = {k: [] for k in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) * 1e3)
        for name, fn in variants.items():
            r[name]["wall_ms"] = stats(t[name])
            r[name]["over_whole"] = round(float(np.median(t[name]) / np.median(t["whole_384x512"])), 3)
            if name.startswith("windowed"):
                torch.cuda.synchronize()
                B.prof_begin()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                prof = B.prof_end()
                k = {n: round(prof[n]["ms"], 3) for n in KERNELS}
                r[name]["profiled"] = dict(wall_ms=round(wall, 3), kernels_ms=k, launches={n: prof[n]["launches"] for n in KERNELS},
                                           share_of_wall=round(sum(k.values()) / wall, 4),
                                           share_of_kernel_time=round(sum(k.values()) / sum(p["ms"] for p in prof.values()), 4))
        # what a shorter last chunk costs: stride 96 leaves windows % 64 rows for the last forward
        last = windows["windowed_stride96_t%d" % L] % 64 or 32
        tiles = nhwc_empty(64, NC * L, FS, FS, fd.device)
        tiles.uniform_(-1, 1)
        lc = {k: [] for k in ("repeat_64", "repeat_last", "alternate_64", "alternate_last")}
        for _ in range(args.rounds):
            for key, sizes in (("repeat", (64, 64, last, last)), ("alternate", (64, last, 64, last))):
                for i, n in enumerate(sizes):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    net.forward(tiles[:n])
                    torch.cuda.synchronize()
                    if key == "alternate" or i % 2 == 1:                  # repeat: only the second forward at a size
                        lc["%s_%s" % (key, "64" if n == 64 else "last")].append((time.perf_counter() - t0) * 1e3)
        r["last_chunk"] = dict(rows=last, **{k: stats(v) for k, v in lc.items()})
        res["nets"]["inputLen%d" % L] = r
        del net, whole, variants
        torch.cuda.empty_cache()
    out = json.dumps(res, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
