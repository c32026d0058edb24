"""Scores of result frames on the device (vf_metrics.hip) against the host path they replace, on the
whole-frame driver's own workload: predLen 16 and 120 frames of 384 x 512 x 3 (valid 360 x 480, a blob mask), as float
N x 3 x H x W and as uint8 N x H x W x 3.
  device  inference.evaluate_frames on tensors that are on the device: the memset, the one launch, the read of the table.
          kernel_ms is the launch alone (vf_prof), wall_ms the call;
  host    what a user does without it, on ONE thread: download both batches, then tests/metrics_ref.py (the same rule in
          vectorised NumPy: integral images for the window sums).  Writing and reading back the PNG files, which the host
          path of a user also pays, is NOT counted.
Reports, as one JSON document (stdout, and --out FILE), over `--rounds` alternating rounds of device and host (median and
the min-max spread of every figure): the times; the bytes the scores need (both batches once, the mask, the table) and
the fraction of the HBM peak rate (8.0 TB/s) the kernel reaches on them; and the kernel's time by phase, from three more
timed variants of the same call per round — without the flicker term (clip=False: no second look at frame t - 1), on
uint8 instead of float (a quarter of the bytes, no byte rule, the same arithmetic), and both.
Not a gate; evidence only.  Usage: python scripts/bench_metrics.py [--rounds 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12
H, W, VH, VW, C = 384, 512, 360, 480, 3


def stats(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4))


def workload(n, rng):
    """truth: smooth frames drifting over time; result: truth with noise inside a blob-shaped hole -> float N x 3 x H x W"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    t = np.arange(n, dtype=np.float32).reshape(n, 1, 1, 1)
    ph = np.arange(C, dtype=np.float32).reshape(1, C, 1, 1)
    truth = (0.5 + 0.4 * np.sin(yy / 23 + t / 5 + ph) * np.cos(xx / 31 - t / 7)).astype(np.float32)
    mask = (((yy - 170) / 90) ** 2 + ((xx - 250) / 130) ** 2 < 1).astype(np.uint8)
    result = truth + mask * rng.standard_normal(truth.shape).astype(np.float32) * np.float32(0.04)
    return result.astype(np.float32), truth, mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import metrics_ref
    import video_filler_amd  # noqa: F401
    from video_filler_amd import inference
    from video_filler_amd.backend import get_backend

    torch.set_num_threads(1)
    B = get_backend()
    rng = np.random.default_rng(0)
    res = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, frame="%d x %d x %d, valid %d x %d" % (H, W, C, VH, VW),
               hbm_peak_bytes_per_s=HBM_PEAK, batches={})
    for n in (16, 120):
        result, truth, mask = workload(n, rng)
        forms = {"float": (torch.from_numpy(result).cuda(), torch.from_numpy(truth).cuda()),
                 "uint8": tuple(torch.from_numpy(metrics_ref.to_bytes(x)).cuda() for x in (result, truth))}
        m = torch.from_numpy(mask).cuda()

        def kernel_ms(a, b, clip):
            B.prof_begin()
            B.frame_metrics(a, b, m, (VH, VW), clip)
            return B.prof_end()["frame_metrics"]

        for form, (a, b) in forms.items():
            got = inference.evaluate_frames(a, b, m, (VH, VW))          # warm: code load; and the check against the host path
            want = metrics_ref.scores(metrics_ref.frame_table(a.cpu().numpy(), b.cpu().numpy(), mask, (VH, VW)))
            assert all(np.array_equal(got[k], want[k], equal_nan=True) for k in want if k != "mean"), "device != host"
            o = forms["uint8"]
            dev = {k: [] for k in ("kernel", "wall", "no_flicker", "uint8", "uint8_no_flicker")}
            host = {"download": [], "scores": []}
            for _ in range(args.rounds):                                 # alternating: device, then host
                st = kernel_ms(a, b, True)
                dev["kernel"].append(st["ms"])
                dev["no_flicker"].append(kernel_ms(a, b, False)["ms"])
                dev["uint8"].append(kernel_ms(o[0], o[1], True)["ms"])
                dev["uint8_no_flicker"].append(kernel_ms(o[0], o[1], False)["ms"])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                inference.evaluate_frames(a, b, m, (VH, VW))
                dev["wall"].append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                ha, hb, hm = a.cpu().numpy(), b.cpu().numpy(), m.cpu().numpy()
                t1 = time.perf_counter()
                metrics_ref.scores(metrics_ref.frame_table(ha, hb, hm, (VH, VW)))
                t2 = time.perf_counter()
                host["download"].append((t1 - t0) * 1e3)
                host["scores"].append((t2 - t1) * 1e3)
            k_ms = float(np.median(dev["kernel"]))
            host_ms = float(np.median(host["download"]) + np.median(host["scores"]))
            r = dict(frames=n, needed_bytes=int(st["bytes"]), kernel_ms=stats(dev["kernel"]), evaluate_frames_wall_ms=stats(dev["wall"]),
                     needed_bytes_per_s=round(st["bytes"] / (k_ms * 1e-3), 0),
                     fraction_of_hbm_peak=round(st["bytes"] / (k_ms * 1e-3) / HBM_PEAK, 4),
                     kernel_variants_ms={k: stats(dev[k]) for k in ("no_flicker", "uint8", "uint8_no_flicker")},
                     # kernel - no_flicker: the second look at frame t - 1; no_flicker - uint8_no_flicker (float only): loading four
                     # times the bytes and the byte rule; uint8_no_flicker: the LDS passes, the windows' arithmetic, the reduction
                     phases_ms=dict(flicker_loads=round(k_ms - float(np.median(dev["no_flicker"])), 4),
                                    float_loads_and_byte_rule=round(float(np.median(dev["no_flicker"]) - np.median(dev["uint8_no_flicker"])), 4)
                                    if form == "float" else 0.0,
                                    passes_and_arithmetic=round(float(np.median(dev["uint8_no_flicker"])), 4)),
                     host_1_thread_ms=dict(download=stats(host["download"]), scores=stats(host["scores"])),
                     host_vs_device_wall=round(host_ms / float(np.median(dev["wall"])), 1))
            res["batches"]["%s_%d" % (form, n)] = r
    out = json.dumps(res, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
