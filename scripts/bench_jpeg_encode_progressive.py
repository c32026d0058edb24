"""Device encode of progressive JPEG files (vf_jpeg_encode_prog) against the device's baseline encoder with
optimised tables (vf_jpeg_encode_opts, optimize=1) and against Pillow (libjpeg-turbo) with progressive=True on the host, which
writes the same bytes.  Two batches at quality 75, 4:2:0: `patches`, 64 frames of 128 x 128 x 3 as the configs[1] batch has
them, and `clip720p`, one clip of 16 frames of 720 x 1280 x 3; float in [0,1].
Reports, as one JSON document (stdout, and --out FILE), over `--rounds` alternating rounds of the three (median and the
min-max spread of every figure), after a warm-up call of each:
  * progressive.encode_ms, baseline_optimize.encode_ms: `--reps` encodes back to back between two events, per encode;
  * progressive.stage_ms and stage_share: the kernels per stage (vf_prof: dct, sum, runs, tables, size, scan, clear, write,
    stuff); `runs` is the part of the run resolution that one wave per image and scan walks in order;
  * pillow_progressive_ms on `--threads` threads (the float-to-byte conversion is not charged to it), and whether its files
    equal the device's;
  * the sizes of the files of the three.
Not a gate; evidence only.  Usage: python scripts/bench_jpeg_encode_progressive.py [--rounds 5] [--reps 10] [--threads 16]
[--out FILE]"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_png import clip, stats  # noqa: E402

STAGES = ("dct", "sum", "runs", "tables", "size", "scan", "clear", "write", "stuff")


def clip720p(frames, rng):
    """photo-like content drifting over the frames, a little sensor noise: float N x 3 x 720 x 1280 in [0,1]"""
    yy, xx = np.mgrid[0:720, 0:1280].astype(np.float32)
    out = np.zeros((frames, 3, 720, 1280), np.float32)
    for t in range(frames):
        base = np.stack([0.5 + 0.25 * np.sin((xx + 3 * t) / (37.0 + 11 * c) + c) * np.cos(yy / (53.0 - 7 * c)) + 0.0001 * (xx - yy)
                         for c in range(3)])
        out[t] = np.clip(base + rng.normal(0, 0.01, base.shape).astype(np.float32), 0, 1)
    return out


def pillow_round(frames_u8, quality, threads):
    from PIL import Image, ImageFile
    ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, 1 << 23)   # Pillow writes a progressive file through one buffer

    def one(a):
        bio = io.BytesIO()
        Image.fromarray(a).save(bio, format="JPEG", quality=quality, subsampling=2, progressive=True)
        return bio.getvalue()

    with ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        files = list(ex.map(one, frames_u8))
        return (time.perf_counter() - t0) * 1e3, files


def measure(B, x, quality, args):
    import torch
    from video_filler_amd.data import encode_jpeg
    xd = torch.from_numpy(x).cuda()
    u8 = np.ascontiguousarray((np.trunc(np.float32(255) * x)).astype(np.uint8).transpose(0, 2, 3, 1))
    prog = encode_jpeg(xd, quality, "420", progressive=True)        # warm: workspace allocation, code load
    base = encode_jpeg(xd, quality, "420", optimize=True)
    plain = encode_jpeg(xd, quality, "420")
    pillow_round(u8[:2], quality, 2)
    dev = {k: [] for k in STAGES + ("kernels", "prog", "base")}
    host, same = [], True

    def timed(**kw):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.reps):
            B.jpeg_encode(xd, quality, "420", **kw)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.reps

    for _ in range(args.rounds):                        # alternating: progressive, baseline, host
        B.prof_begin()
        B.jpeg_encode(xd, quality, "420", progressive=True)
        st = B.prof_end()
        for k in STAGES:
            dev[k].append(st["jpeg_prog_" + k]["ms"])
        dev["kernels"].append(sum(st["jpeg_prog_" + k]["ms"] for k in STAGES))
        dev["prog"].append(timed(progressive=True))
        dev["base"].append(timed(optimize=True))
        ms, pf = pillow_round(u8, quality, args.threads)
        host.append(ms)
        same = same and pf == prog
    kern = float(np.median(dev["kernels"]))
    size = lambda files: sum(len(f) for f in files)
    return dict(frames=len(prog), geometry="%dx%dx3 float [0,1]" % x.shape[2:], quality=quality, sampling="420",
                raw_bytes=int(u8.size), files_equal_pillow=bool(same),
                file_bytes=dict(progressive=size(prog), baseline_optimize=size(base), baseline=size(plain)),
                progressive=dict(encode_ms=stats(dev["prog"]), stage_ms={k: stats(dev[k]) for k in STAGES}, kernels_ms=stats(dev["kernels"]),
                                 stage_share={k: round(float(np.median(dev[k])) / kern, 3) for k in STAGES}),
                baseline_optimize=dict(encode_ms=stats(dev["base"])),
                pillow_progressive_ms={"%d_threads" % args.threads: stats(host)},
                progressive_over_baseline_optimize=round(float(np.median(dev["prog"])) / float(np.median(dev["base"])), 2),
                pillow_over_progressive=round(float(np.median(host)) / float(np.median(dev["prog"])), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import video_filler_amd  # noqa: F401
    from video_filler_amd.backend import get_backend

    B = get_backend()
    rng = np.random.default_rng(0)
    batches = {"patches_64x128x128": np.ascontiguousarray(clip(22, rng)[:64, :, 100:228, 150:278]), "clip720p_16": clip720p(16, rng)}
    res = dict(device=torch.cuda.get_device_name(0), host_cpus=os.cpu_count(), rounds=args.rounds, reps=args.reps, threads=args.threads, cases={})
    for name, x in batches.items():
        res["cases"][name] = measure(B, x, 75, args)
    out = json.dumps(res, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
