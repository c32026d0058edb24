"""Device JPEG encode (vf_jpeg_enc.hip) against Pillow (libjpeg-turbo) on the host, which writes the same
bytes.  Two batches: `clip`, the 120 frames (pred, inpaint, orig x predLen 40) of 384 x 512 x 3 float in [0,1] of one default
test_vid_wholeim clip, and `patches`, 64 frames of 128 x 128 x 3; each at quality 75 4:2:0 and at quality 90 4:4:4.
Reports, as one JSON document (stdout, and --out FILE), over `--rounds` alternating rounds of device and host (median,
and the min-max spread of every figure):
  * encode_ms: `--reps` encodes back to back between two events, per encode: what the kernels cost when launches overlap;
  * stage_ms and stage_share: the kernels per stage (vf_prof: dct, size, scan, clear, write, stuff; with optimize also tables,
    with any option segments) and their shares of the sum;
  * download_ms: the device-to-host copy of the files, timed alone with events;
  * encode_jpeg_wall_ms: wall time of data.encode_jpeg — allocation, kernels, the offsets' and the files' copies, splitting;
  * Pillow on 1 and on `--threads` threads (the float-to-byte conversion is not charged to it), and whether its files
    equal the device's.
--restart-rows R, --restart-blocks B and --optimize are the encoder's options (vf_jpeg_encode_opts; Pillow's
restart_marker_rows, restart_marker_blocks and optimize), given to both sides.
Not a gate; evidence only.  Usage: python scripts/bench_jpeg_encode.py [--rounds 5] [--threads 16] [--restart-rows R]
[--restart-blocks B] [--optimize] [--out FILE]"""
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

STAGES = ("dct", "size", "scan", "clear", "write", "stuff")
PILLOW_SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def pillow_round(frames_u8, quality, sampling, threads, opts):
    from PIL import Image

    def one(a):
        bio = io.BytesIO()
        Image.fromarray(a).save(bio, format="JPEG", quality=quality, subsampling=PILLOW_SUBSAMPLING[sampling],
                                restart_marker_rows=opts[0], restart_marker_blocks=opts[1], optimize=opts[2])
        return bio.getvalue()

    with ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        files = list(ex.map(one, frames_u8))
        return (time.perf_counter() - t0) * 1e3, files


def measure(B, x, quality, sampling, args):
    import torch
    from video_filler_amd.data import encode_jpeg
    xd = torch.from_numpy(x).cuda()
    u8 = np.ascontiguousarray((np.trunc(np.float32(255) * x)).astype(np.uint8).transpose(0, 2, 3, 1))
    opts = (args.restart_rows, args.restart_blocks, args.optimize)
    stages = STAGES + (("tables",) if args.optimize else ()) + (("segments",) if any(opts) else ())
    files = encode_jpeg(xd, quality, sampling, *opts)   # warm: workspace allocation, code load
    total = sum(len(f) for f in files)
    dev = {k: [] for k in stages + ("kernels", "encode", "download", "wall")}
    host = {th: [] for th in (1, args.threads)}
    pin = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    same = True
    for _ in range(args.rounds):                        # alternating: device, then each host setting
        B.prof_begin()
        buf, offs = B.jpeg_encode(xd, quality, sampling, *opts)
        st = B.prof_end()
        for k in stages:
            dev[k].append(st["jpeg_enc_" + k]["ms"])
        dev["kernels"].append(sum(st["jpeg_enc_" + k]["ms"] for k in stages))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.reps):
            B.jpeg_encode(xd, quality, sampling, *opts)
        b.record()
        torch.cuda.synchronize()
        dev["encode"].append(a.elapsed_time(b) / args.reps)
        a.record()
        pin.copy_(buf[:total], non_blocking=True)
        b.record()
        torch.cuda.synchronize()
        dev["download"].append(a.elapsed_time(b))
        t0 = time.perf_counter()
        again = encode_jpeg(xd, quality, sampling, *opts)
        dev["wall"].append((time.perf_counter() - t0) * 1e3)
        assert again == files
        for th, v in host.items():
            ms, pf = pillow_round(u8, quality, sampling, th, opts)
            v.append(ms)
            same = same and pf == files
    kern = float(np.median(dev["kernels"]))
    return dict(frames=len(files), geometry="%dx%dx3 float [0,1]" % x.shape[2:], quality=quality, sampling=sampling,
                restart_rows=opts[0], restart_blocks=opts[1], optimize=opts[2],
                raw_bytes=int(u8.size), file_bytes=total, files_equal_pillow=bool(same),
                encode_ms=stats(dev["encode"]), stage_ms={k: stats(dev[k]) for k in stages}, kernels_ms=stats(dev["kernels"]),
                stage_share={k: round(float(np.median(dev[k])) / kern, 3) for k in stages},
                download_ms=stats(dev["download"]), encode_jpeg_wall_ms=stats(dev["wall"]),
                pillow_ms={"%d_threads" % th: stats(v) for th, v in host.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--restart-rows", type=int, default=0)
    ap.add_argument("--restart-blocks", type=int, default=0)
    ap.add_argument("--optimize", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import video_filler_amd  # noqa: F401
    from video_filler_amd.backend import get_backend

    B = get_backend()
    rng = np.random.default_rng(0)
    big = clip(40, rng)
    batches = {"clip": big, "patches": np.ascontiguousarray(big[:64, :, 100:228, 150:278])}
    res = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, reps=args.reps, threads=args.threads, cases={})
    for name, x in batches.items():
        for quality, sampling in ((75, "420"), (90, "444")):
            res["cases"]["%s_q%d_%s" % (name, quality, sampling)] = measure(B, x, quality, sampling, args)
    out = json.dumps(res, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
