"""Device GIF encode (vf_gif.hip) against Pillow on the host, for the clips of one default
test_vid_wholeim run: 3 clips (result, inpaint, orig) of 119 frames (predLen 120 without the last, as the reference's
shell loop takes them) of 384 x 512 x 3 float in [0,1].  Reports, as one JSON document (stdout, and --out FILE), over
`--rounds` alternating rounds of device and host (median, and the min-max spread of every figure):
  * stage_ms: the kernels per stage (vf_prof: table, map, lzw, pack), kernels_ms their sum;
  * download_ms: the device-to-host copy of the files, timed alone with events;
  * encode_gif_wall_ms: wall time of data.encode_gif — kernels, the offsets' and the files' copies, splitting into bytes;
  * Pillow: `save(..., save_all=True)` of every clip from RGB frames on one thread, and on `--threads` threads with one pool
    over the frames (each frame quantised and LZW-coded as a one-frame GIF, which is where the time goes; stitching the
    frames into clips is not charged).  The float-to-byte conversion is not charged to Pillow either.  File sizes beside
    the times: Pillow's adaptive palette and unchunked LZW against the rule of tests/gif_ref.py.
Not a gate; evidence only.  Usage: python scripts/bench_gif.py [--rounds 5] [--threads 16] [--out FILE]"""
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

STAGES = ("table", "map", "lzw", "pack")


def pillow_clips(clips_u8, delay):
    from PIL import Image
    t0 = time.perf_counter()
    size = 0
    for clip in clips_u8:
        ims = [Image.fromarray(a) for a in clip]
        bio = io.BytesIO()
        ims[0].save(bio, "GIF", save_all=True, append_images=ims[1:], duration=10 * delay, loop=0)
        size += len(bio.getvalue())
    return (time.perf_counter() - t0) * 1e3, size


def pillow_frames(clips_u8, threads):
    from PIL import Image

    def one(a):
        bio = io.BytesIO()
        Image.fromarray(a).save(bio, "GIF")
        return len(bio.getvalue())

    frames = [a for clip in clips_u8 for a in clip]
    with ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        sizes = list(ex.map(one, frames))
        return (time.perf_counter() - t0) * 1e3, int(sum(sizes))


def stats(v):
    return dict(median=round(float(np.median(v)), 3), min=round(float(np.min(v)), 3), max=round(float(np.max(v)), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--pred-len", type=int, default=120)
    ap.add_argument("--delay", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import video_filler_amd  # noqa: F401
    from bench_png import clip
    from video_filler_amd.backend import get_backend, gif_workspace_bytes
    from video_filler_amd.data import encode_gif

    B = get_backend()
    n = args.pred_len - 1
    x = clip(args.pred_len, np.random.default_rng(0)).reshape(3, args.pred_len, 3, 384, 512)[:, :n].copy()
    xd = torch.from_numpy(x).cuda()
    u8 = np.ascontiguousarray((np.trunc(np.float32(255) * x)).astype(np.uint8).transpose(0, 1, 3, 4, 2))
    files = encode_gif(xd, args.delay)                  # warm: workspace allocation, code load
    total = sum(len(f) for f in files)
    dev = {k: [] for k in STAGES + ("kernels", "download", "wall")}
    host = {"clips_1_thread": [], "frames_%d_threads" % args.threads: []}
    sizes = {}
    pin = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    for _ in range(args.rounds):                        # alternating: device, then each host setting
        B.prof_begin()
        buf, offs = B.gif_encode(xd, args.delay)
        st = B.prof_end()
        for k in STAGES:
            dev[k].append(st["gif_" + k]["ms"])
        dev["kernels"].append(sum(st["gif_" + k]["ms"] for k in STAGES))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        pin.copy_(buf[:total], non_blocking=True)
        b.record()
        torch.cuda.synchronize()
        dev["download"].append(a.elapsed_time(b))
        t0 = time.perf_counter()
        again = encode_gif(xd, args.delay)
        dev["wall"].append((time.perf_counter() - t0) * 1e3)
        assert again == files
        ms, sizes["clips"] = pillow_clips(u8, args.delay)
        host["clips_1_thread"].append(ms)
        ms, sizes["frames"] = pillow_frames(u8, args.threads)
        host["frames_%d_threads" % args.threads].append(ms)
    ws_b, out_b = gif_workspace_bytes(3, n, 384, 512)
    res = dict(device=torch.cuda.get_device_name(0), clips=3, frames_per_clip=n, geometry="384x512x3 float [0,1]", rounds=args.rounds,
               delay_cs=args.delay, raw_bytes=int(u8.size), device_file_bytes=total, pillow_save_all_file_bytes=sizes["clips"],
               pillow_single_frame_file_bytes=sizes["frames"], workspace_bytes=ws_b, output_bound_bytes=out_b,
               stage_ms={k: stats(dev[k]) for k in STAGES}, kernels_ms=stats(dev["kernels"]), download_ms=stats(dev["download"]),
               encode_gif_wall_ms=stats(dev["wall"]), pillow_ms={k: stats(v) for k, v in host.items()})
    for k, v in host.items():
        res["speedup_wall_vs_pillow_" + k] = round(float(np.median(v) / np.median(dev["wall"])), 2)
    out = json.dumps(res, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
