"""Device PNG encode (vf_png.hip) against Pillow (libpng + zlib) on the host, for the batch of one default
test_vid_wholeim clip: 120 frames (pred, inpaint, orig x predLen 40) of 384 x 512 x 3 float in [0,1], the shape
WholeImageInpainter returns.  Reports, as one JSON document (stdout, and --out FILE), over `--rounds` alternating rounds
of device and host (median, and the min-max spread of every figure):
  * stage_ms: the kernels per stage (vf_prof: filter, deflate, pack), kernels_ms their sum;
  * download_ms: the device-to-host copy of the files, timed alone with events;
  * encode_png_wall_ms: wall time of data.encode_png — kernels, the offsets' and the files' copies, splitting into bytes;
  * Pillow at compress_level 1 and 6 on 1 and on `--threads` threads (the float-to-byte conversion is not charged to it),
    with the file-size totals of all three beside the times.
With --level 1 the rounds alternate level 0, level 1 (the dense deflate kernel, scope png_deflate_dense) and Pillow at
compress_level 6 on `--threads` threads, and the document holds both levels' stages, walls and file sizes side by side.
Not a gate; evidence only.  Usage: python scripts/bench_png.py [--rounds 5] [--threads 16] [--level 0|1] [--out FILE]"""
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


def clip(pred_len, rng):
    """pred / inpaint / orig of one clip: 360 x 480 photo-like content drifting over the frames, zero-padded to 384 x 512;
    the mask region of pred differs from orig, inpaint mixes them — float N x 3 x 384 x 512 in [0,1]"""
    yy, xx = np.mgrid[0:360, 0:480].astype(np.float32)
    out = np.zeros((3, pred_len, 3, 384, 512), np.float32)
    mask = ((yy - 200) ** 2 + (xx - 260) ** 2 < 70 ** 2)
    for t in range(pred_len):
        base = np.stack([0.5 + 0.25 * np.sin((xx + 3 * t) / (37.0 + 11 * c) + c) * np.cos(yy / (53.0 - 7 * c)) + 0.0003 * (xx - yy)
                         for c in range(3)])
        orig = np.clip(base + rng.normal(0, 0.01, base.shape).astype(np.float32), 0, 1)
        pred = np.clip(base * 0.9 + 0.05 + rng.normal(0, 0.004, base.shape).astype(np.float32), 0, 1)
        out[0, t, :, :360, :480] = pred
        out[1, t, :, :360, :480] = np.where(mask, pred, orig)
        out[2, t, :, :360, :480] = orig
    return out.reshape(3 * pred_len, 3, 384, 512)


def pillow_round(frames_u8, level, threads):
    from PIL import Image

    def one(a):
        bio = io.BytesIO()
        Image.fromarray(a).save(bio, "PNG", compress_level=level)
        return len(bio.getvalue())

    with ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        sizes = list(ex.map(one, frames_u8))
        return (time.perf_counter() - t0) * 1e3, int(sum(sizes))


def stats(v):
    return dict(median=round(float(np.median(v)), 3), min=round(float(np.min(v)), 3), max=round(float(np.max(v)), 3))


def device_round(B, encode_png, xd, level, files, pin, dev):
    """one profiled pass, one timed download and one timed encode_png call at `level`, appended to dev's lists"""
    import torch
    deflate = "png_deflate_dense" if level else "png_deflate"
    total = sum(len(f) for f in files)
    B.prof_begin()
    buf, offs = B.png_encode(xd, level)
    st = B.prof_end()
    ms = {"filter": st["png_filter"]["ms"], "deflate": st[deflate]["ms"], "pack": st["png_pack"]["ms"]}
    for k, v in ms.items():
        dev[k].append(v)
    dev["kernels"].append(sum(ms.values()))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    pin[:total].copy_(buf[:total], non_blocking=True)
    b.record()
    torch.cuda.synchronize()
    dev["download"].append(a.elapsed_time(b))
    t0 = time.perf_counter()
    again = encode_png(xd, level)
    dev["wall"].append((time.perf_counter() - t0) * 1e3)
    assert again == files


def dense_main(args):
    """--level 1: level 0, level 1 and Pillow level 6 on args.threads threads, alternating"""
    import torch
    import video_filler_amd  # noqa: F401
    from video_filler_amd.backend import get_backend
    from video_filler_amd.data import encode_png

    B = get_backend()
    x = clip(args.pred_len, np.random.default_rng(0))
    xd = torch.from_numpy(x).cuda()
    u8 = np.ascontiguousarray((np.trunc(np.float32(255) * x)).astype(np.uint8).transpose(0, 2, 3, 1))
    files = {lv: encode_png(xd, lv) for lv in (0, 1)}                  # warm: workspace allocation, code load
    pin = torch.empty(max(sum(len(f) for f in fl) for fl in files.values()), dtype=torch.uint8, pin_memory=True)
    keys = ("filter", "deflate", "pack", "kernels", "download", "wall")
    dev = {lv: {k: [] for k in keys} for lv in (0, 1)}
    host, size6 = [], 0
    for _ in range(args.rounds):
        for lv in (0, 1):
            device_round(B, encode_png, xd, lv, files[lv], pin, dev[lv])
        ms, size6 = pillow_round(u8, 6, args.threads)
        host.append(ms)
    res = dict(device=torch.cuda.get_device_name(0), frames=len(files[0]), geometry="384x512x3 float [0,1]", rounds=args.rounds,
               raw_bytes=int(u8.size), pillow_level6_file_bytes=size6,
               pillow_ms={"level6_%d_threads" % args.threads: stats(host)})
    for lv in (0, 1):
        d = dev[lv]
        res["level%d" % lv] = dict(file_bytes=sum(len(f) for f in files[lv]), stage_ms={k: stats(d[k]) for k in ("filter", "deflate", "pack")},
                                   kernels_ms=stats(d["kernels"]), download_ms=stats(d["download"]), encode_png_wall_ms=stats(d["wall"]),
                                   speedup_wall_vs_pillow_level6=round(float(np.median(host) / np.median(d["wall"])), 2),
                                   file_bytes_vs_pillow_level6=round(sum(len(f) for f in files[lv]) / size6, 3))
    out = json.dumps(res, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--pred-len", type=int, default=40)
    ap.add_argument("--level", type=int, default=0, choices=(0, 1))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.level:
        return dense_main(args)
    import torch
    import video_filler_amd  # noqa: F401
    from video_filler_amd.backend import get_backend
    from video_filler_amd.data import encode_png

    B = get_backend()
    x = clip(args.pred_len, np.random.default_rng(0))
    xd = torch.from_numpy(x).cuda()
    u8 = np.ascontiguousarray((np.trunc(np.float32(255) * x)).astype(np.uint8).transpose(0, 2, 3, 1))
    files = encode_png(xd)                              # warm: workspace allocation, code load
    total = sum(len(f) for f in files)
    dev = {"filter": [], "deflate": [], "pack": [], "kernels": [], "download": [], "wall": []}
    host = {(lv, th): [] for lv in (1, 6) for th in (1, args.threads)}
    sizes = {}
    pin = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    for _ in range(args.rounds):                        # alternating: device, then each host setting
        B.prof_begin()
        buf, offs = B.png_encode(xd)
        st = B.prof_end()
        for k in ("filter", "deflate", "pack"):
            dev[k].append(st["png_" + k]["ms"])
        dev["kernels"].append(sum(st["png_" + k]["ms"] for k in ("filter", "deflate", "pack")))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        pin.copy_(buf[:total], non_blocking=True)
        b.record()
        torch.cuda.synchronize()
        dev["download"].append(a.elapsed_time(b))
        t0 = time.perf_counter()
        again = encode_png(xd)
        dev["wall"].append((time.perf_counter() - t0) * 1e3)
        assert again == files
        for (lv, th), v in host.items():
            ms, sz = pillow_round(u8, lv, th)
            v.append(ms)
            sizes[lv] = sz
    res = dict(device=torch.cuda.get_device_name(0), frames=len(files), geometry="384x512x3 float [0,1]", rounds=args.rounds,
               raw_bytes=int(u8.size), device_file_bytes=total, pillow_level1_file_bytes=sizes[1], pillow_level6_file_bytes=sizes[6],
               stage_ms={k: stats(dev[k]) for k in ("filter", "deflate", "pack")}, kernels_ms=stats(dev["kernels"]),
               download_ms=stats(dev["download"]), encode_png_wall_ms=stats(dev["wall"]),
               pillow_ms={"level%d_%d_threads" % k: stats(v) for k, v in host.items()})
    res["speedup_wall_vs_pillow_level1_%d_threads" % args.threads] = round(
        float(np.median(host[(1, args.threads)]) / np.median(dev["wall"])), 2)
    res["speedup_wall_vs_pillow_level6_%d_threads" % args.threads] = round(
        float(np.median(host[(6, args.threads)]) / np.median(dev["wall"])), 2)
    out = json.dumps(res, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
