"""Device APNG encode and decode (vf_png.hip, vf_png_decode.hip) against Pillow on the host, for the
clips of one default test_vid_wholeim run as bench_gif.py takes them: 3 clips (result, inpaint, orig) of 119 frames of
384 x 512 x 3 float in [0,1].  Reports, as one JSON document (stdout, and --out FILE), over `--rounds` alternating rounds of
device and host (median, and the min-max spread of every figure; one warm-up call of each device path before the rounds):
  * encode.stage_ms: the kernels per profiling scope (png_filter, png_deflate, apng_pack: the two scans, the offsets and the
    pack), kernels_ms their sum; png_stage_ms / png_kernels_ms: the same frames through vf_png_encode (png_pack instead) —
    the difference is what the container costs;
  * encode.download_ms: the device-to-host copy of the files, timed alone with events around a synchronise;
  * encode.wall_ms / png_wall_ms: wall time of data.encode_apng and of data.encode_png of the same frames;
  * Pillow encode: save(..., save_all=True, format="PNG") of every clip on one thread, and the three clips on a pool of
    `--threads` threads (one clip each: a clip is one serial zlib job per frame inside Pillow);
  * decode.stage_ms (pngd_inflate, pngd_unfilter_full, pngd_expand_full, apng_compose), kernels_ms, wall_ms of
    data.decode_apng of the device's files, and Pillow's seek + convert("RGB") of every frame of the same files.
The float-to-byte conversion is not charged to Pillow.  Not a gate; evidence only.
Usage: python scripts/bench_apng.py [--rounds 3] [--threads 16] [--out FILE]"""
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

ENC = ("png_filter", "png_deflate", "apng_pack")
PNG = ("png_filter", "png_deflate", "png_pack")
DEC = ("pngd_inflate", "pngd_unfilter_full", "pngd_expand_full", "apng_compose")


def pillow_clip(clip, delay):
    from PIL import Image
    ims = [Image.fromarray(a) for a in clip]
    bio = io.BytesIO()
    ims[0].save(bio, "PNG", save_all=True, append_images=ims[1:], duration=10 * delay, loop=0)
    return len(bio.getvalue())


def pillow_decode(files):
    from PIL import Image
    t0 = time.perf_counter()
    n = 0
    for f in files:
        im = Image.open(io.BytesIO(f))
        for k in range(im.n_frames):
            im.seek(k)
            n += np.asarray(im.convert("RGB")).shape[0]
    return (time.perf_counter() - t0) * 1e3, n


def stats(v):
    return dict(median=round(float(np.median(v)), 3), min=round(float(np.min(v)), 3), max=round(float(np.max(v)), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--pred-len", type=int, default=120)
    ap.add_argument("--delay", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import video_filler_amd  # noqa: F401
    from bench_png import clip
    from video_filler_amd.backend import apng_workspace_bytes, get_backend
    from video_filler_amd.data import decode_apng, encode_apng, encode_png

    B = get_backend()
    n = args.pred_len - 1
    x = clip(args.pred_len, np.random.default_rng(0)).reshape(3, args.pred_len, 3, 384, 512)[:, :n].copy()
    xd = torch.from_numpy(x).cuda()
    flat = xd.flatten(0, 1)
    u8 = np.ascontiguousarray((np.trunc(np.float32(255) * x)).astype(np.uint8).transpose(0, 1, 3, 4, 2))
    files = encode_apng(xd, args.delay)                 # warm: workspace allocation, code load
    pngs = encode_png(flat)
    decode_apng(files)
    total = sum(len(f) for f in files)
    keys = ("kernels", "download", "wall", "png_kernels", "png_wall", "dec_kernels", "dec_wall")
    dev = {k: [] for k in keys}
    stage = {"enc": {k: [] for k in ENC}, "png": {k: [] for k in PNG}, "dec": {k: [] for k in DEC}}
    host = {"encode_clips_1_thread": [], "encode_clips_%d_threads" % min(args.threads, 3): [], "decode_1_thread": []}
    sizes = {}
    pin = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    for _ in range(args.rounds):                        # alternating: device, then each host setting
        B.prof_begin()
        buf, offs = B.apng_encode(xd, args.delay, 0)
        st = B.prof_end()
        for k in ENC:
            stage["enc"][k].append(st[k]["ms"])
        dev["kernels"].append(sum(st[k]["ms"] for k in ENC))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        pin.copy_(buf[:total], non_blocking=True)
        b.record()
        torch.cuda.synchronize()
        dev["download"].append(a.elapsed_time(b))
        t0 = time.perf_counter()
        again = encode_apng(xd, args.delay)
        dev["wall"].append((time.perf_counter() - t0) * 1e3)
        assert again == files
        B.prof_begin()
        B.png_encode(flat)
        st = B.prof_end()
        for k in PNG:
            stage["png"][k].append(st[k]["ms"])
        dev["png_kernels"].append(sum(st[k]["ms"] for k in PNG))
        t0 = time.perf_counter()
        assert encode_png(flat) == pngs
        dev["png_wall"].append((time.perf_counter() - t0) * 1e3)
        B.prof_begin()
        B.apng_decode(files)
        st = B.prof_end()
        for k in DEC:
            stage["dec"][k].append(st[k]["ms"])
        dev["dec_kernels"].append(sum(st[k]["ms"] for k in DEC))
        t0 = time.perf_counter()
        outs = decode_apng(files)
        torch.cuda.synchronize()
        dev["dec_wall"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        sizes["pillow"] = sum(pillow_clip(c, args.delay) for c in u8)
        host["encode_clips_1_thread"].append((time.perf_counter() - t0) * 1e3)
        with ThreadPoolExecutor(min(args.threads, 3)) as ex:
            t0 = time.perf_counter()
            list(ex.map(lambda c: pillow_clip(c, args.delay), u8))
            host["encode_clips_%d_threads" % min(args.threads, 3)].append((time.perf_counter() - t0) * 1e3)
        ms, _ = pillow_decode(files)
        host["decode_1_thread"].append(ms)
    for g in range(3):
        assert np.array_equal(outs[g].cpu().numpy(), u8[g]), "the round trip is lossless"
    ws_b, out_b = apng_workspace_bytes(3, n, 384, 512, 3)
    res = dict(device=torch.cuda.get_device_name(0), clips=3, frames_per_clip=n, geometry="384x512x3 float [0,1]", rounds=args.rounds,
               delay_cs=args.delay, raw_bytes=int(u8.size), device_file_bytes=total, png_files_bytes=sum(len(p) for p in pngs),
               pillow_file_bytes=sizes["pillow"], workspace_bytes=ws_b, output_bound_bytes=out_b,
               encode=dict(stage_ms={k: stats(v) for k, v in stage["enc"].items()}, kernels_ms=stats(dev["kernels"]),
                           download_ms=stats(dev["download"]), wall_ms=stats(dev["wall"]),
                           png_stage_ms={k: stats(v) for k, v in stage["png"].items()}, png_kernels_ms=stats(dev["png_kernels"]),
                           png_wall_ms=stats(dev["png_wall"])),
               decode=dict(stage_ms={k: stats(v) for k, v in stage["dec"].items()}, kernels_ms=stats(dev["dec_kernels"]),
                           wall_ms=stats(dev["dec_wall"])),
               pillow_ms={k: stats(v) for k, v in host.items()})
    for k, v in host.items():
        ref = dev["dec_wall"] if k.startswith("decode") else dev["wall"]
        res["speedup_wall_vs_pillow_" + k] = round(float(np.median(v) / np.median(ref)), 2)
    out = json.dumps(res, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
