"""Device PNG decode (vf_png_decode.hip) against Pillow on the host, for two batches:
  masks        256 mask-like 480 x 360 8-bit grey files (a few blobs of 255 on 0, as the reference's masks), Pillow level 6;
  clip_device  the 120 frames of one test_vid_wholeim clip, 384 x 512 x 3, as written by data.encode_png;
  clip_pillow  the same frames as written by Pillow at compress_level 6.
Reports, as one JSON document (stdout, and --out FILE), over `--rounds` alternating rounds of device and host (median and
the min-max spread of every figure):
  * stage_ms: the kernels per stage (vf_prof: inflate, unfilter, expand), kernels_ms their sum;
  * decode_png_wall_ms: wall time of data.decode_png — the inspection and CRCs, packing, upload, kernels, the status read;
  * Pillow's decode (Image.open + load + asarray) on 1 and on `--threads` threads.
Not a gate; evidence only.  Usage: python scripts/bench_png_decode.py [--rounds 5] [--threads 16] [--out FILE]"""
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


def pillow_write(a, level=6):
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(a[..., 0] if a.shape[2] == 1 else a).save(bio, "PNG", compress_level=level)
    return bio.getvalue()


def masks(n, rng):
    yy, xx = np.mgrid[0:360, 0:480]
    out = []
    for _ in range(n):
        m = np.zeros((360, 480), bool)
        for _ in range(int(rng.integers(1, 5))):
            cy, cx, ry, rx = rng.uniform(40, 320), rng.uniform(40, 440), rng.uniform(10, 60), rng.uniform(10, 90)
            m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1
        out.append(pillow_write((m * 255).astype(np.uint8)[..., None]))
    return out


def pillow_round(files, threads):
    from PIL import Image

    def one(f):
        im = Image.open(io.BytesIO(f))
        im.load()
        return np.asarray(im).shape

    with ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        list(ex.map(one, files))
        return (time.perf_counter() - t0) * 1e3


def stats(v):
    return dict(median=round(float(np.median(v)), 3), min=round(float(np.min(v)), 3), max=round(float(np.max(v)), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import video_filler_amd  # noqa: F401
    from bench_png import clip
    from video_filler_amd.backend import get_backend, png_inspect
    from video_filler_amd.data import decode_png, encode_png

    B = get_backend()
    rng = np.random.default_rng(0)
    x = clip(40, rng)
    u8 = np.ascontiguousarray((np.trunc(np.float32(255) * x)).astype(np.uint8).transpose(0, 2, 3, 1))
    batches = {"masks": masks(256, rng), "clip_device": encode_png(torch.from_numpy(x).cuda()),
               "clip_pillow": [pillow_write(a) for a in u8]}
    res = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, batches={})
    for name, files in batches.items():
        infos = [png_inspect(f) for f in files]
        want = np.stack([u8[i] for i in range(len(files))]) if name != "masks" else None
        got = decode_png(files, stack=True)                 # warm: workspace allocation, code load
        if want is not None:
            assert np.array_equal(got.cpu().numpy(), want)
        dev = {"inflate": [], "unfilter": [], "expand": [], "kernels": [], "wall": []}
        host = {1: [], args.threads: []}
        for _ in range(args.rounds):                        # alternating: device, then each host setting
            B.prof_begin()
            B.png_decode(files, None, infos)
            st = B.prof_end()
            for k in ("inflate", "unfilter", "expand"):
                dev[k].append(st["pngd_" + k]["ms"])
            dev["kernels"].append(sum(st["pngd_" + k]["ms"] for k in ("inflate", "unfilter", "expand")))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            decode_png(files, stack=True)
            torch.cuda.synchronize()
            dev["wall"].append((time.perf_counter() - t0) * 1e3)
            for th, v in host.items():
                v.append(pillow_round(files, th))
        r = dict(files=len(files), file_bytes=int(sum(len(f) for f in files)),
                 decoded_bytes=int(sum(i["height"] * i["width"] * i["channels"] for i in infos)),
                 stage_ms={k: stats(dev[k]) for k in ("inflate", "unfilter", "expand")}, kernels_ms=stats(dev["kernels"]),
                 decode_png_wall_ms=stats(dev["wall"]), pillow_ms={"%d_threads" % th: stats(v) for th, v in host.items()})
        r["wall_vs_pillow_%d_threads" % args.threads] = round(float(np.median(host[args.threads]) / np.median(dev["wall"])), 2)
        r["wall_vs_pillow_1_thread"] = round(float(np.median(host[1]) / np.median(dev["wall"])), 2)
        res["batches"][name] = r
    out = json.dumps(res, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
