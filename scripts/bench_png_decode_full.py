"""Device PNG decode under the full rule (vf_png_decode_full) against Pillow on the host, for two sets
  masks   256 mask-like 480 x 360 grey files (a few blobs of 255 on 0, as the reference's masks);
  clip    the 120 frames of one test_vid_wholeim clip, 384 x 512 x 3;
each written by the tests' writer (tests/png_full_cases.py; zlib level 6, the Paeth filter on every row) in four layouts:
plain 8-bit, interlaced 8-bit, plain 16-bit, interlaced 16-bit (a 16-bit sample is the byte times 257).
Reports, as one JSON document (stdout, and --out FILE), over `--rounds` alternating rounds of device and host (median and
the min-max spread of every figure):
  * stage_ms: the kernels per stage (vf_prof: inflate, unfilter, expand), kernels_ms their sum;
  * decode_png_wall_ms: wall time of data.decode_png(full=True) — inspection and CRCs, packing, upload, kernels, status read
    (the second of two calls: the first brings the host's caches back after the Pillow rounds);
  * on the plain 8-bit layouts the same figures of the default entry (vf_png_decode, data.decode_png) beside them, the two
    entries taking turns at going first;
  * Pillow's decode (Image.open + load + asarray) on 1 and on `--threads` threads.
Not a gate; evidence only.  Usage: python scripts/bench_png_decode_full.py [--rounds 5] [--threads 16] [--out FILE]"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

STAGES = ("inflate", "unfilter", "expand")


def mask_images(n, rng):
    yy, xx = np.mgrid[0:360, 0:480]
    out = []
    for _ in range(n):
        m = np.zeros((360, 480), bool)
        for _ in range(int(rng.integers(1, 5))):
            cy, cx, ry, rx = rng.uniform(40, 320), rng.uniform(40, 440), rng.uniform(10, 60), rng.uniform(10, 90)
            m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1
        out.append((m * 255).astype(np.uint8)[..., None])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import video_filler_amd  # noqa: F401
    from bench_png import clip
    from bench_png_decode import pillow_round, stats
    from png_full_cases import write_png
    from video_filler_amd.backend import get_backend, png_inspect, png_inspect_full
    from video_filler_amd.data import decode_png

    B = get_backend()
    rng = np.random.default_rng(0)
    frames = np.ascontiguousarray((np.trunc(np.float32(255) * clip(40, rng))).astype(np.uint8).transpose(0, 2, 3, 1))
    sets = {"masks": mask_images(256, rng), "clip": list(frames)}
    res = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, batches={})

    def measure(files, infos, run, wall, kernels):
        dev = {k: [] for k in STAGES + ("kernels", "wall")}
        B.prof_begin()
        run(files, infos)
        st = B.prof_end()
        for k, name in zip(STAGES, kernels):
            dev[k].append(st[name]["ms"])
        dev["kernels"].append(sum(st[name]["ms"] for name in kernels))
        wall(files)                                         # untimed: the host's caches after the Pillow rounds
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wall(files)
        torch.cuda.synchronize()
        dev["wall"].append((time.perf_counter() - t0) * 1e3)
        return dev

    def report(devs):
        d = {k: [v for r in devs for v in r[k]] for k in devs[0]}
        return dict(stage_ms={k: stats(d[k]) for k in STAGES}, kernels_ms=stats(d["kernels"]), decode_png_wall_ms=stats(d["wall"]))

    for sname, images in sets.items():
        ct = 0 if images[0].shape[2] == 1 else 2
        want = np.stack(images)
        for depth in (8, 16):
            for lace in (False, True):
                with ThreadPoolExecutor(args.threads) as ex:
                    files = list(ex.map(lambda a: write_png(a.astype(np.uint16) * (257 if depth == 16 else 1), ct, depth, lace,
                                                            level=6, filters=4), images))
                name = "%s_%s_%d" % (sname, "interlaced" if lace else "plain", depth)
                infos = [png_inspect_full(f) for f in files]
                assert np.array_equal(decode_png(files, stack=True, full=True).cpu().numpy(), want)   # warm, and checked
                both = depth == 8 and not lace
                if both:
                    old_infos = [png_inspect(f) for f in files]
                    assert np.array_equal(decode_png(files, stack=True).cpu().numpy(), want)
                new, old, host = [], [], {1: [], args.threads: []}
                run_new = lambda: new.append(measure(files, infos, lambda f, i: B.png_decode_full(f, None, i),
                                                     lambda f: decode_png(f, stack=True, full=True),
                                                     ("pngd_inflate", "pngd_unfilter_full", "pngd_expand_full")))
                run_old = lambda: old.append(measure(files, old_infos, lambda f, i: B.png_decode(f, None, i),
                                                     lambda f: decode_png(f, stack=True), ("pngd_inflate", "pngd_unfilter", "pngd_expand")))
                for rnd in range(args.rounds):              # alternating: device, then each host setting
                    for run in ((run_new, run_old) if rnd % 2 == 0 else (run_old, run_new)) if both else (run_new,):
                        run()                               # the two entries take turns at going first
                    for th, v in host.items():
                        v.append(pillow_round(files, th))
                r = dict(files=len(files), file_bytes=int(sum(len(f) for f in files)),
                         inflated_bytes=int(sum(i["inflated_bytes"] for i in infos)), **report(new),
                         pillow_ms={"%d_threads" % th: stats(v) for th, v in host.items()})
                if both:
                    r["default_entry"] = report(old)
                wall = r["decode_png_wall_ms"]["median"]
                r["wall_vs_pillow_%d_threads" % args.threads] = round(float(np.median(host[args.threads]) / wall), 2)
                r["wall_vs_pillow_1_thread"] = round(float(np.median(host[1]) / wall), 2)
                res["batches"][name] = r
                print(name, json.dumps(r), flush=True)
    out = json.dumps(res, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
