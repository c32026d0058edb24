"""Device decode of progressive JPEG files (vf_jpeg.hip) against Pillow (libjpeg-turbo) on the host and
against the baseline device decoder on the same images, for the two loader batches of scripts/bench_jpeg.py:
  * configs[1]: 64 photo-like 537x936 files, q90 4:2:0;
  * configs[2]: 256 files of 360x480, q90 4:2:0,
each written by Pillow three ways: progressive, progressive with a restart interval of one MCU row, and baseline.
Reports, as one JSON document (stdout, and --out FILE), per batch and kind of file:
  * device_ms_per_batch: CUDA events around `reps` back-to-back decodes;
  * stage_ms: the kernels (vf_prof) — jpeg_prog_first is the launch of the first scans (self-synchronising, a block per
    segment), jpeg_prog_refine the launches of the refinement levels (a lane per segment), then IDCT and colour;
    kernels_ms their sum; upload_ms: a pinned host-to-device copy of the staging buffer's size, timed alone;
  * host_call_ms: wall time of one decode call on an idle device (the walk of every scan, packing, enqueueing);
  * Pillow's decode of the same files on 1 and on `--threads` host threads.
Not a gate; evidence only.  Usage: python scripts/bench_jpeg_progressive.py [--reps 10] [--sub 256] [--out FILE]"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_jpeg import photo, pillow_ms  # noqa: E402


def encode(a, **kw):
    from PIL import Image, ImageFile
    ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, 1 << 23)   # Pillow writes a progressive file through one buffer
    bio = io.BytesIO()
    Image.fromarray(a).save(bio, "JPEG", quality=90, subsampling=2, **kw)
    return bio.getvalue()


def measure(B, files, prog, sub, reps):
    import torch
    from video_filler_amd import _lib
    from video_filler_amd.backend import jpeg_inspect
    n = len(files)
    infos = [jpeg_inspect(f, walk=False) for f in files]
    run = (lambda: B.jpeg_prog_decode(files, 3, sub, infos)) if prog else (lambda: B.jpeg_decode(files, 3, sub, infos))
    run()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        got = run()
    b.record()
    torch.cuda.synchronize()
    dev_ms = a.elapsed_time(b) / reps
    assert got[2].cpu().tolist() == [0] * n
    B.prof_begin()
    run()
    stages = B.prof_end()
    host = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        host.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    data = b"".join(files)
    offs = np.cumsum([0] + [len(f) for f in files]).astype(np.int64)
    ws_b, st_b = C.c_size_t(), C.c_size_t()
    query = B.lib.vf_jpeg_prog_workspace_bytes if prog else B.lib.vf_jpeg_workspace_bytes
    _lib.check(query(data, offs.ctypes.data_as(C.c_void_p), n, sub, C.byref(ws_b), C.byref(st_b)))
    src = torch.empty(st_b.value, dtype=torch.uint8, pin_memory=True)
    dst = torch.empty(st_b.value, dtype=torch.uint8, device="cuda")
    dst.copy_(src, non_blocking=True)
    a.record()
    for _ in range(reps):
        dst.copy_(src, non_blocking=True)
    b.record()
    torch.cuda.synchronize()
    kern = sum(v["ms"] for v in stages.values())
    row = dict(device_ms_per_batch=round(dev_ms, 3), device_files_per_s=round(n / dev_ms * 1e3),
               stage_ms={k: round(v["ms"], 3) for k, v in stages.items()}, kernels_ms=round(kern, 3),
               upload_mb=round(st_b.value / 2**20, 1), upload_ms=round(a.elapsed_time(b) / reps, 3),
               host_call_ms=round(float(np.median(host)), 3), sync_rounds=int(got[3].item()))
    if prog:
        row["levels"] = got[4]
    return row, got[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sub", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import video_filler_amd  # noqa: F401
    from video_filler_amd.backend import get_backend

    B = get_backend()
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(0), "subseq_bytes": args.sub, "reps": args.reps, "rows": []}
    for name, H, W, n in (("configs[1] loader: 64 x 537x936 q90 4:2:0", 537, 936, 64),
                          ("configs[2] loader: 256 x 360x480 q90 4:2:0", 360, 480, 256)):
        frames = [photo(H, W, rng) for _ in range(16)]
        row = dict(case=name, files=n)
        outs = {}
        for kind, kw, prog in (("progressive", dict(progressive=True), True),
                               ("progressive_restart_rows_1", dict(progressive=True, restart_marker_rows=1), True),
                               ("baseline", {}, False)):
            base = [encode(a, **kw) for a in frames]
            files = [base[i % 16] for i in range(n)]
            m, outs[kind] = measure(B, files, prog, args.sub, args.reps)
            m["mean_file_bytes"] = int(np.mean([len(f) for f in files]))
            m["pillow_1_thread_ms"] = round(pillow_ms(files, 1), 2)
            m["pillow_threads"] = args.threads
            m["pillow_n_threads_ms"] = round(pillow_ms(files, args.threads), 2)
            m["device_over_pillow_n_threads"] = round(m["pillow_n_threads_ms"] / m["device_ms_per_batch"], 2)
            row[kind] = m
        # the three kinds hold the same coefficients, so the same pixels
        row["same_pixels"] = bool(torch.equal(outs["progressive"], outs["baseline"]) and
                                  torch.equal(outs["progressive_restart_rows_1"], outs["baseline"]))
        for kind in ("progressive", "progressive_restart_rows_1"):
            row[kind]["device_over_baseline_device"] = round(row["baseline"]["device_ms_per_batch"] / row[kind]["device_ms_per_batch"], 3)
        res["rows"].append(row)
    out = json.dumps(res, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
