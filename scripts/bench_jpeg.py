"""Device JPEG decode (vf_jpeg.hip) against Pillow (libjpeg-turbo) on the host, for the two loaders:
  * configs[1]: a batch of 64 photo-like 537x936 files, q90 4:2:0 (train.lua's loader);
  * configs[2]: 16 clips x 16 frames of 360x480, q90 4:2:0 (the video loader), as one batch of 256 files.
Reports, as one JSON document (stdout, and --out FILE), for each subsequence size of --subs:
  * device_ms_per_batch: CUDA events around `reps` back-to-back decodes (host work of one batch overlaps the device
    work of the one before);
  * stage_ms: the kernels (vf_prof), kernels_ms their sum; upload_ms: a pinned host-to-device copy of the staging
    buffer's size, timed alone; the rest of device_ms_per_batch is launch gaps and the host not keeping up;
  * host_call_ms: wall time of one decode call on an idle device (header reads in Python, the one parse of the scan
    data, packing, enqueueing);
  * the synchronisation rounds;
then the header-only inspection alone, and Pillow's decode of the same files on 1 and on `--threads` host threads.
--restart-rows 0,1,2,4,8,16 measures something else and nothing of the above: the configs[1] batch written by the device
encoder (data.encode_jpeg, q90 4:2:0) once per listed restart interval in rows of MCUs (0: none), and the decoder's time,
rate, kernels and synchronisation rounds on each set of files at --subs' first size, over --rounds alternating rounds: does
a workgroup per restart segment make the decoder faster?
Not a gate; evidence only.  Usage: python scripts/bench_jpeg.py [--reps 20] [--subs 128,256,512,1024] [--out FILE]
[--restart-rows 0,1,2,4,8,16 [--rounds 5]]"""
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


def photo(h, w, rng):
    """smooth colour structure plus sensor-like noise (the size of file a q90 photo gives)"""
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([128 + 60 * np.sin(xx / rng.uniform(20, 50)) + 30 * np.cos(yy / rng.uniform(15, 40)),
                  128 + 50 * np.sin((xx + yy) / rng.uniform(30, 70)), 128 + 40 * np.cos(xx / 17.0 - yy / 29.0)], -1)
    return np.clip(a + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(a):
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(a).save(bio, "JPEG", quality=90, subsampling=2)
    return bio.getvalue()


def pillow_ms(files, threads):
    from PIL import Image

    def dec(f):
        return np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))

    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(dec, files[:threads]))
        t0 = time.perf_counter()
        list(ex.map(dec, files))
        return (time.perf_counter() - t0) * 1e3


def restart_sweep(B, rows, sub, args):
    """the decoder on the same frames written with each restart interval"""
    import torch
    from video_filler_amd.backend import jpeg_inspect
    from video_filler_amd.data import encode_jpeg
    rng = np.random.default_rng(0)
    frames = np.stack([photo(537, 936, rng) for _ in range(16)])
    sets, sync = {}, {}
    for r in rows:
        base = encode_jpeg(frames, 90, "420", restart_rows=r)
        files = [base[i % 16] for i in range(64)]
        infos = [jpeg_inspect(f, walk=False) for f in files]
        B.jpeg_decode(files, 3, sub, infos)                # warm
        sets[r] = (files, infos, [], [])
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.rounds):                           # alternating over the intervals
        for r, (files, infos, ms, kern) in sets.items():
            a.record()
            for _ in range(args.reps):
                _, _, status, rounds = B.jpeg_decode(files, 3, sub, infos)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b) / args.reps)
            B.prof_begin()
            B.jpeg_decode(files, 3, sub, infos)
            kern.append(sum(v["ms"] for v in B.prof_end().values()))
            assert status.cpu().tolist() == [0] * 64
            sync[r] = int(rounds.item())
    out = []
    for r, (files, infos, ms, kern) in sets.items():
        med, rounds = float(np.median(ms)), sync[r]
        out.append(dict(restart_rows=r, segments_per_file=jpeg_inspect(files[0])["segments"], mean_file_bytes=int(np.mean([len(f) for f in files])),
                        device_ms_per_batch=dict(median=round(med, 3), min=round(min(ms), 3), max=round(max(ms), 3)),
                        device_files_per_s=round(64 / med * 1e3), kernels_ms=round(float(np.median(kern)), 3), sync_rounds=rounds))
    return dict(case="configs[1] loader: 64 x 537x936 q90 4:2:0, written by encode_jpeg", subseq_bytes=sub, rounds=args.rounds,
                reps=args.reps, rows=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--subs", default="128,256,512,1024")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--restart-rows", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    import video_filler_amd  # noqa: F401
    import ctypes as C
    from video_filler_amd import _lib
    from video_filler_amd.backend import get_backend, jpeg_inspect

    B = get_backend()
    rng = np.random.default_rng(0)
    subs = [int(v) for v in args.subs.split(",")]
    res = {"device": torch.cuda.get_device_name(0), "rows": []}
    if args.restart_rows is not None:
        res = {"device": res["device"], "restart_sweep": restart_sweep(B, [int(v) for v in args.restart_rows.split(",")], subs[0], args)}
        out = json.dumps(res, indent=1)
        print(out)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(out + "\n")
        return
    base = {}
    for H, W in ((537, 936), (360, 480)):
        base[(H, W)] = [encode(photo(H, W, rng)) for _ in range(16)]
    for name, H, W, n in (("configs[1] loader: 64 x 537x936 q90 4:2:0", 537, 936, 64),
                          ("configs[2] loader: 16 clips x 16 frames 360x480 q90 4:2:0", 360, 480, 256)):
        files = [base[(H, W)][i % 16] for i in range(n)]
        infos = [jpeg_inspect(f, walk=False) for f in files]
        per_sub = []
        for sub in subs:
            B.jpeg_decode(files, 3, sub, infos)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                _, _, status, rounds = B.jpeg_decode(files, 3, sub, infos)
            b.record()
            torch.cuda.synchronize()
            dev_ms = a.elapsed_time(b) / args.reps
            assert status.cpu().tolist() == [0] * n
            B.prof_begin()
            B.jpeg_decode(files, 3, sub, infos)
            stages = B.prof_end()
            host = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                B.jpeg_decode(files, 3, sub, infos)
                host.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            data = b"".join(files)
            offs = np.cumsum([0] + [len(f) for f in files]).astype(np.int64)
            ws_b, st_b = C.c_size_t(), C.c_size_t()
            _lib.check(B.lib.vf_jpeg_workspace_bytes(data, offs.ctypes.data_as(C.c_void_p), n, sub, C.byref(ws_b), C.byref(st_b)))
            src = torch.empty(st_b.value, dtype=torch.uint8, pin_memory=True)
            dst = torch.empty(st_b.value, dtype=torch.uint8, device="cuda")
            dst.copy_(src, non_blocking=True)
            a.record()
            for _ in range(args.reps):
                dst.copy_(src, non_blocking=True)
            b.record()
            torch.cuda.synchronize()
            up_ms = a.elapsed_time(b) / args.reps
            kern = sum(v["ms"] for v in stages.values())
            per_sub.append(dict(subseq_bytes=sub, sync_rounds=int(rounds.item()), device_ms_per_batch=round(dev_ms, 3),
                                device_files_per_s=round(n / dev_ms * 1e3),
                                stage_ms={k: round(v["ms"], 3) for k, v in stages.items()}, kernels_ms=round(kern, 3),
                                upload_mb=round(st_b.value / 2**20, 1), upload_ms=round(up_ms, 3),
                                rest_ms=round(dev_ms - kern - up_ms, 3), host_call_ms=round(float(np.median(host)), 3)))
        t0 = time.perf_counter()
        for _ in range(args.reps):
            [jpeg_inspect(f, walk=False) for f in files]
        inspect_ms = (time.perf_counter() - t0) * 1e3 / args.reps
        p1 = pillow_ms(files, 1)
        pN = pillow_ms(files, args.threads)
        best = min(per_sub, key=lambda r: r["device_ms_per_batch"])
        res["rows"].append(dict(
            case=name, files=n, mean_file_bytes=int(np.mean([len(f) for f in files])), device=per_sub,
            header_inspect_ms_per_batch=round(inspect_ms, 3), pillow_1_thread_ms=round(p1, 2), pillow_threads=args.threads,
            pillow_n_threads_ms=round(pN, 2), pillow_n_threads_files_per_s=round(n / pN * 1e3),
            best_subseq_bytes=best["subseq_bytes"], speedup_vs_pillow_n_threads=round(pN / best["device_ms_per_batch"], 2)))
    out = json.dumps(res, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
