"""decode_jpeg(layouts=True) (vf_jpeg_decode_layouts) measured on the two loader batches of
scripts/bench_jpeg.py: configs[1], 64 photo-like files of 537x936, and configs[2], 256 files of 360x480, all q90.
Per batch, as one JSON document (stdout, and --out FILE):
  (a) old_entry: ordinary 4:2:0 files (Pillow's) through vf_jpeg_decode — the figure to hold against the parent commit's;
  (b) layouts_same_files: the same files through vf_jpeg_decode_layouts;
  (c) 440, 420_one_scan, 420_three_scans (the same coefficients as 420_one_scan, one scan per component) and rgb_444,
      written by the fixture generator's writer, through vf_jpeg_decode_layouts, against Pillow on 1 and --threads threads.
Each row: device_ms_per_batch (CUDA events around `reps` back-to-back decodes; median, min, max over --rounds alternating
rounds), stage_ms (vf_prof), host_call_ms.  --old-entry measures (a) alone and uses nothing this decoder added, so that it
runs on the parent commit as well: --root DIR imports the package from another checkout of the repository.  The writer
is plain Python and slow: --cache FILE.npz keeps the files it wrote (made if absent).
Not a gate; evidence only.  Usage: python scripts/bench_jpeg_layouts.py [--reps 10] [--rounds 5] [--sub 256] [--out FILE]
[--old-entry [--root DIR]] [--cache FILE.npz]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (("configs[1] loader: 64 x 537x936 q90", 537, 936, 64), ("configs[2] loader: 256 x 360x480 q90", 360, 480, 256))
DISTINCT = 4                        # frames written per batch; the batch repeats them


def files_for(H, W, cache):
    """{kind: DISTINCT files}"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from bench_jpeg import encode, photo
    key = "%dx%d/" % (H, W)
    if cache and os.path.exists(cache):
        z = np.load(cache)
        kinds = sorted({k.split("/")[1] for k in z.files if k.startswith(key)})
        if kinds:
            return {kind: [z["%s%s/%d" % (key, kind, i)].tobytes() for i in range(DISTINCT)] for kind in kinds}
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_jpeg_layouts_golden as G
    rng = np.random.default_rng(0)
    frames = [photo(H, W, rng) for _ in range(DISTINCT)]
    out = {"420_pillow": [encode(a) for a in frames],
           "440": [G.write(a, G.LAYOUTS["440"], quality=90) for a in frames],
           "420_one_scan": [G.write(a, G.LAYOUTS["420"], quality=90) for a in frames],
           "420_three_scans": [G.write(a, G.LAYOUTS["420"], [[0], [1], [2]], quality=90) for a in frames],
           "rgb_444": [G.write(a, G.LAYOUTS["444"], quality=90, marker="adobe0", rgb=True) for a in frames]}
    if cache:
        old = dict(np.load(cache)) if os.path.exists(cache) else {}
        old.update({"%s%s/%d" % (key, kind, i): np.frombuffer(f, np.uint8) for kind, fs in out.items() for i, f in enumerate(fs)})
        np.savez_compressed(cache, **old)
    return out


def timed(run, reps, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        got = run()
    b.record()
    torch.cuda.synchronize()
    assert got[2].cpu().tolist() == [0] * n
    return a.elapsed_time(b) / reps


def finish(B, run, ms, reps):
    import torch
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
    return dict(device_ms_per_batch=dict(median=round(float(np.median(ms)), 3), min=round(min(ms), 3), max=round(max(ms), 3)),
                rounds_ms=[round(v, 3) for v in ms], stage_ms={k: round(v["ms"], 3) for k, v in stages.items()},
                kernels_ms=round(sum(v["ms"] for v in stages.values()), 3), host_call_ms=round(float(np.median(host)), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sub", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--old-entry", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--cache", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import video_filler_amd  # noqa: F401
    from video_filler_amd.backend import get_backend, jpeg_inspect
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from bench_jpeg import pillow_ms

    B = get_backend()
    res = {"device": torch.cuda.get_device_name(0), "subseq_bytes": args.sub, "reps": args.reps,
           "rounds": args.rounds, "rows": []}
    for name, H, W, n in BATCHES:
        kinds = files_for(H, W, args.cache)
        sets = {}
        for kind, base in kinds.items():
            files = [base[i % DISTINCT] for i in range(n)]
            if kind == "420_pillow":
                infos = [jpeg_inspect(f, walk=False) for f in files]
                sets["old_entry"] = (files, lambda files=files, infos=infos: B.jpeg_decode(files, 3, args.sub, infos))
            if not args.old_entry:
                from video_filler_amd.backend import jpeg_inspect_layouts
                infos = [jpeg_inspect_layouts(f) for f in files]
                sets["layouts_same_files" if kind == "420_pillow" else kind] = (
                    files, lambda files=files, infos=infos: B.jpeg_decode_layouts(files, 3, args.sub, infos))
        ms = {k: [] for k in sets}
        for k, (_, run) in sets.items():
            run()
        torch.cuda.synchronize()
        for _ in range(args.rounds):            # alternating over the kinds
            for k, (_, run) in sets.items():
                ms[k].append(timed(run, args.reps, n))
        row = dict(case=name, files=n)
        for k, (files, run) in sets.items():
            row[k] = finish(B, run, ms[k], args.reps)
            row[k]["mean_file_bytes"] = int(np.mean([len(f) for f in files]))
            if not args.old_entry and k != "layouts_same_files":
                row[k]["pillow_1_thread_ms"] = round(pillow_ms(files, 1), 2)
                row[k]["pillow_threads"] = args.threads
                row[k]["pillow_n_threads_ms"] = round(pillow_ms(files, args.threads), 2)
                row[k]["device_over_pillow_n_threads"] = round(row[k]["pillow_n_threads_ms"] / row[k]["device_ms_per_batch"]["median"], 2)
        if not args.old_entry:
            a, b = sets["420_one_scan"][1](), sets["420_three_scans"][1]()
            row["three_scans_same_pixels"] = bool(torch.equal(a[0], b[0]))
        res["rows"].append(row)
    out = json.dumps(res, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
