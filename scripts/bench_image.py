"""Loader cost on the device against the host restatement: is a training run loader-bound?

Reports, as one JSON document (stdout, and --out FILE):
  * device time per ImageBatcher.add (train.lua's loader: loadSize 350, fineSize 128) from decoded uint8 360x480 and
    512x683 frames already on the device (CUDA events around `reps` back-to-back adds), and the wall time per add
    from HOST frames (includes the upload);
  * wall time per ClipBatcher.add_frames (datavid loader: predLen 4 and 16, loadSize 350, mask state, the
    dark-crop read-back that synchronises every sample);
  * the same work by tests/image_ref.py (NumPy float32 restatement) on one host thread.
Not a gate; evidence only.  Usage: python scripts/bench_image.py [--reps 200] [--host-reps 3] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def device_us(fn, reps, torch):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def wall_us(fn, reps, torch=None):
    fn()
    if torch is not None:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    if torch is not None:
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import image_ref as R
    import video_filler_amd  # noqa: F401
    from video_filler_amd.data import ClipBatcher, ImageBatcher, load_size

    torch.set_num_threads(1)
    rng = np.random.default_rng(0)
    fs, loadSize = 128, 350
    res = {"loadSize": loadSize, "fineSize": fs, "device": torch.cuda.get_device_name(0), "rows": []}

    for H, W in ((360, 480), (512, 683)):
        frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        ib = ImageBatcher(64, 3, fs, loadSize, rng=np.random.default_rng(1))
        dframe = torch.from_numpy(frame).cuda()
        hframe = torch.from_numpy(frame)

        def add(x):
            if ib.n == ib.B:
                ib.batch()
            ib.add(x)

        dev = device_us(lambda: add(dframe), args.reps, torch)
        wall_host_in = wall_us(lambda: add(hframe), args.reps, torch)
        h, w = load_size(H, W, loadSize)
        d = ib.draw(H, W)
        host = wall_us(lambda: R.hook2d(R.decoded_to_float(frame), h, w, fs, d["w1"], d["h1"], d["flip"]), args.host_reps)
        res["rows"].append(dict(what="ImageBatcher.add", frame="%dx%d uint8" % (H, W), scaled="%dx%d" % (h, w),
                                device_us=round(dev, 2), wall_us_from_host_frame=round(wall_host_in, 2),
                                host_image_ref_us=round(host, 1), host_over_device=round(host / dev, 1)))

    H, W = 360, 480
    for predLen in (4, 16):
        frames = rng.integers(0, 256, (predLen, H, W, 3), dtype=np.uint8)
        mask = np.zeros((1, H, W), np.uint8)
        mask[:, 120:240, 160:320] = 1
        cb = ClipBatcher(16, predLen * 3, fs, rng=np.random.default_rng(2))
        cb.set_mask(torch.from_numpy(mask))
        dframes = torch.from_numpy(frames).cuda()

        def add_frames():
            if cb.n == cb.B:
                cb.batch()
            cb.add_frames(dframes, loadSize)

        wall = wall_us(add_frames, args.reps, torch)
        h, w = load_size(H, W, loadSize)
        state = [mask]

        def host_ref():
            clip = R.load_cont(np.stack([R.decoded_to_float(f) for f in frames]), h, w)
            state[0] = R.scale(state[0], w, h)
            return clip[:, 10:10 + fs, 20:20 + fs] * np.float32(2) + np.float32(-1)

        host = wall_us(host_ref, args.host_reps)
        res["rows"].append(dict(what="ClipBatcher.add_frames", frame="%d x %dx%d uint8" % (predLen, H, W), scaled="%dx%d" % (h, w),
                                wall_us_incl_readback=round(wall, 2), host_image_ref_us=round(host, 1),
                                host_over_device=round(host / wall, 1)))
    out = json.dumps(res, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
