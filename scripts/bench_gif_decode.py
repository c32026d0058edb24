"""Device GIF decode (vf_gif_decode.hip) against Pillow on the host, for the clips of one default
test_vid_wholeim run: 3 clips of 119 frames of 384 x 512, as two sets of files — the ones data.encode_gif writes (full
frames, a local table each, a Clear every 3824 pixels) and the same quantised frames written by Pillow with save_all=True,
optimize=True (delta rectangles with transparency, one unchunked stream per frame).  Reports, as one JSON document (stdout,
and --out FILE), per set, over `--rounds` alternating rounds of device and host (median, and the min-max spread):
  * stage_ms: the two kernels (vf_prof: gifd_lzw, gifd_compose), kernels_ms their sum;
  * decode_gif_wall_ms: wall time of data.decode_gif — the host's walk and packing, the upload, the kernels, the status read;
  * Pillow: seek(k) + convert("RGB") of every frame of every file on one thread, and on a pool of `--threads` threads over
    the files (a GIF's frames depend on one another, so a file is the unit; 3 files keep 3 threads busy).
The device's frames are compared with Pillow's once, outside the timing.  Not a gate; evidence only.
Usage: python scripts/bench_gif_decode.py [--rounds 5] [--threads 16] [--out FILE]"""
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

STAGES = ("lzw", "compose")


def pillow_file(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    out = []
    for k in range(im.n_frames):
        im.seek(k)
        out.append(np.asarray(im.convert("RGB")))
    return out


def pillow_decode(files, threads):
    t0 = time.perf_counter()
    if threads == 1:
        got = [pillow_file(f) for f in files]
    else:
        with ThreadPoolExecutor(threads) as ex:
            got = list(ex.map(pillow_file, files))
    return (time.perf_counter() - t0) * 1e3, got


def pillow_delta_files(frames_u8, delay):
    """the decoded frames of every clip, written by Pillow as delta frames"""
    from PIL import Image
    out = []
    for clip in frames_u8:
        ims = [Image.fromarray(a) for a in clip]
        bio = io.BytesIO()
        ims[0].save(bio, "GIF", save_all=True, optimize=True, append_images=ims[1:], duration=10 * delay, loop=0)
        out.append(bio.getvalue())
    return out


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
    from video_filler_amd.backend import get_backend, gif_decode_workspace_bytes, gif_inspect
    from video_filler_amd.data import decode_gif, encode_gif

    B = get_backend()
    n = args.pred_len - 1
    x = clip(args.pred_len, np.random.default_rng(0)).reshape(3, args.pred_len, 3, 384, 512)[:, :n].copy()
    own = encode_gif(torch.from_numpy(x).cuda(), args.delay)
    frames = [t.cpu().numpy() for t in decode_gif(own)]         # warm: workspace allocation, code load
    sets = {"encode_gif_files": own, "pillow_delta_files": pillow_delta_files(frames, args.delay)}
    res = dict(device=torch.cuda.get_device_name(0), clips=3, frames_per_clip=n, geometry="384x512", rounds=args.rounds,
               threads=args.threads, sets={})
    for name, files in sets.items():
        infos = [gif_inspect(f) for f in files]
        want = pillow_decode(files, 1)[1]
        got = decode_gif(files)
        equal = all(np.array_equal(g.cpu().numpy(), np.stack(w)) for g, w in zip(got, want))
        dev = {k: [] for k in STAGES + ("kernels", "wall")}
        host = {"1_thread": [], "%d_threads_over_files" % args.threads: []}
        for _ in range(args.rounds):                            # alternating: device, then each host setting
            B.prof_begin()
            B.gif_decode(files, False, infos)
            st = B.prof_end()
            for k in STAGES:
                dev[k].append(st["gifd_" + k]["ms"])
            dev["kernels"].append(sum(st["gifd_" + k]["ms"] for k in STAGES))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            decode_gif(files)
            torch.cuda.synchronize()
            dev["wall"].append((time.perf_counter() - t0) * 1e3)
            host["1_thread"].append(pillow_decode(files, 1)[0])
            host["%d_threads_over_files" % args.threads].append(pillow_decode(files, args.threads)[0])
        ws_b, st_b = gif_decode_workspace_bytes(files)
        fi = [f for s in infos for f in s["frame_info"]]
        r = dict(file_bytes=sum(len(f) for f in files), frames=len(fi), decoded_bytes=sum(s["frames"] * s["height"] * s["width"] * 3 for s in infos),
                 rect_pixels=sum(s["rect_pixels"] for s in infos), frames_with_transparency=sum(f["transparency"] >= 0 for f in fi),
                 sub_rectangles=sum((f["w"], f["h"]) != (512, 384) for f in fi), equals_pillow=bool(equal), workspace_bytes=ws_b,
                 staging_bytes=st_b, stage_ms={k: stats(dev[k]) for k in STAGES}, kernels_ms=stats(dev["kernels"]),
                 decode_gif_wall_ms=stats(dev["wall"]), pillow_ms={k: stats(v) for k, v in host.items()})
        for k, v in host.items():
            r["speedup_wall_vs_pillow_" + k] = round(float(np.median(v) / np.median(dev["wall"])), 2)
        res["sets"][name] = r
    out = json.dumps(res, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
