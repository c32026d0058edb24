"""Contact sheets on the device (vf_display.hip + vf_png.hip) against the host: tests/display_ref.py's
numpy restatement of image.toDisplayTensor followed by Pillow's PNG encode of the sheet.  Two cases, the scripts' own:
demo.lua's sheet (42 x 3 x 128 x 128, nrow 6) and test.lua's (128 x 3 x 128 x 128, nrow 10), pretty_output-like content
in [0,1] already on the device.  Reports, as one JSON document (stdout, and --out FILE), over `--rounds` alternating
rounds of device and host (median and min-max of every figure):
  * display_kernels_ms: the two display kernels by event timing (vf_prof: one scope around both launches);
  * device_ms: what inference.save_sheet does on the device, wall time ending in the download of the file —
    display_tensor, data.encode_png (kernels, the offsets' and the file's copies) — without writing the file;
  * host_display_ms, host_png_ms (Pillow, compress_level 1 and 6; the float-to-byte rule is charged to it, as the device
    applies it inside its encoder), and their sums against device_ms.
Not a gate; evidence only.  Usage: python scripts/bench_display.py [--rounds 7] [--out FILE]"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {"demo.lua": dict(N=42, nrow=6), "test.lua": dict(N=128, nrow=10)}


def pretty_like(N, rng, fs=128):
    """rows 2i / 2i+1 as the scripts build them: a photo-like image with a white hole, the same image with a smooth patch"""
    yy, xx = np.mgrid[0:fs, 0:fs].astype(np.float32)
    out = np.empty((N, 3, fs, fs), np.float32)
    for i in range(0, N, 2):
        base = np.stack([0.5 + 0.3 * np.sin((xx + 5 * i) / (17.0 + 5 * c) + c) * np.cos(yy / (23.0 - 3 * c)) for c in range(3)])
        base = np.clip(base + rng.normal(0, 0.02, base.shape).astype(np.float32), 0, 1)
        out[i] = base
        out[i, :, fs // 4:3 * fs // 4, fs // 4:3 * fs // 4] = 1
        out[i + 1] = base
        out[i + 1, :, fs // 4:3 * fs // 4, fs // 4:3 * fs // 4] = base[:, ::2, ::2] * 0.9 + 0.05
    return out


def stats(v):
    return dict(median=round(float(np.median(v)), 3), min=round(float(np.min(v)), 3), max=round(float(np.max(v)), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from PIL import Image
    import display_ref
    import png_ref
    import video_filler_amd  # noqa: F401
    from video_filler_amd import data, inference
    from video_filler_amd.backend import get_backend

    B = get_backend()
    res = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, cases={})
    for name, c in CASES.items():
        x = pretty_like(c["N"], np.random.default_rng(0))
        xd = torch.from_numpy(x).cuda()
        want = display_ref.to_display_tensor(x, 0, c["nrow"])
        grid = inference.display_tensor(xd, nrow=c["nrow"])                  # warm: code load, encoder workspace
        assert np.array_equal(grid.cpu().numpy(), want)
        (png,) = data.encode_png(grid.unsqueeze(0))
        assert np.array_equal(png_ref.read_png(png), png_ref.chw_to_hwc_bytes(want[None])[0])
        t = {k: [] for k in ("kernels", "device", "host_display", "host_png1", "host_png6")}
        sizes = {}
        for _ in range(args.rounds):
            B.prof_begin()
            B.display_tensor(xd, 0, c["nrow"])
            t["kernels"].append(B.prof_end()["display_tensor"]["ms"])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            (again,) = data.encode_png(inference.display_tensor(xd, nrow=c["nrow"]).unsqueeze(0))    # ends in the download
            t["device"].append((time.perf_counter() - t0) * 1e3)
            assert again == png
            t0 = time.perf_counter()
            g = display_ref.to_display_tensor(x, 0, c["nrow"])
            t["host_display"].append((time.perf_counter() - t0) * 1e3)
            for lv in (1, 6):
                t0 = time.perf_counter()
                bio = io.BytesIO()
                Image.fromarray(png_ref.chw_to_hwc_bytes(g[None])[0]).save(bio, "PNG", compress_level=lv)
                t["host_png%d" % lv].append((time.perf_counter() - t0) * 1e3)
                sizes[lv] = len(bio.getvalue())
        r = dict(pack="%d x 3 x 128 x 128" % c["N"], nrow=c["nrow"], grid="%d x %d x %d" % want.shape, grid_bytes=int(want.nbytes),
                 device_file_bytes=len(png), pillow_level1_file_bytes=sizes[1], pillow_level6_file_bytes=sizes[6],
                 display_kernels_ms=stats(t["kernels"]), device_ms=stats(t["device"]), host_display_ms=stats(t["host_display"]),
                 host_png_level1_ms=stats(t["host_png1"]), host_png_level6_ms=stats(t["host_png6"]))
        for lv in (1, 6):
            r["host_over_device_level%d" % lv] = round(float((np.median(t["host_display"]) + np.median(t["host_png%d" % lv]))
                                                             / np.median(t["device"])), 2)
        res["cases"][name] = r
    out = json.dumps(res, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
