"""train_wholeim_input.lua's loader on the device against the two ways to make its batch without it.

Per SAMPLE wall time, each ending in the dark test's read-back (which synchronises), for decoded uint8 360x480 frames
already on the device, loadSize 360, fineSize 128, a 3 x 3 array, batch 4:
  fused     PatchArrayBatcher.add: the mask rescale, one vf_patch_array_prepare launch, the read-back;
  unfused   the same rows from entry points that predate it — image_scale, image_scale_u8 — and torch indexing
            (fill, shift, flip, windows, channels-last copy, the double sum); checked equal to the fused rows first;
  host      tests/patch_array_ref.py (NumPy float32) on one host thread, plus the upload of the three rows.
The device variants are timed in alternating rounds of `reps` samples; min / median / max over the rounds is the spread.
Not a gate; evidence only.  Usage: python scripts/bench_patch_array.py [--reps 200] [--rounds 7] [--host-reps 3] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def spread(v):
    v = sorted(v)
    return dict(min=round(v[0], 2), median=round(v[len(v) // 2], 2), max=round(v[-1], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import image_ref as R
    import patch_array_ref as PA
    import video_filler_amd  # noqa: F401
    from video_filler_amd import data
    from video_filler_amd.backend import nhwc_empty

    torch.set_num_threads(1)
    rng = np.random.default_rng(0)
    H, W, fs, loadSize, Bn, arr, mv = 360, 480, 128, 360, 4, 3, 110.0 / 255.0
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(Bn)]
    dframes = [torch.from_numpy(f).cuda() for f in frames]
    mask0 = np.zeros((1, H, W), np.uint8)
    mask0[:, 40:110, 50:210] = 1
    draws = np.random.default_rng(1)
    ds = [data.draw_patch_array(H, W, loadSize, draws) for _ in range(Bn)]
    dev = dframes[0].device

    pb = data.PatchArrayBatcher(Bn, 3, fs, loadSize, arr, arr, mv, rng=np.random.default_rng(2))
    pb.set_mask(torch.from_numpy(mask0))
    turn = [0]

    def fused():
        if pb.n == pb.B:
            pb.batch()
        k = turn[0] = (turn[0] + 1) % Bn
        pb.add(dframes[k], decisions=ds[k])

    rows = [nhwc_empty(Bn, c, fs, fs, dev) for c in (3 * arr * arr, 12, 12)]
    state = [torch.from_numpy(mask0).cuda()]
    mvt = torch.tensor(mv, dtype=torch.float32, device=dev)

    def unfused_row(k, n):
        d = ds[k]
        h, w = d["height"], d["width"]
        inp = data.image_scale(dframes[k], w, h, layout="hwc")
        state[0] = m = data.image_scale(state[0], w, h)
        mi = torch.where(m.bool(), mvt, inp)
        ch, cw = d["crop_h"] - 1, d["crop_w"] - 1
        tin, tmi, tm = torch.zeros_like(inp), torch.zeros_like(inp), torch.zeros_like(inp)
        tin[:, :h - ch, :w - cw] = inp[:, ch:, cw:]
        tmi[:, :h - ch, :w - cw] = mi[:, ch:, cw:]
        tm[:, :h - ch, :w - cw] = m[:, ch:, cw:]
        if d["flip"]:
            tin, tmi, tm = tin.flip(2), tmi.flip(2), tm.flip(2)
        total = tin[:, :fs, :fs].double().sum()
        sh, sw = (h - fs) // (arr - 1), (w - fs) // (arr - 1)
        wins = [(i * sh, j * sw) for i in range(arr) for j in range(arr)]
        rows[0][n] = torch.cat([tmi[:, y:y + fs, x:x + fs] for y, x in wins]) * 2 + -1
        four = [wins[i * arr + j] for i in range(2) for j in range(2)]
        rows[1][n] = torch.cat([tin[:, y:y + fs, x:x + fs] for y, x in four]) * 2 + -1
        rows[2][n] = torch.cat([tm[:, y:y + fs, x:x + fs] for y, x in four])
        return total.item() / (3 * fs * fs)

    def unfused():
        k = turn[0] = (turn[0] + 1) % Bn
        unfused_row(k, k)

    # the two device paths give the same rows and the same mean before they are timed
    chk = data.PatchArrayBatcher(Bn, 3, fs, loadSize, arr, arr, mv, rng=np.random.default_rng(2))
    chk.set_mask(torch.from_numpy(mask0))
    for k in range(Bn):
        chk.add(dframes[k], decisions=ds[k])
        mean = unfused_row(k, k)
        assert mean == chk.last["mean"] or abs(mean - chk.last["mean"]) < 1e-10 * mean, (mean, chk.last["mean"])
    for a, b in zip(chk.batch(), rows):
        assert torch.equal(a, b), "the unfused composition does not give the fused rows"
    state[0] = torch.from_numpy(mask0).cuda()

    t_f, t_u = [], []
    for _ in range(args.rounds):
        t_f.append(wall_us(fused, args.reps, torch))
        t_u.append(wall_us(unfused, args.reps, torch))

    hstate = [mask0]

    def host():
        k = turn[0] = (turn[0] + 1) % Bn
        masked, full, maskout, s, hstate[0] = PA.sample(R.decoded_to_float(frames[k]), hstate[0], ds[k], fs, arr, arr, mv)
        for j, a in enumerate((masked, full, maskout)):
            rows[j][k] = torch.from_numpy(a).cuda()

    t_h = [wall_us(host, args.host_reps, torch) for _ in range(3)]
    f, u, h = spread(t_f), spread(t_u), spread(t_h)
    res = dict(device=torch.cuda.get_device_name(0), frame="%dx%d uint8" % (H, W), loadSize=loadSize, fineSize=fs,
               array="%dx%d" % (arr, arr), batch=Bn, reps=args.reps, rounds=args.rounds, unit="us per sample, wall, incl. read-back",
               fused_add=f, unfused_device_composition=u, host_numpy_plus_upload=h,
               unfused_over_fused=round(u["median"] / f["median"], 2), host_over_fused=round(h["median"] / f["median"], 1),
               fused_rounds=[round(v, 2) for v in t_f], unfused_rounds=[round(v, 2) for v in t_u])
    out = json.dumps(res, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
