"""Writes tests/golden/gif_decode_cases.npz: the Pillow-written files of the GIF decoder's tests (tests/gif_decode_cases.py).
Run from the repository root: python tests/golden/make_gif_decode_golden.py.  Needs Pillow (made with 12.2.0).

Every file is saved with save_all=True, optimize=True — delta rectangles, and transparency where Pillow finds it worth it —
some with disposal=...; palette images of 2, 4, 16 and 256 colours give tables of 4, 4, 16 and 256 entries (Pillow writes
minimum code size 8 whatever the palette; code sizes 2 .. 7 come from the hand-assembled files).  AGREED names the
files of the Pillow-agreed class (gif_decode_cases.py has its definition): for those, Pillow's own decode must equal
gif_decode_ref's rule here and now, or this script fails; for the others it must differ, so that a label cannot go stale
unnoticed.  The archive holds the files' bytes and the agreed names, nothing else.
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gif_cases  # noqa: E402
import gif_decode_cases as cases  # noqa: E402
import gif_decode_ref  # noqa: E402

W, H = 24, 20


def p_image(idx, pal):
    im = Image.fromarray(np.asarray(idx, np.uint8), "P")
    im.putpalette(np.asarray(pal, np.uint8).tobytes())
    return im


def save(frames, **kw):
    b = io.BytesIO()
    frames[0].save(b, format="GIF", save_all=True, append_images=frames[1:], optimize=True, **kw)
    return b.getvalue()


def moving_block(n, colours, seed):
    """a fixed noise background with a solid block that moves: every frame differs from the one before in two small places"""
    pal = cases.palette(colours, 200 + seed)
    back = cases.noise_idx(H, W, colours - 1, seed)
    out = []
    for k in range(n):
        f = back.copy()
        f[2 + 2 * k:7 + 2 * k, 3 + 3 * k:9 + 3 * k] = colours - 1
        out.append(p_image(f, pal))
    return out


def main():
    files = {}
    files["pil/delta"] = save(moving_block(6, 16, 1), duration=50, loop=0)
    files["pil/delta_d2"] = save(moving_block(6, 16, 2), duration=40, loop=2, disposal=2)
    files["pil/delta_d3"] = save(moving_block(6, 16, 3), duration=[10, 20, 30, 40, 50, 60], disposal=[1, 3, 1, 3, 3, 1])
    files["pil/delta_d12"] = save(moving_block(5, 8, 4), duration=30, disposal=[1, 2, 1, 2, 1])
    for n in (2, 4, 16, 256):
        frames = [p_image(cases.noise_idx(12, 16, n, 10 * n + k), cases.palette(n, 300 + n)) for k in range(2)]
        files["pil/p%d" % n] = save(frames, duration=20)
    files["pil/rgb_photo"] = save([Image.fromarray(gif_cases.photo(H, W, seed=40 + k)) for k in range(3)], duration=100, loop=0)
    files["pil/interlace"] = save(moving_block(3, 4, 5), duration=10, interlace=True)
    agreed = []
    for name, data in sorted(files.items()):
        ref, status, meta = gif_decode_ref.decode(data, alpha=True)
        assert status == 0, name
        same = cases.agrees_with_pillow(data, ref)
        fi = meta["frame_info"]
        print("%-16s %5d bytes, %d frames, code sizes %s, disposals %s, %d with transparency, %d sub-rectangles: %s" % (
            name, len(data), len(fi), sorted({f["min_code_size"] for f in fi}), [f["disposal"] for f in fi],
            sum(f["transparency"] >= 0 for f in fi), sum((f["w"], f["h"]) != (meta["width"], meta["height"]) for f in fi),
            "agrees with Pillow" if same else "differs from Pillow"))
        assert same == (name in AGREED), "%s: %s, but its label says otherwise" % (name, "agrees" if same else "differs")
        if same:
            agreed.append(name)
    np.savez_compressed(os.path.join(HERE, "gif_decode_cases.npz"), agreed=np.array(agreed),
                        **{k: np.frombuffer(v, np.uint8) for k, v in files.items()})


AGREED = {"pil/delta", "pil/delta_d3", "pil/p2", "pil/p4", "pil/p16", "pil/p256", "pil/rgb_photo", "pil/interlace", "pil/delta_d2",
          "pil/delta_d12"}

if __name__ == "__main__":
    main()
