"""Regenerate tests/golden/png_dense_cases.npz: what the level-1 PNG encoder's tests (tests/test_gpu_png_dense.py,
tests/test_png_dense_ref.py) are held to, so the GPU test runs neither the slow host matcher nor zlib's.

Keys: `frame/<name>` (uint8 H x W x C) for the small cases that are not fixtures of png_cases.npz themselves (cuts of its
`decode` and `padded`, and the boundary frames of tests/png_dense_cases.py); `tok/<name>` (int16 [tokens][2]: a literal
is (byte, 0), a match (length, distance)) and `cnt/<name>` (tokens per chunk) the tokens the rule of
tests/png_dense_ref.py gives for every small case; `sz0/<name>` and `szh/<name>` the yardsticks S_Z(6, 0) and
S_Z(6, HIST) (png_dense_ref.zlib_chunked_size: zlib level 6 on every 8 KiB chunk by itself, without and with the HIST
bytes before it as its dictionary) for photo, decode and padded, which depend on the zlib build and are therefore
recorded; `hist` and `chunk` the sizes they were made with.  Usage: python tests/golden/make_png_dense_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import png_dense_cases as cases  # noqa: E402
import png_dense_ref as dense  # noqa: E402
import png_ref  # noqa: E402


def main():
    fx = cases.fixtures()
    arrays = {"chunk": np.int64(dense.CHUNK), "hist": np.int64(dense.HIST)}
    for name, a in cases.small_cases(fx).items():
        if name not in cases.SMALL_FIXTURES:
            arrays["frame/" + name] = a
        s = png_ref.filter_stream(a)
        chunks = [dense.tokens(s, k) for k in range(-(-len(s) // dense.CHUNK))]
        for k, toks in enumerate(chunks):
            o = k * dense.CHUNK
            assert dense.replay(toks, s[max(0, o - dense.HIST):o]) == s[o:o + dense.CHUNK], (name, k)
        arrays["tok/" + name], arrays["cnt/" + name] = cases.pack_tokens(chunks)
        print(name, a.shape, len(chunks), "chunks", int(arrays["cnt/" + name].sum()), "tokens")
    for name in cases.SIZED:
        arrays["sz0/" + name] = np.int64(dense.zlib_chunked_size(fx[name], 6, 0))
        arrays["szh/" + name] = np.int64(dense.zlib_chunked_size(fx[name], 6, dense.HIST))
        print(name, "S_Z(6, 0)", int(arrays["sz0/" + name]), "S_Z(6, HIST)", int(arrays["szh/" + name]))
    np.savez_compressed(cases.GOLD, **arrays)
    print(cases.GOLD, os.path.getsize(cases.GOLD), "bytes")
    assert os.path.getsize(cases.GOLD) < 1 << 20


if __name__ == "__main__":
    main()
