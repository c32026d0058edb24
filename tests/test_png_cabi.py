"""vf_png_workspace_bytes is a host-only entry: it answers, and refuses, without a GPU."""
import ctypes as C

import pytest

import video_filler_amd  # noqa: F401
from video_filler_amd import _lib, backend


def _query(n, H, W, Cc):
    lib = _lib.load()
    ws, out = C.c_size_t(), C.c_size_t()
    rc = lib.vf_png_workspace_bytes(n, H, W, Cc, C.byref(ws), C.byref(out))
    return rc, ws.value, out.value, lib.vf_last_error().decode()


def test_workspace_query_answers_without_a_gpu():
    rc, ws, out, _ = _query(120, 384, 512, 3)
    assert rc == 0
    stream = 384 * (512 * 3 + 1)
    chunks = -(-stream // backend.PNG_CHUNK)
    # every chunk stored: 5 + 12 bytes each, plus signature, IHDR, zlib header and trailer, IEND
    assert out == 120 * (stream + 17 * chunks + 8 + 25 + 6 + 12)
    assert ws >= 120 * stream + out
    assert _query(1, 1, 1, 1)[0] == 0 and _query(1, 16384, 16384, 3)[0] == 0
    assert backend.png_workspace_bytes(2, 5, 7, 1)[1] == 2 * (5 * 8 + 17 + 51)


@pytest.mark.parametrize("geom,word", [((1, 8, 8, 2), "2 channels"), ((1, 8, 8, 4), "4 channels"), ((1, 0, 8, 3), "0x8"),
                                       ((1, 8, 0, 1), "8x0"), ((1, 16385, 8, 3), "16385x8"), ((1, 8, 16385, 3), "8x16385"),
                                       ((0, 8, 8, 3), "0 frames")])
def test_workspace_query_refuses_what_the_encoder_does_not_take(geom, word):
    rc, _, _, err = _query(*geom)
    assert rc != 0 and "vf_png_workspace_bytes" in err and word in err, err
    with pytest.raises(ValueError, match=word):
        backend.png_workspace_bytes(*geom)


def test_save_frames_refuses_a_prefix_given_twice(tmp_path):
    import numpy as np
    from video_filler_amd import inference
    x = np.zeros((1, 4, 4, 3), np.uint8)
    with pytest.raises(AssertionError, match="pred, pred"):
        inference.save_frames(str(tmp_path / "d"), x, pred=x)
    assert not (tmp_path / "d").exists()
