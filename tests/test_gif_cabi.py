"""vf_gif_workspace_bytes is a host-only entry, and vf_gif_encode checks its arguments before it touches the device: both
answer, and refuse, without a GPU."""
import ctypes as C

import numpy as np
import pytest

import video_filler_amd  # noqa: F401
from video_filler_amd import _lib, backend

import gif_cases
import gif_ref


def _query(clips, frames, H, W):
    lib = _lib.load()
    ws, out = C.c_size_t(), C.c_size_t()
    rc = lib.vf_gif_workspace_bytes(clips, frames, H, W, C.byref(ws), C.byref(out))
    return rc, ws.value, out.value, lib.vf_last_error().decode()


def test_chunk_is_the_reference_chunk():
    assert backend.GIF_CHUNK == gif_ref.CHUNK <= 3838 and gif_ref.FIRST + gif_ref.CHUNK <= 4096


def test_workspace_query_answers_without_a_gpu():
    rc, ws, out, _ = _query(3, 119, 384, 512)
    assert rc == 0
    npix = 384 * 512
    chunks = -(-npix // backend.GIF_CHUNK)
    d = (12 * npix + 12 * chunks + 9 + 7) // 8               # every pixel a 12-bit code, a Clear or EOI per chunk, the first Clear
    assert out == 3 * (13 + 19 + 1 + 119 * (8 + 10 + 768 + 1 + d + -(-d // 255) + 1))
    assert ws >= 3 * 119 * npix
    assert _query(1, 1, 1, 1)[0] == 0 and _query(1, 1, 16384, 16384)[0] == 0 and _query(1, 65535, 1, 1)[0] == 0
    assert backend.gif_workspace_bytes(3, 119, 384, 512) == (ws, out)


@pytest.mark.parametrize("geom,word", [((1, 2, 0, 8), "0x8"), ((1, 2, 8, 0), "8x0"), ((1, 2, 16385, 8), "16385x8"),
                                       ((1, 2, 8, 16385), "8x16385"), ((1, 0, 8, 8), "0 frames"), ((1, 65536, 8, 8), "65536 frames"),
                                       ((0, 2, 8, 8), "0 clips")])
def test_workspace_query_refuses_what_the_encoder_does_not_take(geom, word):
    rc, _, _, err = _query(*geom)
    assert rc != 0 and "vf_gif_workspace_bytes" in err and word in err, err
    with pytest.raises(ValueError, match=word):
        backend.gif_workspace_bytes(*geom)


@pytest.mark.parametrize("delay", [-1, 65536])
def test_encode_refuses_a_delay_out_of_range_before_it_needs_a_device(delay):
    lib = _lib.load()
    rc = lib.vf_gif_encode(None, None, 1, 1, 2, 8, 8, delay, None, 0, None, 0, None)
    err = lib.vf_last_error().decode()
    assert rc != 0 and "vf_gif_encode" in err and "delay of %d" % delay in err, err
    from video_filler_amd import data
    with pytest.raises(ValueError, match="delay=%d" % delay):
        data.encode_gif(np.zeros((2, 8, 8, 3), np.uint8), delay)


@pytest.mark.parametrize("geom", [(3, 37, 53), (2, 71, 59)])
def test_output_bound_covers_uniform_random_frames(geom):
    n, H, W = geom
    clip = np.stack([gif_cases.noise(H, W, seed=20 + i) for i in range(n)])
    size = len(gif_ref.encode(clip, 10))
    bound = backend.gif_workspace_bytes(1, n, H, W)[1]
    print("%dx%dx%d: %d bytes, bound %d" % (n, H, W, size, bound))
    assert size <= bound


def test_save_gifs_refuses_before_any_backend_exists(tmp_path):
    from video_filler_amd import inference
    x = np.zeros((1, 4, 4, 3), np.uint8)
    with pytest.raises(ValueError, match="predLen = 1"):
        inference.save_gifs(str(tmp_path / "d" / "clip"), x)
    x = np.zeros((3, 4, 4, 3), np.uint8)
    with pytest.raises(ValueError, match="result, result"):
        inference.save_gifs(str(tmp_path / "d" / "clip"), x, result=x)
    with pytest.raises(ValueError, match="nothing to save"):
        inference.save_gifs(str(tmp_path / "d" / "clip"))
    assert not (tmp_path / "d").exists()
