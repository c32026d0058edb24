"""vf_jpeg_encode_prog_workspace_bytes is a host-only entry: it answers, and refuses, without a GPU; its bounds grow with the
batch and the frame and hold every golden file; vf_jpeg_encode_prog refuses bad arguments before it touches the context; the
Python entry points refuse a restart interval together with progressive=True before they touch the backend."""
import ctypes as C
import os

import numpy as np
import pytest

import video_filler_amd  # noqa: F401
from video_filler_amd import _lib, backend

import jpeg_enc_prog_ref


def _query(n, H, W, Cc, sub):
    lib = _lib.load()
    ws, out = C.c_size_t(), C.c_size_t()
    rc = lib.vf_jpeg_encode_prog_workspace_bytes(n, H, W, Cc, sub, C.byref(ws), C.byref(out))
    return rc, ws.value, out.value, lib.vf_last_error().decode()


def test_workspace_query_answers_without_a_gpu():
    blocks = 24 * 32 * 6                                 # 384 x 512 at 4:2:0: 24 x 32 MCUs of six blocks
    rc, ws, out, _ = _query(120, 384, 512, 3, 2)
    assert rc == 0 and out == 120 * (2 * (496 * blocks + 10) + 192 + 10 * 590 + 2)
    assert ws >= 120 * blocks * (128 + 496)              # the coefficients and the unstuffed stream
    assert (ws, out) == backend.jpeg_encode_prog_workspace_bytes(120, 384, 512, 3, "420")
    assert _query(1, 8, 8, 1, 0)[2] == 2 * (496 + 6) + 192 + 6 * 590 + 2
    assert _query(1, 8, 8, 1, 0)[2] == _query(1, 8, 8, 1, 2)[2]          # grey ignores the sampling
    # more room than the baseline encoder asks for the same batch
    assert out > backend.jpeg_encode_workspace_bytes(120, 384, 512, 3, "420")[1]


def test_the_bounds_are_monotone():
    last = (0, 0)
    for n in (1, 2, 3, 64, 65535):
        pair = _query(n, 37, 53, 3, 2)[1:3]
        assert pair[0] > last[0] and pair[1] > last[1]
        last = pair
    for axis in (0, 1):
        last = (0, 0)
        for side in (1, 8, 9, 16, 17, 100, 1000, 16384):
            H, W = (side, 40) if axis == 0 else (40, side)
            pair = _query(2, H, W, 3, 2)[1:3]
            assert pair[0] >= last[0] and pair[1] >= last[1], (axis, side)
            if side % 16 == 1:                           # a new row or column of MCUs
                assert pair[0] > last[0] and pair[1] > last[1]
            last = pair
    # 4:2:0 pads to more blocks than 4:4:4 never: whole MCUs of six against three blocks per 8 x 8 of luma
    assert _query(1, 64, 64, 3, 0)[2] > _query(1, 64, 64, 3, 1)[2] > _query(1, 64, 64, 3, 2)[2] > _query(1, 64, 64, 1, 0)[2]


def test_the_output_bound_holds_every_golden_file():
    z = np.load(jpeg_enc_prog_ref.GOLD)
    for name in z["names"].tolist():
        shape = z["frame/" + name].shape if "frame/" + name in z.files else jpeg_enc_prog_ref.FORMULAS[str(z["formula/" + name])]().shape
        _, out = backend.jpeg_encode_prog_workspace_bytes(1, *shape, str(z["sampling/" + name]))
        assert out >= z["file/" + name].size, name


GEOMETRY = [((1, 0, 8, 3, 2), "H = 0"), ((1, 8, 0, 3, 2), "W = 0"), ((1, 16385, 8, 3, 2), "H = 16385"), ((1, 8, 16385, 1, 2), "W = 16385"),
            ((1, 8, 8, 2, 2), "C = 2"), ((1, 8, 8, 3, 3), "subsampling = 3"), ((0, 8, 8, 3, 2), "n = 0")]


@pytest.mark.parametrize("geom,word", GEOMETRY)
def test_workspace_query_names_the_argument_it_refuses(geom, word):
    rc, _, _, err = _query(*geom)
    assert rc != 0 and "vf_jpeg_encode_prog_workspace_bytes" in err and word in err, err
    with pytest.raises(ValueError, match=word):
        backend._encoder_bytes("vf_jpeg_encode_prog_workspace_bytes", *geom)


def test_the_encode_entry_refuses_before_anything_else():
    """vf_jpeg_encode_prog with a null context: the checks run, and name the argument, before anything touches it"""
    lib = _lib.load()
    for geom, word in GEOMETRY:
        n, H, W, Cc, sub = geom
        rc = lib.vf_jpeg_encode_prog(None, None, 1, n, H, W, Cc, 75, sub, None, 0, None, 0, None)
        err = lib.vf_last_error().decode()
        assert rc != 0 and "vf_jpeg_encode_prog:" in err and word in err, err
    for q in (0, 101):
        rc = lib.vf_jpeg_encode_prog(None, None, 1, 1, 8, 8, 3, q, 2, None, 0, None, 0, None)
        err = lib.vf_last_error().decode()
        assert rc != 0 and "vf_jpeg_encode_prog:" in err and "quality = %d" % q in err, err
    rc = lib.vf_jpeg_encode_prog(None, None, 2, 1, 8, 8, 3, 75, 2, None, 0, None, 0, None)
    assert rc != 0 and "kind 2" in lib.vf_last_error().decode()
    rc = lib.vf_jpeg_encode_prog(None, None, 1, 1, 8, 8, 3, 75, 2, None, 0, None, 0, None)
    assert rc != 0 and "workspace holds 0 bytes" in lib.vf_last_error().decode()


def test_python_refuses_an_interval_in_a_progressive_file_before_the_backend(monkeypatch, tmp_path):
    from video_filler_amd import data, inference

    def no_backend(*a, **k):
        raise AssertionError("the backend was asked for")
    monkeypatch.setattr(data, "get_backend", no_backend)
    monkeypatch.setattr(inference, "display_tensor", no_backend)
    x = np.zeros((1, 8, 8, 3), np.uint8)
    for kw, word in ((dict(restart_rows=1), "restart_rows=1 with progressive=True"), (dict(restart_blocks=3), "restart_blocks=3 with progressive=True"),
                     (dict(restart_rows=2, restart_blocks=3), "restart_rows=2 with progressive=True")):
        with pytest.raises(ValueError, match="encode_jpeg: " + word):
            data.encode_jpeg(x, progressive=True, **kw)
        with pytest.raises(ValueError, match="display_jpeg: " + word):
            inference.display_jpeg(np.zeros((1, 3, 8, 8), np.float32), progressive=True, **kw)
        with pytest.raises(ValueError, match="save_frames_jpg: " + word):
            inference.save_frames_jpg(str(tmp_path / "d"), np.zeros((1, 3, 8, 8), np.float32), progressive=True, **kw)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="encode_jpeg: progressive=%r" % (bad,)):
            data.encode_jpeg(x, progressive=bad)
        with pytest.raises(ValueError, match="save_frames_jpg: progressive=%r" % (bad,)):
            inference.save_frames_jpg(str(tmp_path / "d"), np.zeros((1, 3, 8, 8), np.float32), progressive=bad)
    assert not os.path.exists(str(tmp_path / "d"))


def test_progressive_reaches_the_backend_and_optimize_is_accepted(monkeypatch):
    """a stub backend: encode_jpeg(progressive=True) asks for jpeg_encode with progressive set, with optimize on or off"""
    from video_filler_amd import data
    calls = []

    class Stub:
        def from_host(self, t):
            return t

        def jpeg_encode(self, frames, quality, subsampling, restart_rows, restart_blocks, optimize, progressive):
            calls.append((quality, subsampling, restart_rows, restart_blocks, optimize, progressive))
            raise RuntimeError("stub")
    monkeypatch.setattr(data, "get_backend", lambda: Stub())
    x = np.zeros((1, 8, 8, 3), np.uint8)
    for kw in (dict(progressive=True), dict(progressive=True, optimize=True), dict()):
        with pytest.raises(RuntimeError, match="stub"):
            data.encode_jpeg(x, 80, "422", **kw)
    assert calls == [(80, "422", 0, 0, 0, 1), (80, "422", 0, 0, 1, 1), (80, "422", 0, 0, 0, 0)]
