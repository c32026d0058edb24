"""vf_jpeg_encode_opts_workspace_bytes is a host-only entry: it answers, and refuses, without a GPU; with every option off it is
vf_jpeg_encode_workspace_bytes; its output bound holds every golden file; the Python entry points refuse bad options before
they touch the backend."""
import ctypes as C
import os

import numpy as np
import pytest

import video_filler_amd  # noqa: F401
from video_filler_amd import _lib, backend

import jpeg_enc_opts_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_encode_opts_cases.npz")


def _query(n, H, W, Cc, sub, rr, rb, opt):
    lib = _lib.load()
    ws, out = C.c_size_t(), C.c_size_t()
    rc = lib.vf_jpeg_encode_opts_workspace_bytes(n, H, W, Cc, sub, rr, rb, opt, C.byref(ws), C.byref(out))
    return rc, ws.value, out.value, lib.vf_last_error().decode()


def test_workspace_query_answers_without_a_gpu():
    blocks = 24 * 32 * 6                                 # 384 x 512 at 4:2:0: 24 x 32 MCUs of six blocks
    for geom in ((120, 384, 512, 3, 2), (1, 1, 1, 1, 0), (3, 37, 53, 3, 0)):
        rc, ws, out, _ = _query(*geom, 0, 0, 0)
        assert rc == 0 and (ws, out) == backend.jpeg_encode_workspace_bytes(*geom[:4], ("444", "422", "420")[geom[4]])
    ws0, out0 = _query(120, 384, 512, 3, 2, 0, 0, 0)[1:3]
    assert out0 == 120 * (2 * 216 * blocks + 626)
    # an interval: DRI and four bytes per segment in the bound, 16 bytes per segment in the workspace
    rc, ws, out, _ = _query(120, 384, 512, 3, 2, 1, 0, 0)
    assert rc == 0 and out == 120 * (2 * 216 * blocks + 626 + 4 * 24 + 6) and ws >= ws0 + 120 * 24 * 16
    assert _query(120, 384, 512, 3, 2, 1, 7, 0)[2] == out                      # rows win
    assert _query(120, 384, 512, 3, 2, 0, 1, 0)[2] == 120 * (2 * 216 * blocks + 626 + 4 * 768 + 6)
    assert _query(120, 384, 512, 3, 2, 0, 65535, 0)[2] == 120 * (2 * 216 * blocks + 626 + 4 + 6)     # DRI, one segment
    assert _query(1, 264, 16384, 1, 0, 32, 0, 0)[2] == 2 * 216 * 33 * 2048 + 626 + 4 * 2 + 6          # the clamp: two segments
    # optimize: the bound stays, the workspace holds the counters (4 x 256 x 4 bytes), the code table and the DHT segments
    rc, ws, out, _ = _query(120, 384, 512, 3, 2, 0, 0, 1)
    assert rc == 0 and out == out0 and ws >= ws0 + 120 * (4096 + 4 * (2 * 12 + 2 * 256) + 4 * 277)
    assert backend.jpeg_encode_opts_workspace_bytes(2, 8, 8, 3, "444", restart_blocks=1)[1] == 2 * (2 * 216 * 3 + 626 + 4 + 6)
    assert backend.jpeg_encode_opts_workspace_bytes(2, 8, 8, 3, "444", optimize=True)[1] == 2 * (2 * 216 * 3 + 626)


def test_the_output_bound_holds_every_golden_file():
    z = np.load(GOLD)
    for name in z["names"].tolist():
        shape = z["frame/" + name].shape if "frame/" + name in z.files else getattr(jpeg_enc_opts_ref, str(z["formula/" + name]))().shape
        _, rr, rb, opt = (int(v) for v in z["options/" + name])
        _, out = backend.jpeg_encode_opts_workspace_bytes(1, *shape, str(z["sampling/" + name]), rr, rb, bool(opt))
        assert out >= z["file/" + name].size, name


@pytest.mark.parametrize("opts,word", [((-1, 0, 0), "restart_rows = -1"), ((65536, 0, 0), "restart_rows = 65536"),
                                       ((0, -1, 0), "restart_blocks = -1"), ((0, 65536, 0), "restart_blocks = 65536"),
                                       ((1, 65536, 0), "restart_blocks = 65536"), ((0, 0, 2), "optimize = 2"),
                                       ((0, 0, -1), "optimize = -1")])
def test_workspace_query_names_the_option_it_refuses(opts, word):
    rc, _, _, err = _query(1, 8, 8, 3, 2, *opts)
    assert rc != 0 and "vf_jpeg_encode_opts_workspace_bytes" in err and word in err, err


def test_workspace_query_still_names_the_geometry_it_refuses():
    for geom, word in (((1, 0, 8, 3, 2), "H = 0"), ((1, 8, 8, 2, 2), "C = 2"), ((1, 8, 8, 3, 3), "subsampling = 3"), ((0, 8, 8, 3, 2), "n = 0")):
        rc, _, _, err = _query(*geom, 1, 0, 1)
        assert rc != 0 and "vf_jpeg_encode_opts_workspace_bytes" in err and word in err, err


def test_the_encode_entry_refuses_options_before_anything_else():
    """vf_jpeg_encode_opts with a null context: the checks run, and name the argument, before anything touches it."""
    lib = _lib.load()
    for opts, word in (((70000, 0, 0), "restart_rows = 70000"), ((0, 70000, 0), "restart_blocks = 70000"), ((0, 0, 3), "optimize = 3")):
        rc = lib.vf_jpeg_encode_opts(None, None, 1, 1, 8, 8, 3, 75, 2, *opts, None, 0, None, 0, None)
        err = lib.vf_last_error().decode()
        assert rc != 0 and "vf_jpeg_encode_opts:" in err and word in err, err


def test_python_refuses_bad_options_before_the_backend(monkeypatch, tmp_path):
    from video_filler_amd import data, inference

    def no_backend(*a, **k):
        raise AssertionError("the backend was asked for")
    monkeypatch.setattr(data, "get_backend", no_backend)
    monkeypatch.setattr(inference, "display_tensor", no_backend)
    x = np.zeros((1, 8, 8, 3), np.uint8)
    for kw, word in ((dict(restart_rows=-1), "restart_rows=-1"), (dict(restart_rows=65536), "restart_rows=65536"),
                     (dict(restart_blocks=65536), "restart_blocks=65536"), (dict(restart_blocks=1.0), "restart_blocks=1.0"),
                     (dict(restart_rows=True), "restart_rows=True"), (dict(optimize=1), "optimize=1"),
                     (dict(optimize="yes"), "optimize='yes'")):
        with pytest.raises(ValueError, match="encode_jpeg: " + word):
            data.encode_jpeg(x, **kw)
        with pytest.raises(ValueError, match="display_jpeg: " + word):
            inference.display_jpeg(np.zeros((1, 3, 8, 8), np.float32), **kw)
        with pytest.raises(ValueError, match=word):
            inference.save_frames_jpg(str(tmp_path / "d"), np.zeros((1, 3, 8, 8), np.float32), **kw)
    assert not os.path.exists(str(tmp_path / "d"))
    with pytest.raises(ValueError, match="restart_blocks = 65536"):
        backend.jpeg_encode_opts_workspace_bytes(1, 8, 8, 3, "420", restart_blocks=65536)
