"""vf_jpeg_encode_workspace_bytes is a host-only entry: it answers, and refuses, without a GPU; data.encode_jpeg refuses
bad arguments before it touches the backend."""
import ctypes as C
import os

import numpy as np
import pytest

import video_filler_amd  # noqa: F401
from video_filler_amd import _lib, backend

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_encode_cases.npz")


def _query(n, H, W, Cc, sub):
    lib = _lib.load()
    ws, out = C.c_size_t(), C.c_size_t()
    rc = lib.vf_jpeg_encode_workspace_bytes(n, H, W, Cc, sub, C.byref(ws), C.byref(out))
    return rc, ws.value, out.value, lib.vf_last_error().decode()


def test_workspace_query_answers_without_a_gpu():
    rc, ws, out, _ = _query(120, 384, 512, 3, 2)
    assert rc == 0
    blocks = 24 * 32 * 6                                 # 16 x 16 MCUs of four luma and two chroma blocks
    assert out == 120 * (2 * 216 * blocks + 626)         # include/vf_hip.h has the derivation
    assert ws >= 120 * blocks * (128 + 216)              # the coefficients and the unstuffed stream
    assert _query(1, 1, 1, 1, 0)[0] == 0 and _query(1, 16384, 16384, 3, 0)[0] == 0 and _query(65535, 8, 8, 1, 7)[0] == 0
    assert backend.jpeg_encode_workspace_bytes(2, 8, 8, 3, "420")[1] == 2 * (2 * 216 * 6 + 626)
    assert backend.jpeg_encode_workspace_bytes(2, 8, 8, 3, "444")[1] == 2 * (2 * 216 * 3 + 626)


def test_the_output_bound_holds_every_golden_file():
    z = np.load(GOLD)
    for name in z["names"].tolist():
        H, W, Cc = z["frame/" + name].shape
        _, out = backend.jpeg_encode_workspace_bytes(1, H, W, Cc, str(z["sampling/" + name]))
        assert out >= z["file/" + name].size, name


@pytest.mark.parametrize("geom,word", [((1, 0, 8, 3, 2), "H = 0"), ((1, 8, 16385, 3, 2), "W = 16385"), ((1, 8, 8, 2, 2), "C = 2"),
                                       ((1, 8, 8, 3, 3), "subsampling = 3"), ((0, 8, 8, 3, 2), "n = 0"), ((65536, 8, 8, 1, 0), "n = 65536")])
def test_workspace_query_names_the_argument_it_refuses(geom, word):
    rc, _, _, err = _query(*geom)
    assert rc != 0 and "vf_jpeg_encode_workspace_bytes" in err and word in err, err


def test_encode_jpeg_refuses_bad_arguments_before_the_backend(monkeypatch):
    from video_filler_amd import data

    def no_backend():
        raise AssertionError("the backend was asked for")
    monkeypatch.setattr(data, "get_backend", no_backend)
    x = np.zeros((1, 8, 8, 3), np.uint8)
    for q in (0, 101, 75.0):
        with pytest.raises(ValueError, match="quality"):
            data.encode_jpeg(x, quality=q)
    with pytest.raises(ValueError, match="subsampling='411'"):
        data.encode_jpeg(x, subsampling="411")
    with pytest.raises(ValueError, match="3 dimensions"):
        data.encode_jpeg(x[0])
    with pytest.raises(ValueError, match="dtype"):
        data.encode_jpeg(x.astype(np.int32))
    with pytest.raises(ValueError, match="unknown|subsampling"):
        backend.jpeg_encode_workspace_bytes(1, 8, 8, 3, "411")
