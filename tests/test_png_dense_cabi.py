"""The level entries of the PNG and APNG encoders (vf_png_encode_level, vf_apng_encode_level) are exported
and bound, refuse a bad level by name before they touch the device, and leave the workspace queries as they were."""
import ctypes as C

import pytest

import video_filler_amd  # noqa: F401
from video_filler_amd import _lib, backend

PNG_ARGS = (1, 2, 8, 8, 3)                    # kind, n, H, W, C
APNG_ARGS = (1, 1, 2, 8, 8, 3, 10, 0)         # kind, g, n, H, W, C, delay, loop


def test_level_entries_are_exported_bound_and_declared():
    lib = _lib.load()
    for name in ("vf_png_encode_level", "vf_apng_encode_level"):
        assert hasattr(lib, name) and name in _lib.header_symbols()
        assert getattr(lib, name).argtypes is not None and C.c_int32 in getattr(lib, name).argtypes
    assert len(lib.vf_png_encode_level.argtypes) == len(lib.vf_png_encode.argtypes) + 1
    assert len(lib.vf_apng_encode_level.argtypes) == len(lib.vf_apng_encode.argtypes) + 1
    assert backend.PNG_LEVELS == (0, 1) and backend.PNG_HIST == backend.PNG_CHUNK == 8192


@pytest.mark.parametrize("level", [2, -1, 9])
def test_a_bad_level_is_refused_before_the_device_is_touched(level):
    lib = _lib.load()
    rc = lib.vf_png_encode_level(None, None, *PNG_ARGS, level, None, 0, None, 0, None)
    err = lib.vf_last_error().decode()
    assert rc != 0 and "vf_png_encode_level" in err and "level" in err and str(level) in err, err
    rc = lib.vf_apng_encode_level(None, None, *APNG_ARGS, level, None, 0, None, 0, None)
    err = lib.vf_last_error().decode()
    assert rc != 0 and "vf_apng_encode_level" in err and "level" in err and str(level) in err, err
    for who in ("png_encode", "encode_apng"):
        with pytest.raises(ValueError, match="level"):
            backend.png_level(who, level)
    for bad in (True, 1.0, "1", None):
        with pytest.raises(ValueError, match="level"):
            backend.png_level("encode_png", bad)


@pytest.mark.parametrize("level", [0, 1])
def test_a_good_level_goes_on_to_the_checks_of_the_plain_entries(level):
    """the geometry, kind and buffer checks are the plain entries', under the level entry's name"""
    lib = _lib.load()
    for args, word in (((1, 2, 8, 8, 2), "2 channels"), ((1, 2, 0, 8, 3), "0x8"), ((7, 2, 8, 8, 3), "kind 7"), (PNG_ARGS, "workspace")):
        rc = lib.vf_png_encode_level(None, None, *args, level, None, 0, None, 0, None)
        err = lib.vf_last_error().decode()
        assert rc != 0 and "vf_png_encode_level" in err and word in err, err
    for args, word in (((1, 1, 2, 8, 8, 2, 10, 0), "2 channels"), ((1, 1, 2, 8, 8, 3, 70000, 0), "delay"), (APNG_ARGS, "workspace")):
        rc = lib.vf_apng_encode_level(None, None, *args, level, None, 0, None, 0, None)
        err = lib.vf_last_error().decode()
        assert rc != 0 and "vf_apng_encode_level" in err and word in err, err
    rc = lib.vf_png_encode(None, None, *PNG_ARGS, None, 0, None, 0, None)
    assert rc != 0 and "vf_png_encode:" in lib.vf_last_error().decode()


def test_workspace_queries_hold_for_both_levels_and_refuse_what_they_refused():
    lib = _lib.load()
    ws, out = C.c_size_t(), C.c_size_t()
    assert lib.vf_png_workspace_bytes(120, 384, 512, 3, C.byref(ws), C.byref(out)) == 0
    stream = 384 * (512 * 3 + 1)
    chunks = -(-stream // backend.PNG_CHUNK)
    assert out.value == 120 * (stream + 17 * chunks + 8 + 25 + 6 + 12)
    assert ws.value == backend.png_workspace_bytes(120, 384, 512, 3)[0]
    for geom, word in (((1, 8, 8, 2), "2 channels"), ((1, 16385, 8, 3), "16385x8"), ((0, 8, 8, 3), "0 frames")):
        assert lib.vf_png_workspace_bytes(*geom, C.byref(ws), C.byref(out)) != 0
        assert word in lib.vf_last_error().decode()
    assert lib.vf_apng_workspace_bytes(1, 2, 8, 8, 3, 70000, 0, C.byref(ws), C.byref(out)) != 0
    assert "delay" in lib.vf_last_error().decode()


def test_save_frames_refuses_a_bad_level_before_the_directory_is_made(tmp_path):
    import numpy as np
    from video_filler_amd import inference
    x = np.zeros((1, 4, 4, 3), np.uint8)
    for fn, args in ((inference.save_frames, (str(tmp_path / "d"), x)), (inference.save_apngs, (str(tmp_path / "e" / "clip"), x))):
        with pytest.raises(ValueError, match="level"):
            fn(*args, level=2)
    assert not (tmp_path / "d").exists() and not (tmp_path / "e").exists()
