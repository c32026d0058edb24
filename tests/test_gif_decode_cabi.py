"""The host-only entries of the GIF decoder (vf_gif_inspect, vf_gif_decode_workspace_bytes) against the
definition's metadata (tests/gif_decode_ref.py) on every fixture of tests/gif_decode_cases.py.  No GPU."""
import os
import re

import pytest

import gif_decode_cases as cases
import gif_decode_ref as R

import video_filler_amd  # noqa: F401
from video_filler_amd import backend, data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_inspect_equals_the_reference_metadata_on_every_fixture():
    seen = 0
    for name, c in sorted(cases.fixtures().items()):
        if c.kind == "malformed":
            continue
        want = R.parse(c.data)
        got = backend.gif_inspect(c.data)
        for k in ("width", "height", "frames", "loop", "global_table_size", "version", "supported", "reason"):
            assert got[k] == want[k], (name, k, got[k], want[k])
        assert got["frame_info"] == want["frame_info"], name
        assert got["rect_pixels"] == sum(f["w"] * f["h"] for f in want["frame_info"])
        assert got["supported"] == (c.kind != "unsupported")
        assert tuple(got["frame_info"][0]) == R.FRAME_KEYS == backend.GIF_FRAME_KEYS
        seen += 1
    assert seen == len(cases.fixtures()) - len(cases.of_kind("malformed")) == 45
    info = data.gif_info(cases.fixtures()["hand/extensions"].data)
    assert (info["loop"], info["frames"], info["version"]) == (7, 2, 89)
    assert [f["delay"] for f in info["frame_info"]] == [7, 9] and [f["transparency"] for f in info["frame_info"]] == [-1, 2]
    assert data.gif_info(cases.fixtures()["hand/screen_3x5_87a"].data)["loop"] == -1


def test_frame_rows_stop_at_frame_cap():
    import ctypes as C
    import numpy as np
    from video_filler_amd import _lib
    lib = _lib.load()
    d = cases.fixtures()["hand/frames_70"].data
    info = (C.c_int64 * 8)()
    rows = np.full((6, 12), -7, np.int64)
    assert lib.vf_gif_inspect(d, len(d), info, rows.ctypes.data_as(C.c_void_p), 5, None, 0) == 0
    assert info[2] == 70 and (rows[5] == -7).all() and (rows[:5, 4] > 0).all()
    assert lib.vf_gif_inspect(d, len(d), None, None, 0, None, 0) != 0 and b"NULL" in lib.vf_last_error()


def test_malformed_files_fail_and_unsupported_ones_say_why():
    for name in cases.of_kind("malformed"):
        c = cases.fixtures()[name]
        with pytest.raises(ValueError, match=re.escape(c.what)):
            backend.gif_inspect(c.data)
        with pytest.raises(ValueError, match=re.escape(c.what)):
            data.gif_info(c.data)
    for name in cases.of_kind("unsupported"):
        c = cases.fixtures()[name]
        info = backend.gif_inspect(c.data)
        assert not info["supported"] and c.what in info["reason"]


def test_workspace_bytes_refuses_with_the_file_named():
    good = cases.fixtures()["hand/rects_d01"].data
    ws, stage = backend.gif_decode_workspace_bytes([good, good])
    assert 0 < stage < ws and ws % 256 == 0 and stage % 256 == 0
    assert backend.gif_decode_workspace_bytes([good, good], alpha=True) == (ws, stage)
    for name in cases.of_kind("malformed") + cases.of_kind("unsupported"):
        c = cases.fixtures()[name]
        with pytest.raises(ValueError, match=r"image 2: .*" + re.escape(c.what)):
            backend.gif_decode_workspace_bytes([good, good, c.data, good])
    with pytest.raises(ValueError, match="image 1: unsupported"):
        backend.gif_decode_workspace_bytes([good, cases.fixtures()["hand/wide_16385"].data])
    for name in cases.of_kind("corrupt"):                     # the headers are sound: the stream is the device's to judge
        assert backend.gif_decode_workspace_bytes([cases.fixtures()[name].data])[0] > 0


def test_constants_mirror_the_source():
    src = open(os.path.join(ROOT, "video-filler_amd", "csrc", "vf_gif_decode.hip")).read()
    assert int(re.search(r"constexpr int kTok = (\d+);", src).group(1)) == backend.GIF_DECODE_TOKENS == cases.TOKENS
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vf_hip.h")).read(), flags=re.S)
    enum = dict((k, int(v)) for k, v in re.findall(r"VF_GIF_(\w+) = (\d+)", hdr))
    assert enum == {"OK": R.OK, "BAD_CODE": R.BAD_CODE, "SHORT_DATA": R.SHORT_DATA, "BAD_INDEX": R.BAD_INDEX}
    assert backend.GIF_STATUS == {0: "ok", **R.STATUS_WORD}
