"""The host side of decode_jpeg(layouts=True) through the C-ABI, no GPU: vf_jpeg_inspect_layouts against
the Python parse of tests/jpeg_layouts_ref.py, the refusals (and the unchanged ones of vf_jpeg_inspect for the same
bytes), vf_jpeg_layouts_coefficients_host (the device's own decode functions, run on the host) against the Python rule
on every fixture, and damaged copies of three fixtures: every one ends in a status or a parse error and leaves the guard
bands around the coefficient buffer untouched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import jpeg_layouts_ref as R
import video_filler_amd  # noqa: F401
from video_filler_amd import _lib, data
from video_filler_amd.backend import (jpeg_inspect, jpeg_inspect_layouts, jpeg_layouts_coefficients, jpeg_layouts_workspace_bytes,
                                      jpeg_prog_coefficients, jpeg_scans_inspect)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "jpeg_layouts_cases.npz"))
NAMES = sorted(k[4:] for k in GOLDEN.files if k.startswith("jpg/"))
DAMAGED = ["scans_y_cb_cr_420_37x53_drichange", "410_17x33_smooth_q100", "prog_411_32x32"]


def _file(name):
    return GOLDEN["jpg/" + name].tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_inspect_equals_the_parse(name):
    f = _file(name)
    info, P = jpeg_inspect_layouts(f), R.parse(f)
    assert info["supported"] and info["reason"] == "" and info["sof"] == P["sof"] and info["precision"] == 8
    assert (info["height"], info["width"]) == GOLDEN["ref/" + name].shape[:2] == (P["height"], P["width"])
    assert info["components"] == len(P["comps"]) and info["sampling"] == [(c[1], c[2]) for c in P["comps"]]
    assert info["colour"] == P["colour"] and info["scans"] == len(P["scans"])
    hs, vs, mcux, mcuy, _, _ = R.PR.geometry(P)
    assert info["blocks_per_mcu"] == sum(h * v for h, v in zip(hs, vs)) and info["blocks"] == mcux * mcuy * info["blocks_per_mcu"]
    assert info["levels"] == (3 if P["sof"] == 0xC2 else 1)         # every scan of a sequential file is a first scan
    assert data.jpeg_info(f, layouts=True) == info


# the default inspector's word on the same bytes: today's reasons
OLD_REASON = (("440_", "(4:4:4, 4:2:2 and 4:2:0 only)"), ("411_", "(4:4:4, 4:2:2 and 4:2:0 only)"), ("11_22_22_", "4:2:0 only"),
              ("rgb_adobe0_sub0", "RGB colour transform (Adobe transform 0)"), ("rgb_ids_sub0", "RGB components"),
              ("scans_y_cb_cr_444", "multi-scan sequential"), ("scans_ycb_cr_420", "multi-scan sequential"),
              ("sof1_slots23_420", "one beyond baseline's two"), ("prog_", "progressive"))


@pytest.mark.parametrize("prefix,why", OLD_REASON)
def test_default_inspector_keeps_its_reasons(prefix, why):
    hit = [n for n in NAMES if n.startswith(prefix)]
    assert hit
    for n in hit:
        info = jpeg_inspect(_file(n))
        assert not info["supported"] and why in info["reason"], (n, info["reason"])
    if prefix == "prog_":
        for n in hit:                                               # and the progressive entry keeps its own
            info = jpeg_scans_inspect(_file(n))
            assert not info["supported"] and ("4:2:0 only" in info["reason"] or "RGB" in info["reason"]), (n, info["reason"])
            with pytest.raises(ValueError):
                jpeg_prog_coefficients(_file(n))


def test_ordinary_files_are_supported_too():
    for z in ("jpeg_cases.npz", "jpeg_progressive_cases.npz"):
        g = np.load(os.path.join(HERE, "golden", z))
        for k in g.files:
            if k.startswith("jpg/"):
                info = jpeg_inspect_layouts(g[k].tobytes())
                assert info["supported"], (k, info["reason"])


def test_refusals():
    good = _file(NAMES[0])
    for key, why in (("fractional", r"sampling 3x1,2x1,1x1 \(fractional"), ("blocks18", r"sampling 4x4,1x1,1x1 \(18 blocks"),
                     ("missing", "incomplete: component 2 is in no scan"), ("cmyk", "4 components")):
        f = GOLDEN["bad/" + key].tobytes()
        info = jpeg_inspect_layouts(f)
        assert not info["supported"] and re.search(why, info["reason"]), (key, info["reason"])
        with pytest.raises(ValueError, match="vf_jpeg_layouts: image 1: unsupported: .*" + why):
            jpeg_layouts_workspace_bytes([good, f])
        with pytest.raises(ValueError, match=why):
            jpeg_layouts_coefficients(f)
    twice = GOLDEN["bad/twice"].tobytes()
    with pytest.raises(ValueError, match="scan 2: component 1 is coded in two scans"):
        jpeg_inspect_layouts(twice)
    with pytest.raises(ValueError, match="vf_jpeg_layouts: image 2: scan 2: component 1 is coded in two scans"):
        jpeg_layouts_workspace_bytes([good, good, twice])
    ws, st = jpeg_layouts_workspace_bytes([good, _file(NAMES[-1])])
    assert ws > st > 0
    # baseline (SOF0) keeps its two table slots; SOF1 has four
    f = bytearray(_file("sof1_slots23_420_37x53"))
    f[f.index(b"\xff\xc1") + 1] = 0xC0
    info = jpeg_inspect_layouts(bytes(f))
    assert not info["supported"] and "one beyond baseline's two" in info["reason"]


@pytest.mark.parametrize("name", NAMES)
def test_host_coefficients_equal_the_rule(name):
    f = _file(name)
    want = R.mcu_layout(f, R.coefficients(f)[0])
    for sub in (0, 16):              # walked in order; synchronised over subsequences of 16 bytes, as the device does
        got, status = jpeg_layouts_coefficients(f, subseq_bytes=sub)
        assert status == 0, sub
        np.testing.assert_array_equal(got, want, err_msg="subseq_bytes=%d" % sub)


def _guarded(f):
    """vf_jpeg_layouts_coefficients_host into a buffer with a guard band on either side, both ways -> (return code,
    status) of the in-order walk, or None for a file the parse refuses; the guard bands must be intact."""
    lib = _lib.load()
    try:
        info = jpeg_inspect_layouts(f)
    except ValueError:
        return None
    if not info["supported"]:
        return None
    blocks, guard = info["blocks"], 4096
    res = []
    for sub in (0, 16):
        buf = np.full(2 * guard + 64 * blocks, 0x5A5A, np.int16)
        status = C.c_int32(-1)
        rc = lib.vf_jpeg_layouts_coefficients_host(f, len(f), sub, C.c_void_p(buf.ctypes.data + 2 * guard), blocks, C.byref(status))
        assert (buf[:guard] == 0x5A5A).all() and (buf[-guard:] == 0x5A5A).all()
        assert rc == 0 and status.value in (0, 1, 2)
        res.append(status.value)
    assert (res[0] != 0) == (res[1] != 0), res
    return res[0]


@pytest.mark.parametrize("name", DAMAGED)
def test_truncated_copies_end_in_a_status_or_a_parse_error(name):
    f = _file(name)
    scans = R.parse(f)["scans"]
    for s in scans:
        for keep in (0.0, 0.5, 0.95):
            mid = s["begin"] + int((s["end"] - s["begin"]) * keep)
            while f[mid - 1] == 0xFF:
                mid -= 1
            st = _guarded(f[:mid] + f[s["end"]:])                   # this scan cut short, the later ones kept
            assert st is None or st in (1, 2), (s["components"], keep, st)
    assert _guarded(f[:scans[-1]["begin"] + 3]) in (None, 1, 2)     # the file cut off, no EOI


@pytest.mark.parametrize("name", DAMAGED)
@pytest.mark.parametrize("seed", range(8))
def test_bit_flipped_copies_end_in_a_status_or_the_rule(name, seed):
    f = bytearray(_file(name))
    scans = R.parse(bytes(f))["scans"]
    s = scans[seed % len(scans)]
    rng = np.random.default_rng(seed)
    for at in rng.integers(s["begin"] + 1, s["end"], 6):
        if f[at] == 0xFF or f[at - 1] == 0xFF:
            continue
        f[at] = (f[at] ^ (1 << int(rng.integers(0, 7)))) & 0x7F      # never a new 0xFF: the marker structure stays
    f = bytes(f)
    st = _guarded(f)
    if st == 0:                      # damage that is valid data to any decoder: then it is the rule's data too
        np.testing.assert_array_equal(jpeg_layouts_coefficients(f)[0], R.mcu_layout(f, R.coefficients(f)[0]))


def test_room_for_the_coefficients_is_checked():
    f = _file(NAMES[0])
    lib = _lib.load()
    blocks = jpeg_inspect_layouts(f)["blocks"]
    buf = np.zeros(64 * blocks, np.int16)
    st = C.c_int32(0)
    assert lib.vf_jpeg_layouts_coefficients_host(f, len(f), 0, buf.ctypes.data_as(C.c_void_p), blocks - 1, C.byref(st)) != 0
    assert b"room for" in lib.vf_last_error()
