"""The host side of the progressive JPEG decoder through the C-ABI, no GPU: vf_jpeg_scans_inspect against
the Python parse of tests/jpeg_prog_ref.py, the refusals, vf_jpeg_prog_coefficients_host (the device's own decode
functions, run on the host) against the Python rule on every fixture, and a corruption matrix on that host entry: every
case ends in a status and leaves the guard bands around the coefficient buffer untouched."""
import ctypes as C
import os

import numpy as np
import pytest

import jpeg_prog_ref as R
import video_filler_amd  # noqa: F401
from video_filler_amd import _lib, data
from video_filler_amd.backend import jpeg_inspect, jpeg_prog_coefficients, jpeg_prog_workspace_bytes, jpeg_scans_inspect

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_progressive_cases.npz"))
NAMES = sorted(k[4:] for k in GOLDEN.files if k.startswith("jpg/"))
BIG = "420_360x480_photo_q90_none"


def _file(name):
    return GOLDEN["jpg/" + name].tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_scans_inspect_equals_the_parse(name):
    f = _file(name)
    info, P = jpeg_scans_inspect(f), R.parse(f)
    assert info["supported"] and info["reason"] == "" and info["sof"] == 0xC2 and info["precision"] == 8
    assert (info["height"], info["width"]) == GOLDEN["ref/" + name].shape[:2] == (P["height"], P["width"])
    gray = len(P["comps"]) == 1
    assert info["components"] == (1 if gray else 3) and len(info["scans"]) == (6 if gray else 10)
    hs, vs, mcux, mcuy, bw, bh = R.geometry(P)
    assert (info["h_samp"], info["v_samp"]) == (hs[0], vs[0])
    assert info["blocks_per_mcu"] == sum(h * v for h, v in zip(hs, vs)) and info["blocks"] == mcux * mcuy * info["blocks_per_mcu"]
    for got, want in zip(info["scans"], P["scans"]):
        for k in ("components", "Ss", "Se", "Ah", "Al", "restart_interval", "begin", "end"):
            assert got[k] == want[k], (k, got, {x: want[x] for x in got if x in want})
        assert got["segments"] == len(want["segments"])
        assert got["units"] == len(R.scan_units(P, want))
        if want["restart_interval"]:
            assert got["segments"] == -(-got["units"] // want["restart_interval"])
    assert data.jpeg_scans(f) == info["scans"]
    # libjpeg's default script in its own order has 3 levels; so have the permuted files
    assert info["levels"] == 3 and sorted({s["level"] for s in info["scans"]}) == [0, 1, 2]
    assert not jpeg_inspect(f)["supported"] and jpeg_inspect(f)["reason"] == "progressive"   # the baseline inspector stays


def test_restart_rows_change_the_interval_between_scans():
    info = jpeg_scans_inspect(_file("420_127x129_smooth_q100_r1"))
    assert len({s["restart_interval"] for s in info["scans"]}) > 1
    assert all(s["segments"] > 1 for s in info["scans"])


def test_levels_of_the_default_script():
    s = jpeg_scans_inspect(_file(BIG))["scans"]
    assert [x["level"] for x in s] == [0, 0, 0, 0, 0, 1, 1, 1, 1, 2]
    g = jpeg_scans_inspect(_file("L_7x9_noise_q5_none"))["scans"]
    assert [x["level"] for x in g] == [0, 0, 0, 1, 1, 2]


def test_refusals():
    for key, why in (("incomplete", "incomplete progression"), ("disorder", "progression out of order"), ("cmyk", "4 components")):
        f = GOLDEN["bad/" + key].tobytes()
        info = jpeg_scans_inspect(f)
        assert not info["supported"] and why in info["reason"], (key, info["reason"])
        with pytest.raises(ValueError, match="image 0: unsupported: .*" + why):
            jpeg_prog_workspace_bytes([f])
        with pytest.raises(ValueError, match=why):
            jpeg_prog_coefficients(f)
    with pytest.raises(ValueError, match=r"scan 5: bad progression parameters .*Ah=3 Al=1"):
        jpeg_scans_inspect(GOLDEN["bad/badsos"].tobytes())
    with pytest.raises(ValueError, match="image 1: scan 5: bad progression"):
        jpeg_prog_workspace_bytes([_file(NAMES[0]), GOLDEN["bad/badsos"].tobytes()])
    base = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz"))
    info = jpeg_scans_inspect(base["jpg/420_7x9_checker_q100_r1"].tobytes())
    assert not info["supported"] and info["reason"] == "not progressive" and info["scans"] == []


def _sos(f, k):
    """offset of the k-th SOS marker"""
    P = R.parse(f)
    return f.rindex(b"\xff\xda", 0, P["scans"][k]["begin"])


def test_malformed_scan_headers():
    f = _file("420_8x8_smooth_q5_none")
    for k, (off, val, what) in {1: (8, 64, "Se=64"), 2: (7, 0, "Ss=0 Se=63"), 5: (9, 0x2E, "Al=14"), 4: (7, 70, "Ss=70")}.items():
        b = bytearray(f)
        b[_sos(f, k) + off] = val
        with pytest.raises(ValueError, match="scan %d: bad progression parameters .*%s" % (k, what)):
            jpeg_scans_inspect(bytes(b))
    b = bytearray(f)
    b[_sos(f, 1) + 6] = 0x03          # AC slot 3: never defined
    with pytest.raises(ValueError, match="scan 1: names AC Huffman table 3"):
        jpeg_scans_inspect(bytes(b))
    b = bytearray(f)
    b[_sos(f, 6) + 6] = 0x33          # a DC refinement scan reads no table: any slot will do
    assert jpeg_scans_inspect(bytes(b))["supported"]
    # an interleaved AC scan: Ss > 0 with two components
    s0 = _sos(f, 0)
    b = bytearray(f)
    b[s0 + 4 + 2 * 3 + 1] = 1         # Ss of the 3-component DC scan
    b[s0 + 4 + 2 * 3 + 2] = 5
    with pytest.raises(ValueError, match="scan 0: bad progression parameters .*with 3 components"):
        jpeg_scans_inspect(bytes(b))


@pytest.mark.parametrize("name", NAMES)
def test_host_coefficients_equal_the_rule(name):
    f = _file(name)
    coef, _, _ = R.coefficients(f)
    want = R.mcu_layout(f, coef)
    for sub in (0, 8, 16, 1024):     # walked in order; the first scans synchronised over subsequences of 8, 16, 1024 bytes
        got, status = jpeg_prog_coefficients(f, subseq_bytes=sub)
        assert status == 0, sub
        np.testing.assert_array_equal(got, want, err_msg="subseq_bytes=%d" % sub)


def _guarded(f):
    """vf_jpeg_prog_coefficients_host into a buffer with a guard band on either side, twice: every scan walked in order,
    and the first scans synchronised over 16-byte subsequences.  -> (return code, status, intact) of the walk; the other
    way must agree on all but the status word itself (which lane meets the damage first decides between 1 and 2)."""
    lib = _lib.load()
    blocks, guard = jpeg_scans_inspect(f)["blocks"], 4096
    res = []
    for sub in (0, 16):
        buf = np.full(2 * guard + 64 * blocks, 0x5A5A, np.int16)
        status = C.c_int32(-1)
        rc = lib.vf_jpeg_prog_coefficients_host(f, len(f), sub, C.c_void_p(buf.ctypes.data + 2 * guard), blocks, C.byref(status))
        res.append((rc, status.value, bool((buf[:guard] == 0x5A5A).all() and (buf[-guard:] == 0x5A5A).all())))
    assert res[0][0] == res[1][0] and res[0][2] == res[1][2] and (res[0][1] != 0) == (res[1][1] != 0) and res[1][1] in (0, 1, 2), res
    return res[0]


def _cut_scan(f, k, keep):
    """the file with scan k's entropy-coded data cut down to its first `keep` of it (a fraction), the later scans kept"""
    s = R.parse(f)["scans"][k]
    mid = s["begin"] + int((s["end"] - s["begin"]) * keep)
    while f[mid - 1] == 0xFF:
        mid -= 1
    return f[:mid] + f[s["end"]:]


@pytest.mark.parametrize("scan,kind", [(0, "DC first"), (1, "AC first"), (4, "AC first"), (5, "AC refine"), (6, "DC refine"), (9, "AC refine")])
@pytest.mark.parametrize("keep", [0.0, 0.5, 0.97])
def test_truncation_inside_a_scan_ends_in_a_status(scan, kind, keep):
    rc, status, intact = _guarded(_cut_scan(_file(BIG), scan, keep))
    assert rc == 0 and status in (1, 2) and intact, (kind, rc, status, intact)


def test_truncated_file_ends_in_short_data():
    f = _file(BIG)
    s = R.parse(f)["scans"][9]
    rc, status, intact = _guarded(f[:s["begin"] + 100])     # no EOI either: libjpeg supplies one
    assert rc == 0 and status == 2 and intact


@pytest.mark.parametrize("scan", [5, 7, 8, 9])
def test_flipped_bytes_at_the_head_of_a_refinement_scan(scan):
    """The first thing an AC refinement scan reads is a Huffman symbol (the EOB run starts at 0), and no JPEG table
    assigns the all-ones code of any length (jpeg_make_d_derived_tbl refuses one that does).  With the scan's first four
    bytes flipped to FF 00 FF 00 — sixteen one-bits after unstuffing — that symbol is a bad code, whatever the table."""
    f = bytearray(_file(BIG))
    s = R.parse(bytes(f))["scans"][scan]
    assert s["Ah"] > 0 and s["Ss"] > 0 and s["end"] - s["begin"] > 8
    f[s["begin"]:s["begin"] + 4] = b"\xff\x00\xff\x00"
    rc, status, intact = _guarded(bytes(f))
    assert rc == 0 and status == 1 and intact


@pytest.mark.parametrize("scan", [5, 7, 9])
@pytest.mark.parametrize("seed", range(6))
def test_flipped_bytes_inside_a_refinement_scan(scan, seed):
    """Random damage further in.  A flipped correction bit is valid data to any decoder, so not every case can end in a
    status; one that ends without has decoded exactly what the rule decodes from the damaged file."""
    f = bytearray(_file(BIG))
    s = R.parse(bytes(f))["scans"][scan]
    rng = np.random.default_rng(100 * scan + seed)
    for at in rng.integers(s["begin"] + 1, s["end"], 8):
        if f[at] == 0xFF or f[at - 1] == 0xFF:
            continue
        f[at] = (f[at] ^ int(rng.integers(1, 255))) & 0x7F     # never a new 0xFF: the marker structure stays
    f = bytes(f)
    rc, status, intact = _guarded(f)
    assert rc == 0 and intact and status in (0, 1, 2)
    if status == 0:
        coef, _, _ = R.coefficients(f)
        np.testing.assert_array_equal(jpeg_prog_coefficients(f)[0], R.mcu_layout(f, coef).astype(np.int16))


def test_eob_run_longer_than_the_scan():
    """A flat grey file codes each AC scan as one EOB run over its 272 blocks; with the frame's height patched from 127 to
    63 the scans have 136."""
    f = bytearray(_file("L_127x129_flat_q5_none"))
    sof = f.index(b"\xff\xc2")
    assert (f[sof + 5] << 8 | f[sof + 6]) == 127
    f[sof + 5:sof + 7] = bytes([0, 63])
    info = jpeg_scans_inspect(bytes(f))
    assert info["supported"] and info["scans"][1]["units"] == 136
    rc, status, intact = _guarded(bytes(f))
    assert rc == 0 and status == 1 and intact


def test_room_for_the_coefficients_is_checked():
    f = _file(NAMES[0])
    lib = _lib.load()
    blocks = jpeg_scans_inspect(f)["blocks"]
    buf = np.zeros(64 * blocks, np.int16)
    st = C.c_int32(0)
    assert lib.vf_jpeg_prog_coefficients_host(f, len(f), 0, buf.ctypes.data_as(C.c_void_p), blocks - 1, C.byref(st)) != 0
    assert b"room for" in lib.vf_last_error()
