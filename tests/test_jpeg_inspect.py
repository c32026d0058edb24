"""The host-only JPEG inspector (vf_jpeg_inspect): geometry, sampling, restart interval and scan range of
baseline files; progressive, CMYK and 4:1:1 files reported as unsupported; malformed headers rejected with a message;
the header-only sizes of vf_jpeg_workspace_bytes against the exact plan the decode makes.
Encodes with Pillow when it is importable, otherwise reads the committed fixtures (tests/golden/jpeg_cases.npz)."""
import ctypes as C
import io
import os

import numpy as np
import pytest

import video_filler_amd  # noqa: F401
from video_filler_amd import _lib, data
from video_filler_amd.backend import jpeg_inspect, jpeg_inspect_layouts

try:
    from PIL import Image
except ImportError:   # pragma: no cover - the fixtures cover the same files
    Image = None

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz"))


def _fixture(key):
    return GOLDEN[key].tobytes()


def _pillow(a, **kw):
    bio = io.BytesIO()
    Image.fromarray(a).save(bio, "JPEG", **kw)
    return bio.getvalue()


def _eoi_at_end(buf, info):
    assert buf[info["scan_end"]:info["scan_end"] + 2] == b"\xff\xd9"
    assert buf.rindex(b"\xff\xda") < info["scan_begin"]


@pytest.mark.parametrize("name", sorted(k[4:] for k in GOLDEN.files if k.startswith("jpg/")))
def test_fixture_geometry(name):
    buf = _fixture("jpg/" + name)
    ref = GOLDEN["ref/" + name]
    info = jpeg_inspect(buf)
    mode = name.split("_")[0]
    assert info["supported"] and info["reason"] == ""
    assert (info["height"], info["width"]) == ref.shape[:2]
    assert info["components"] == (1 if mode == "L" else 3)
    assert (info["h_samp"], info["v_samp"]) == {"444": (1, 1), "422": (2, 1), "420": (2, 2), "L": (1, 1)}[mode]
    assert info["sof"] in (0xC0, 0xC1) and info["precision"] == 8
    _eoi_at_end(buf, info)
    assert 0 < info["scan_begin"] < info["scan_end"] == len(buf) - 2
    rst = name.rsplit("_", 1)[1]
    assert (info["restart_interval"] > 0) == (rst != "none")
    if info["restart_interval"]:
        hs, vs = info["h_samp"], info["v_samp"]
        mcus = -(-info["width"] // (8 * hs)) * -(-info["height"] // (8 * vs))
        assert info["segments"] == -(-mcus // info["restart_interval"])
        assert buf.count(b"\xff\xd0") >= 1 or info["segments"] == 1
    else:
        assert info["segments"] == 1
    assert data.jpeg_info(buf) == info
    assert data.jpeg_info(np.frombuffer(buf, np.uint8)) == info


@pytest.mark.skipif(Image is None, reason="Pillow encodes the files")
@pytest.mark.parametrize("sub,hv", [(0, (1, 1)), (1, (2, 1)), (2, (2, 2))])
def test_pillow_geometry_and_restarts(sub, hv):
    a = np.random.default_rng(3).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    for kw, ri in ((dict(), 0), (dict(restart_marker_blocks=3), 3), (dict(restart_marker_rows=1), -(-53 // (8 * hv[0])))):
        buf = _pillow(a, quality=80, subsampling=sub, **kw)
        info = jpeg_inspect(buf)
        assert info["supported"], info
        assert (info["width"], info["height"], info["components"]) == (53, 37, 3)
        assert (info["h_samp"], info["v_samp"]) == hv
        assert info["restart_interval"] == ri
        mcus = -(-53 // (8 * hv[0])) * -(-37 // (8 * hv[1]))
        assert info["segments"] == (-(-mcus // ri) if ri else 1)
        assert buf.count(b"\xff\xd0") + buf.count(b"\xff\xd1") >= (1 if ri and mcus > ri else 0)
        _eoi_at_end(buf, info)


def _luma_sampling(buf, hv):
    # Pillow's subsampling="4:1:1" writes 2x2: a 4:1:1 (4x1) or 4:4:0 (1x2) header is a patched SOF0 sampling byte
    b = bytearray(buf)
    b[b.index(b"\xff\xc0") + 11] = hv
    return bytes(b)


def _unsupported_files():
    if Image is None:
        return {k: _fixture("bad/" + k) for k in ("progressive", "cmyk", "411", "440")}
    a = np.random.default_rng(4).integers(0, 256, (24, 40, 3), dtype=np.uint8)
    bio = io.BytesIO()
    Image.new("CMYK", (40, 24), (1, 2, 3, 4)).save(bio, "JPEG")
    f444 = _pillow(a, subsampling=0)
    return {"progressive": _pillow(a, progressive=True), "cmyk": bio.getvalue(), "411": _luma_sampling(f444, 0x41),
            "440": _luma_sampling(f444, 0x12)}


@pytest.mark.parametrize("kind,why", [("progressive", "progressive"), ("cmyk", "CMYK"), ("411", "sampling 4x1"),
                                      ("440", "sampling 1x2")])
def test_unsupported_kinds(kind, why):
    for buf in (_unsupported_files()[kind], _fixture("bad/" + kind)):
        info = jpeg_inspect(buf)
        assert not info["supported"]
        assert why in info["reason"]
        assert info["width"] == 40 and info["height"] == 24
        assert data.jpeg_info(buf)["supported"] is False


def test_malformed_headers_raise_with_a_message():
    buf = _fixture("jpg/420_360x480_noise_q90_none")
    info = jpeg_inspect(buf)
    for cut in (0, 1, 3, 20, 100, info["scan_begin"] - 5):
        with pytest.raises(ValueError) as e:
            jpeg_inspect(buf[:cut])
        assert str(e.value)
    sos = buf.index(b"\xff\xda")
    with pytest.raises(ValueError, match="SOS"):
        jpeg_inspect(buf[:sos] + b"\xff\xd9")
    with pytest.raises(ValueError, match="SOI"):
        jpeg_inspect(b"\x89PNG\r\n\x1a\n" + bytes(64))
    with pytest.raises(ValueError):
        data.jpeg_info(buf[:50])


def test_fill_bytes_inside_the_scan_are_rejected():
    # 0xFF fill bytes before a stuffed 0xFF00: libjpeg-turbo's fast path and its slow path disagree on them
    buf = _fixture("jpg/420_360x480_noise_q90_none")
    info = jpeg_inspect(buf)
    k = buf.index(b"\xff\x00", info["scan_begin"])
    with pytest.raises(ValueError, match="fill bytes"):
        jpeg_inspect(buf[:k] + b"\xff" + buf[k:])


def _oversubscribed(buf):
    """buf with every symbol of its first AC Huffman table moved to code length 1: more codes than 1 bit holds."""
    b = bytearray(buf)
    i = 0
    while True:
        i = b.index(b"\xff\xc4", i)
        if b[i + 4] >> 4 == 1:
            break
        i += 2
    b[i + 5] = sum(b[i + 5:i + 21])
    b[i + 6:i + 21] = bytes(15)
    return bytes(b)


def test_oversubscribed_huffman_table_is_malformed():
    # libjpeg stops on it (JERR_BAD_HUFF_TABLE); building its lookahead table would write past the table
    good = _fixture("jpg/420_360x480_noise_q90_none")
    bad = _oversubscribed(good)
    for walk in (True, False):
        with pytest.raises(ValueError, match="bad Huffman table"):
            jpeg_inspect(bad, walk=walk)
    lib = _lib.load()
    data = good + bad
    offs = np.array([0, len(good), len(data)], np.int64)
    ws, st = C.c_size_t(), C.c_size_t()
    assert lib.vf_jpeg_workspace_bytes(data, offs.ctypes.data_as(C.c_void_p), 2, 256, C.byref(ws), C.byref(st)) == 2
    assert b"image 1: bad Huffman table" in lib.vf_last_error()


def test_component_twice_in_the_scan_is_malformed():
    b = bytearray(_fixture("jpg/420_360x480_noise_q90_none"))
    sos = b.index(b"\xff\xda")
    assert b[sos + 4] == 3
    b[sos + 7] = b[sos + 5]     # the second scan component names the first one again
    with pytest.raises(ValueError, match="twice"):
        jpeg_inspect(bytes(b), walk=False)


@pytest.mark.parametrize("name", sorted(k[4:] for k in GOLDEN.files if k.startswith(("jpg/", "bad/"))))
def test_headers_only_mode_agrees(name):
    buf = _fixture(("jpg/" if "jpg/" + name in GOLDEN.files else "bad/") + name)
    full, head = jpeg_inspect(buf), jpeg_inspect(buf, walk=False)
    assert head["scan_end"] == head["segments"] == -1
    assert {k: v for k, v in full.items() if k not in ("scan_end", "segments")} == \
        {k: v for k, v in head.items() if k not in ("scan_end", "segments")}


NAMES = sorted(k[4:] for k in GOLDEN.files if k.startswith("jpg/"))


def _with_restart_interval(buf, ri):
    """buf with its DRI marker (if any) dropped and one of `ri` MCUs put before the SOS."""
    b = bytearray(buf)
    sos = b.index(b"\xff\xda")
    k = b.find(b"\xff\xdd\x00\x04", 0, sos)
    if k >= 0:
        del b[k:k + 6]
        sos -= 6
    b[sos:sos] = b"\xff\xdd\x00\x04" + ri.to_bytes(2, "big")
    return bytes(b)


def _bound_batches():
    """name -> files: every fixture alone (the restart ones among them), all of them as one batch, and two hand-made files
    that strain a header-only bound: the smallest scan with a segment's fixed costs on it (grey 8x8, restart interval 1),
    and a scan of stuffed 0xFF00 pairs, whose compacted length is half its stuffed one and which spans several chunks."""
    d = {n: [_fixture("jpg/" + n)] for n in NAMES}
    d["all"] = [_fixture("jpg/" + n) for n in NAMES]
    d["grey_8x8_ri1"] = [_with_restart_interval(_fixture("jpg/L_8x8_flat_q5_b1"), 1)]
    big = _fixture("jpg/420_360x480_noise_q90_none")
    d["stuffed"] = [big[:jpeg_inspect(big, walk=False)["scan_begin"]] + b"\xff\x00" * 5000 + b"\xff\xd9"]
    return d


BOUND_BATCHES = _bound_batches()


def _sizes(entry, files, sub):
    lib = _lib.load()
    joined = b"".join(files)
    offs = np.cumsum([0] + [len(f) for f in files]).astype(np.int64)
    ws, st = C.c_size_t(), C.c_size_t()
    assert getattr(lib, entry)(joined, offs.ctypes.data_as(C.c_void_p), len(files), sub, C.byref(ws), C.byref(st)) == 0, lib.vf_last_error()
    return ws.value, st.value


@pytest.mark.parametrize("sub", [8, 16, 256, 1024])
@pytest.mark.parametrize("name", sorted(BOUND_BATCHES))
def test_header_only_sizes_cover_the_exact_plan(name, sub):
    # vf_jpeg_decode plans as the layouts entry does, from the walked scan; vf_jpeg_workspace_bytes reads the headers only
    files = BOUND_BATCHES[name]
    if name == "grey_8x8_ri1":
        info = jpeg_inspect(files[0])
        assert info["supported"] and (info["width"], info["height"], info["restart_interval"], info["segments"]) == (8, 8, 1, 1)
    bound, exact = _sizes("vf_jpeg_workspace_bytes", files, sub), _sizes("vf_jpeg_layouts_workspace_bytes", files, sub)
    assert bound[0] >= exact[0] and bound[1] >= exact[1], (bound, exact)


@pytest.mark.parametrize("name", NAMES)
def test_walked_scan_equals_the_layouts_walk_and_the_bytes(name):
    buf = _fixture("jpg/" + name)
    info, lay = jpeg_inspect(buf), jpeg_inspect_layouts(buf)
    assert info["supported"] and lay["supported"] and lay["scans"] == 1 and lay["levels"] == 1
    assert (info["width"], info["height"], info["components"], info["sof"]) == (lay["width"], lay["height"], lay["components"], lay["sof"])
    sos = buf.index(b"\xff\xda")
    assert info["scan_begin"] == sos + 2 + int.from_bytes(buf[sos + 2:sos + 4], "big")
    eoi = buf.rindex(b"\xff\xd9")
    assert info["scan_end"] == eoi
    # inside entropy-coded data a 0xFF is followed by 0x00 or by a restart marker, so the pairs can be counted as bytes
    scan = buf[info["scan_begin"]:eoi]
    assert info["segments"] == 1 + sum(scan.count(bytes([0xFF, 0xD0 + r])) for r in range(8))
    dri = buf.find(b"\xff\xdd\x00\x04", 0, sos)
    assert info["restart_interval"] == (int.from_bytes(buf[dri + 4:dri + 6], "big") if dri >= 0 else 0)
    mcus = lay["blocks"] // lay["blocks_per_mcu"]
    assert info["segments"] == (-(-mcus // info["restart_interval"]) if info["restart_interval"] else 1)


def test_path_items(tmp_path):
    buf = _fixture(sorted(k for k in GOLDEN.files if k.startswith("jpg/L_"))[0])
    p = tmp_path / "x.jpg"
    p.write_bytes(buf)
    assert data.jpeg_info(str(p)) == jpeg_inspect(buf)
