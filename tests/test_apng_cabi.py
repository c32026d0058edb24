"""The host-only APNG entries answer, and refuse, without a GPU: vf_apng_workspace_bytes, and
vf_apng_encode's argument checks, which come before it touches the device."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

import video_filler_amd  # noqa: F401
from video_filler_amd import _lib, backend

import apng_ref
import png_ref


def _query(g, n, H, W, Cc, delay=10, loop=0):
    lib = _lib.load()
    ws, out = C.c_size_t(), C.c_size_t()
    rc = lib.vf_apng_workspace_bytes(g, n, H, W, Cc, delay, loop, C.byref(ws), C.byref(out))
    return rc, ws.value, out.value, lib.vf_last_error().decode()


def test_workspace_query_answers_without_a_gpu():
    rc, ws, out, _ = _query(3, 119, 384, 512, 3)
    assert rc == 0
    stream = 384 * (512 * 3 + 1)
    chunks = -(-stream // backend.PNG_CHUNK)
    assert out == 3 * (119 * (stream + 21 * chunks + 6 + 38) + 65)
    assert ws >= 3 * 119 * (stream + chunks * 8224)
    assert backend.apng_workspace_bytes(3, 119, 384, 512, 3) == (ws, out)
    for geom in ((1, 1, 1, 1, 1), (1, 1, 16384, 16384, 3), (65535, 1, 1, 1, 3), (1, 65535, 1, 1, 1), (1, 2, 8, 8, 3, 0, 65535),
                 (1, 2, 8, 8, 3, 65535, 0)):
        assert _query(*geom)[0] == 0, geom
    # the png encoder of the same frames needs no less workspace for what the two share
    assert ws >= backend.png_workspace_bytes(357, 384, 512, 3)[0]


@pytest.mark.parametrize("geom,word", [((1, 2, 8, 8, 2), "2 channels"), ((1, 2, 16385, 8, 3), "16385x8"), ((1, 2, 8, 16385, 1), "8x16385"),
                                       ((1, 2, 0, 8, 3), "0x8"), ((1, 0, 8, 8, 3), "n: a clip of 0 frames"),
                                       ((1, 65536, 8, 8, 3), "n: a clip of 65536 frames"), ((0, 2, 8, 8, 3), "g: a batch of 0 clips"),
                                       ((65536, 2, 8, 8, 3), "g: a batch of 65536 clips"), ((1, 2, 8, 8, 3, 65536, 0), "delay: 65536"),
                                       ((1, 2, 8, 8, 3, -1, 0), "delay: -1"), ((1, 2, 8, 8, 3, 10, -1), "loop: -1"),
                                       ((1, 2, 8, 8, 3, 10, 65536), "loop: 65536"),
                                       ((1, 65535, 16384, 16384, 3), "n: 65535 frames of 98306 chunks")])
def test_workspace_query_refuses_naming_the_argument(geom, word):
    rc, _, _, err = _query(*geom)
    assert rc != 0 and "vf_apng_workspace_bytes" in err and word in err, err
    with pytest.raises(ValueError, match=word):
        backend.apng_workspace_bytes(*geom)


def test_sequence_numbers_stay_below_2_to_the_31():
    """n * (chunks + 1) < 2^31: 21844 frames of 98306 chunks is the longest clip of the largest frame that fits"""
    assert -(-16384 * (16384 * 3 + 1) // backend.PNG_CHUNK) == 98306 and 21844 * 98307 < 1 << 31 <= 21845 * 98307
    assert _query(1, 21844, 16384, 16384, 3)[0] == 0
    rc, _, _, err = _query(1, 21845, 16384, 16384, 3)
    assert rc != 0 and "n: 21845 frames" in err


def test_encode_refuses_before_it_needs_a_device():
    lib = _lib.load()
    for args, word in (((1, 1, 2, 8, 8, 3, 65536, 0), "delay: 65536"), ((1, 1, 2, 8, 8, 3, 10, -1), "loop: -1"),
                       ((1, 1, 2, 8, 8, 2, 10, 0), "2 channels"), ((1, 1, 0, 8, 8, 3, 10, 0), "n: a clip of 0 frames"),
                       ((2, 1, 2, 8, 8, 3, 10, 0), "kind 2")):
        rc = lib.vf_apng_encode(None, None, *args, None, 0, None, 0, None)
        err = lib.vf_last_error().decode()
        assert rc != 0 and "vf_apng_encode" in err and word in err, err
    rc = lib.vf_apng_encode(None, None, 1, 1, 2, 8, 8, 3, 10, 0, None, 0, None, 1 << 30, None)
    assert rc != 0 and "workspace holds 0 bytes" in lib.vf_last_error().decode()
    from video_filler_amd import data
    with pytest.raises(ValueError, match="delay=65536"):
        data.encode_apng(np.zeros((2, 8, 8, 3), np.uint8), 65536)
    with pytest.raises(ValueError, match="loop=-1"):
        data.encode_apng(np.zeros((2, 8, 8, 3), np.uint8), 10, -1)
    with pytest.raises(ValueError, match="loop=2.5"):
        data.encode_apng(np.zeros((2, 8, 8, 3), np.uint8), 10, 2.5)


@pytest.mark.parametrize("geom", [(3, 33, 85, 3), (2, 64, 127, 1), (2, 1, 1, 1)])
def test_output_bound_is_a_file_of_stored_blocks(geom):
    """the bound is the size of a file whose every chunk is a stored block: assemble one from level-0 streams cut at 8 KiB"""
    import struct
    import zlib
    n, H, W, Cc = geom
    rng = np.random.default_rng(1)
    files = []
    for _ in range(n):
        raw = b"".join(b"\0" + rng.integers(0, 256, W * Cc, dtype=np.uint8).tobytes() for _ in range(H))
        parts = [raw[i:i + png_ref.CHUNK] for i in range(0, len(raw), png_ref.CHUNK)]
        idats = []
        for k, p in enumerate(parts):
            d = (b"\x78\x9c" if k == 0 else b"") + bytes([k == len(parts) - 1]) + struct.pack("<HH", len(p), len(p) ^ 0xFFFF) + p
            if k == len(parts) - 1:
                d += struct.pack(">I", zlib.adler32(raw))
            idats.append(apng_ref.chunk(b"IDAT", d))
        ihdr = struct.pack(">IIBBBBB", W, H, 8, 2 if Cc == 3 else 0, 0, 0, 0)
        files.append(apng_ref.SIGNATURE + apng_ref.chunk(b"IHDR", ihdr) + b"".join(idats) + apng_ref.chunk(b"IEND", b""))
    f = apng_ref.assemble(files, 10, 0)
    assert getattr(Image.open(io.BytesIO(f)), "n_frames", 1) == n
    bound = backend.apng_workspace_bytes(1, n, H, W, Cc)[1]
    assert len(f) == bound - 4 * len(parts)                  # the bound counts fdAT framing for frame 0's IDATs too


def test_save_apngs_refuses_before_any_backend_exists(tmp_path):
    from video_filler_amd import inference
    x = np.zeros((3, 4, 4, 3), np.uint8)
    with pytest.raises(ValueError, match="result, result"):
        inference.save_apngs(str(tmp_path / "d" / "clip"), x, result=x)
    with pytest.raises(ValueError, match="nothing to save"):
        inference.save_apngs(str(tmp_path / "d" / "clip"))
    with pytest.raises(ValueError, match="share one type"):
        inference.save_apngs(str(tmp_path / "d" / "clip"), x, x[:2])
    assert not (tmp_path / "d").exists()


# ------------------------------------------------------------------------------------------------ the decoder's host entries
import apng_cases  # noqa: E402
import apng_decode_ref  # noqa: E402

FX = apng_cases.fixtures()


@pytest.mark.parametrize("name", sorted(FX["good"]) + ["corrupt/" + k for k in sorted(FX["corrupt"])])
def test_inspect_equals_the_reference_metadata(name):
    f = FX["corrupt"][name[8:]][0] if name.startswith("corrupt/") else FX["good"][name]
    info, rows = apng_decode_ref.metadata(f)
    d = backend.apng_inspect(f)
    assert {k: d[k] for k in info} == info and d["reason"] == ""
    assert [[r[k] for k in backend.APNG_FRAME_KEYS] for r in d["frame_info"]] == rows
    assert backend.APNG_FRAME_KEYS == apng_decode_ref.FRAME_KEYS
    from video_filler_amd import data
    assert data.apng_info(np.frombuffer(f, np.uint8)) == d


def test_inspect_fills_no_more_rows_than_the_caller_has():
    lib = _lib.load()
    f = FX["good"]["background_then_smaller"]
    info = (C.c_int64 * 12)()
    rows = np.full((3, 9), -7, np.int64)
    assert lib.vf_apng_inspect(f, len(f), info, rows.ctypes.data_as(C.c_void_p), 2, None, 0) == 0
    assert info[6] == 5 and (rows[2] == -7).all() and (rows[:2, 2] > 0).all()
    assert lib.vf_apng_inspect(f, len(f), info, None, 0, None, 0) == 0
    assert lib.vf_apng_inspect(f, len(f), info, None, 2, None, 0) != 0 and "NULL" in lib.vf_last_error().decode()


@pytest.mark.parametrize("name", sorted(FX["malformed"]))
def test_malformed_files_say_why(name):
    f, word = FX["malformed"][name]
    with pytest.raises(ValueError, match="vf_apng_inspect: ") as e:
        backend.apng_inspect(f)
    assert word in str(e.value)
    with pytest.raises(ValueError, match="vf_apng_decode_workspace_bytes: image 1: ") as e:
        backend.apng_decode_workspace_bytes([FX["good"]["edges"], f])
    assert word in str(e.value)


@pytest.mark.parametrize("name", sorted(FX["unsupported"]))
def test_unsupported_files_say_why(name):
    f, word = FX["unsupported"][name]
    d = backend.apng_inspect(f)
    assert not d["supported"] and word in d["reason"]
    ref = apng_decode_ref.parse(f)
    assert not ref["supported"] and d["frames"] == ref["frames"]
    with pytest.raises(ValueError, match="image 2: unsupported: ") as e:
        backend.apng_decode_workspace_bytes([FX["good"]["edges"], FX["good"]["plain_png"], f], True)
    assert word in str(e.value)


def test_decode_workspace_query_counts_frames():
    files = [FX["good"][k] for k in ("edges", "plain_png", "rgba16_adam7", "many_fdats")]
    ws, stage = backend.apng_decode_workspace_bytes(files)
    frames = sum(apng_decode_ref.parse(f)["frames"] for f in files)
    assert stage >= 1232 * frames and ws > stage
    assert backend.apng_decode_workspace_bytes(files, True) == (ws, stage)      # the output is the caller's
    one = FX["good"]["one_frame"]
    many = apng_cases.build(1, 1, 0, 8, [apng_cases.frame(apng_cases.pix(1, 1, 0, 8, 1))] * 255)
    assert backend.apng_decode_workspace_bytes([many] * 257)[0] > 0                  # 65535 frames: the most one call takes
    with pytest.raises(ValueError, match="65536 frames in one batch"):
        backend.apng_decode_workspace_bytes([many] * 257 + [one])
    lib = _lib.load()
    offs = np.array([0, len(one)], np.int64)
    ws_b, st_b = C.c_size_t(), C.c_size_t()
    assert lib.vf_apng_decode_workspace_bytes(one, offs.ctypes.data_as(C.c_void_p), 1, 2, C.byref(ws_b), C.byref(st_b)) != 0
    assert "alpha 2" in lib.vf_last_error().decode()
