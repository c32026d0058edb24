"""tests/png_load_ref.py (the restated image.load for PNG) against Pillow, and the host-only entry points of
the device decoder (vf_png_inspect, vf_png_decode_workspace_bytes) against it.  No GPU."""
import ctypes as C
import io
import os
import struct
import zlib

import numpy as np
import pytest

import png_load_ref
import video_filler_amd  # noqa: F401
from video_filler_amd import _lib, data
from video_filler_amd.backend import png_decode_workspace_bytes, png_inspect

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "png_decode_cases.npz"))
GOOD = sorted(k[5:] for k in GOLDEN.files if k.startswith("good/"))
BAD = sorted(k[4:] for k in GOLDEN.files if k.startswith("bad/"))


def _file(name):
    return GOLDEN["good/" + name].tobytes()


def _chunk(typ, body=b"", crc=None):
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body) if crc is None else crc)


def _png(*chunks):
    return png_load_ref.SIGNATURE + b"".join(chunks)


IHDR = _chunk(b"IHDR", struct.pack(">IIBBBBB", 2, 2, 8, 0, 0, 0, 0))
IDAT = _chunk(b"IDAT", zlib.compress(bytes(6)))
IEND = _chunk(b"IEND")


@pytest.mark.parametrize("name", GOOD)
def test_restatement_equals_pillow(name):
    Image = pytest.importorskip("PIL.Image")
    f = _file(name)
    im = Image.open(io.BytesIO(f))
    im.load()
    d = png_load_ref.parse(f)
    if d["trns"] is not None and d["color_type"] != 3:  # a colour key: no byte rule for the file's own channels
        with pytest.raises(png_load_ref.PngUnsupported, match="tRNS on colour type"):
            png_load_ref.load(f)
        want = np.asarray(im)
        want = np.repeat(want[..., None], 3, 2) if want.ndim == 2 else want
        assert want.shape[2] == 3 and np.array_equal(png_load_ref.load(f, 3), want)
        if d["color_type"] == 0:
            assert np.array_equal(png_load_ref.load(f, 1), want[..., :1])
        return
    mine = png_load_ref.load(f)
    if im.mode == "1":                                  # Pillow's bool -> 0 / 255: the replicated byte (L;2 and L;4 come as L)
        want = np.asarray(im).astype(np.uint8)[..., None] * np.uint8(255)
    elif im.mode == "P":
        want = np.asarray(im.convert("RGBA" if "transparency" in im.info else "RGB"))
    else:
        want = np.asarray(im)
        want = want[..., None] if want.ndim == 2 else want
    assert mine.dtype == np.uint8 and mine.shape == want.shape and np.array_equal(mine, want)
    # image.load(path, 3)
    three = png_load_ref.load(f, 3)
    assert three.shape == mine.shape[:2] + (3,)
    if d["color_type"] in (0, 4):
        assert all(np.array_equal(three[..., c], mine[..., 0]) for c in range(3))
        assert np.array_equal(png_load_ref.load(f, 1), mine[..., :1])
    else:
        assert np.array_equal(three, mine[..., :3])
        with pytest.raises(png_load_ref.PngUnsupported, match="channels=1"):
            png_load_ref.load(f, 1)


def test_grey_below_8_bits_is_bit_replication():
    for depth, mul in ((1, 255), (2, 85), (4, 17)):
        W = 11
        vals = (np.arange(3 * W) * 5 % (1 << depth)).reshape(3, W)
        bits = np.zeros((3, -(-W * depth // 8) * 8), np.uint8)
        for x in range(W):
            for k in range(depth):
                bits[:, x * depth + k] = (vals[:, x] >> (depth - 1 - k)) & 1
        rows = np.packbits(bits, axis=1)
        raw = b"".join(b"\x00" + r.tobytes() for r in rows)
        f = _png(_chunk(b"IHDR", struct.pack(">IIBBBBB", W, 3, depth, 0, 0, 0, 0)), _chunk(b"IDAT", zlib.compress(raw)), IEND)
        assert np.array_equal(png_load_ref.load(f)[..., 0], vals * mul)
    for name in ("hand/grey2", "hand/grey4"):
        assert set(np.unique(png_load_ref.load(_file(name))).tolist()) <= set(range(0, 256, 17 if name.endswith("4") else 85))
    assert png_load_ref.load_float(_file("pil/L8_l6")).dtype == np.float32


@pytest.mark.parametrize("name", GOOD)
def test_png_info_fields(name):
    f = _file(name)
    info, ref = data.png_info(f), png_load_ref.parse(f)
    for k in ("width", "height", "bit_depth", "color_type", "interlace", "channels", "inflated_bytes"):
        assert info[k] == ref[k], k
    assert info["idat_bytes"] == sum(len(b) for b in ref["idat"]) and info["idat_chunks"] == len(ref["idat"])
    assert info["palette_entries"] == (0 if ref["plte"] is None else len(ref["plte"]))
    assert info["trns_entries"] == (0 if ref["trns"] is None else len(ref["trns"]) if ref["color_type"] == 3 else 1)
    assert info["supported"] is True and info["reason"] == ""
    assert png_inspect(f) == info == data.png_info(np.frombuffer(f, np.uint8))


def test_masks_are_what_the_issue_says():
    infos = {k: data.png_info(_file(k)) for k in GOOD if k.startswith("mask/")}
    assert len(infos) == 7
    assert (infos["mask/mask"]["bit_depth"], infos["mask/mask"]["color_type"]) == (1, 0)
    assert sum(1 for i in infos.values() if i["bit_depth"] == 8 and (i["width"], i["height"]) == (480, 360)) == 6


def test_unsupported_files_say_why():
    Image = pytest.importorskip("PIL.Image")
    a = (np.arange(40 * 24).reshape(24, 40) * 50 % 65536).astype(np.uint16)
    bio = io.BytesIO()
    Image.fromarray(a).save(bio, "PNG")
    info = data.png_info(bio.getvalue())
    assert info["supported"] is False and "16-bit" in info["reason"] and info["bit_depth"] == 16
    with pytest.raises(ValueError, match="image 1: unsupported: 16-bit"):
        png_decode_workspace_bytes([_file("pil/L8_l6"), bio.getvalue()])
    lace = bytearray(_file("pil/RGB_l6"))               # Pillow writes no Adam7: the IHDR flag alone makes the file unsupported
    lace[8 + 8 + 12] = 1
    lace[8 + 8 + 13:8 + 8 + 17] = struct.pack(">I", zlib.crc32(bytes(lace[12:8 + 8 + 13])))
    info = data.png_info(bytes(lace))
    assert info["supported"] is False and "Adam7" in info["reason"] and info["interlace"] == 1
    assert png_load_ref.parse(bytes(lace))["reason"] == info["reason"]
    with pytest.raises(ValueError, match="image 1: unsupported: Adam7"):
        png_decode_workspace_bytes([_file("pil/L8_l6"), bytes(lace)])
    with pytest.raises(ValueError, match="image 0: unsupported: colour file with channels=1"):
        png_decode_workspace_bytes([_file("pil/RGB_l6")], channels=1)


MALFORMED = [
    ("signature", b"\x89PNG\r\n\x1a\r" + IHDR + IDAT + IEND, "signature"),
    ("ihdr_not_first", _png(_chunk(b"gAMA", bytes(4)), IHDR, IDAT, IEND), "IHDR is not the first"),
    ("illegal_ihdr", _png(_chunk(b"IHDR", struct.pack(">IIBBBBB", 2, 2, 4, 2, 0, 0, 0)), IDAT, IEND), "illegal IHDR"),
    ("zero_width", _png(_chunk(b"IHDR", struct.pack(">IIBBBBB", 0, 2, 8, 0, 0, 0, 0)), IDAT, IEND), "illegal IHDR"),
    ("no_plte", _png(_chunk(b"IHDR", struct.pack(">IIBBBBB", 2, 2, 8, 3, 0, 0, 0)), IDAT, IEND), "no PLTE"),
    ("plte_after_idat", _png(_chunk(b"IHDR", struct.pack(">IIBBBBB", 2, 2, 8, 2, 0, 0, 0)), IDAT, _chunk(b"PLTE", bytes(3)), IEND),
     "PLTE after IDAT"),
    ("idat_not_consecutive", _png(IHDR, IDAT, _chunk(b"tEXt", b"a\x00b"), IDAT, IEND), "not consecutive"),
    ("no_iend", _png(IHDR, IDAT), "no IEND"),
    ("chunk_past_file", _png(IHDR, IDAT, IEND)[:-20], "runs past the end"),
    ("crc_ihdr", _png(_chunk(b"IHDR", struct.pack(">IIBBBBB", 2, 2, 8, 0, 0, 0, 0), crc=1), IDAT, IEND), "wrong CRC on chunk .*IHDR"),
    ("crc_idat", _png(IHDR, _chunk(b"IDAT", zlib.compress(bytes(6)), crc=7), IEND), "wrong CRC on chunk .*IDAT"),
    ("crc_plte", _png(_chunk(b"IHDR", struct.pack(">IIBBBBB", 2, 2, 8, 3, 0, 0, 0)), _chunk(b"PLTE", bytes(6), crc=3), IDAT, IEND),
     "wrong CRC on chunk .*PLTE"),
    ("crc_trns", _png(_chunk(b"IHDR", struct.pack(">IIBBBBB", 2, 2, 8, 3, 0, 0, 0)), _chunk(b"PLTE", bytes(6)),
                      _chunk(b"tRNS", b"\x07", crc=4), IDAT, IEND), "wrong CRC on chunk .*tRNS"),
    ("crc_iend", _png(IHDR, IDAT, _chunk(b"IEND", crc=9)), "wrong CRC on chunk .*IEND"),
    ("zlib_method", _png(IHDR, _chunk(b"IDAT", b"\x79\x9c" + zlib.compress(bytes(6))[2:]), IEND), "zlib header"),
    ("zlib_dictionary", _png(IHDR, _chunk(b"IDAT", b"\x78\xbb" + zlib.compress(bytes(6))[2:]), IEND), "zlib header"),
    ("zlib_fcheck", _png(IHDR, _chunk(b"IDAT", b"\x78\x9d" + zlib.compress(bytes(6))[2:]), IEND), "zlib header"),
]


@pytest.mark.parametrize("name,f,word", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_malformed_files_raise_naming_the_fault(name, f, word):
    with pytest.raises(ValueError, match=word):
        png_inspect(f)
    with pytest.raises(ValueError, match=word):
        data.png_info(f)
    with pytest.raises(png_load_ref.PngError):
        png_load_ref.parse(f)
    if not name.startswith("crc"):                      # the size query reads the chunk headers alone
        with pytest.raises(ValueError, match="image 1: .*" + word):
            png_decode_workspace_bytes([_png(IHDR, IDAT, IEND), f])


def test_unchecked_ancillary_crc_and_good_minimal_file():
    pal = _png(_chunk(b"IHDR", struct.pack(">IIBBBBB", 2, 2, 8, 3, 0, 0, 0)), _chunk(b"PLTE", bytes(6)), _chunk(b"tRNS", b"\x07"),
               IDAT, IEND)
    assert data.png_info(pal)["trns_entries"] == 1 and png_load_ref.load(pal).shape == (2, 2, 4)
    f = _png(IHDR, _chunk(b"tEXt", b"k\x00v", crc=5), IDAT, IEND)
    assert data.png_info(f)["supported"] and png_load_ref.load(f).shape == (2, 2, 1)


def test_workspace_query_is_host_only():
    files = [_file(n) for n in GOOD[:5]]
    ws, st = png_decode_workspace_bytes(files)
    assert st > sum(data.png_info(f)["idat_bytes"] for f in files) and ws >= st + sum(data.png_info(f)["inflated_bytes"] for f in files)
    lib = _lib.load()
    blob = b"".join(files)
    offs = np.cumsum([0] + [len(f) for f in files]).astype(np.int64)
    a, b = C.c_size_t(), C.c_size_t()
    assert lib.vf_png_decode_workspace_bytes(blob, offs.ctypes.data_as(C.c_void_p), 5, 0, C.byref(a), C.byref(b)) == 0
    assert (a.value, b.value) == (ws, st)
    assert lib.vf_png_decode_workspace_bytes(blob, offs.ctypes.data_as(C.c_void_p), 5, 2, C.byref(a), C.byref(b)) == 2


@pytest.mark.parametrize("name", BAD)
def test_bad_fixtures_have_good_headers_and_the_restatement_refuses_them(name):
    f = GOLDEN["bad/" + name].tobytes()
    assert data.png_info(f)["supported"]
    with pytest.raises(png_load_ref.PngError):
        png_load_ref.load(f)


def test_lua_binding_declares_the_entry_points():
    with open(os.path.join(os.path.dirname(HERE), "video-filler_amd", "lua", "hipnn.lua")) as fh:
        text = fh.read()
    for fn in ("vf_png_inspect", "vf_png_decode_workspace_bytes", "vf_png_decode", "vf_png_bytes_to_float"):
        assert "int %s(" % fn in text and fn in _lib.SIGNATURES
