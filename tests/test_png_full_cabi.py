"""The host-only entries of the full PNG rule (vf_png_inspect_full, vf_png_decode_full_workspace_bytes):
the workspace arithmetic against tests/png_full_ref.py, the 2^31 refusal by header alone, and the malformed-file errors,
which are vf_png_inspect's.  No GPU."""
import re
import struct
import zlib

import pytest

import png_full_cases as cases
import png_full_ref
import video_filler_amd  # noqa: F401
from video_filler_amd.backend import (png_decode_full_workspace_bytes, png_decode_workspace_bytes, png_inspect,
                                      png_inspect_full)

DESCRIPTOR = 1232      # sizeof(PngdImage), as DESIGN.md 5.6 states it
up256 = lambda v: (v + 255) // 256 * 256


def _sizes(files, channels, out_kind):
    """the query's arithmetic restated: descriptors and streams are staged; inflated and unfiltered bytes follow"""
    stage, inf, raw = up256(DESCRIPTOR * len(files)), 0, 0
    for f in files:
        d = png_full_ref.parse(f)
        assert d["inflated_bytes"] == sum(h * (1 + rb) for w, h, rb in d["passes"])
        stage += up256(sum(map(len, d["idat"])) - 2 + 8)
        inf += up256(d["inflated_bytes"])
        oc = channels or d["channels"]
        direct = not d["interlace"] and out_kind == 0 and d["bit_depth"] == 8 and d["color_type"] != 3 and \
            oc == png_full_ref.SAMPLES[d["color_type"]]
        if not direct:
            raw += up256(sum(h * rb for w, h, rb in d["passes"]))
    return stage + inf + raw, stage


@pytest.mark.parametrize("channels,out_kind", [(None, 0), (3, 0), (None, 1)])
def test_workspace_arithmetic(channels, out_kind):
    names = [n for n in sorted(cases.GOOD) if n.endswith(("_17x23", "_4x5", "_1x1", "_131x19"))] + [cases.TRNS, cases.SPLIT]
    files = [cases.GOOD[n]["file"] for n in names]
    plain = cases.write_png(cases.random_pixels(9, 17, 2, 8, 1), 2, 8, False)       # the direct route, when out_kind is 0
    assert png_decode_full_workspace_bytes(files + [plain], channels, out_kind) == _sizes(files + [plain], channels, out_kind)
    for f in files[::7]:
        assert png_decode_full_workspace_bytes([f], channels, out_kind) == _sizes([f], channels, out_kind)


def test_plain_files_need_what_the_default_entry_needs():
    """both entries count the one descriptor: equal sizes for plain 8-bit files, also where up256(1112 n) and
    up256(1232 n), the two descriptors there once were, differ (n = 3, 7)"""
    plain = [cases.write_png(cases.random_pixels(33, 70, 0, 4, 2), 0, 4, False),                   # expanded
             cases.write_png(cases.random_pixels(9, 17, 2, 8, 1), 2, 8, False),                     # direct with the file's channels
             cases.write_png(cases.random_pixels(5, 4, 3, 2, 3), 3, 2, False, plte=cases.palette(2)),
             cases.write_png(cases.random_pixels(70, 3, 4, 8, 4), 4, 8, False),
             cases.write_png(cases.random_pixels(1, 1, 0, 8, 5), 0, 8, False),
             cases.write_png(cases.random_pixels(8, 8, 6, 8, 6), 6, 8, False),
             cases.write_png(cases.random_pixels(17, 23, 0, 1, 7), 0, 1, False)]
    assert up256(1112 * 3) != up256(1232 * 3) and up256(1112 * 7) != up256(1232 * 7)
    for n in (1, 3, 7):
        for channels in (None, 3):
            files = plain[:n]
            full, default = png_decode_full_workspace_bytes(files, channels, 0), png_decode_workspace_bytes(files, channels)
            assert default == full == _sizes(files, channels, 0), (n, channels)


def _header_only(W, H, depth, ct, lace):
    z = zlib.compress(b"\0")
    return b"\x89PNG\r\n\x1a\n" + cases.chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, ct, 0, 0, lace)) + \
        cases.chunk(b"IDAT", z) + cases.chunk(b"IEND")


def test_an_inflated_size_of_2_31_or_more_is_refused_by_header_alone():
    for lace in (0, 1):
        f = _header_only(16384, 16384, 16, 6, lace)
        d = png_inspect_full(f)
        assert not d["supported"] and "2^31" in d["reason"] and d["inflated_bytes"] >= 1 << 31
        assert d["inflated_bytes"] == png_full_ref.parse(f)["inflated_bytes"] and d["reason"] == png_full_ref.parse(f)["reason"]
        with pytest.raises(ValueError, match=r"image 1: unsupported: inflated size of 2\^31"):
            png_decode_full_workspace_bytes([cases.GOOD[cases.TRNS]["file"], f])
    ok = _header_only(16384, 16384, 16, 2, 1)              # 6 bytes per pixel: below 2^31
    assert png_inspect_full(ok)["supported"] and png_inspect_full(ok)["inflated_bytes"] < 1 << 31
    big = _header_only(16385, 1, 8, 0, 1)
    assert png_inspect_full(big)["reason"] == "larger than 16384 per side"


def test_what_stays_unsupported_by_channels():
    grey_trns = cases.write_png(cases.random_pixels(5, 4, 0, 16, 3), 0, 16, True, trns=b"\0\7")
    assert png_inspect_full(grey_trns)["supported"]
    with pytest.raises(ValueError, match="image 0: unsupported: tRNS on colour type 0"):
        png_decode_full_workspace_bytes([grey_trns])
    assert png_decode_full_workspace_bytes([grey_trns], 1)[0] > 0
    with pytest.raises(ValueError, match="image 0: unsupported: colour file with channels=1"):
        png_decode_full_workspace_bytes([cases.GOOD["c2d16_lace_3x3"]["file"]], 1)
    with pytest.raises(ValueError, match="out_kind 2"):
        png_decode_full_workspace_bytes([grey_trns], 1, 2)


def _malformed():
    good = cases.GOOD["c6d16_lace_9x17"]["file"]
    at = good.index(b"IDAT")
    wrong_crc = bytearray(good)
    wrong_crc[at + 6] ^= 1
    no_iend = good[:-12]
    bad_ihdr = bytearray(_header_only(3, 3, 16, 3, 1))      # a palette at 16 bits
    two = good[:33] + good[8:33] + good[33:]
    past = good[:at - 4] + struct.pack(">I", 1 << 20) + good[at:]
    return [bytes(wrong_crc), no_iend, bytes(bad_ihdr), two, past, b"\x89PNG\r\n\x1a\r" + bytes(40), good[:20]]


@pytest.mark.parametrize("i", range(7))
def test_malformed_files_raise_what_the_default_inspect_raises(i):
    f = _malformed()[i]
    with pytest.raises(ValueError) as old:
        png_inspect(f)
    with pytest.raises(ValueError) as new:
        png_inspect_full(f)
    strip = lambda e: re.sub(r"^vf_png_inspect(_full)?: ", "", str(e.value))
    assert strip(old) == strip(new) and strip(new)
    if i:                                                  # the size query walks the chunk headers and computes no CRC
        with pytest.raises(ValueError, match="image 1: " + re.escape(strip(new))):
            png_decode_full_workspace_bytes([cases.GOOD[cases.TRNS]["file"], f])
