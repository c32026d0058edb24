"""What the default PNG rule refuses, through its host-only entries (vf_png_inspect, vf_png_decode_workspace_bytes;
DESIGN.md 5.6): the reason texts, their precedence, the return codes and the message prefixes, next to what the full rule
says of the same files.  Both rules share one host path, so this table pins what tells them apart.  No GPU."""
import ctypes as C
import struct
import zlib

import pytest

import png_full_cases as cases
import png_load_ref
import video_filler_amd  # noqa: F401
from video_filler_amd import _lib
from video_filler_amd.backend import _joined, png_inspect, png_inspect_full

KEY0 = "tRNS on colour type 0 with the file's channels (alpha from a colour key)"
KEY2 = "tRNS on colour type 2 with the file's channels (alpha from a colour key)"
GREY1 = "colour file with channels=1 (rgb2y is not a byte rule)"


def _header_only(W, H, depth, ct, lace):
    return b"\x89PNG\r\n\x1a\n" + cases.chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, ct, 0, 0, lace)) + \
        cases.chunk(b"IDAT", zlib.compress(b"\0")) + cases.chunk(b"IEND")


def _png(H, W, ct, depth, lace=False, **kw):
    if ct == 3:
        kw.setdefault("plte", cases.palette(depth))
    return cases.write_png(cases.random_pixels(H, W, ct, depth, 7), ct, depth, lace, **kw)


GOOD = _png(4, 5, 0, 8)
# name -> (file, channels, the default inspect's reason, the default query's reason, whether the full inspect supports it)
TABLE = {
    "deep": (_png(5, 4, 0, 16), 0, "16-bit samples", "16-bit samples", True),
    "lace": (_png(5, 4, 2, 8, True), 0, "Adam7 interlace", "Adam7 interlace", True),
    "deep_lace": (_png(5, 4, 6, 16, True), 0, "16-bit samples", "16-bit samples", True),             # png_parse's precedence
    "deep_lace_large": (_header_only(16385, 1, 16, 0, 1), 0, "16-bit samples", "16-bit samples", False),
    "lace_large": (_header_only(16385, 1, 8, 0, 1), 0, "Adam7 interlace", "Adam7 interlace", False),
    "large": (_header_only(1, 16385, 8, 0, 0), 0, "larger than 16384 per side", "larger than 16384 per side", False),
    "rgb_grey": (_png(5, 4, 2, 8), 1, "", GREY1, True),
    "palette_grey": (_png(5, 4, 3, 4), 1, "", GREY1, True),
    "rgba_grey": (_png(5, 4, 6, 8), 1, "", GREY1, True),
    "grey_key": (_png(5, 4, 0, 8, trns=b"\0\7"), 0, "", KEY0, True),
    "rgb_key": (_png(5, 4, 2, 8, trns=b"\0\7\0\x08\0\x09"), 0, "", KEY2, True),
    "deep_key": (_png(5, 4, 0, 16, trns=b"\0\7"), 0, "16-bit samples", "16-bit samples", True),     # the file's rule first
}


def _query(files, channels):
    """vf_png_decode_workspace_bytes itself -> (return code, the error's text)"""
    lib = _lib.load()
    data, offs = _joined(files)
    ws_b, st_b = C.c_size_t(), C.c_size_t()
    rc = lib.vf_png_decode_workspace_bytes(data, offs.ctypes.data_as(C.c_void_p), len(files), channels, C.byref(ws_b), C.byref(st_b))
    return rc, lib.vf_last_error().decode()


@pytest.mark.parametrize("name", sorted(TABLE))
def test_the_default_rule_refuses_what_it_refused(name):
    f, channels, inspect_why, query_why, full_ok = TABLE[name]
    d = png_inspect(f)
    assert d["supported"] == (not inspect_why) and d["reason"] == inspect_why
    if inspect_why:
        ref = png_load_ref.parse(f)
        assert (ref["supported"], ref["reason"]) == (False, inspect_why)
        assert d["inflated_bytes"] == ref["inflated_bytes"]        # one pass, whatever the interlace flag says
    for at, files in ((0, [f]), (1, [GOOD, f]), (2, [GOOD, GOOD, f, GOOD])):
        assert _query(files, channels) == (3, "vf_png_decode: image %d: unsupported: %s" % (at, query_why))
    full = png_inspect_full(f)
    assert full["supported"] == full_ok and (full["reason"] == "larger than 16384 per side") == (not full_ok)
    for k in ("width", "height", "bit_depth", "color_type", "interlace", "channels", "idat_bytes", "idat_chunks", "palette_entries",
              "trns_entries"):
        assert d[k] == full[k], k


def test_the_first_two_are_the_full_rules_own():
    for name in ("deep", "lace"):
        assert png_inspect_full(TABLE[name][0])["supported"] and not png_inspect(TABLE[name][0])["supported"]


def test_a_plain_file_is_one_pass_under_either_rule():
    d, full = png_inspect(GOOD), png_inspect_full(GOOD)
    assert "passes" not in d and d["supported"] and full["supported"] and d["reason"] == full["reason"] == ""
    assert d["inflated_bytes"] == full["inflated_bytes"] == 4 * (1 + 5)
    assert full["passes"] == [(5, 4, 5)] + [(0, 0, 0)] * 6
    assert "passes" not in png_inspect_full(GOOD, passes=False)
    assert _query([GOOD], 0)[0] == 0 and _query([GOOD], 3)[0] == 0


def test_a_truncated_file_is_malformed_under_either_rule_with_its_own_prefix():
    lib = _lib.load()
    for f, text in ((GOOD[:20], "chunk IHDR at byte 8 runs past the end of the file"), (GOOD[:15], "truncated chunk header at byte 8"),
                    (GOOD[:-12], "no IEND chunk")):
        info, why = (C.c_int64 * 12)(), C.create_string_buffer(160)
        assert lib.vf_png_inspect(f, len(f), info, why, 160) == 2
        assert lib.vf_last_error().decode() == "vf_png_inspect: " + text
        assert lib.vf_png_inspect_full(f, len(f), info, None, why, 160) == 2
        assert lib.vf_last_error().decode() == "vf_png_inspect_full: " + text
        assert _query([GOOD, f], 0) == (2, "vf_png_decode: image 1: " + text)
