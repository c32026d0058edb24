"""The host reference of the PNG encoder's tests (tests/png_ref.py) against Pillow, and its own rules."""
import io
import os

import numpy as np
import pytest

import png_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_cases.npz")


def fixtures():
    z = np.load(GOLD)
    return {k[6:]: z[k] for k in z.files if k.startswith("frame/")}


def test_reader_decodes_pillow_files_to_pillows_pixels():
    Image = pytest.importorskip("PIL.Image")
    for name, a in fixtures().items():
        for level in (1, 6):
            bio = io.BytesIO()
            Image.fromarray(a[..., 0] if a.shape[2] == 1 else a).save(bio, "PNG", compress_level=level)
            got = png_ref.read_png(bio.getvalue())
            back = np.asarray(Image.open(io.BytesIO(bio.getvalue())))
            assert np.array_equal(got, back.reshape(got.shape)), name
            assert np.array_equal(got, a), name


def _tiny_png():
    """A valid file made with zlib alone: 3 x 2 RGB, filter None."""
    import struct
    import zlib
    img = np.arange(18, dtype=np.uint8).reshape(2, 3, 3)
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(2))

    def chunk(t, b):
        return struct.pack(">I", len(b)) + t + b + struct.pack(">I", zlib.crc32(t + b))
    return img, png_ref.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", 3, 2, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) + \
        chunk(b"IEND", b"")


def test_reader_rejects_a_flipped_crc_byte_and_a_flipped_adler_byte():
    import struct
    import zlib
    img, f = _tiny_png()
    assert np.array_equal(png_ref.read_png(f), img)
    idat = f.index(b"IDAT")
    (n,) = struct.unpack(">I", f[idat - 4:idat])
    crc_at = idat + 4 + n
    bad = bytearray(f)
    bad[crc_at + 1] ^= 0x10
    with pytest.raises(png_ref.PngError, match="CRC"):
        png_ref.read_png(bytes(bad))
    # the Adler-32 is the last four bytes of the IDAT data: flip one and mend the chunk CRC, so only zlib can notice
    bad = bytearray(f)
    bad[crc_at - 2] ^= 0x01
    bad[crc_at:crc_at + 4] = struct.pack(">I", zlib.crc32(bytes(bad[idat:crc_at])))
    with pytest.raises(png_ref.PngError, match="zlib"):
        png_ref.read_png(bytes(bad))
    with pytest.raises(png_ref.PngError):
        png_ref.read_png(f[:-1])
    with pytest.raises(png_ref.PngError):
        png_ref.read_png(b"\x88" + f[1:])


def test_byte_rule_truncates():
    x = np.array([0.999999, 1.0, -0.5, -0.0, 0.0, 2.0, np.nan, np.inf, -np.inf, 0.5, 254.9999 / 255], np.float32)
    assert png_ref.float_to_bytes(x).tolist() == [254, 255, 0, 0, 0, 255, 0, 255, 0, 127, 254]
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    lo, hi = np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2))
    for v in (lo, k, hi):                              # the rule is float32 arithmetic, whatever k / 255 rounds to
        want = np.trunc(np.float32(255) * np.clip(v, 0, 1).astype(np.float32)).astype(np.uint8)
        assert np.array_equal(png_ref.float_to_bytes(v), want)
    assert (png_ref.float_to_bytes(lo)[1:] <= np.arange(1, 256)).all()


def test_heuristic_picks_every_filter_over_the_fixtures_and_streams_round_trip():
    import zlib
    seen = set()
    for name, a in fixtures().items():
        types, _ = png_ref.choose_filters(a)
        seen |= set(types.tolist())
        s = png_ref.filter_stream(a)
        assert len(s) == a.shape[0] * (a.shape[1] * a.shape[2] + 1)
        import struct

        def chunk(t, b):
            return struct.pack(">I", len(b)) + t + b + struct.pack(">I", zlib.crc32(t + b))
        f = png_ref.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", a.shape[1], a.shape[0], 8, 2 if a.shape[2] == 3 else 0, 0, 0, 0)) + \
            chunk(b"IDAT", zlib.compress(s, 1)) + chunk(b"IEND", b"")
        img, got_types, _ = png_ref.read_png(f, want_filters=True)
        assert np.array_equal(img, a) and np.array_equal(got_types, types), name
    assert seen == {0, 1, 2, 3, 4}
    assert png_ref.choose_filters(np.zeros((2, 4, 3), np.uint8))[0].tolist() == [0, 0]      # a tie: None


def test_yardstick_matches_the_fixture():
    z = np.load(GOLD)
    assert int(z["chunk"]) == png_ref.CHUNK
    a = z["frame/decode"]
    assert png_ref.huffman_only_size(a) == int(z["sh/decode"])
