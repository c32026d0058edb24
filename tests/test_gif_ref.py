"""tests/gif_ref.py, the definition the device GIF encoder (vf_gif.hip) must equal byte for byte, against an
independent reader (Pillow) and against its own strict reader.  Host only."""
import io

import numpy as np
import pytest

from PIL import Image as PIL_Image

import gif_cases
import gif_ref

GEOMETRIES = [(53, 37), (71, 59), (96, 64), (1, 1), (1, 300), (300, 1)]
# Quantiser quality against Pillow's quantize(256, MEDIANCUT, dither NONE), mean squared error over the frame.  Measured
# (this test prints it): photo 192 x 256: 12.17 against 19.55 (-37.7 %), smooth 192 x 256: 3.60 against 8.43 (-57.3 %);
# 384 x 512: -38.3 % and -42.1 %.  The rule here is never worse on the fixtures, so the margin is zero.
Q = 0.0
# Size of the chunked stream against the same coder with the standard Clear policy, for GIF_CHUNK = 3824.  Measured (printed
# here): photo 192 x 256 -2.0 %, smooth 192 x 256 +3.9 %; the largest, rounded up.  (At 384 x 512, where the unchunked
# dictionary lives far longer than a chunk: +9.0 % and +41.7 %; at GIF_CHUNK = 2048 +17 % and +70 %.)
M = 0.05


@pytest.fixture(scope="module")
def big():
    out = {}
    for name, mk in (("photo", gif_cases.photo), ("smooth", gif_cases.smooth)):
        fr = mk(192, 256)
        out[name] = (fr,) + gif_ref.quantize(fr)
    return out


def mse(a, b):
    return float(((a.astype(np.int64) - b.astype(np.int64)) ** 2).mean())


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_pillow_and_the_strict_reader_accept_every_fixture(geom):
    H, W = geom
    stats = {512: 0, 1024: 0, 2048: 0}
    for i, (name, fr) in enumerate(gif_cases.contents(H, W).items()):
        D = (5, 10)[i % 2]
        clip = np.stack([fr, fr[::-1, ::-1].copy(), fr])
        data = gif_ref.encode(clip, D)
        r = gif_ref.read_gif(data)
        assert r["size"] == (W, H) and r["loop"] == 0 and r["delays"] == [D] * 3
        assert all(c == -(-H * W // gif_ref.CHUNK) for c in r["clears"])
        im = PIL_Image.open(io.BytesIO(data))
        assert im.n_frames == 3 and im.info["loop"] == 0
        for k in range(3):
            im.seek(k)
            assert im.info["duration"] == 10 * D
            want = r["tables"][k][r["frames"][k]]
            assert np.array_equal(np.asarray(im.convert("RGB")), want), "%s frame %d" % (name, k)
            table, idx = gif_ref.quantize(clip[k])
            assert np.array_equal(table, r["tables"][k]) and np.array_equal(idx, r["frames"][k])
            if len(np.unique(clip[k].reshape(-1, 3), axis=0)) <= 256:
                assert np.array_equal(want, clip[k]), "%s: <= 256 colours must round-trip" % name
        for k, v in gif_ref.lzw(r["frames"][0], want_stats=True)[1].items():
            if k in stats:
                stats[k] += v
    if H * W >= gif_ref.CHUNK:
        geom_hits = {(71, 59): (512, 1024), (96, 64): (1024, 2048)}[geom]
        assert all(stats[k] >= 1 for k in geom_hits), stats


def test_every_width_boundary_occurs_and_is_followed_by_a_wider_code():
    seen = {512: 0, 1024: 0, 2048: 0}
    for H, W in ((71, 59), (96, 64)):
        fr = gif_cases.boundary(H, W)
        table, idx = gif_ref.quantize(fr)
        assert np.array_equal(table[idx], fr)
        data, stats = gif_ref.lzw(idx, want_stats=True)
        for k in seen:
            seen[k] += stats[k]
        got, clears = gif_ref._unlzw(data, H * W)
        assert np.array_equal(got, idx.reshape(-1)) and clears == 2
    assert all(v >= 1 for v in seen.values()), seen
    # the first chunk of the 71 x 59 frame makes 767 codes: its last code is 10 bits wide, the Clear behind it 11
    assert gif_ref.code_width(767) == 10 and gif_ref.code_width(768) == 11
    assert gif_ref.code_width(255) == 9 and gif_ref.code_width(256) == 10 and gif_ref.code_width(1792) == 12
    assert gif_ref.code_width(gif_ref.CHUNK + 1) == 12 and gif_ref.FIRST + gif_ref.CHUNK <= 4096


def test_the_strict_reader_rejects_one_wrong_structural_byte():
    fr = gif_cases.photo(53, 37)
    data = gif_ref.encode(np.stack([fr, fr]), 5)
    gif_ref.read_gif(data)
    first_block = 32 + 8 + 10 + 768 + 1
    assert data[first_block] == 255, "the frame's data is longer than one sub-block"
    spots = {"signature": 4, "logical screen flags": 10, "loop count": 29, "disposal": 32 + 3, "transparent index": 32 + 6,
             "descriptor flags": 32 + 8 + 9, "image left": 32 + 8 + 1, "minimum code size": first_block - 1,
             "sub-block length": first_block, "trailer": len(data) - 1}
    for what, at in spots.items():
        bad = bytearray(data)
        bad[at] ^= 0x01
        with pytest.raises(gif_ref.GifError):
            gif_ref.read_gif(bytes(bad))
            pytest.fail("a wrong %s was accepted" % what)
    with pytest.raises(gif_ref.GifError):
        gif_ref.read_gif(data + b"\x00")
    with pytest.raises(gif_ref.GifError):
        gif_ref.read_gif(data[:-2] + b"\x3b")


def test_table_rules():
    # <= 256 colours: ascending, zero-padded, lossless
    fr = gif_cases.n_colours(20, 20, 256)
    table, idx = gif_ref.quantize(fr)
    keys = table.astype(np.int64) @ np.array([65536, 256, 1])
    assert np.all(np.diff(keys) > 0) and np.array_equal(table[idx], fr)
    fr = gif_cases.two_colour(9, 11)
    table, idx = gif_ref.quantize(fr)
    assert table[:2].tolist() == [[0, 32, 0], [255, 255, 255]] and not table[2:].any() and np.array_equal(table[idx], fr)
    # 257 colours: median cut; every entry is the rounded mean of the pixels of its box, the index the nearest entry
    fr = gif_cases.n_colours(20, 20, 257)
    table, idx = gif_ref.quantize(fr)
    assert not np.array_equal(table[idx], fr)
    px = fr.reshape(-1, 3).astype(np.int64)
    d = ((px[:, None, :] - table[None].astype(np.int64)) ** 2).sum(2)
    assert np.array_equal(idx.reshape(-1), d.argmin(1))
    # two colours in one histogram cell besides 255 others: nothing can split that cell
    hist = np.zeros((32, 32, 32), np.int64)
    hist[3, 4, 5] = 10
    assert gif_ref.median_cut_boxes(hist) == [(3, 3, 4, 4, 5, 5)]
    hist[3, 4, 9] = 10
    hist[20, 4, 5] = 1
    assert gif_ref.median_cut_boxes(hist) == [(3, 3, 4, 4, 5, 5), (20, 20, 4, 4, 5, 5), (3, 3, 4, 4, 9, 9)]


def test_quality_is_not_below_pillows_median_cut(big):
    for name, (fr, table, idx) in big.items():
        ours = mse(table[idx], fr)
        pq = PIL_Image.fromarray(fr).quantize(256, method=PIL_Image.Quantize.MEDIANCUT, dither=PIL_Image.Dither.NONE)
        theirs = mse(np.asarray(pq.convert("RGB")), fr)
        print("%s: mse %.3f, Pillow %.3f (%+.1f %%)" % (name, ours, theirs, 100 * (ours / theirs - 1)))
        assert ours <= (1 + Q) * theirs


def test_chunked_stream_is_close_to_the_unchunked_one(big):
    for name, (_, _, idx) in big.items():
        ours, base = len(gif_ref.lzw(idx)), gif_ref.lzw_unchunked_size(idx)
        print("%s: %d bytes, unchunked %d (%+.1f %%)" % (name, ours, base, 100 * (ours / base - 1)))
        assert ours <= (1 + M) * base
