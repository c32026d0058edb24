"""tests/png_dense_ref.py, the rule of the PNG encoder's level 1, on the CPU: its recording inflate against
zlib's, its tokens against the bytes they stand for and the window they may reach into, its size estimate against the
recorded yardsticks, and the recorded fixture against what the running NumPy and zlib compute."""
import io
import zlib

import numpy as np
import pytest

import png_dense_cases as cases
import png_dense_ref as dense
import png_ref


@pytest.fixture(scope="module")
def gold():
    return cases.load()


@pytest.fixture(scope="module")
def estimates():
    fx = cases.fixtures()
    return {name: dense.estimate_size(fx[name]) for name in ("photo", "decode", "padded", "noise")}


def payloads():
    fx = cases.fixtures()
    return [png_ref.filter_stream(fx["photo_grey"]), png_ref.filter_stream(fx["dramp"])[:20000], bytes(3000), b"abc" * 700 + bytes(range(256)),
            cases.noise_bytes(5000, 1).tobytes(), b"", b"x"]


@pytest.mark.parametrize("level", [1, 6, 9])
def test_tokens_of_replays_to_what_zlib_decompresses(level):
    for data in payloads():
        z = zlib.compress(data, level)
        blocks = dense.tokens_of(z)
        assert dense.replay([t for b in blocks for t in b]) == zlib.decompress(z) == data
        zd = data[:1000][::-1] + b"dictionary"
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY, zd)
        raw = co.compress(data) + co.flush()
        blocks = dense.tokens_of(raw, raw=True)
        do = zlib.decompressobj(-15, zd)
        assert dense.replay([t for b in blocks for t in b], zd) == do.decompress(raw) == data
    # fixed and stored blocks, and the empty stored blocks of a sync flush, which are skipped
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_FIXED)
    raw = co.compress(b"hello hello hello") + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(b" again") + co.flush()
    blocks, kinds = dense.tokens_of(raw, raw=True, kinds=True)
    assert kinds == ["fixed", "fixed"] and dense.replay(blocks[0]) == b"hello hello hello"
    assert dense.replay(blocks[1], b"hello hello hello") == b" again"
    co = zlib.compressobj(0, zlib.DEFLATED, -15)
    raw = co.compress(b"stored bytes") + co.flush()
    blocks, kinds = dense.tokens_of(raw, raw=True, kinds=True)
    assert kinds == ["stored"] and blocks == [list(b"stored bytes")]


def test_tokens_of_reads_pillow_files():
    Image = pytest.importorskip("PIL.Image")
    fx = cases.fixtures()
    for name in ("photo_grey", "dramp", "flat"):
        a = fx[name]
        bio = io.BytesIO()
        Image.fromarray(a[..., 0] if a.shape[2] == 1 else a).save(bio, "PNG", compress_level=6)
        data = bio.getvalue()
        idat, pos = b"", 8
        while pos < len(data):
            n = int.from_bytes(data[pos:pos + 4], "big")
            if data[pos + 4:pos + 8] == b"IDAT":
                idat += data[pos + 8:pos + 8 + n]
            pos += 12 + n
        blocks = dense.tokens_of(idat)
        assert dense.replay([t for b in blocks for t in b]) == zlib.decompress(idat)


def token_places(toks):
    p = 0
    for t in toks:
        yield p, t
        p += t[0] if isinstance(t, tuple) else 1


def test_rule_tokens_reproduce_every_chunk_inside_the_window(gold):
    z, frames, toks = gold
    assert int(z["chunk"]) == dense.CHUNK and int(z["hist"]) == dense.HIST
    assert set(toks) == set(frames) and len(frames) == 16
    for name, a in frames.items():
        s = png_ref.filter_stream(a)
        assert len(toks[name]) == -(-len(s) // dense.CHUNK)
        for k, tk in enumerate(toks[name]):
            o = k * dense.CHUNK
            n = min(dense.CHUNK, len(s) - o)
            assert dense.replay(tk, s[max(0, o - dense.HIST):o]) == s[o:o + n], (name, k)
            for p, t in token_places(tk):
                if isinstance(t, tuple):
                    assert 3 <= t[0] <= 258 and p + t[0] <= n, "%s chunk %d: a match crosses the chunk's end" % (name, k)
                    assert 1 <= t[1] <= min(dense.HIST, o) + p and t[1] <= 32768, "%s chunk %d: distance %d at %d" % (name, k, t[1], p)


def test_recorded_tokens_are_what_the_rule_gives_here(gold):
    _, frames, toks = gold
    made = cases.small_cases()
    for name in ("decode_crop", "padded_band", "row9000", "flat_run", "period_hist", "one_chunk", "flat", "noise_grey"):
        assert np.array_equal(made[name], frames[name])
        s = png_ref.filter_stream(frames[name])
        assert [dense.tokens(s, k) for k in range(len(toks[name]))] == toks[name], name


def test_boundary_cases_hold_what_they_are_for(gold):
    _, frames, toks = gold
    assert [len(png_ref.filter_stream(frames[n])) for n in ("one_chunk", "two_chunks", "row9000")] == [8192, 16384, 9001]
    assert any(t == (258, 1) for t in toks["flat_run"][1]) and toks["flat_run"][1][0] == (258, 1)
    for k in (1, 2):
        assert any(isinstance(t, tuple) and t[1] == dense.HIST for t in toks["period_hist"][k])
    for k in (1, 2, 3):           # a period of HIST + 128: no position before 128 can reach it
        for p, t in token_places(toks["period_longer"][k]):
            assert not isinstance(t, tuple) or (p >= 128 and t[1] == dense.HIST + 128) or t[0] < 8, (k, p, t)


def test_recorded_yardsticks_are_the_design_tables_and_the_running_zlibs(gold):
    z, _, _ = gold
    want = {"photo": (335928, 330433), "decode": (32015, 27996), "padded": (33314, 28919)}
    fx = cases.fixtures()
    for name, (s0, sh) in want.items():
        assert (int(z["sz0/" + name]), int(z["szh/" + name])) == (s0, sh)
    for name in ("decode", "padded"):     # zlib's output depends on its build: the running one against the record
        assert dense.zlib_chunked_size(fx[name], 6, 0) == want[name][0]
        assert dense.zlib_chunked_size(fx[name], 6, dense.HIST) == want[name][1]


def test_estimate_is_below_zlib_level_6_without_history_on_smooth_frames(gold, estimates):
    z, _, _ = gold
    for name in ("decode", "padded"):
        print(name, estimates[name], int(z["sz0/" + name]))
        assert estimates[name] < int(z["sz0/" + name])


def test_estimate_is_not_above_level_0_where_matches_do_not_pay(estimates):
    fx = cases.fixtures()
    stream = len(png_ref.filter_stream(fx["noise"]))
    stored = stream + 5 * -(-stream // dense.CHUNK) + png_ref.framing_bytes(stream)      # level 0's file: every chunk stored
    print(estimates["photo"], estimates["noise"], stored)
    assert estimates["photo"] <= 289654        # level 0's file
    assert estimates["noise"] <= stored == 37096
