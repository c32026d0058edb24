"""Level 1 of the device PNG encoder (k_png_deflate_dense in vf_png.hip) against its rule
(tests/png_dense_ref.py, through the tokens recorded in tests/golden/png_dense_cases.npz) and against level 0: every file
is a valid PNG of exactly the frame with libpng's filters and level 0's chunks; the tokens of every coded chunk are the
rule's, or level 0's where those code strictly smaller (the rule's fallback); no reference leaves the window; the files are the same on every run and in every batch; level 0 is untouched;
the sizes stand where DESIGN.md 5.3 says."""
import os

import numpy as np
import pytest
import torch

import apng_ref
import png_dense_cases as cases
import png_dense_ref as dense
import png_ref

pytestmark = pytest.mark.gpu

CHUNK, HIST = dense.CHUNK, dense.HIST
# Level 1 against the recorded S_Z(6, HIST) (zlib level 6 on every chunk with the same 8 KiB of history): the excess measured
# on an MI355X, decode -3.60 % (26 988 bytes against 27 996) and padded -3.87 % (27 801 against 28 919), the larger rounded up
# to the next whole percent (DESIGN.md 5.3 has the table).  Sizes are deterministic: no other margin.
M_HIST = -0.03


def enc0(frames):
    from video_filler_amd.data import encode_png
    return encode_png(frames, level=0)


def enc1(frames):
    from video_filler_amd.data import encode_png
    return encode_png(frames, level=1)


@pytest.fixture(scope="module")
def gold():
    return cases.load()


@pytest.fixture(scope="module")
def small_files(hipb, gold):
    """every small case's level-1 file, encoded alone, once"""
    _, frames, _ = gold
    return {name: enc1(a[None])[0] for name, a in frames.items()}


@pytest.fixture(scope="module")
def small_files0(hipb, gold):
    """the same at level 0: the tokens a chunk may fall back to"""
    _, frames, _ = gold
    return {name: enc0(a[None])[0] for name, a in frames.items()}


@pytest.fixture(scope="module")
def fixture_files(hipb):
    fx = cases.fixtures()
    return fx, {name: enc1(a[None])[0] for name, a in fx.items()}, {name: enc0(a[None])[0] for name, a in fx.items()}


def idat_data(f):
    out, pos = b"", 8
    while pos < len(f):
        n = int.from_bytes(f[pos:pos + 4], "big")
        if f[pos + 4:pos + 8] == b"IDAT":
            out += f[pos + 8:pos + 8 + n]
        pos += 12 + n
    return out


def check_file(f, want):
    img, types, idats = png_ref.read_png(f, want_filters=True)
    assert img.shape == want.shape and np.array_equal(img, want)
    assert np.array_equal(types, png_ref.choose_filters(want)[0])
    stream = want.shape[0] * (want.shape[1] * want.shape[2] + 1)
    assert len(idats) == -(-stream // CHUNK)
    return idats


def places(toks):
    p = 0
    for t in toks:
        yield p, t
        p += t[0] if isinstance(t, tuple) else 1


def chunk_tokens(f, frame):
    """-> (token lists, block types, the filtered stream): one deflate block per chunk, each standing for its own bytes
    behind its history, every distance inside the window"""
    s = png_ref.filter_stream(frame)
    blocks, kinds = dense.tokens_of(idat_data(f), kinds=True)
    assert len(blocks) == -(-len(s) // CHUNK)
    for k, tk in enumerate(blocks):
        o = k * CHUNK
        n = min(CHUNK, len(s) - o)
        assert dense.replay(tk, s[max(0, o - HIST):o]) == s[o:o + n], "chunk %d does not stand for its own bytes" % k
        for p, t in places(tk):
            if isinstance(t, tuple):
                assert p + t[0] <= n and t[1] <= min(HIST, o) + p, "chunk %d: match %r at %d leaves the window" % (k, t, p)
    return blocks, kinds, s


def assert_rule_tokens(name, f, frame, want, f0):
    """-> (chunks that show the rule's tokens, the block types).  A stored chunk shows none: its bytes are there instead
    (checked by chunk_tokens).  A chunk may show level 0's tokens (f0: the level-0 file) only as level 0's very IDAT, and
    no IDAT is larger than level 0's."""
    blocks, kinds, s = chunk_tokens(f, frame)
    blocks0 = dense.tokens_of(idat_data(f0))
    idats, idats0 = png_ref.read_png(f, want_filters=True)[2], png_ref.read_png(f0, want_filters=True)[2]
    assert all(x <= y for x, y in zip(idats, idats0)), "%s: a chunk larger than level 0's: %r against %r" % (name, idats, idats0)
    coded = 0
    for k, (got, kind) in enumerate(zip(blocks, kinds)):
        if kind == "stored":
            continue
        if got != want[k] and got == blocks0[k]:
            print("%s, chunk %d: level 0's tokens (%d bytes)" % (name, k, idats0[k]))
            assert idats[k] == idats0[k]
            continue
        coded += 1
        if got != want[k]:
            i = next((j for j, (x, y) in enumerate(zip(got, want[k])) if x != y), min(len(got), len(want[k])))
            at = sum(t[0] if isinstance(t, tuple) else 1 for t in got[:i])
            raise AssertionError("%s, chunk %d: token %d at position %d is %r, the rule gives %r (%d tokens against %d)" % (
                name, k, i, at, got[i] if i < len(got) else None, want[k][i] if i < len(want[k]) else None, len(got), len(want[k])))
    return coded, kinds


# ------------------------------------------------------------------------------------------------------------ 1. contract
def test_every_fixture_and_small_case_is_a_valid_png_of_the_frame(hipb, gold, small_files, fixture_files):
    from video_filler_amd.data import decode_png
    _, frames, _ = gold
    fx, files1, _ = fixture_files
    for group, fl in ((fx, files1), (frames, small_files)):
        for name, a in group.items():
            check_file(fl[name], a)
        back = decode_png([fl[name] for name in group])
        for name, t in zip(group, back):
            assert np.array_equal(t.cpu().numpy(), group[name]), name


# -------------------------------------------------------------------------------------------------------------- 2. tokens
@pytest.mark.parametrize("name", list(cases.SMALL_FIXTURES) + ["decode_crop", "padded_band"])
def test_tokens_are_the_rules(hipb, gold, small_files, small_files0, name):
    _, frames, toks = gold
    coded, kinds = assert_rule_tokens(name, small_files[name], frames[name], toks[name], small_files0[name])
    print(name, kinds, coded)
    if name == "photo_grey" or name.startswith("noise"):
        return         # noise is stored; photographic rows may fall back to level 0's tokens
    assert coded == len(kinds), "%s: %d of %d chunks show the rule's tokens: %r" % (name, coded, len(kinds), kinds)


# ---------------------------------------------------------------------------------------------------------- 3. boundaries
@pytest.mark.parametrize("shape", [(1, 1, 3), (1, 1, 1)])
def test_one_pixel(hipb, shape):
    a = np.full(shape, 201, np.uint8)
    (f,) = enc1(a[None])
    check_file(f, a)
    chunk_tokens(f, a)


@pytest.mark.parametrize("name", ["one_chunk", "two_chunks", "row9000", "flat_run", "period_hist", "period_longer"])
def test_boundary_cases(hipb, gold, small_files, small_files0, name):
    _, frames, toks = gold
    a, f = frames[name], small_files[name]
    idats = check_file(f, a)
    coded, kinds = assert_rule_tokens(name, f, a, toks[name], small_files0[name])
    blocks, _, s = chunk_tokens(f, a)
    if name == "one_chunk":
        assert len(s) == CHUNK and len(idats) == 1
    if name == "two_chunks":
        assert len(s) == 2 * CHUNK and len(idats) == 2
    if name == "row9000":
        assert len(s) == CHUNK + 809 and len(idats) == 2 and coded == 2
    if name == "flat_run":                   # one run of zeros over three chunks: each chunk's tokens end at its own end
        assert coded == 3 and blocks[1][0] == (258, 1) and blocks[2][0] == (258, 1)
        assert all(sum(t[0] if isinstance(t, tuple) else 1 for t in b) == CHUNK for b in blocks)
    if name == "period_hist":                # a byte period of exactly HIST: the window's far end is in reach
        for k in (1, 2):
            assert kinds[k] == "dynamic" and any(isinstance(t, tuple) and t[1] == HIST for t in blocks[k]), k
    if name == "period_longer":              # HIST + 128: out of reach before position 128 of a chunk
        for k in (1, 2, 3):
            for p, t in places(blocks[k]):
                if kinds[k] != "stored" and isinstance(t, tuple) and t[0] >= 8:
                    assert p >= 128 and t[1] == HIST + 128, (k, p, t)


def test_second_frame_of_a_batch_does_not_reach_into_the_first(hipb, gold):
    """frame 1 begins with the bytes frame 0 ends with, which the workspace holds right in front of it"""
    _, frames, _ = gold
    a = frames["period_hist"]
    b = np.ascontiguousarray(np.roll(a, 1, axis=0))        # its first rows are a's last: a match at distance HIST is on offer
    files = enc1(np.stack([a, b]))
    blocks, kinds, _ = chunk_tokens(files[1], b)           # chunk 0: every distance is at most its position
    assert files[1] == enc1(b[None])[0] and files[0] == enc1(a[None])[0]
    flat = np.zeros((2, 192, 127, 1), np.uint8)
    f0, f1 = enc1(flat)
    assert f0 == f1
    assert chunk_tokens(f1, flat[1])[0][0][0] == 0, "the first token of a frame is a literal"


# ------------------------------------------------------------------------------------------ 4. determinism and batching
def test_same_bytes_over_repeats_and_batch_compositions(hipb, fixture_files):
    fx, files1, _ = fixture_files
    a, b, c = fx["photo"], fx["padded"], cases.texture(384, 512, 3)
    first = enc1(np.stack([a, b, c]))
    assert first[0] == files1["photo"] and first[1] == files1["padded"]
    for _ in range(2):
        assert enc1(np.stack([a, b, c])) == first
    assert enc1(np.stack([c, a])) == [first[2], first[0]]
    assert enc1(np.stack([b, b, a, c, b])) == [first[1], first[1], first[0], first[2], first[1]]
    check_file(first[2], c)


def test_257_files_of_one_batch_stand_where_the_sizes_before_them_say(hipb):
    a = ((np.arange(257) * 37) & 255).astype(np.uint8).reshape(257, 1, 1, 1)
    buf, offsets = hipb.png_encode(torch.from_numpy(a).cuda(), level=1)
    offs = offsets.cpu().tolist()
    files = enc1(a)
    assert len(files) == 257
    assert offs == np.concatenate([[0], np.cumsum([len(f) for f in files])]).tolist()
    assert buf[:offs[-1]].cpu().numpy().tobytes() == b"".join(files)
    for i, f in enumerate(files):
        check_file(f, a[i])
    assert [files[255], files[256]] == enc1(a[255:256]) + enc1(a[256:])


def test_float_frames_and_their_bytes_give_the_same_files(hipb):
    x = (cases.noise_bytes(2 * 3 * 37 * 53, 9).reshape(2, 3, 37, 53).astype(np.float32) - 32) / np.float32(190)
    x[:, :, 10:30] = np.linspace(-0.1, 1.1, 53, dtype=np.float32)           # ramps, so that chunks are coded
    want = png_ref.chw_to_hwc_bytes(x)
    files = enc1(torch.from_numpy(x))
    assert files == enc1(want)
    for i, f in enumerate(files):
        check_file(f, want[i])


# ------------------------------------------------------------------------------------------------------ 5. level 0 untouched
def test_level_0_is_the_encoder_without_the_argument(hipb, fixture_files):
    from video_filler_amd.data import encode_png
    fx, files1, files0 = fixture_files
    for name, a in fx.items():
        assert encode_png(a[None]) == [files0[name]], name
    assert any(files0[n] != files1[n] for n in fx)


# --------------------------------------------------------------------------------------------------------------- 6. sizes
def test_sizes(hipb, gold, fixture_files):
    z, _, _ = gold
    fx, files1, files0 = fixture_files
    for name in fx:
        print("%s: level 1 %d bytes, level 0 %d" % (name, len(files1[name]), len(files0[name])))
    for name in cases.SIZED:
        s0, sh = int(z["sz0/" + name]), int(z["szh/" + name])
        n1 = len(files1[name])
        print("%s: level 1 %d bytes, S_Z(6, 0) %d (%+.2f %%), S_Z(6, HIST) %d (%+.2f %%)" % (
            name, n1, s0, 100.0 * (n1 / s0 - 1), sh, 100.0 * (n1 / sh - 1)))
    for name in fx:
        assert len(files1[name]) <= len(files0[name]), name
    for name in ("decode", "padded"):
        assert len(files1[name]) < int(z["sz0/" + name]), name
        assert len(files1[name]) <= (1 + M_HIST) * int(z["szh/" + name]), name


# ---------------------------------------------------------------------------------------------------------------- 7. APNG
def test_apng_is_assembled_from_the_level_1_files(hipb, gold):
    from video_filler_amd.data import decode_apng, encode_apng
    _, frames, _ = gold
    a = frames["decode_crop"]
    clip = np.stack([a, a[::-1].copy(), np.ascontiguousarray(a[:, ::-1])])
    (f,) = encode_apng(clip[None], delay=7, loop=2, level=1)
    assert f == apng_ref.assemble(enc1(clip), 7, 2)
    assert f != encode_apng(clip[None], delay=7, loop=2)[0]
    assert encode_apng(clip[None], delay=7, loop=2, level=0) == encode_apng(clip[None], delay=7, loop=2)
    (back,) = decode_apng([f])
    assert np.array_equal(back.cpu().numpy(), clip)


# ----------------------------------------------------------------------------------------------------------- 8. refusals
@pytest.mark.parametrize("level", [2, -1])
def test_a_bad_level_is_refused_by_name(hipb, tmp_path, level):
    from video_filler_amd import inference
    from video_filler_amd.data import encode_apng, encode_png
    a = np.zeros((2, 4, 4, 3), np.uint8)
    with pytest.raises(ValueError, match="level"):
        encode_png(a, level=level)
    with pytest.raises(ValueError, match="level"):
        encode_apng(a[None], level=level)
    with pytest.raises(ValueError, match="level"):
        hipb.png_encode(torch.from_numpy(a).cuda(), level=level)
    d = tmp_path / "frames"
    with pytest.raises(ValueError, match="level"):
        inference.save_frames(str(d), torch.zeros(2, 3, 4, 4), level=level)
    assert not d.exists() and os.listdir(str(tmp_path)) == []


def test_save_frames_at_level_1_writes_the_level_1_files(hipb, tmp_path):
    from video_filler_amd import inference
    x = torch.from_numpy(cases.texture(40, 60, 3).astype(np.float32).transpose(2, 0, 1)[None] / np.float32(255))
    paths = inference.save_frames(str(tmp_path / "f"), pred=x, level=1)
    with open(paths[0], "rb") as fh:
        assert fh.read() == enc1(x)[0]
