"""The device APNG encoder (vf_apng_encode in vf_png.hip) against its definition: every file equals
apng_ref.assemble(data.encode_png(frames of the clip), delay, loop) byte for byte — for grey and RGB, bytes and floats,
clips of 1, 2 and 5 frames, alone and in a batch, stored and coded blocks, one chunk and several, on every run — and an
independent reader (Pillow) gets the frames' bytes back."""
import io
import os

import numpy as np
import pytest
import torch

import apng_ref
import png_ref

pytestmark = pytest.mark.gpu

# H, W, C: a pixel; a stream of exactly 8192 bytes, one chunk; a second chunk of 256 bytes; again exactly 8192, grey; four
# chunks, so that fdAT numbering runs inside a frame
GEOMETRIES = [(1, 1, 3), (1, 1, 1), (32, 85, 3), (33, 85, 3), (64, 127, 1), (64, 128, 3), (64, 128, 1)]


def enc(clips, delay=10, loop=0):
    from video_filler_amd.data import encode_apng
    return encode_apng(clips, delay, loop)


def png(frames):
    from video_filler_amd.data import encode_png
    return encode_png(frames)


def frame(kind, H, W, C, seed):
    """noise: stored blocks; flat and ramp: coded blocks; mixed: noise above a ramp, both kinds in one frame"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "noise":
        f = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    elif kind == "flat":
        f = np.full((H, W, C), seed * 37 & 255, np.uint8)
    elif kind == "ramp":
        f = np.stack([(xx * (c + 1) + yy * 2 + seed) & 255 for c in range(C)], -1).astype(np.uint8)
    else:
        f = np.stack([(xx + yy * (c + 1) + seed) & 255 for c in range(C)], -1).astype(np.uint8)
        f[:H // 2] = rng.integers(0, 256, (H // 2, W, C), dtype=np.uint8)
    return f


KINDS = ("noise", "flat", "ramp", "mixed")


def clip(n, H, W, C, first):
    return np.stack([frame(KINDS[(first + j) % 4], H, W, C, 11 * first + j) for j in range(n)])


def first_difference(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


def check(files, clips, delay, loop, what):
    assert len(files) == len(clips)
    for i, (f, c) in enumerate(zip(files, clips)):
        want = apng_ref.assemble(png(c), delay, loop)
        assert f == want, "%s, clip %d: %d bytes against %d, first difference at %d" % (what, i, len(f), len(want), first_difference(f, want))


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_files_equal_the_rule_byte_for_byte(hipb, geom):
    H, W, C = geom
    stream = H * (W * C + 1)
    if geom in ((32, 85, 3), (64, 127, 1)):
        assert stream == 8192
    if geom == (33, 85, 3):
        assert stream == 8192 + 256
    if geom == (64, 128, 3):
        assert -(-stream // png_ref.CHUNK) == 4
    for n in (1, 2, 5):
        batch = np.stack([clip(n, H, W, C, g) for g in range(3)])
        for delay, loop in ((0, 0), (65535, 3), (10, 0)):
            files = enc(batch, delay, loop)
            check(files, batch, delay, loop, "%dx%dx%d n=%d delay=%d loop=%d" % (H, W, C, n, delay, loop))
        for g in range(3):                                   # each clip alone equals its place in the batch
            assert enc(batch[g:g + 1], 10, 0) == [files[g]]
        assert enc(batch[1], 10, 0) == [files[1]]            # a 4-D input is one clip
    assert enc(batch, 10, 0) == files                        # two runs identical


@pytest.mark.parametrize("geom", [(33, 85, 3), (64, 127, 1), (1, 1, 1)])
def test_float_input_follows_the_truncating_rule(hipb, geom):
    H, W, C = geom
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    near = np.concatenate([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2)),
                           np.array([-0.0, -1e-9, -3.5, 1.0000001, 7.0, np.inf, -np.inf, np.nan, 0.999999, 1e-45, 0.5], np.float32)])
    rng = np.random.default_rng(5)
    x = rng.uniform(-0.25, 1.25, (3, 2, C, H, W)).astype(np.float32)
    m = min(near.size, x[0].size)
    x[0].reshape(-1)[:m] = near[:m]
    x[2].reshape(-1)[-m:] = near[::-1][:m]
    u8 = np.stack([png_ref.chw_to_hwc_bytes(c) for c in x])
    files = enc(torch.from_numpy(x), 7, 2)
    check(files, u8, 7, 2, "float %dx%dx%d" % geom)
    assert enc(u8, 7, 2) == files
    assert enc(torch.from_numpy(x).double().cuda(), 7, 2) == files
    for f, c in zip(files, x):                               # the float frames themselves through encode_png
        assert f == apng_ref.assemble(png(torch.from_numpy(c)), 7, 2)


@pytest.mark.parametrize("geom", [(1, 1, 3), (33, 85, 3), (64, 127, 1), (64, 128, 3)])
def test_pillow_reads_the_frames_back_and_decode_png_gives_frame_0(hipb, geom):
    from PIL import Image
    from video_filler_amd import data
    H, W, C = geom
    for n, delay, loop in ((1, 10, 0), (5, 3, 3)):
        c = clip(n, H, W, C, 2)
        (f,) = enc(c, delay, loop)
        im = Image.open(io.BytesIO(f))
        assert im.size == (W, H) and getattr(im, "n_frames", 1) == n
        for k in range(n):
            im.seek(k)
            got = np.asarray(im.convert("L" if C == 1 else "RGB")).reshape(H, W, C)
            assert np.array_equal(got, c[k]), "frame %d" % k
            if n > 1:
                assert im.info["duration"] == 10 * delay and im.info["loop"] == loop
        r = apng_ref.read(f)
        assert r["frames"] == n and r["loop"] == loop and r["seqs"] == list(range(len(r["seqs"])))
        assert r["delays"] == [(delay, 100)] * n
        (d0,) = data.decode_png([f])                         # the existing decoder, unchanged: the default image
        assert np.array_equal(d0.cpu().numpy().reshape(H, W, C), c[0])
        assert data.png_info(f)["idat_chunks"] == -(-H * (W * C + 1) // png_ref.CHUNK)


def test_257_clips_and_300_frames_stand_where_the_scans_say(hipb):
    """257 clips: one into the second 256-wide round of the file-offset scan; 300 frames: one round and a tail of the clip scan"""
    k = np.arange(257 * 2)
    clips = np.stack([k & 255, (k * 7) & 255, k >> 8], -1).astype(np.uint8).reshape(257, 2, 1, 1, 3)
    files = enc(clips)
    assert len(files) == 257
    one = png(clips.reshape(-1, 1, 1, 3))
    for g, f in enumerate(files):
        assert f == apng_ref.assemble(one[2 * g:2 * g + 2], 10, 0)
    long = np.stack([frame(KINDS[j % 4], 3, 5, 3, j) for j in range(300)])
    (f,) = enc(long, 1, 0)
    assert f == apng_ref.assemble(png(long), 1, 0)


def test_refusals_name_the_argument(hipb):
    with pytest.raises(ValueError, match="16385"):
        enc(np.zeros((1, 1, 1, 16385, 3), np.uint8))
    with pytest.raises(ValueError, match="2 channels"):
        enc(np.zeros((1, 2, 4, 4, 2), np.uint8))
    with pytest.raises(ValueError, match="delay=70000"):
        enc(np.zeros((1, 2, 4, 4, 3), np.uint8), 70000)
    with pytest.raises(ValueError, match="loop=-1"):
        enc(np.zeros((1, 2, 4, 4, 3), np.uint8), 10, -1)
    with pytest.raises(ValueError, match="0 frames"):
        enc(np.zeros((1, 0, 4, 4, 3), np.uint8))
    with pytest.raises(ValueError, match="3 dimensions"):
        enc(np.zeros((4, 4, 3), np.uint8))
    with pytest.raises(ValueError, match="int32"):
        enc(np.zeros((1, 2, 4, 4, 3), np.int32))


def test_save_apngs_writes_the_named_files_and_keeps_the_last_frame(hipb, tmp_path):
    from PIL import Image
    from video_filler_amd import inference
    outs = [torch.from_numpy(clip(4, 64, 96, 3, g).astype(np.float32).transpose(0, 3, 1, 2) / np.float32(255)).cuda() for g in range(3)]
    name = str(tmp_path / "clips" / "v0")
    paths = inference.save_apngs(name, *outs)
    assert paths == [name + s for s in ("_result.png", "_inpaint.png", "_orig.png")]
    assert sorted(os.listdir(tmp_path / "clips")) == ["v0_inpaint.png", "v0_orig.png", "v0_result.png"]
    for p, t in zip(paths, outs):
        with open(p, "rb") as fh:
            data = fh.read()
        im = Image.open(io.BytesIO(data))
        assert im.n_frames == 4 and im.info["duration"] == 100 and im.info["loop"] == 0
        u8 = png_ref.chw_to_hwc_bytes(t.cpu().numpy())
        im.seek(3)
        assert np.array_equal(np.asarray(im.convert("RGB")), u8[3])
        assert [data] == enc(t) and data == apng_ref.assemble(png(u8), 10, 0)
    (p,) = inference.save_apngs(str(tmp_path / "vid" / "result"), pred=outs[0], delay=5)
    assert os.path.basename(p) == "result_pred.png"
    with open(p, "rb") as fh:
        assert [fh.read()] == enc(outs[0], 5)
