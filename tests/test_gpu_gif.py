"""The device GIF encoder (vf_gif.hip) against its definition, tests/gif_ref.py: byte equality for every
fixture in clips of 1, 2 and 5 frames, the float rule, independence of batch and position, determinism, save_gifs."""
import io
import os

import numpy as np
import pytest
import torch

import gif_cases
import gif_ref
import png_ref

pytestmark = pytest.mark.gpu

# 53 x 37: less than one chunk, more than one sub-block; 71 x 59: a whole chunk and a tail of 365; 96 x 64: a whole chunk and
# a tail of 2320 (the 2048 boundary fits in it); a pixel; a row; a column
GEOMETRIES = [(53, 37), (71, 59), (96, 64), (1, 1), (1, 300), (300, 1)]
_BODIES = {}


def enc(clips, delay=10):
    from video_filler_amd.data import encode_gif
    return encode_gif(clips, delay)


def bodies(H, W):
    """name -> (frame, its bytes from image descriptor to block terminator by the reference): computed once per geometry"""
    if (H, W) not in _BODIES:
        _BODIES[H, W] = {k: (fr, gif_ref.frame_body(fr)) for k, fr in gif_cases.contents(H, W).items()}
    return _BODIES[H, W]


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_files_equal_the_reference_byte_for_byte(hipb, geom):
    H, W = geom
    fx = bodies(H, W)
    names = list(fx)
    if H * W >= gif_ref.CHUNK:
        assert "boundary" in names
    for n in (1, 2, 5):
        clips = [[names[(i + j) % len(names)] for j in range(n)] for i in range(len(names))]     # every fixture in every position
        batch = np.stack([np.stack([fx[k][0] for k in c]) for c in clips])
        for delay in (5, 10):
            files = enc(batch, delay)
            assert len(files) == len(clips)
            for c, f in zip(clips, files):
                want = gif_ref.assemble([fx[k][1] for k in c], W, H, delay)
                assert f == want, "%dx%d, clip %s, delay %d: %d bytes against %d, first difference at %d" % (
                    H, W, c, delay, len(f), len(want), next((i for i, (x, y) in enumerate(zip(f, want)) if x != y), -1))
    f = enc(batch[:1], 10)[0]                                        # an independent reader agrees
    from PIL import Image
    im = Image.open(io.BytesIO(f))
    r = gif_ref.read_gif(f)
    assert im.n_frames == 5 and im.info["loop"] == 0 and im.info["duration"] == 100
    for k in range(5):
        im.seek(k)
        assert np.array_equal(np.asarray(im.convert("RGB")), r["tables"][k][r["frames"][k]])


def test_float_input_follows_the_truncating_rule(hipb):
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    near = np.concatenate([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2)),
                           np.array([-0.0, -1e-9, -3.5, 1.0000001, 7.0, np.inf, -np.inf, np.nan, 0.999999, 1e-45, 0.5], np.float32)])
    rng = np.random.default_rng(5)
    x = rng.uniform(-0.25, 1.25, (2, 3, 37, 53)).astype(np.float32)
    x.reshape(-1)[:near.size] = near
    x[1].reshape(-1)[-near.size:] = near[::-1]
    u8 = png_ref.chw_to_hwc_bytes(x)
    (want,) = enc(u8, 5)
    assert want == gif_ref.encode(u8, 5)
    assert enc(torch.from_numpy(x), 5) == [want]
    assert enc(torch.from_numpy(x).double().cuda()[None], 5) == [want]


def test_a_clip_and_a_frame_are_the_same_wherever_they_stand(hipb):
    fx = bodies(71, 59)
    a = np.stack([fx[k][0] for k in ("photo", "boundary", "noise")])
    b = np.stack([fx[k][0] for k in ("two_colour", "photo", "colours_257")])
    c = np.stack([fx[k][0] for k in ("constant", "colours_256", "photo")])
    (alone,) = enc(a)
    assert enc(np.stack([a, b, c]))[0] == alone and enc(np.stack([b, c, a]))[2] == alone
    # the photo frame's span, graphic control extension to terminator: first of a, second of b, third of c
    span = len(gif_ref.control(10)) + len(fx["photo"][1])
    fa, fb, fc = enc(np.stack([a, b, c]))
    at_b = 32 + 8 + len(fx["two_colour"][1])
    at_c = 32 + 16 + len(fx["constant"][1]) + len(fx["colours_256"][1])
    assert fa[32:32 + span] == fb[at_b:at_b + span] == fc[at_c:at_c + span] == gif_ref.control(10) + fx["photo"][1]
    assert len(fc) == at_c + span + 1


def test_two_runs_give_the_same_bytes(hipb):
    fx = bodies(96, 64)
    batch = np.stack([np.stack([fx[k][0] for k in ("photo", "noise", "colours_257", "boundary")])] * 3)
    first = enc(batch)
    assert enc(batch) == first and first[0] == first[1] == first[2]


def test_more_chunks_than_dictionaries_take_turns(hipb):
    """32 768 dictionaries at most live in the workspace; a batch of more chunks than that walks them in rounds"""
    H, W, n = 1, 300, 33000
    kinds = [gif_cases.noise(H, W, seed=s) for s in range(3)] + [gif_cases.photo(H, W), gif_cases.two_colour(H, W)]
    body = [gif_ref.frame_body(fr) for fr in kinds]
    pick = np.random.default_rng(9).integers(0, len(kinds), n)
    (f,) = enc(torch.from_numpy(np.stack(kinds))[torch.from_numpy(pick)])
    assert f == gif_ref.assemble([body[i] for i in pick], W, H, 10)


def bands(H, W):
    """at most 256 colours (the reference's lossless path), in runs of several lengths: chunks of many different bit counts"""
    yy, xx = np.mgrid[0:H, 0:W]
    g = (((xx // 7) * 3 + (yy // 5) * 11 + (xx * yy) // 4096) & 255).astype(np.uint8)
    return np.stack([g, 255 - g, g // 2], -1)


@pytest.mark.parametrize("geom", [(1024, 956), (1024, 957)])
def test_a_frame_of_256_and_of_257_chunks(hipb, geom):
    """1024 x 956 pixels are exactly 256 chunks, one whole 256-wide round of the frame's bit-offset scan; 1024 x 957 are 257,
    one chunk into the second round"""
    H, W = geom
    assert -(-H * W // gif_ref.CHUNK) == (256 if W == 956 else 257) and (W != 956 or H * W % gif_ref.CHUNK == 0)
    fr = bands(H, W)
    assert len(np.unique(fr.reshape(-1, 3), axis=0)) <= 256
    (f,) = enc(fr[None])
    assert f == gif_ref.encode(fr[None], 10)
    assert enc(fr[None]) == [f]


def test_257_clips_stand_where_the_sizes_before_them_say(hipb):
    """257 clips of one 1 x 1 frame: clip 257 is the first of the second 256-wide round of the file-offset scan"""
    k = np.arange(257)
    clips = np.stack([k & 255, (k * 7) & 255, k >> 8], -1).astype(np.uint8).reshape(257, 1, 1, 1, 3)
    files = enc(clips)
    assert len(files) == 257 and enc(clips) == files
    for c, f in zip(clips, files):
        assert f == gif_ref.encode(c, 10)


def test_refusals_name_the_argument(hipb):
    with pytest.raises(ValueError, match="16385"):
        enc(np.zeros((1, 1, 1, 16385, 3), np.uint8))
    with pytest.raises(ValueError, match="1 channels"):
        enc(np.zeros((1, 2, 4, 4, 1), np.uint8))
    with pytest.raises(ValueError, match="delay=70000"):
        enc(np.zeros((1, 2, 4, 4, 3), np.uint8), 70000)


def test_save_gifs_writes_the_three_clips(hipb, tmp_path):
    from PIL import Image
    from video_filler_amd import inference
    outs = [torch.from_numpy(np.stack([gif_cases.photo(64, 96, seed=30 + 4 * g + i) for i in range(4)]).astype(np.float32)
                             .transpose(0, 3, 1, 2) / np.float32(255)).cuda() for g in range(3)]
    name = str(tmp_path / "clips" / "v0")
    paths = inference.save_gifs(name, *outs)
    assert paths == [name + s for s in ("_result.gif", "_inpaint.gif", "_orig.gif")]
    assert sorted(os.listdir(tmp_path / "clips")) == ["v0_inpaint.gif", "v0_orig.gif", "v0_result.gif"]
    for p, t in zip(paths, outs):
        with open(p, "rb") as fh:
            data = fh.read()
        im = Image.open(io.BytesIO(data))
        assert im.n_frames == 3 and im.info["duration"] == 100 and im.info["loop"] == 0
        assert [data] == enc(t[:3]) and data == gif_ref.encode(png_ref.chw_to_hwc_bytes(t[:3].cpu().numpy()), 10)
    # test_vid.lua:140-147: one clip, delay 5
    (p,) = inference.save_gifs(str(tmp_path / "vid" / "result"), pred=outs[0], delay=5)
    assert os.path.basename(p) == "result_pred.gif"
    with open(p, "rb") as fh:
        assert [fh.read()] == enc(outs[0][:3], 5)
