"""The device GIF decoder (vf_gif_decode.hip) against its definition, tests/gif_decode_ref.py, byte for byte,
on every fixture of tests/gif_decode_cases.py: alone and in one mixed batch, RGB and RGBA; the corrupt fixtures' status words
(bounded decoding of bad data: every access of the kernels is bounded by construction, whatever the stream holds); the round
trip through the device encoder; scoring two clips save_gifs wrote; and the fallback."""
import numpy as np
import pytest
import torch

import gif_cases
import gif_decode_cases as cases
import gif_decode_ref as R
import gif_ref
import metrics_ref

pytestmark = pytest.mark.gpu


def dec(files, **kw):
    from video_filler_amd.data import decode_gif
    return decode_gif(files, **kw)


def _same(got, want):
    return tuple(got.shape) == want.shape and got.dtype == torch.uint8 and got.is_cuda and np.array_equal(got.cpu().numpy(), want)


def test_every_fixture_alone_rgb_and_rgba(hipb):
    for name in cases.of_kind("good"):
        data = cases.fixtures()[name].data
        want = cases.reference(name)[0]
        (rgba,) = dec([data], alpha=True)
        assert _same(rgba, want), name
        (rgb,) = dec([data])
        assert _same(rgb, want[..., :3]), name


def test_one_mixed_batch_equals_the_files_alone(hipb):
    names = cases.of_kind("good")
    assert len(names) == 37
    files = [cases.fixtures()[n].data for n in names]
    shapes = {cases.reference(n)[0].shape[:3] for n in names}
    assert len(shapes) > 12                                   # different screens and frame counts in one call
    for alpha in (False, True):
        got = dec(files, alpha=alpha)
        assert len(got) == len(names)
        for n, g in zip(names, got):
            want = cases.reference(n)[0]
            assert _same(g, want if alpha else want[..., :3]), n


def test_same_bytes_twice_and_split_over_two_batches(hipb):
    pick = ["hand/noise_deferred", "hand/frames_70", "hand/interlaced", "pil/delta_d3", "hand/constant_200x200", "hand/tokens_1984"]
    files = [cases.fixtures()[n].data for n in pick]
    first = [t.cpu().numpy() for t in dec(files)]
    again = [t.cpu().numpy() for t in dec(files)]
    split = [t.cpu().numpy() for t in dec(files[:2]) + dec(files[2:][::-1])[::-1]]
    for n, a, b, c in zip(pick, first, again, split):
        assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, cases.reference(n)[0][..., :3]), n


def test_corrupt_fixtures_raise_with_item_and_status(hipb):
    good = ["hand/rects_d013", "hand/noise_standard", "pil/p4"]
    names = cases.of_kind("corrupt")
    assert len(names) == 7
    for name in names:
        c = cases.fixtures()[name]
        word = R.STATUS_WORD[c.status]
        with pytest.raises(ValueError, match=r"decode_gif: item 0: corrupt image data \(%s\)" % word):
            dec([c.data])
        with pytest.raises(ValueError, match=r"decode_gif: item 2: corrupt image data \(%s\)" % word):
            dec([cases.fixtures()[good[0]].data, cases.fixtures()[good[1]].data, c.data, cases.fixtures()[good[2]].data])
    # the status words themselves, and the good files of a batch that holds every corrupt one
    order = [good[0]] + names[:4] + [good[1]] + names[4:] + [good[2]]
    out, offs, status = hipb.gif_decode([cases.fixtures()[n].data for n in order], True)
    st = status.cpu().tolist()
    for j, n in enumerate(order):
        assert st[j] == cases.fixtures()[n].status, n
        if n in good:
            want = cases.reference(n)[0]
            assert np.array_equal(out[offs[j]:offs[j + 1]].cpu().numpy().reshape(want.shape), want), n


def test_malformed_files_are_refused_before_any_launch(hipb):
    good = cases.fixtures()["hand/rects_d01"].data
    for name in cases.of_kind("malformed"):
        c = cases.fixtures()[name]
        with pytest.raises(ValueError, match=r"decode_gif: item 1: .*" + c.what):
            dec([good, c.data])


def test_round_trip_through_the_device_encoder(hipb):
    from video_filler_amd.data import encode_gif
    clips = np.stack([np.stack([gif_cases.photo(64, 80, seed=50 + 3 * g + k) for k in range(3)]) for g in range(2)])
    lossless = np.stack([gif_cases.n_colours(64, 80, 256, seed=60 + k) for k in range(3)])
    files = encode_gif(clips) + encode_gif(lossless[None])
    got = dec(files)
    for g, clip in enumerate(clips):
        want = np.stack([t[i] for t, i in (gif_ref.quantize(f) for f in clip)])
        assert _same(got[g], want), g
    assert _same(got[2], lossless)                            # at most 256 colours are stored losslessly
    rgba = dec(files[2:], alpha=True)[0].cpu().numpy()
    assert np.array_equal(rgba[..., :3], lossless) and (rgba[..., 3] == 255).all()


def test_scoring_two_clips_that_save_gifs_wrote(hipb, tmp_path):
    from video_filler_amd import inference
    outs = [torch.from_numpy(np.stack([gif_cases.photo(64, 80, seed=70 + 5 * g + k) for k in range(4)]).astype(np.float32)
                             .transpose(0, 3, 1, 2) / np.float32(255)).cuda() for g in range(2)]
    name = str(tmp_path / "v0")
    result, orig = inference.save_gifs(name, outImages=outs[0], fullImages=outs[1])
    a, b = inference.load_gif_clip(result), inference.load_gif_clip(orig)
    assert a.shape == (3, 3, 64, 80) and a.dtype == torch.float32 and a.is_cuda and a.is_contiguous()
    ra, rb = (R.decode(open(p, "rb").read())[0] for p in (result, orig))
    assert np.array_equal(a.cpu().numpy(), (ra.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2))
    got = inference.evaluate_frames(a, b)
    want = metrics_ref.scores(metrics_ref.frame_table(ra, rb))
    for k in ("psnr", "ssim", "mae", "flicker"):
        assert np.array_equal(got[k], want[k]) and got["mean"][k] == want["mean"][k], k
    assert np.isfinite(got["psnr"]).all() and (got["ssim"] < 1).all()


def test_fallback_receives_exactly_the_unsupported_files(hipb):
    wide = cases.fixtures()["hand/wide_16385"].data
    good = [cases.fixtures()[n].data for n in ("hand/rects_d01", "pil/delta")]
    with pytest.raises(ValueError, match="decode_gif: item 1 is not supported by the device decoder: .*16384"):
        dec([good[0], wide, good[1]])
    seen = []

    def fallback(data):
        seen.append(data)
        return R.decode(data)[0]
    got = dec([good[0], wide, good[1], wide], fallback=fallback)
    assert seen == [wide, wide]
    assert _same(got[1], R.decode(wide)[0]) and got[1].shape == (1, 1, 16385, 3)
    assert _same(got[0], cases.reference("hand/rects_d01")[0][..., :3]) and _same(got[2], cases.reference("pil/delta")[0][..., :3])
    # bytes, a uint8 array and a tensor are the same item (load_gif_clip above took a path)
    arr = np.frombuffer(good[0], np.uint8)
    for item in (bytearray(good[0]), arr, torch.from_numpy(arr.copy())):
        assert _same(dec([item])[0], cases.reference("hand/rects_d01")[0][..., :3])
