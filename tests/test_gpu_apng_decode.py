"""The device APNG decoder (vf_apng_decode in vf_png_decode.hip) against its definition,
tests/apng_decode_ref.py: every good fixture with and without alpha, alone and in one mixed batch with plain PNGs, corrupt
frame streams, unsupported files through the fallback, the round trip through encode_apng, and the lossless clip scores."""
import numpy as np
import pytest
import torch

import apng_cases
import apng_decode_ref as ref
import png_ref

pytestmark = pytest.mark.gpu

FX = apng_cases.fixtures()
_WANT = {}


def want(name):
    """the reference's RGBA canvases of a good fixture: computed once"""
    if name not in _WANT:
        _WANT[name] = ref.decode(FX["good"][name], alpha=True)
    return _WANT[name]


def dec(items, alpha=False, fallback=None):
    from video_filler_amd.data import decode_apng
    return decode_apng(items, alpha, fallback)


@pytest.mark.parametrize("name", sorted(FX["good"]))
def test_each_fixture_alone(hipb, name):
    f = FX["good"][name]
    for alpha in (False, True):
        (got,) = dec([f], alpha)
        w = want(name) if alpha else want(name)[..., :3]
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == w.shape
        g = got.cpu().numpy()
        assert np.array_equal(g, w), "%s alpha=%s: first differing frame %d" % (
            name, alpha, next(k for k in range(len(w)) if not np.array_equal(g[k], w[k])))


def test_one_mixed_batch(hipb):
    names = sorted(FX["good"])
    names = names + names[::-3]                              # some files twice, at other places
    for alpha in (False, True):
        outs = dec([FX["good"][n] for n in names], alpha)
        assert len(outs) == len(names)
        base = outs[0].untyped_storage().data_ptr()
        for n, o in zip(names, outs):
            assert o.untyped_storage().data_ptr() == base, "views of one buffer"
            assert np.array_equal(o.cpu().numpy(), want(n) if alpha else want(n)[..., :3]), n


def test_inspection_equals_the_reference(hipb):
    from video_filler_amd import data
    for name, f in FX["good"].items():
        info, rows = ref.metadata(f)
        d = data.apng_info(f)
        assert {k: d[k] for k in info} == info, name
        assert [[r[k] for k in ref.FRAME_KEYS] for r in d["frame_info"]] == rows, name


@pytest.mark.parametrize("name", sorted(FX["corrupt"]))
def test_a_corrupt_frame_stream_raises_with_its_status(hipb, name):
    from video_filler_amd.backend import PNG_STATUS
    f, status = FX["corrupt"][name]
    good = FX["good"]["edges"]
    with pytest.raises(ValueError, match=r"item 1: corrupt image data \(%s\)" % PNG_STATUS[status]):
        dec([good, f, good])
    from video_filler_amd.backend import get_backend, apng_inspect
    B = get_backend()
    buf, offs, st = B.apng_decode([good, f, good], True)     # the neighbours of a corrupt file are whole
    assert st.cpu().tolist() == [0, status, 0]
    w = want("edges")
    for j in (0, 2):
        assert np.array_equal(buf[offs[j]:offs[j + 1]].view(*w.shape).cpu().numpy(), w)
    assert apng_inspect(f)["supported"]


@pytest.mark.parametrize("name", sorted(FX["malformed"]))
def test_malformed_files_raise_before_a_launch(hipb, name):
    f, word = FX["malformed"][name]
    with pytest.raises(ValueError, match="decode_apng: item 1: ") as e:
        dec([FX["good"]["edges"], f])
    assert word in str(e.value)


def test_unsupported_files_reach_the_fallback(hipb):
    seen = []

    def fallback(data):
        seen.append(data)
        d = ref.parse(data)
        return np.full((min(d["frames"], 2), 3, 5, 3), len(seen), np.uint8)
    names = [n for n in sorted(FX["unsupported"]) if n != "frames_65536"]
    items = [FX["good"]["rgba"]] + [FX["unsupported"][n][0] for n in names]
    outs = dec(items, False, fallback)
    assert seen == items[1:]
    assert np.array_equal(outs[0].cpu().numpy(), want("rgba")[..., :3])
    for k, o in enumerate(outs[1:]):
        assert o.is_cuda and tuple(o.shape[1:]) == (3, 5, 3) and int(o.max()) == k + 1
    for n in sorted(FX["unsupported"]):
        f, word = FX["unsupported"][n]
        with pytest.raises(ValueError, match="item 0 is not supported by the device decoder") as e:
            dec([f])
        assert word in str(e.value), n


def clips(G, N, H, W, C, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty((G, N, H, W, C), np.uint8)
    for g in range(G):
        for j in range(N):
            smooth = np.stack([(xx * (c + 2) + yy * (j + 1) + 31 * g) & 255 for c in range(C)], -1)
            out[g, j] = np.where(((yy // 8 + j) % 2 == 0)[..., None], smooth, rng.integers(0, 256, (H, W, C)))
    return out


@pytest.mark.parametrize("geom", [(3, 5, 33, 85, 3), (2, 2, 64, 127, 1), (1, 1, 1, 1, 3), (2, 3, 64, 128, 3)])
def test_round_trip_through_encode_apng(hipb, geom):
    from video_filler_amd import data
    G, N, H, W, C = geom
    u8 = clips(G, N, H, W, C, 3)
    x = u8.astype(np.float32).transpose(0, 1, 4, 2, 3) / np.float32(255) + np.float32(0.001)     # floats between two bytes
    truth = np.stack([png_ref.chw_to_hwc_bytes(c) for c in x])
    for files, t in ((data.encode_apng(u8, 4, 2), u8), (data.encode_apng(torch.from_numpy(x)), truth)):
        outs = dec(files, True)
        for g in range(G):
            got = outs[g].cpu().numpy()
            assert got.shape == (N, H, W, 4) and (got[..., 3] == 255).all()
            assert np.array_equal(got[..., :3], np.broadcast_to(t[g], (N, H, W, 3)) if C == 1 else t[g])
            assert np.array_equal(ref.decode(files[g], alpha=True), got)
        d = data.apng_info(files[0])
        assert d["frames"] == N and d["animated"] and d["default_is_frame"] and d["channels"] == C


def test_apng_scores_zero_error_where_gif_does_not(hipb, tmp_path):
    from video_filler_amd import inference
    N, H, W = 4, 64, 96
    rng = np.random.default_rng(8)
    u8 = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)          # far more than 256 colours a frame
    assert len(np.unique(u8[0].reshape(-1, 3), axis=0)) > 256
    clip = torch.from_numpy(u8.astype(np.float32).transpose(0, 3, 1, 2) / np.float32(255)).cuda()
    truth = torch.from_numpy(png_ref.chw_to_hwc_bytes(clip.cpu().numpy()).astype(np.float32).transpose(0, 3, 1, 2) / np.float32(255)).cuda()
    (p,) = inference.save_apngs(str(tmp_path / "a" / "clip"), orig=clip)
    back = inference.load_apng_clip(p)
    assert back.dtype == torch.float32 and tuple(back.shape) == (N, 3, H, W) and torch.equal(back, truth)
    s = inference.evaluate_frames(back, truth)
    assert (s["mae"] == 0).all() and np.isinf(s["psnr"]).all() and (s["flicker"] == 0).all(), s
    (q,) = inference.save_gifs(str(tmp_path / "g" / "clip"), orig=clip)
    lossy = inference.evaluate_frames(inference.load_gif_clip(q), truth[:-1])
    assert (lossy["mae"] > 0).all() and np.isfinite(lossy["psnr"]).all(), lossy
