"""The device JPEG encoder (vf_jpeg_enc.hip) against libjpeg: every file equals, byte for byte, the file
Pillow wrote (tests/golden/jpeg_encode_cases.npz) or the numpy restatement of the rule (tests/jpeg_enc_ref.py, itself held
to Pillow by tests/test_jpeg_enc_ref.py); alone and in a batch, from bytes and from floats, on every run; and the Python
entry points on top of it write what they say."""
import os

import numpy as np
import pytest
import torch

import jpeg_enc_ref

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_encode_cases.npz")
_gold = {}


def gold():
    """name -> (frame, quality, sampling, file bytes), and the archive; read once"""
    if not _gold:
        z = np.load(GOLD)
        _gold["z"] = z
        _gold["cases"] = {n: (z["frame/" + n], int(z["quality/" + n]), str(z["sampling/" + n]), z["file/" + n].tobytes())
                          for n in z["names"].tolist()}
    return _gold["cases"], _gold["z"]


def enc(frames, quality=75, subsampling="420"):
    from video_filler_amd.data import encode_jpeg
    return encode_jpeg(frames, quality, subsampling)


def first_difference(got, want):
    n = min(len(got), len(want))
    d = np.flatnonzero(np.frombuffer(got[:n], np.uint8) != np.frombuffer(want[:n], np.uint8))
    return "%d bytes against %d, first difference at %s" % (len(got), len(want), int(d[0]) if d.size else "the end of the shorter")


def test_every_golden_case_is_libjpegs_file(hipb):
    cases, _ = gold()
    bad = []
    for name, (frame, q, s, want) in cases.items():
        (got,) = enc(frame[None], q, s)
        if got != want:
            bad.append("%s: %s" % (name, first_difference(got, want)))
    assert not bad, "\n".join(bad)


def test_a_batch_holds_the_files_of_its_frames(hipb):
    cases, _ = gold()
    base = cases["37x53_444"][0]
    frames = np.stack([base, base[::-1].copy(), base[:, ::-1].copy(), 255 - base, np.roll(base, 7, 1)])
    for q, s in ((75, "420"), (90, "422"), (100, "444")):
        want = [jpeg_enc_ref.encode(f, q, s) for f in frames]
        files = enc(frames, q, s)
        assert files == want, [first_difference(a, b) for a, b in zip(files, want) if a != b]
        assert [enc(f[None], q, s)[0] for f in frames] == want                     # n = 1
        assert enc(torch.from_numpy(frames).cuda(), q, s) == want                  # a device tensor
    buf, offsets = hipb.jpeg_encode(torch.from_numpy(frames).cuda(), 75, "420")
    offs = offsets.cpu().tolist()
    assert offs[0] == 0 and all(b > a for a, b in zip(offs, offs[1:])) and offs[-1] <= buf.numel()
    assert buf[:offs[-1]].cpu().numpy().tobytes() == b"".join(enc(frames))
    grey = np.ascontiguousarray(frames[..., 1:2])
    assert enc(grey, 60, "444") == [jpeg_enc_ref.encode(f, 60) for f in grey]      # grey frames ignore the sampling


def test_257_files_of_one_batch_stand_where_the_sizes_before_them_say(hipb):
    """file 257 is the first of the second 256-wide round of the file-offset scan"""
    a = ((np.arange(257 * 3) * 37) & 255).astype(np.uint8).reshape(257, 1, 1, 3)
    assert enc(a, 85) == [jpeg_enc_ref.encode(f, 85) for f in a]


def test_float_input_follows_the_truncating_byte_rule(hipb):
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    near = np.concatenate([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2)),
                           np.array([-0.0, -1e-9, -3.5, 1.0000001, 7.0, np.inf, -np.inf, np.nan, 0.999999, 1e-45, 0.5], np.float32)])
    rng = np.random.default_rng(5)
    x = rng.uniform(-0.25, 1.25, (2, 3, 37, 53)).astype(np.float32)
    x.reshape(-1)[:near.size] = near
    x[1].reshape(-1)[-near.size:] = near[::-1]
    with np.errstate(invalid="ignore"):
        v = np.minimum(np.maximum(np.where(np.isnan(x), np.float32(0), x), np.float32(0)), np.float32(1))
        want = (np.float32(255) * v).astype(np.uint8).transpose(0, 2, 3, 1).copy()      # vf_savepng_byte on the host
    assert want.min() == 0 and want.max() == 255
    for arr, b in ((x, want), (x[:, :1].copy(), want[..., :1].copy())):
        files = enc(torch.from_numpy(arr), 90, "422")
        assert files == enc(b, 90, "422") == [jpeg_enc_ref.encode(f, 90, "422") for f in b]
    assert enc(torch.from_numpy(x).cuda()) == enc(want)


def test_round_trip_through_the_device_decoder(hipb):
    from video_filler_amd import data
    cases, z = gold()
    names = [n for n in cases if "decoded/" + n in z.files]
    assert len(names) == 6
    for name in names:
        frame, q, s, want = cases[name]
        files = enc(frame[None], q, s)
        assert files == [want]
        (got,) = data.decode_jpeg(files)
        assert np.array_equal(got.cpu().numpy(), z["decoded/" + name]), name
    try:
        from PIL import Image
    except ImportError:
        return
    import io
    for name in names:
        frame, _, s, _ = cases[name]
        (f,) = enc(frame[None], 92, s)
        (got,) = data.decode_jpeg([f])
        assert np.array_equal(got.cpu().numpy(), np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))), name


def test_determinism_over_repeats_and_batch_compositions(hipb):
    cases, _ = gold()
    noise, q, s, want = cases["100x75_noise_q100"]
    batch = np.stack([np.roll(noise, k, 0) for k in range(8)])
    first = enc(batch, q, s)
    assert first[0] == want
    assert enc(batch, q, s) == first
    assert enc(batch[::-1].copy(), q, s) == first[::-1]


def test_save_frames_jpg_and_display_jpeg(hipb, tmp_path):
    from video_filler_amd import inference
    rng = np.random.default_rng(3)
    groups = [torch.from_numpy(rng.uniform(-0.1, 1.1, (2, 3, 24, 40)).astype(np.float32)) for _ in range(3)]
    d = str(tmp_path / "frames" / "clip0")
    paths = inference.save_frames_jpg(d, *groups, quality=80, subsampling="422")
    names = ["%s_%d.jpg" % (p, i) for p in ("pred", "inpaint", "orig") for i in (1, 2)]
    assert [os.path.basename(p) for p in paths] == names and sorted(os.listdir(d)) == sorted(names)
    want = enc(torch.cat(groups, 0), 80, "422")
    for p, w in zip(paths, want):
        with open(p, "rb") as fh:
            assert fh.read() == w
    paths = inference.save_frames_jpg(str(tmp_path / "vid"), pred=groups[0])
    assert [os.path.basename(p) for p in paths] == ["pred_1.jpg", "pred_2.jpg"]
    with open(paths[1], "rb") as fh:
        assert fh.read() == enc(groups[0])[1]
    # save_frames still writes PNG files under the same rules
    paths = inference.save_frames(str(tmp_path / "png"), pred=groups[0])
    assert [os.path.basename(p) for p in paths] == ["pred_1.png", "pred_2.png"]
    with open(paths[0], "rb") as fh:
        assert fh.read(8) == b"\x89PNG\r\n\x1a\n"

    pack = torch.from_numpy(rng.uniform(-1, 1, (6, 3, 16, 16)).astype(np.float32))
    jpg = inference.display_jpeg(pack, quality=85, nrow=3, padding=2)
    sheet = inference.display_tensor(pack, nrow=3, padding=2)
    assert jpg == enc(sheet.unsqueeze(0), 85)[0]
    sof = jpg.index(b"\xff\xc0")
    assert (int.from_bytes(jpg[sof + 5:sof + 7], "big"), int.from_bytes(jpg[sof + 7:sof + 9], "big")) == tuple(sheet.shape[1:])
    assert tuple(sheet.shape) == (3, 36, 54)


# 256 x 1024 grey: 4096 blocks, sixteen tiles of the per-block scan (256 blocks each).  672 x 1024 grey noise at quality 100: a
# stream of more than 256 chunks of 4096 bytes, the second round of the per-image 0xFF scan.  129 x 131 at 4:2:0: ragged in both
# directions with more than one tile.
@pytest.mark.parametrize("shape,q,s", [((256, 1024, 1), 50, "420"), ((672, 1024, 1), 100, "420"), ((129, 131, 3), 95, "420")])
def test_streams_longer_than_one_workgroup(hipb, shape, q, s):
    rng = np.random.default_rng(shape[0])
    a = rng.integers(0, 256, shape, dtype=np.uint8)
    want = jpeg_enc_ref.encode(a, q, s)
    if shape[0] == 672:
        assert len(want) > 257 * 4096
    (got,) = enc(a[None], q, s)
    assert got == want, first_difference(got, want)


def test_refusals_name_the_argument(hipb):
    with pytest.raises(ValueError, match="C = 2"):
        enc(np.zeros((1, 4, 4, 2), np.uint8))
    with pytest.raises(ValueError, match="W = 16385"):
        enc(np.zeros((1, 1, 16385, 1), np.uint8))
    from video_filler_amd._lib import VfError
    with pytest.raises(VfError, match="quality = 0"):
        hipb.jpeg_encode(torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda"), 0, "420")
