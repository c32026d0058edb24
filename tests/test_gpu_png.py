"""The device PNG encoder (vf_png.hip) against the host reference of tests/png_ref.py: every file is a
valid PNG by a strict reader, decodes to exactly the bytes the rule gives, carries the filter the restated libpng
heuristic picks on every row, is the same file alone and in any batch, and is within the size caps."""
import os

import numpy as np
import pytest
import torch

import png_ref

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_cases.npz")
# Size margin over S_H (png_ref.huffman_only_size: zlib's dynamic codes, the same chunks, no matcher).  It covers only the
# difference between zlib's length-limited code construction and the encoder's (exact Huffman lengths, cut to 15 bits and
# repaired when they must be) plus what a match priced by estimate can lose against the literals it replaced.  Excess
# measured on an MI355X (this test prints it): photo +0.05 % (289 654 bytes against 289 512), decode -38.27 %,
# padded -43.66 %; the largest, rounded up.
MARGIN = 0.001


def gold():
    z = np.load(GOLD)
    return z, {k[6:]: z[k] for k in z.files if k.startswith("frame/")}


def enc(frames):
    from video_filler_amd.data import encode_png
    return encode_png(frames)


def check_file(f, want):
    img, types, idats = png_ref.read_png(f, want_filters=True)
    assert img.shape == want.shape and np.array_equal(img, want)
    assert np.array_equal(types, png_ref.choose_filters(want)[0])
    return types, idats


def test_fixtures_alone_and_batched(hipb):
    z, fx = gold()
    from video_filler_amd.backend import PNG_CHUNK
    assert int(z["chunk"]) == PNG_CHUNK == png_ref.CHUNK
    alone, seen = {}, set()
    for name, a in fx.items():
        (f,) = enc(a[None])
        types, idats = check_file(f, a)
        seen |= set(types.tolist())
        stream = a.shape[0] * (a.shape[1] * a.shape[2] + 1)
        assert len(idats) == -(-stream // PNG_CHUNK)
        alone[name] = f
    assert seen == {0, 1, 2, 3, 4}, "every filter type must occur in some fixture's output"
    by_shape = {}
    for name, a in fx.items():
        by_shape.setdefault(a.shape, []).append(name)
    assert any(len(v) > 1 for v in by_shape.values())
    for names in by_shape.values():
        files = enc(np.stack([fx[n] for n in names]))
        for n, f in zip(names, files):
            assert f == alone[n], "%s: the file differs between alone and batched" % n
    # ---- the size caps
    for name in ("noise", "noise_grey"):
        a = fx[name]
        stream = a.shape[0] * (a.shape[1] * a.shape[2] + 1)
        cap = stream + 17 * -(-stream // PNG_CHUNK) + 8 + 25 + 6 + 12
        print("%s: %d bytes, cap %d" % (name, len(alone[name]), cap))
        assert len(alone[name]) <= cap
    for name in ("flat", "flat_grey"):
        a = fx[name]
        raw = a.shape[0] * (a.shape[1] * a.shape[2] + 1)
        print("%s: %d bytes, raw %d, raw / 50 = %d" % (name, len(alone[name]), raw, raw // 50))
        assert len(alone[name]) <= raw / 50
    for name in ("photo", "decode", "padded"):
        sh, s6 = int(z["sh/" + name]), int(z["s6/" + name])
        print("%s: %d bytes, S_H %d (excess %+.2f %%), S_6 %d (ratio %.3f)" % (name, len(alone[name]), sh,
              100.0 * (len(alone[name]) / sh - 1), s6, len(alone[name]) / s6))
        assert len(alone[name]) <= sh * (1 + MARGIN)


def test_float_input_follows_the_truncating_rule(hipb):
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    near = np.concatenate([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2)),
                           np.array([-0.0, -1e-9, -3.5, 1.0000001, 7.0, np.inf, -np.inf, np.nan, 0.999999, 1e-45, 0.5], np.float32)])
    rng = np.random.default_rng(5)
    x = rng.uniform(-0.25, 1.25, (2, 3, 37, 53)).astype(np.float32)
    x.reshape(-1)[:near.size] = near
    x[1].reshape(-1)[-near.size:] = near[::-1]
    for arr in (x, x[:, :1].copy()):
        files = enc(torch.from_numpy(arr))
        want = png_ref.chw_to_hwc_bytes(arr)
        for i, f in enumerate(files):
            check_file(f, want[i])
    # the same frames given as bytes make the same files
    assert enc(png_ref.chw_to_hwc_bytes(x)) == enc(torch.from_numpy(x))
    # float64 and device tensors go the same way
    assert enc(torch.from_numpy(x).double().float().cuda()) == enc(x)


def synth(H, W, C):
    """integer arithmetic only: texture, flat bands and bands that are regular only after filtering"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    planes = []
    for c in range(C):
        v = (xx * xx * 3 + yy * 7 + (xx * yy) // 5 + 31 * c) & 255
        v = np.where((yy // 16) % 3 == 1, 200 - 40 * c, v)                              # flat bands
        v = np.where((yy // 16) % 3 == 2, ((xx * 2654435761 + yy * 40503 + c * 977) >> 7) & 255, v)
        planes.append(v)
    return np.stack(planes, -1).astype(np.uint8)


# (256, 8191, 1) and (257, 8191, 1): rows of 8192 filtered bytes, so exactly 256 chunks, one whole 256-wide round of the frame's
# chunk-offset scan, and 257, one chunk into the second round
@pytest.mark.parametrize("shape", [(1, 1, 3), (1, 1, 1), (1, 300, 3), (300, 1, 3), (1, 9000, 1), (129, 131, 3), (128, 128, 1),
                                   (384, 512, 3), (1024, 1024, 3), (256, 8191, 1), (257, 8191, 1)])
def test_geometries(hipb, shape):
    from video_filler_amd.backend import PNG_CHUNK
    a = synth(*shape)
    files = enc(np.stack([a, a[::-1, ::-1].copy()]))
    _, idats = check_file(files[0], a)
    check_file(files[1], a[::-1, ::-1])
    stream = shape[0] * (shape[1] * shape[2] + 1)
    assert len(idats) == -(-stream // PNG_CHUNK)
    if shape[0] == 1024:
        assert len(idats) >= 300, "a stream several hundred chunks long"
    assert enc(a[None]) == files[:1]


def test_257_files_of_one_batch_stand_where_the_sizes_before_them_say(hipb):
    """257 frames of 1 x 1 x 1: file 257 is the first of the second 256-wide round of the file-offset scan"""
    a = ((np.arange(257) * 37) & 255).astype(np.uint8).reshape(257, 1, 1, 1)
    buf, offsets = hipb.png_encode(torch.from_numpy(a).cuda())
    offs = offsets.cpu().tolist()
    files = enc(a)
    assert len(files) == 257 and enc(a) == files
    assert offs == np.concatenate([[0], np.cumsum([len(f) for f in files])]).tolist()
    assert buf[:offs[-1]].cpu().numpy().tobytes() == b"".join(files)
    for i, f in enumerate(files):
        check_file(f, a[i])
    assert [files[255], files[256]] == enc(a[255:256]) + enc(a[256:])


def test_determinism_over_repeats_and_batch_compositions(hipb):
    _, fx = gold()
    a, b, c = fx["photo"], fx["padded"], synth(384, 512, 3)
    first = enc(np.stack([a, b, c]))
    for _ in range(2):
        assert enc(np.stack([a, b, c])) == first
    assert enc(np.stack([c, a])) == [first[2], first[0]]
    assert enc(np.stack([b, b, a, c, b])) == [first[1], first[1], first[0], first[2], first[1]]


def test_refusals_name_the_geometry(hipb):
    with pytest.raises(ValueError, match="2 channels"):
        enc(np.zeros((1, 4, 4, 2), np.uint8))
    with pytest.raises(ValueError, match="16385"):
        enc(np.zeros((1, 1, 16385, 1), np.uint8))


def test_save_frames_writes_what_the_script_writes(hipb, tmp_path):
    from video_filler_amd import inference
    predLen, fs, nc = 2, 128, 3

    class Half:                                        # a stand-in generator: evaluate() and forward() are all the driver uses
        def evaluate(self):
            pass

        def forward(self, x):
            y = x.clone()
            hipb.scale_shift(y, 0.5, 0.1)
            return y
    rng = np.random.default_rng(11)
    full = torch.from_numpy(rng.uniform(-1.2, 1.2, (predLen * nc, fs, 2 * fs)).astype(np.float32))
    padmask = torch.from_numpy((rng.uniform(0, 1, (nc, fs, 2 * fs)) > 0.7).astype(np.uint8))
    outs = inference.WholeImageInpainter(Half(), predLen, inputLen=1, fineSize=fs, nc=nc)(full, padmask)
    d = str(tmp_path / "frames" / "clip0")
    paths = inference.save_frames(d, *outs)
    names = ["%s_%d.png" % (p, i) for p in ("pred", "inpaint", "orig") for i in range(1, predLen + 1)]
    assert [os.path.basename(p) for p in paths] == names and sorted(os.listdir(d)) == sorted(names)
    for gi, t in enumerate(outs):
        want = png_ref.chw_to_hwc_bytes(t.cpu().numpy())
        for i in range(predLen):
            with open(paths[gi * predLen + i], "rb") as fh:
                check_file(fh.read(), want[i])
    # test_vid.lua:138: one prefix
    paths = inference.save_frames(str(tmp_path / "vid"), pred=outs[0])
    assert [os.path.basename(p) for p in paths] == ["pred_1.png", "pred_2.png"]
    with open(paths[1], "rb") as fh:
        check_file(fh.read(), png_ref.chw_to_hwc_bytes(outs[0].cpu().numpy())[1])
