"""What the codec stages share on the host and on the device: the batch decoders' staging buffers taken in
turn, one stager per decoder (backend._Stager), and the one frame reader (vf_block.h: vf_frame_byte), whose two kinds of
source must give the same bytes in every stage that reads through it."""
import os

import numpy as np
import pytest
import torch

import png_load_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _smallest(npz, prefix, keep):
    g = np.load(os.path.join(HERE, "golden", npz))
    names = sorted((k for k in g.files if k.startswith(prefix) and keep(g[k].tobytes())), key=lambda k: (g[k].size, k))[:3]
    return g, [k[len(prefix):] for k in names]


def test_stagers_take_turns_per_decoder(hipb):
    """Six single-file decodes, the two decoders alternating, nothing synchronised in between: the third call of a decoder
    packs into the pinned buffer its first call uploaded from, so it has to wait for that call and for no other, and the
    other decoder's calls in between must not move its turn."""
    from video_filler_amd.backend import jpeg_inspect, png_inspect
    jg, jnames = _smallest("jpeg_cases.npz", "jpg/", lambda f: jpeg_inspect(f, walk=False)["supported"])
    pg, pnames = _smallest("png_decode_cases.npz", "good/", lambda f: png_inspect(f)["supported"])
    assert len(jnames) == 3 and len(pnames) == 3
    got = []
    for jn, pn in zip(jnames, pnames):
        got.append(hipb.jpeg_decode([jg["jpg/" + jn].tobytes()], 3)[:3])
        got.append(hipb.png_decode([pg["good/" + pn].tobytes()], 3))
    torch.cuda.synchronize()
    want = []
    for jn, pn in zip(jnames, pnames):
        r = jg["ref/" + jn]
        want.append(np.repeat(r, 3, -1) if r.shape[2] == 1 else r)
        want.append(png_load_ref.load(pg["good/" + pn].tobytes(), 3))
    for i, ((buf, offs, status), w) in enumerate(zip(got, want)):
        assert status.cpu().tolist() == [0], i
        assert offs.tolist() == [0, w.size], i
        np.testing.assert_array_equal(buf[:w.size].cpu().numpy(), w.reshape(-1), err_msg="call %d" % i)


def _batch(shape, shift):
    """float32 N x C x H x W: -0.5, 1.5 and NaN, then values k/255 - 1e-3 and k/255 + 1e-3 (the byte rule gives k - 1 and k)"""
    ramp = (np.arange(256, dtype=np.float64)[:, None] / 255 + np.array([-1e-3, 1e-3])).reshape(-1)
    count = int(np.prod(shape))
    v = np.concatenate([[-0.5, 1.5, np.nan], ramp[(np.arange(count - 3) * 37 + shift) % ramp.size]])
    return np.roll(v, shift).astype(np.float32).reshape(shape)


def _twin(x):
    """the uint8 N x H x W x C batch of x by the rule stated on the host: clamp to [0, 1] (NaN -> 0), float32(255) * v, truncate"""
    v = np.fmin(np.fmax(x, np.float32(0)), np.float32(1))
    return np.ascontiguousarray((np.float32(255) * v).astype(np.uint8).transpose(0, 2, 3, 1))


@pytest.mark.parametrize("shape", [(2, 3, 1, 1), (2, 3, 3, 5), (2, 1, 3, 5)])
def test_float_and_byte_frames_agree(hipb, shape):
    """Two frames and five columns: a wrong frame or row stride in the shared reader shows; three channels at five columns:
    PNG's byte-in-row split shows."""
    from video_filler_amd import data
    x, y = _batch(shape, 0), _batch(shape, 101)
    xb, yb = _twin(x), _twin(y)
    assert xb.min() == 0 and xb.max() == 255 and np.isnan(x).sum() == 1
    assert data.encode_png(x) == data.encode_png(xb)
    for sub in ("420", "444"):
        assert data.encode_jpeg(x, subsampling=sub) == data.encode_jpeg(xb, subsampling=sub), sub
    if shape[1] == 3:
        assert data.encode_gif(x) == data.encode_gif(xb)
    tf, cols = data.frame_metrics(x, y)
    tb, _ = data.frame_metrics(xb, yb)
    assert torch.equal(tf, tb)
    assert tf[:, 0, cols.index("sae")].min() > 0                     # the two batches differ in every frame: no table of zeros
