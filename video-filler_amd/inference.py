"""Inference drivers: test_vid.lua (one forward of the clip) and test_vid_wholeim.lua (whole frames, tile loop).

The generator runs in evaluate() mode (BatchNorm uses its running statistics), so tiles are independent and the
whole-image loop — one net:forward per 128x128 tile in the reference (test_vid_wholeim.lua:159-205) — becomes ONE
forward over all tiles: `vf_tiles_gather` builds the NHWC batch (incl. the script's vertical-flip rule for the first
three tiles of the top row), `vf_tiles_scatter` writes the output tiles back into the planar frames.
"""
import math

import torch

from .backend import get_backend, nhwc_empty


def predict_clip(net, input_image):
    """test_vid.lua:47-48,100-106: net:evaluate(); pred = net:forward(input_image); returns (input, pred) mapped back
    to [0,1] (`add(1):mul(0.5)`, :112-114).  input_image: predLen x nc x fs x fs in [-1,1]."""
    B = get_backend()
    net.evaluate()
    x = B.from_host(input_image).float()
    if not (x.dim() == 4 and x.permute(0, 2, 3, 1).is_contiguous()):
        x = x.contiguous(memory_format=torch.channels_last)
    pred = net.forward(x)
    out_in, out_pred = x.clone(), pred.clone()
    B.scale_shift(out_in, 0.5, 0.5)
    B.scale_shift(out_pred, 0.5, 0.5)
    return out_in, out_pred


def whole_frame_sizes(loadSize, fineSize=128):
    """test_vid_wholeim.lua:109-111: (inh, inw, outh, outw) for frames of the script's 360 x 480 geometry.  inw =
    loadSize * 480 / 360 is truncated by the tensor constructor; outw is computed from the UNtruncated value."""
    inw = loadSize * 480 / 360
    return int(loadSize), int(inw), math.ceil(loadSize / fineSize) * fineSize, math.ceil(inw / fineSize) * fineSize


def load_whole_frames(frames, mask, loadSize=360, fineSize=128, maskValue=110.0 / 255.0):
    """test_vid_wholeim.lua:109-141, 208-212 (loadImages and padmask) on the device: the (fullImages, padmask) that
    WholeImageInpainter takes.

    frames: predLen decoded frames, uint8 predLen x H x W x nc (or float predLen x nc x H x W in [0,1]); host or device.
    mask: the Byte mask (`data.byte_mask` of the decoded mask image), 1 or nc x Hm x Wm (or Hm x Wm); expanded to nc
    channels as the script does.  Every frame is scaled to inh x inw, maskedFill'ed with maskValue where the scaled
    Byte mask is > 0.3 (`scMask`), zero-padded bottom-right to outh x outw and mapped by mul(2):add(-1) (padding
    becomes -1): one launch for the whole clip.  The script's second image.scale to the same size is a copy and is
    not repeated.  padmask is the scaled Byte mask, zero-padded the same way.  mid_mask stays the caller's (the
    script's construction indexes the height axis with inw, :154-158).
    Returns (fullImages (predLen*nc) x outh x outw float, padmask nc x outh x outw uint8), on the device."""
    from .data import _frames
    B = get_backend()
    t = torch.as_tensor(frames)
    hwc = t.dtype == torch.uint8
    src, N, nc, H, W = _frames(t, hwc)
    inh, inw, outh, outw = whole_frame_sizes(loadSize, fineSize)
    m = torch.as_tensor(mask)
    assert m.dtype == torch.uint8, "the mask is a ByteTensor (data.byte_mask)"
    m = m.reshape(-1, m.shape[-2], m.shape[-1])
    m = B.from_host(m.expand(nc, m.shape[1], m.shape[2])).contiguous()       # torch.expand(mask, 3, h, w):byte()
    smask = B.empty(1, nc, inh, inw, dtype=torch.uint8)
    B.image_scale_u8(m.unsqueeze(0), smask)
    full = B.empty(N, nc, outh, outw)
    B.image_whole_frames(src, hwc, full, inh, inw, smask[0], float(maskValue))
    padmask = B.zeros(nc, outh, outw, dtype=torch.uint8)
    padmask[:, :inh, :inw] = smask[0]
    return full.view(N * nc, outh, outw), padmask


class WholeImageInpainter:
    """test_vid_wholeim.lua:150-226 with every tile in one batch."""

    def __init__(self, net, predLen, inputLen=1, fineSize=128, nc=3, netI=None):
        assert predLen % inputLen == 0, "I don't do padding in time dim (test_vid_wholeim.lua:40)"
        self.net, self.netI = net, netI
        self.predLen, self.inputLen, self.fs, self.nc = predLen, inputLen, fineSize, nc
        net.evaluate()
        if netI is not None:
            netI.evaluate()

    def __call__(self, fullImages, padmask, mid_mask=None):
        """fullImages: (predLen*nc) x outh x outw planar in [-1,1], padded bottom-right to multiples of fineSize
        (:137-141); padmask: nc x outh x outw Byte (:209-212).  Returns (outImages, inpaintImages, fullImages) in
        [0,1] (:222-224), predLen x nc x outh x outw."""
        B = get_backend()
        fs, nc, predLen = self.fs, self.nc, self.predLen
        full = B.from_host(fullImages).float().contiguous()
        C, H, W = full.shape
        assert C == nc * predLen and H % fs == 0 and W % fs == 0
        G = predLen // self.inputLen                  # opt.batchSize = predLen / inputLen (:41)
        ncin = nc * self.inputLen
        TY, TX = H // fs, W // fs
        # :167 — tiles (h == 1, w in {1, fs+1, 2fs+1}) are flipped vertically on the way in and out
        flips = torch.zeros(TY * TX, dtype=torch.uint8)
        flips[:min(3, TX)] = 1
        flips = B.from_host(flips)
        tiles = nhwc_empty(TY * TX * G, ncin, fs, fs, full.device)
        B.tiles_gather(full, tiles, G, flips)
        if self.netI is None:
            out_tiles = self.net.forward(tiles)
        else:                                         # :181-190: initializer net, fillIn, then the generator
            assert self.inputLen == 1, "inpaint_utils.fillIn: the mask must have as many channels as a batch row"
            mid = self.netI.forward(tiles)
            mm = B.from_host(mid_mask).float().contiguous()
            tmask = nhwc_empty(TY * TX, nc, fs, fs, full.device)
            # :183-189 — the mask tile is sliced UN-flipped (`mid_mask[{{}, {h, h+fs-1}, {w, w+fs-1}}]`) and applied to the
            # flipped patch: the script flips the image tile only, and so does this
            B.tiles_gather(mm, tmask, 1, None)
            tmask = tmask.repeat_interleave(G, dim=0).contiguous(memory_format=torch.channels_last)
            filled = torch.empty_like(tiles)
            B.masked_compose(filled, tiles, mid, tmask)
            out_tiles = self.net.forward(filled)
        ncout = out_tiles.shape[1]
        assert G * ncout == predLen * nc, "out_image:view(predLen, nc, fs, fs) (:200) needs %d output channels" % (predLen * nc // G)
        out = B.empty(G * ncout, H, W)
        B.tiles_scatter(out_tiles, out, G, flips)
        outImages = out.view(predLen, nc, H, W)
        pm = B.from_host(padmask).float().contiguous()
        pm = pm.unsqueeze(0).expand(predLen, nc, H, W).contiguous()
        inpaint = torch.empty_like(outImages)
        B.masked_compose(inpaint, full.view(predLen, nc, H, W), outImages, pm)      # :214-220
        fullv = full.clone()
        for t in (outImages, inpaint, fullv):         # :222-224
            B.scale_shift(t, 0.5, 0.5)
        return outImages, inpaint, fullv.view(predLen, nc, H, W)


def save_frames(dirname, outImages=None, inpaintImages=None, fullImages=None, **named):
    """test_vid_wholeim.lua:226-242 (and test_more_complex.lua:200-214): `image.save` of every frame of the three results
    of WholeImageInpainter as dirname/pred_%d.png, inpaint_%d.png and orig_%d.png, numbered from 1.  The directory is
    created; all 3 * predLen frames are encoded on the device in ONE call (data.encode_png) and the host only writes
    the files.  Tensors are predLen x nc x H x W in [0,1] (image.savePNG's truncating byte rule applies), or uint8
    predLen x H x W x nc.  Other prefixes go by keyword: save_frames(dirname, pred=out_pred) is test_vid.lua:138's
    pred_i.png.  Returns the paths, in the order pred, inpaint, orig (then the keywords'), frames innermost."""
    import os
    from .data import encode_png
    groups = [(p, t) for p, t in (("pred", outImages), ("inpaint", inpaintImages), ("orig", fullImages)) if t is not None]
    groups += list(named.items())
    assert groups, "save_frames: nothing to save"
    prefixes = [p for p, _ in groups]
    assert len(set(prefixes)) == len(prefixes), "save_frames: prefix given twice (%s); one would overwrite the other" % ", ".join(prefixes)
    B = get_backend()
    ts = [B.from_host(torch.as_tensor(t)) for _, t in groups]
    assert all(t.dim() == 4 for t in ts) and len({(t.dtype, tuple(t.shape[1:])) for t in ts}) == 1, \
        "save_frames: the tensors of one call share one type and one frame size"
    os.makedirs(dirname, exist_ok=True)
    files = encode_png(torch.cat(ts, 0))
    paths, k = [], 0
    for (prefix, _), t in zip(groups, ts):
        for i in range(t.shape[0]):
            path = os.path.join(dirname, "%s_%d.png" % (prefix, i + 1))
            with open(path, "wb") as fh:
                fh.write(files[k])
            k += 1
            paths.append(path)
    return paths
