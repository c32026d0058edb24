"""Inference drivers: test_vid.lua (one forward of the clip), test_vid_wholeim.lua (whole frames, tile loop), and
test.lua / demo.lua (centre inpainting of the train.lua nets) with the contact sheets the scripts save.

The generator runs in evaluate() mode (BatchNorm uses its running statistics), so tiles are independent and the
whole-image loop — one net:forward per 128x128 tile in the reference (test_vid_wholeim.lua:159-205) — becomes ONE
forward over all tiles: `vf_tiles_gather` builds the NHWC batch (incl. the script's vertical-flip rule for the first
three tiles of the top row), `vf_tiles_scatter` writes the output tiles back into the planar frames.
`WindowedInpainter` is that loop for clips of any size and length: windows that overlap in y, x and t, blended on the
device.
"""
import math

import torch

from . import data
from .backend import get_backend, is_nhwc, nhwc_empty, to_nhwc


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


# ------------------------------------------------------------------------- overlapped, blended windows
def window_origins(n, size, stride):
    """Where the windows of one axis start: 0, stride, 2 stride, ... while a window of `size` fits into n samples, and one
    more at n - size if the last of them ends before n.  Nothing is padded.  ValueError, naming the argument, for n < size,
    stride outside [1, size], or 2 stride < size (an overlap of more than half a window: more than three covers)."""
    n, size, stride = int(n), int(size), int(stride)
    if size < 1:
        raise ValueError("window_origins: size=%d must be >= 1" % size)
    if n < size:
        raise ValueError("window_origins: n=%d is smaller than the window size=%d; nothing is padded" % (n, size))
    if not 1 <= stride <= size:
        raise ValueError("window_origins: stride=%d must lie in [1, size=%d]" % (stride, size))
    if 2 * stride < size:
        raise ValueError("window_origins: stride=%d: 2 stride must be >= size=%d (an overlap of at most half a window)" % (stride, size))
    o = list(range(0, n - size + 1, stride))
    if o[-1] + size < n:
        o.append(n - size)
    return o


def window_weights(size, stride):
    """The integer taper of a window along one axis: w(i) = min(i + 1, size - i, r + 1), r = size - stride.  Two regular
    neighbours sum to r + 1 wherever they overlap; r = 0 gives 1 everywhere."""
    window_origins(size, size, stride)           # the same refusals
    r = int(size) - int(stride)
    return [min(i + 1, size - i, r + 1) for i in range(int(size))]


class WindowedInpainter:
    """Whole clips of any size and length through a fineSize generator: windows of inputLen frames x fineSize x fineSize
    that overlap in y, x (stride) and t (stride_t; default inputLen, no temporal overlap), every window one batch row, the
    outputs blended with integer tapered weights in a fixed order (tests/window_blend_ref.py is the
    rule).  No padding, no seams at tile borders, no vertical-flip rule.  Windows go through the net in chunks of at most
    max_tiles, so device memory beyond the clip and its results is one accumulator and one chunk in and out, and the result
    does not depend on max_tiles by a bit.  The initializer-net (netI) path of WholeImageInpainter is not offered here."""

    def __init__(self, net, inputLen=1, fineSize=128, nc=3, stride=96, stride_t=None, max_tiles=64):
        self.net, self.L, self.fs, self.nc = net, int(inputLen), int(fineSize), int(nc)
        self.stride = int(stride)
        self.stride_t = self.L if stride_t is None else int(stride_t)
        self.max_tiles = int(max_tiles)
        if self.max_tiles < 1:
            raise ValueError("WindowedInpainter: max_tiles=%d must be >= 1" % self.max_tiles)
        try:
            window_weights(self.fs, self.stride)
        except ValueError as e:
            raise ValueError("WindowedInpainter: stride=%d does not fit fineSize=%d (%s)" % (self.stride, self.fs, e)) from None
        try:
            window_weights(self.L, self.stride_t)
        except ValueError as e:
            raise ValueError("WindowedInpainter: stride_t=%d does not fit inputLen=%d (%s)" % (self.stride_t, self.L, e)) from None
        net.evaluate()

    def plan(self, F, H, W):
        """(ot, oy, ox): the origins of the windows of an F-frame H x W clip.  ValueError for a clip smaller than a window."""
        for name, n, size in (("F", F, self.L), ("H", H, self.fs), ("W", W, self.fs)):
            if n < size:
                raise ValueError("WindowedInpainter: frames: %s=%d is smaller than a window (%d); nothing is padded" % (name, n, size))
        return (window_origins(F, self.L, self.stride_t), window_origins(H, self.fs, self.stride),
                window_origins(W, self.fs, self.stride))

    def __call__(self, frames, mask):
        """frames: F x nc x H x W in [-1,1], already mask-filled (load_whole_frames(...) cropped to [:inh, :inw]), F >=
        inputLen and H, W >= fineSize; mask: nc x H x W Byte, non-zero = hole.  Returns (outImages, inpaintImages,
        fullImages) in [0,1], each F x nc x H x W: what WholeImageInpainter returns, for save_frames, save_apngs, save_gifs
        and evaluate_frames."""
        B = get_backend()
        x = B.from_host(torch.as_tensor(frames)).float().contiguous()
        if x.dim() != 4 or x.shape[1] != self.nc:
            raise ValueError("WindowedInpainter: frames are F x nc=%d x H x W, got %s" % (self.nc, tuple(x.shape)))
        F, nc, H, W = x.shape
        m = B.from_host(torch.as_tensor(mask)).contiguous()
        if m.dtype != torch.uint8 or tuple(m.shape) != (nc, H, W):
            raise ValueError("WindowedInpainter: mask is a Byte tensor nc x H x W = %s, got %s %s" % ((nc, H, W), m.dtype, tuple(m.shape)))
        ot, oy, ox = self.plan(F, H, W)
        NW = len(ot) * len(oy) * len(ox)
        geo = (self.L, self.fs, self.stride, self.stride_t)
        acc = B.zeros(F, nc, H, W)
        tiles = nhwc_empty(min(self.max_tiles, NW), self.L * nc, self.fs, self.fs, x.device)
        for w0 in range(0, NW, self.max_tiles):
            chunk = tiles[:min(self.max_tiles, NW - w0)]
            B.windows_gather(x, chunk, geo, w0)
            out_tiles = to_nhwc(self.net.forward(chunk))
            assert tuple(out_tiles.shape) == tuple(chunk.shape), \
                "the net returns %s for a batch %s: it must give inputLen * nc channels of fineSize x fineSize" % (tuple(out_tiles.shape), tuple(chunk.shape))
            B.windows_accumulate(out_tiles, acc, geo, w0)
        outImages, inpaint, fullv = torch.empty_like(acc), torch.empty_like(acc), torch.empty_like(acc)
        B.windows_finish(acc, geo, outImages, x, m, inpaint, fullv)
        return outImages, inpaint, fullv


def _write_files(paths, blobs):
    """One file per (path, bytes) pair -> the paths."""
    for path, blob in zip(paths, blobs):
        with open(path, "wb") as fh:
            fh.write(blob)
    return paths


def _save_frame_groups(who, ext, encode, dirname, outImages, inpaintImages, fullImages, named):
    """save_frames and save_frames_jpg: dirname/<prefix>_%d.<ext> for every frame of every group, numbered from 1, all of
    them through ONE call of `encode` (a batch -> a list of bytes).  -> the paths: pred, inpaint, orig, then the keywords',
    frames innermost."""
    import os
    groups = [(p, t) for p, t in (("pred", outImages), ("inpaint", inpaintImages), ("orig", fullImages)) if t is not None]
    groups += list(named.items())
    assert groups, "%s: nothing to save" % who
    prefixes = [p for p, _ in groups]
    assert len(set(prefixes)) == len(prefixes), "%s: prefix given twice (%s); one would overwrite the other" % (who, ", ".join(prefixes))
    B = get_backend()
    ts = [B.from_host(torch.as_tensor(t)) for _, t in groups]
    assert all(t.dim() == 4 for t in ts) and len({(t.dtype, tuple(t.shape[1:])) for t in ts}) == 1, \
        "%s: the tensors of one call share one type and one frame size" % who
    os.makedirs(dirname, exist_ok=True)
    paths = [os.path.join(dirname, "%s_%d.%s" % (prefix, i + 1, ext)) for (prefix, _), t in zip(groups, ts) for i in range(t.shape[0])]
    return _write_files(paths, encode(torch.cat(ts, 0)))


def save_frames(dirname, outImages=None, inpaintImages=None, fullImages=None, level=0, **named):
    """test_vid_wholeim.lua:226-242 (and test_more_complex.lua:200-214): `image.save` of every frame of the three results
    of WholeImageInpainter as dirname/pred_%d.png, inpaint_%d.png and orig_%d.png, numbered from 1.  The directory is
    created; all 3 * predLen frames are encoded on the device in ONE call (data.encode_png) and the host only writes
    the files.  Tensors are predLen x nc x H x W in [0,1] (image.savePNG's truncating byte rule applies), or uint8
    predLen x H x W x nc.  Other prefixes go by keyword: save_frames(dirname, pred=out_pred) is test_vid.lua:138's
    pred_i.png.  level is encode_png's (1: the dense encoder, smaller files).  Returns the paths, in the order pred, inpaint,
    orig (then the keywords'), frames innermost."""
    from .backend import png_level
    from .data import encode_png
    level = png_level("save_frames", level)      # refused before the directory is made
    return _save_frame_groups("save_frames", "png", lambda t: encode_png(t, level), dirname, outImages, inpaintImages, fullImages, named)


def save_frames_jpg(dirname, outImages=None, inpaintImages=None, fullImages=None, quality=75, subsampling="420", restart_rows=0,
                    restart_blocks=0, optimize=False, progressive=False, **named):
    """save_frames with `image.save` given a .jpg name: dirname/pred_%d.jpg, inpaint_%d.jpg and orig_%d.jpg, the frames a
    JPEG folder of the loaders holds.  Same tensors, same rules, same order of the returned paths; all frames are encoded
    on the device in ONE call (data.encode_jpeg at `quality` and `subsampling`: libjpeg's default compression, byte for
    byte; restart_rows, restart_blocks, optimize and progressive are encode_jpeg's) and the host only writes the files."""
    from .data import _jpeg_options, encode_jpeg
    _jpeg_options("save_frames_jpg", restart_rows, restart_blocks, optimize, progressive)      # refused before the directory is made
    return _save_frame_groups("save_frames_jpg", "jpg",
                              lambda t: encode_jpeg(t, quality, subsampling, restart_rows, restart_blocks, optimize, progressive),
                              dirname, outImages, inpaintImages, fullImages, named)


def save_gifs(name, outImages=None, inpaintImages=None, fullImages=None, delay=10, **named):
    """test_vid_wholeim.lua:244-257 (and test_more_complex.lua:216-229): the `convert -delay 10 pred_1.png ...
    pred_{predLen-1}.png name_result.gif` that ends the video drivers, and the same for inpaint_* -> name_inpaint.gif and
    orig_* -> name_orig.gif, without the PNGs and without ImageMagick: all clips are encoded on the device in ONE call
    (data.encode_gif) and the host only writes the files.  Tensors are predLen x 3 x H x W in [0,1] (image.savePNG's
    truncating byte rule applies) or uint8 predLen x H x W x 3.  Like the reference's shell loop
    (`for ((a=1; a<predLen; a++))`) a clip holds frames 1 .. predLen-1: the LAST frame is not in it.  With predLen < 2
    that command has no input; here that is a ValueError.  Other clips go by keyword as name_<key>.gif:
    test_vid.lua:140-147 (`convert -delay 5 pred_*.png result.gif`) is save_gifs(dir + "/result", pred=pred_image,
    delay=5), which writes dir/result_pred.gif.  The parent directory is created.  Returns the paths, in the order
    result, inpaint, orig, then the keywords'."""
    import os
    groups = [(p, t) for p, t in (("result", outImages), ("inpaint", inpaintImages), ("orig", fullImages)) if t is not None]
    groups += list(named.items())
    if not groups:
        raise ValueError("save_gifs: nothing to save")
    keys = [p for p, _ in groups]
    if len(set(keys)) != len(keys):
        raise ValueError("save_gifs: clip given twice (%s); one would overwrite the other" % ", ".join(keys))
    ts = [t if torch.is_tensor(t) else torch.as_tensor(t) for _, t in groups]
    if not all(t.dim() == 4 for t in ts) or len({(t.dtype, tuple(t.shape)) for t in ts}) != 1:
        raise ValueError("save_gifs: the clips of one call are 4-D and share one type, length and frame size")
    if ts[0].shape[0] < 2:
        raise ValueError("save_gifs: predLen = %d; the clip holds frames 1 .. predLen-1, which is none" % ts[0].shape[0])
    from .data import encode_gif
    B = get_backend()
    files = encode_gif(torch.stack([B.from_host(t)[:-1] for t in ts]), delay)
    os.makedirs(os.path.dirname(os.path.abspath(name)), exist_ok=True)
    return _write_files(["%s_%s.gif" % (name, key) for key in keys], files)


def save_apngs(name, outImages=None, inpaintImages=None, fullImages=None, delay=10, level=0, **named):
    """save_gifs without its loss: name_result.png, name_inpaint.png, name_orig.png and name_<key>.png as animated PNG
    files, all clips encoded on the device in ONE call (data.encode_apng); the host only writes the files.
    Tensors are predLen x C x H x W in [0,1] (image.savePNG's truncating byte rule applies) or uint8 predLen x H x W x C,
    C = 1 or 3.  Every frame keeps its exact bytes, and unlike save_gifs the clip holds ALL predLen frames: the frame
    save_gifs drops is a quirk of the reference's `convert` loop, and no reference command writes these files.  Each file
    is also a plain PNG of its first frame, and loops forever.  level is encode_apng's.  The parent directory is created.
    Returns the paths, in the order result, inpaint, orig, then the keywords'."""
    import os
    from .backend import png_level
    level = png_level("save_apngs", level)
    groups = [(p, t) for p, t in (("result", outImages), ("inpaint", inpaintImages), ("orig", fullImages)) if t is not None]
    groups += list(named.items())
    if not groups:
        raise ValueError("save_apngs: nothing to save")
    keys = [p for p, _ in groups]
    if len(set(keys)) != len(keys):
        raise ValueError("save_apngs: clip given twice (%s); one would overwrite the other" % ", ".join(keys))
    ts = [t if torch.is_tensor(t) else torch.as_tensor(t) for _, t in groups]
    if not all(t.dim() == 4 for t in ts) or len({(t.dtype, tuple(t.shape)) for t in ts}) != 1:
        raise ValueError("save_apngs: the clips of one call are 4-D and share one type, length and frame size")
    from .data import encode_apng
    B = get_backend()
    files = encode_apng(torch.stack([B.from_host(t) for t in ts]), delay, level=level)
    os.makedirs(os.path.dirname(os.path.abspath(name)), exist_ok=True)
    return _write_files(["%s_%s.png" % (name, key) for key in keys], files)


def load_apng_clip(item):
    """An APNG file (bytes, a path, a uint8 array or tensor) as the clip the drivers hold: float N x 3 x H x W in [0,1] on the
    device — every frame composited on the device (data.decode_apng), b / 255 as a correctly rounded
    float32 division, then the layout change.  What save_apngs wrote comes back without loss:
    evaluate_frames(load_apng_clip(name + "_result.png"), load_apng_clip(name + "_orig.png")) scores the frames' own bytes.
    ValueError for a malformed, unsupported or corrupt file."""
    (frames,) = data.decode_apng([item])
    return get_backend().png_bytes_to_float(frames).permute(0, 3, 1, 2).contiguous()


def load_gif_clip(item):
    """A GIF file (bytes, a path, a uint8 array or tensor) as the clip the drivers hold: float N x 3 x H x W in [0,1] on the
    device — every frame composited on the device (data.decode_gif), b / 255 as a correctly rounded
    float32 division, then the layout change.  The form save_frames and evaluate_frames take:
    evaluate_frames(load_gif_clip(name + "_result.gif"), load_gif_clip(name + "_orig.gif")) scores what save_gifs'
    256-colour tables cost.  ValueError for a malformed, unsupported or corrupt file."""
    (frames,) = data.decode_gif([item])
    return get_backend().png_bytes_to_float(frames).permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------------- scores
def scores_from_table(table):
    """data.frame_metrics' int64 table N x 2 x 6 (a host array) -> the dict evaluate_frames returns: float64 from the
    integers.  mse = sse / n is not returned; psnr = 10 log10(255^2 n / sse), inf for sse = 0; ssim = ssim_q /
    (ssim_n 2^30); mae = sae / n; flicker / n.  A region without samples, or without windows, gives nan."""
    import numpy as np
    t = np.asarray(table, np.int64)
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for reg, pre in ((0, ""), (1, "hole_")):
            n, sse, sae, sq, sn, fl = (t[:, reg, k].astype(np.float64) for k in range(len(data.METRIC_COLUMNS)))
            out[pre + "psnr"] = 10.0 * np.log10(65025.0 * n / sse)
            out[pre + "ssim"] = sq / (sn * float(1 << 30))
            out[pre + "mae"] = sae / n
            out[pre + "flicker"] = fl / n
        out["mean"] = {k: (float(np.mean(v[1:])) if len(v) > 1 else 0.0) if k.endswith("flicker") else float(np.mean(v))
                       for k, v in out.items()}
    return out


def evaluate_frames(result, truth, mask=None, valid=None):
    """How good an inpainted clip is, from the tensors the drivers already hold on the device: one call
    (data.frame_metrics), one small table read back.  result, truth: predLen frames each — what
    WholeImageInpainter.__call__ returns and save_frames accepts: float predLen x nc x H x W in [0,1] or uint8
    predLen x H x W x nc, nc = 1 or 3, host or device.  The scores are those of the BYTES save_frames would write
    (image.savePNG's truncating rule), so they equal what anybody measures from the PNG files, without the files.
    mask: the hole, uint8 H x W, non-zero = hole; the drivers' padmask (nc x H x W) is accepted and its first channel
    taken.  valid = (vh, vw): the rows and columns that are picture; the bottom-right padding beyond them has no
    influence.  `whole_frame_sizes` gives it — for test_vid_wholeim.lua:

        inh, inw, outh, outw = whole_frame_sizes(loadSize)
        outImages, inpaintImages, fullImages = WholeImageInpainter(net, predLen)(full, padmask)
        scores = evaluate_frames(inpaintImages, gt, padmask, valid=(inh, inw))

    with gt the frames of the data set's gt/ folder (:123-126) scaled and padded as `full` was, in [0,1].
    Returns a dict of float64 arrays of predLen entries: psnr, ssim (uniform 7 x 7 windows, scikit-image's default
    form, per channel), mae (in byte units), flicker (mean |(a_t - a_{t-1}) - (b_t - b_{t-1})|, 0 for the first frame),
    and hole_psnr, hole_ssim, hole_mae, hole_flicker over the hole alone (a window belongs to the hole when its centre
    does); and under "mean" the clip means of all eight (flicker over the frames t >= 1).  nan where a region has no
    samples or no whole window (no mask; a frame below 7 x 7); psnr inf for identical frames.  DESIGN.md 5.7 has the
    rule, tests/metrics_ref.py pins it."""
    m = None if mask is None else torch.as_tensor(mask)
    if m is not None and m.dim() == 3:
        m = m[0]
    table, _ = data.frame_metrics(result, truth, m, valid, clip=True)
    return scores_from_table(table.cpu().numpy())


# --------------------------------------------------------------------------- test.lua / demo.lua and the sheets
def _check_display_args(x, padding, nrow):
    """toDisplayTensor's argument checks, on the host and before any backend exists: -> the tensor."""
    if isinstance(x, (list, tuple, dict)):
        raise ValueError("display_tensor: a table of %d images; only a packed N x C x h x w tensor is laid out" % len(x))
    t = torch.as_tensor(x)
    if t.dim() != 4 or t.shape[1] not in (1, 3) or t.numel() == 0:
        raise ValueError("display_tensor: a tensor of shape %s; only a packed N x C x h x w tensor with C = 1 or 3 is laid out "
                         "(2-D images and K x h x w channel grids are not)" % (tuple(t.shape),))
    if int(padding) != padding or padding < 0 or padding % 2:
        raise ValueError("display_tensor: padding=%r must be an even integer >= 0 (images sit at padding/2)" % (padding,))
    if int(nrow) != nrow or nrow < 1:
        raise ValueError("display_tensor: nrow=%r must be an integer >= 1" % (nrow,))
    return t


def display_tensor(x, padding=0, nrow=6, scaleeach=False, min=None, max=None, symmetric=False, saturate=True):
    """image.toDisplayTensor(x, padding, nrow, scaleeach, min, max, symmetric, saturate) on the device, for the input form
    the scripts use: a packed float tensor N x C x h x w with C = 1 or 3, host or device; a channels-last tensor is read
    where it lies.  Returns the device grid C x (h+padding)*ymaps x (w+padding)*xmaps, xmaps = min(nrow, N), normalised
    by image.minmax (whole grid, or every image first with scaleeach); DESIGN.md 5.4 has the rule, tests/display_ref.py
    pins it and the kernels equal it bit for bit.  Inputs must be finite: what NaN or Inf do is unspecified.  Tables,
    2-D inputs, K x h x w channel grids, C outside {1, 3} and odd or negative padding raise ValueError."""
    t = _check_display_args(x, padding, nrow)
    B = get_backend()
    t = B.from_host(t).float()
    if not (t.is_contiguous() or is_nhwc(t)):
        t = t.contiguous()
    return B.display_tensor(t, int(padding), int(nrow), scaleeach, min, max, symmetric, saturate)


def predict_center(net, image_ctx, overlapPred=0, noise=None, fill=data.CENTER_FILL):
    """test.lua:39,79-104 (= demo.lua:31,59-79): net:evaluate(); cut the centre out of the loader's batch (image_ctx:
    B x 3 x fs x fs in [-1,1], host or device) and paint the hole with the mean colour (data.center_prepare); pred =
    net:forward(input), or net:forward({input, noise}) for a noiseGen net (noise: B x nz x 1 x 1); paste pred into the
    hole, map everything by add(1):mul(0.5) and build the script's pretty_output — one kernel (vf_center_finish).
    Returns (pretty_output 2B x 3 x fs x fs, image_ctx B x 3 x fs x fs, pred_center and real_center B x 3 x fs/2 x fs/2),
    all in [0,1] on the device; pretty_output's rows 2i / 2i+1 are the input with a white hole / the context with the
    prediction pasted in."""
    B = get_backend()
    net.evaluate()
    x = torch.as_tensor(image_ctx)
    assert x.dim() == 4 and x.shape[1] == 3, "test.lua paints channels 1-3 by name (:82-84, :122-124): nc = 3, got %s" % (tuple(x.shape),)
    ctx, real_center = data.center_prepare(x, overlapPred, fill)
    pred = net.forward(ctx if noise is None else [ctx, B.from_host(torch.as_tensor(noise)).float()])
    nB, nc, fs, _ = ctx.shape
    pretty, pasted, pred_center = B.empty(2 * nB, nc, fs, fs), B.empty(nB, nc, fs, fs), B.empty(nB, nc, fs // 2, fs // 2)
    B.center_finish(ctx, to_nhwc(pred), overlapPred, pretty, pasted, pred_center)
    # add(1):mul(0.5) and scale_shift's x * 0.5 + 0.5 give the same bits: halving is exact, so either form rounds once, the sum
    # x + 1 at its own binade — no second mapping kernel for the one tensor that only needs the map
    B.scale_shift(real_center, 0.5, 0.5)
    return pretty, pasted, pred_center, real_center


def load_demo_images(images, inputSize=128):
    """demo.lua:49-55: decoded frames (uint8 N x H x W x 3, or float N x 3 x H x W in [0,1]; host or device) ->
    image.scale to inputSize x inputSize -> mul(2):add(-1): the N x 3 x inputSize x inputSize batch predict_center takes."""
    B = get_backend()
    t = torch.as_tensor(images)
    hwc = t.dtype == torch.uint8
    src, N, nc, H, W = data._frames(t, hwc)
    out = B.empty(N, nc, int(inputSize), int(inputSize))
    B.image_scale(src, hwc, out)
    B.scale_shift(out, 2.0, -1.0)
    return out


def save_sheet(path, x, level=0, **display_args):
    """image.save(path, image.toDisplayTensor(x, ...)) (test.lua:129, demo.lua:96): display_tensor, data.encode_png of the
    one grid (image.savePNG's byte rule is applied inside the encoder; no byte copy of the sheet is made), then the file
    is written; level is encode_png's.  Returns path."""
    from .backend import png_level
    level = png_level("save_sheet", level)
    grid = display_tensor(x, **display_args)
    (png,) = data.encode_png(grid.unsqueeze(0), level)
    with open(path, "wb") as fh:
        fh.write(png)
    return path


def display_jpeg(x, quality=75, restart_rows=0, restart_blocks=0, optimize=False, progressive=False, **display_args):
    """The payload of the training scripts' disp.image(x, ...) (train_vid_weighted.lua:553-588, train.lua likewise): the
    contact sheet display_tensor builds of x, compressed as one JPEG on the device (data.encode_jpeg at `quality`, 4:2:0
    for an RGB sheet; image.savePNG's byte rule is applied inside the encoder; restart_rows, restart_blocks and optimize
    and progressive are encode_jpeg's: optimize=True is the smaller payload, progressive=True the file a browser shows
    while it arrives).  Returns the file's bytes."""
    data._jpeg_options("display_jpeg", restart_rows, restart_blocks, optimize, progressive)      # refused before the sheet is built
    grid = display_tensor(x, **display_args)
    (jpg,) = data.encode_jpeg(grid.unsqueeze(0), quality, "420", restart_rows, restart_blocks, optimize, progressive)
    return jpg


def save_clip_sheet(path, input_image, pred_image, level=0):
    """test_vid.lua:131-137,149: pretty_output[2i-1] = input_image[i], pretty_output[2i] = pred_image[i] (predict_clip's two
    results, predLen x nc x fs x fs in [0,1]), saved as toDisplayTensor(pretty_output, 0, 10); level is save_sheet's."""
    from .backend import png_level
    level = png_level("save_clip_sheet", level)
    B = get_backend()
    a, b = B.from_host(torch.as_tensor(input_image)).float(), B.from_host(torch.as_tensor(pred_image)).float()
    assert a.dim() == 4 and a.shape == b.shape, "input_image and pred_image are predLen x nc x fs x fs"
    pretty = torch.stack([a, b], 1).reshape(2 * a.shape[0], *a.shape[1:])
    return save_sheet(path, pretty, level=level, padding=0, nrow=10)
