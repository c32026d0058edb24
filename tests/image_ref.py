"""NumPy float32 restatement of Torch7's image.scale (bilinear mode; image.c scaleLinear_rowcol / scaleBilinear, as
restated in DESIGN.md 5.1) and of the three loaders that call it.  Op by op in float32, one rounding per operation,
vectorised over the axis that is not being resized.  The device kernels (csrc/vf_image.hip) must match it bit for bit.
Not a test module: the tests import it."""
import math

import numpy as np

F1 = np.float32(1)


def fi_byte(x):
    """image.c FromIntermediate for Byte: x += 0.5, clamp to [0, 255], truncate (kept in float32)."""
    x = np.asarray(x, np.float32) + np.float32(0.5)
    return np.where(x <= 0, np.float32(0), np.where(x >= 255, np.float32(255), np.trunc(x))).astype(np.float32)


def rowcol(s, D, byte=False):
    """scaleLinear_rowcol along the last axis: s (..., S) float32 -> (..., D) float32.  byte: round every computed
    value through FromIntermediate (the destination is a ByteTensor)."""
    s = np.asarray(s, np.float32)
    S = s.shape[-1]
    fi = fi_byte if byte else (lambda v: v)
    d = np.empty(s.shape[:-1] + (D,), np.float32)
    if D > S:
        if S == 1:
            d[..., :D - 1] = s[..., :1]
        else:
            scale = np.float32(S - 1) / np.float32(D - 1)
            for k in range(D - 1):
                f = np.float32(k) * scale
                i = int(f)
                f = np.float32(f - np.float32(i))
                d[..., k] = fi((F1 - f) * s[..., i] + f * s[..., min(i + 1, S - 1)])
        d[..., D - 1] = s[..., S - 1]
    elif D < S:
        scale = np.float32(S) / np.float32(D)
        i0, f0 = 0, np.float32(0)
        for k in range(D):
            f1 = np.float32(k + 1) * scale
            i1 = int(f1)
            f1 = np.float32(f1 - np.float32(i1))
            acc = (F1 - f0) * s[..., i0]
            n = F1 - f0
            for t in range(i0 + 1, i1):
                acc = acc + s[..., t]
                n = n + F1
            if i1 < S:
                acc = acc + f1 * s[..., i1]
                n = n + f1
            d[..., k] = fi(acc / n)
            i0, f0 = i1, f1
    else:
        d[...] = s
    return d


def scale(src, width, height):
    """image.scale(src, width, height): src C x H x W (float32, or uint8 for the Byte path) -> C x height x width of the
    same type.  Rows first, then columns; the intermediate has the source's type (Byte: rounded)."""
    byte = np.asarray(src).dtype == np.uint8
    width, height = int(width), int(height)
    tmp = rowcol(np.asarray(src, np.float32), width, byte)
    out = rowcol(tmp.swapaxes(-1, -2), height, byte).swapaxes(-1, -2)
    return np.ascontiguousarray(out.astype(np.uint8) if byte else out)


def decoded_to_float(hwc):
    """image.load(path, nc, 'float') of a decoded uint8 H x W x C frame: C x H x W, b / 255 in float32."""
    return np.ascontiguousarray(np.asarray(hwc, np.uint8).transpose(2, 0, 1).astype(np.float32) / np.float32(255))


def byte_mask(decoded):
    """image.load(maskName):byte(): the [0,1] float image truncated to Byte, so only 255 becomes 1."""
    return (np.asarray(decoded) == 255).astype(np.uint8)


def hook2d(img, height, width, fs, w1, h1, flip):
    """data/donkey_folder.lua:40-88 with the draws passed in: scale C x H x W float to height x width, crop fs x fs at
    0-based (w1, h1), hflip, mul(2):add(-1)."""
    out = scale(img, width, height)[:, h1:h1 + fs, w1:w1 + fs]
    if flip:
        out = out[:, :, ::-1]
    return np.ascontiguousarray(out * np.float32(2) + np.float32(-1))


def load_cont(frames, height, width):
    """datavid/donkey_folder.lua:71-105 (loadContImages): predLen x nc x H x W float frames, channel-stacked, scaled."""
    frames = np.asarray(frames, np.float32)
    P, nc, H, W = frames.shape
    return scale(frames.reshape(P * nc, H, W), width, height)


def whole_sizes(loadSize, fineSize):
    """test_vid_wholeim.lua:109-111: (inh, inw, outh, outw); inw is truncated by the tensor constructor, outw is not."""
    inw = loadSize * 480 / 360
    return loadSize, int(inw), math.ceil(loadSize / fineSize) * fineSize, math.ceil(inw / fineSize) * fineSize


def whole_frames(frames, mask, loadSize, fineSize, maskValue):
    """test_vid_wholeim.lua:109-141, 208-212.  frames: predLen x nc x H x W float; mask: Byte (1 or nc) x Hm x Wm.
    Returns (fullImages (predLen*nc) x outh x outw in [-1,1], padmask nc x outh x outw Byte)."""
    frames = np.asarray(frames, np.float32)
    P, nc = frames.shape[:2]
    inh, inw, outh, outw = whole_sizes(loadSize, fineSize)
    mask = np.ascontiguousarray(np.broadcast_to(mask, (nc,) + mask.shape[1:]))
    smask = scale(mask, inw, inh)
    scMask = smask > 0.3
    images = np.zeros((P, nc, outh, outw), np.float32)
    for i in range(P):
        im = scale(frames[i], inw, inh)
        im[scMask] = np.float32(maskValue)
        images[i, :, :inh, :inw] = scale(im.copy(), inw, inh)
    images = images * np.float32(2) + np.float32(-1)
    padmask = np.zeros((nc, outh, outw), np.uint8)
    padmask[:, :inh, :inw] = smask
    return images.reshape(P * nc, outh, outw), padmask
