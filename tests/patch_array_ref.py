"""NumPy restatement of train_wholeim_input.lua's loader (datavid/donkey_wholeim.lua:49-74 loadImage, :141-215
trainHook), written the way the Lua reads: the three shifted zero arrays are materialised, then
flipped, then sliced with the 1-based window loop.  Float32, one rounding per operation.  The device kernel
(vf_patch_array_prepare) must match it bit for bit.  Not a test module: the tests import it."""
import numpy as np

import image_ref as R

NC = 3
MAXCROP_W, MAXCROP_H = 100, 70


def load_image(img, mask, height, width):
    """loadImage (:49-74) with the sizes passed in: img 3 x H x W float32 in [0,1] and the module-global Byte mask
    1 x Hm x Wm -> (the scaled frame, the NEW mask state: image.scale of the old one to the frame's size)."""
    return R.scale(np.asarray(img, np.float32), width, height), R.scale(np.asarray(mask, np.uint8), width, height)


def train_hook(inp, mask, ss, arrh, arrw, crop_w, crop_h, flip, maskValue):
    """trainHook (:141-215) after loadImage, the draws passed in (crop_w, crop_h 1-based).  inp: 3 x iH x iW float32,
    mask: 1 x iH x iW Byte.  Returns (out 12 x ss x ss, maskout 12 x ss x ss, masked 3*arrh*arrw x ss x ss, topleft_sum):
    out and masked in [-1,1]; topleft_sum is the double sum of the dark test's patch (:188-189; its mean is the sum
    over 3*ss*ss).  ValueError where the reference is not defined."""
    inp = np.asarray(inp, np.float32)
    nc, iH, iW = inp.shape
    if nc != NC:
        raise ValueError("the hook writes channel triples: nc=%d" % nc)
    if arrh < 2 or arrw < 2:
        raise ValueError("a %dx%d array divides by zero" % (arrh, arrw))
    steph = (iH - ss) // (arrh - 1)                                   # :153-154
    stepw = (iW - ss) // (arrw - 1)
    if steph < 2 or stepw < 2:
        raise ValueError("steps %d, %d over %dx%d: floor(h/step) does not number the windows" % (steph, stepw, iH, iW))
    if not (1 <= crop_h <= iH and 1 <= crop_w <= iW):
        raise ValueError("crop (%d,%d) outside %dx%d" % (crop_w, crop_h, iW, iH))
    out = np.full((NC * 2 * 2, ss, ss), np.nan, np.float32)           # torch.Tensor(...): uninitialised
    maskout = np.full((NC * 2 * 2, ss, ss), np.nan, np.float32)
    masked = np.full((NC * arrw * arrh, ss, ss), np.nan, np.float32)
    expandedmask = np.broadcast_to(np.asarray(mask, np.uint8), inp.shape)
    maskedinput = inp.copy()
    maskedinput[expandedmask != 0] = np.float32(maskValue)            # :162-164
    tmpinput = np.zeros(inp.shape, np.float32)                        # :169-174
    tmpmask = np.zeros(inp.shape, np.uint8)
    tmpmaskedinput = np.zeros(inp.shape, np.float32)
    tmpinput[:, 0:iH - crop_h + 1, 0:iW - crop_w + 1] = inp[:, crop_h - 1:iH, crop_w - 1:iW]
    tmpmask[:, 0:iH - crop_h + 1, 0:iW - crop_w + 1] = expandedmask[:, crop_h - 1:iH, crop_w - 1:iW]
    tmpmaskedinput[:, 0:iH - crop_h + 1, 0:iW - crop_w + 1] = maskedinput[:, crop_h - 1:iH, crop_w - 1:iW]
    if flip:                                                          # :177-181 image.hflip: over the full width
        tmpmask, tmpinput, tmpmaskedinput = tmpmask[:, :, ::-1], tmpinput[:, :, ::-1], tmpmaskedinput[:, :, ::-1]
    inp, expandedmask, maskedinput = tmpinput.copy(), tmpmask.copy(), tmpmaskedinput.copy()
    topleft_sum = float(inp[:, 0:ss, 0:ss].astype(np.float64).sum())  # :188-189 (TH's mean: a double sum)
    cntpatch = -2
    for h in range(1, iH - ss + 2, steph):                            # :196-211, 1-based
        for w in range(1, iW - ss + 2, stepw):
            cntpatch += 3
            if cntpatch + 2 > masked.shape[0]:
                raise ValueError("the loop visits more than %dx%d windows over %dx%d" % (arrh, arrw, iH, iW))
            masked[cntpatch - 1:cntpatch + 2] = maskedinput[:, h - 1:h + ss - 1, w - 1:w + ss - 1]
            h1, w1 = h // steph, w // stepw
            if h1 <= 1 and w1 <= 1:
                idx = (h1 * 2 + w1) * NC + 1
                out[idx - 1:idx + 2] = inp[:, h - 1:h + ss - 1, w - 1:w + ss - 1]
                maskout[idx - 1:idx + 2] = expandedmask[:, h - 1:h + ss - 1, w - 1:w + ss - 1]
    if cntpatch + 2 != masked.shape[0]:
        raise ValueError("the loop visits fewer than %dx%d windows over %dx%d" % (arrh, arrw, iH, iW))
    assert not (np.isnan(out).any() or np.isnan(maskout).any() or np.isnan(masked).any())
    out = out * np.float32(2) + np.float32(-1)                        # :212-213
    masked = masked * np.float32(2) + np.float32(-1)
    return out, maskout, masked, topleft_sum


def sample(img, mask, d, ss=128, arrh=3, arrw=3, maskValue=110.0 / 255.0):
    """loadImage + trainHook with the decisions d = {height, width, crop_w, crop_h, flip}: (masked, out, maskout) in the
    order dataset:sample returns them (dataset_wholeim.lua:400-429), the top-left sum, and the new mask state."""
    inp, state = load_image(img, mask, d["height"], d["width"])
    out, maskout, masked, s = train_hook(inp, state, ss, arrh, arrw, d["crop_w"], d["crop_h"], d["flip"], maskValue)
    return masked, out, maskout, s, state


def by_index(inp, mask, ss, arrh, arrw, crop_w, crop_h, flip, maskValue):
    """The same three tensors by an index formula: output pixel (p, y, x), p = ih * arrw + iw, reads the scaled pixel
    (ih*steph + y + crop_h-1, X' + crop_w-1), X = iw*stepw + x, X' = iW-1-X when flipped — or zero beyond the frame."""
    inp = np.asarray(inp, np.float32)
    _, iH, iW = inp.shape
    steph, stepw = (iH - ss) // (arrh - 1), (iW - ss) // (arrw - 1)
    out = np.zeros((12, ss, ss), np.float32)
    maskout = np.zeros((12, ss, ss), np.float32)
    masked = np.zeros((3 * arrh * arrw, ss, ss), np.float32)
    for p in range(arrh * arrw):
        ih, iw = divmod(p, arrw)
        for y in range(ss):
            for x in range(ss):
                X = iw * stepw + x
                sy, sx = ih * steph + y + crop_h - 1, (iW - 1 - X if flip else X) + crop_w - 1
                v, m = np.zeros(3, np.float32), 0
                if sy < iH and sx < iW:
                    v, m = inp[:, sy, sx], int(mask[0, sy, sx] != 0)
                masked[3 * p:3 * p + 3, y, x] = (np.float32(maskValue) if m else v) * np.float32(2) + np.float32(-1)
                if ih <= 1 and iw <= 1:
                    q = 2 * ih + iw
                    out[3 * q:3 * q + 3, y, x] = v * np.float32(2) + np.float32(-1)
                    maskout[3 * q:3 * q + 3, y, x] = m
    return out, maskout, masked
