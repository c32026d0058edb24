"""Host reference for the contact sheets (vf_display.hip).  NumPy only; float32, literal and slow.

Torch7's `image` package is not part of the reference, so `image.toDisplayTensor` and `image.minmax` are restated here
from memory of the 2016-era package, for the one input form the inference scripts use (a packed Float tensor
N x C x h x w, C = 1 or 3).  This file is the pin: the device kernels must equal it bit for bit, and
tests/test_display_ref.py holds it to hand-computed cases.

* `minmax(t, min, max, symmetric, saturate)`: image.minmax{tensor, min, max, symm, saturate} on a Float tensor.  Lua
  numbers are doubles; a number that meets the tensor (`add(-min)`, `div(max)`) is cast to float once, there.
* `to_display_tensor(...)`: the layout on a grid filled with `packed:max()`, and where minmax runs.
* `center_finish(ctx, pred, ov)`: the tail of test.lua / demo.lua (test.lua:98-128).
Inputs are finite; what NaN or Inf do is unspecified."""
import math

import numpy as np

F = np.float32


def minmax(t, min=None, max=None, symmetric=False, saturate=False):
    """-> a new float32 array.  `fmin` starts at 0 as in the package, so `symmetric` with `min` given and `max` absent
    leaves a divisor of 0 and nothing is divided."""
    t = np.array(t, dtype=F)
    if min is None and max is None:
        saturate = False                                    # saturate useless if min/max inferred
    fmin = F(0)
    if min is None:
        if symmetric:
            fmin = np.maximum(np.abs(t.min()), np.abs(t.max()))
            min = -fmin
        else:
            min = t.min()
    if min != 0:
        t = t + F(-min)                                     # tensor:add(-min)
    if max is None:
        d = F(2.0 * float(fmin)) if symmetric else t.max()  # fmin * 2, or the SHIFTED tensor's max(): fl32(tmax - min)
    else:
        d = F(float(max) - float(min))                      # max - min in double, cast once by tensor:div
    if d != 0:
        t = t / d                                           # IEEE float32 division
    if saturate:
        t = np.where(t > 1, F(1), np.where(t < 0, F(0), t)).astype(F)
    assert t.dtype == F
    return t


def grid_shape(N, C, h, w, padding=0, nrow=6):
    xmaps = min(nrow, N)
    ymaps = math.ceil(N / xmaps)
    return xmaps, ymaps, (C, (h + padding) * ymaps, (w + padding) * xmaps)


def to_display_tensor(x, padding=0, nrow=6, scaleeach=False, min=None, max=None, symmetric=False, saturate=True):
    packed = np.array(x, dtype=F)
    if packed.ndim != 4 or packed.shape[1] not in (1, 3):
        raise ValueError("only packed N x C x h x w tensors with C = 1 or 3, got %s" % (packed.shape,))
    if padding < 0 or padding % 2:
        raise ValueError("padding=%r must be even and >= 0" % (padding,))
    N, C, h, w = packed.shape
    if scaleeach:
        for i in range(N):
            packed[i] = minmax(packed[i], min, max, symmetric, saturate)
    xmaps, ymaps, shape = grid_shape(N, C, h, w, padding, nrow)
    height, width = h + padding, w + padding
    grid = np.full(shape, packed.max(), dtype=F)
    k = 0
    for y in range(ymaps):
        for x_ in range(xmaps):
            if k >= N:
                break
            y0, x0 = y * height + padding // 2, x_ * width + padding // 2
            grid[:, y0:y0 + h, x0:x0 + w] = packed[k]
            k += 1
    if not scaleeach:
        grid = minmax(grid, min, max, symmetric, saturate)
    return grid


def unit(x):
    """add(1):mul(0.5) in float32"""
    return ((np.asarray(x, F) + F(1)) * F(0.5)).astype(F)


def center_finish(ctx, pred, ov):
    """ctx: B x C x fs x fs (the generator input, hole painted), pred: B x C x fs/2 x fs/2, both planar here, [-1,1].
    -> (pretty_output 2B x C x fs x fs, pasted context B x C x fs x fs, mapped prediction B x C x fs/2 x fs/2)."""
    ctx, pred = np.asarray(ctx, F), np.asarray(pred, F)
    B, C, fs, _ = ctx.shape
    if fs % 4 or fs // 2 - 2 * ov <= 0 or ov < 0:
        raise ValueError("fineSize=%d, overlapPred=%d: fineSize %% 4 must be 0 and the hole non-empty" % (fs, ov))
    assert pred.shape == (B, C, fs // 2, fs // 2)
    lo, hi = fs // 4 + ov, fs // 2 + fs // 4 - ov
    pasted = ctx.copy()
    pasted[:, :, lo:hi, lo:hi] = pred[:, :, ov:fs // 2 - ov, ov:fs // 2 - ov]           # test.lua:98
    inp = unit(ctx)                                                                       # :101
    pasted = unit(pasted)                                                                 # :102
    inp[:, :, lo:hi, lo:hi] = F(1)                                                        # :122-124
    pretty = np.empty((2 * B, C, fs, fs), F)
    pretty[0::2] = inp                                                                    # :126
    pretty[1::2] = pasted                                                                 # :127
    return pretty, pasted, unit(pred)
