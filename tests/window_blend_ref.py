"""Host reference for the overlapped, blended inference windows (vf_pipeline.hip: vf_windows_gather / _accumulate /
_finish; inference.WindowedInpainter).  NumPy only; float32, literal and slow.

The rule is the project's own (no reference script blends windows); this file is its definition and the kernels must
equal it bit for bit.

* `origins(n, size, stride)`: where the windows of one axis start.  0, stride, 2 stride, ... while the window fits, and
  one more at n - size if the last one ends before n.  Nothing is padded.  2 stride >= size is required, so two regular
  windows at most cover a sample, and with the clamped last one three.
* `weights(size, stride)`: integer taper, w(i) = min(i + 1, size - i, r + 1) with r = size - stride.  Between two regular
  neighbours the two weights sum to r + 1; r = 0 gives 1 everywhere.
* A window is (it, iy, ix), its number (it NY + iy) NX + ix, and it is batch row `number`; channel k of the row is frame
  ot[it] + k // nc, colour k % nc.  Its weight at a sample is the product of the three axis weights.
* `blend`: per output sample acc = 0, then for every covering window in ascending number acc = fl(acc + fl(float(w) v))
  (two roundings, no FMA), and out = fl(acc / float(sum of w)).  The sum of w is an integer from the geometry.
* `finish`: the masked paste (test_vid_wholeim.lua:214-220) and add(1):mul(0.5) (:222-224).

Why every integer here is exact in float32: per axis a sample has at most 3 covers, each of weight <= r + 1, so the
per-axis sum is <= 3 (r + 1) and the sum of products is <= 27 (ry + 1)(rx + 1)(rt + 1).  With fineSize 128 the spatial
overlaps are <= 64, so that is 27 * 65 * 65 * (rt + 1) = 114075 (rt + 1): below 2^24 for every rt + 1 <= 147, i.e. any
inputLen up to 292.  `check_exact` asserts the bound for a given plan; a plan beyond it is refused."""
import numpy as np

F32 = np.float32
MUTANTS = ("uniform", "drop_last", "swap_yx", "k_mod_L")


def origins(n, size, stride):
    if size < 1:
        raise ValueError("size=%r must be >= 1" % (size,))
    if n < size:
        raise ValueError("n=%r is smaller than the window size=%r; nothing is padded" % (n, size))
    if not 1 <= stride <= size:
        raise ValueError("stride=%r must lie in [1, size=%r]" % (stride, size))
    if 2 * stride < size:
        raise ValueError("stride=%r: 2 stride must be >= size=%r (an overlap of at most half a window)" % (stride, size))
    o = list(range(0, n - size + 1, stride))
    if o[-1] + size < n:
        o.append(n - size)
    return o


def weights(size, stride):
    r = size - stride
    return np.array([min(i + 1, size - i, r + 1) for i in range(size)], np.int64)


def axis_weight_sum(n, size, stride):
    """integer sum of the weights of all windows over each of the n samples of one axis, and the number of covers"""
    w = weights(size, stride)
    s, c = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for o in origins(n, size, stride):
        s[o:o + size] += w
        c[o:o + size] += 1
    return s, c


class Plan:
    """The windows of a clip of F frames H x W: windows of L frames x fs x fs, strides stride_t / stride."""

    def __init__(self, F, H, W, L, fs, stride, stride_t=None):
        stride_t = L if stride_t is None else stride_t
        self.F, self.H, self.W, self.L, self.fs, self.stride, self.stride_t = F, H, W, L, fs, stride, stride_t
        self.ot, self.oy, self.ox = origins(F, L, stride_t), origins(H, fs, stride), origins(W, fs, stride)
        self.wt, self.ws = weights(L, stride_t), weights(fs, stride)
        self.NT, self.NY, self.NX = len(self.ot), len(self.oy), len(self.ox)
        self.NW = self.NT * self.NY * self.NX
        check_exact(self)

    def window(self, w):
        it, rem = divmod(w, self.NY * self.NX)
        iy, ix = divmod(rem, self.NX)
        return self.ot[it], self.oy[iy], self.ox[ix]

    def weight_sum(self):
        """int64 F x H x W: the sum over all windows of the product weights = the product of the three per-axis sums"""
        st, _ = axis_weight_sum(self.F, self.L, self.stride_t)
        sy, _ = axis_weight_sum(self.H, self.fs, self.stride)
        sx, _ = axis_weight_sum(self.W, self.fs, self.stride)
        return st[:, None, None] * sy[None, :, None] * sx[None, None, :]


def check_exact(plan):
    """every weight and every weight sum is an integer below 2^24, hence exact as a float32"""
    rt, rs = plan.L - plan.stride_t, plan.fs - plan.stride
    bound = 27 * (rs + 1) * (rs + 1) * (rt + 1)
    if bound >= 1 << 24:
        raise ValueError("stride_t=%r, stride=%r: weight sums up to %d are not exact in float32" % (plan.stride_t, plan.stride, bound))
    assert int(plan.weight_sum().max()) <= bound


def gather(frames, plan):
    """frames F x nc x H x W -> the window batch NW x (L nc) x fs x fs (NCHW here; the device batch is NHWC)"""
    F, nc, H, W = frames.shape
    out = np.empty((plan.NW, plan.L * nc, plan.fs, plan.fs), F32)
    for w in range(plan.NW):
        t, y, x = plan.window(w)
        out[w] = frames[t:t + plan.L, :, y:y + plan.fs, x:x + plan.fs].reshape(plan.L * nc, plan.fs, plan.fs)
    return out


def _window_weight(plan, mutant):
    w3 = plan.wt[:, None, None] * plan.ws[None, :, None] * plan.ws[None, None, :]
    return np.ones_like(w3) if mutant == "uniform" else w3


def _place(plan, w, mutant):
    """(t, y, x) where window w is blended, or None if the (mutant) rule leaves it out"""
    t, y, x = plan.window(w)
    it, rem = divmod(w, plan.NY * plan.NX)
    iy, ix = divmod(rem, plan.NX)
    if mutant == "drop_last" and ((plan.NT > 1 and it == plan.NT - 1) or (plan.NY > 1 and iy == plan.NY - 1) or (plan.NX > 1 and ix == plan.NX - 1)):
        return None
    if mutant == "swap_yx":                                                # each table read with the other axis' index, kept inside the frame
        y = min(plan.ox[min(iy, plan.NX - 1)], plan.H - plan.fs)
        x = min(plan.oy[min(ix, plan.NY - 1)], plan.W - plan.fs)
    return t, y, x


def accumulate(acc, tiles, plan, nc, w0=0, mutant=None):
    """adds windows [w0, w0 + len(tiles)) to acc (F x nc x H x W float32) in ascending window number: two roundings per
    cover.  The mutants are wrong rules that the tests must be able to tell from the right one."""
    L, fs = plan.L, plan.fs
    w3 = _window_weight(plan, mutant).astype(F32)[:, None]                 # L x 1 x fs x fs, integers: exact
    for j in range(len(tiles)):
        at = _place(plan, w0 + j, mutant)
        if at is None:
            continue
        t, y, x = at
        if mutant == "k_mod_L":
            v = tiles[j].reshape(nc, L, fs, fs).transpose(1, 0, 2, 3)     # frame k % L, colour k // L
        else:
            v = tiles[j].reshape(L, nc, fs, fs)                            # frame k // nc, colour k % nc
        region = acc[t:t + L, :, y:y + fs, x:x + fs]
        region[...] = region + w3 * v.astype(F32)                          # fl(acc + fl(w v)): numpy rounds each operation


def mutant_weight_sum(plan, mutant):
    """the divisor a mutant rule would use: the sum of ITS weights where ITS windows lie (0 where none does)"""
    s = np.zeros((plan.F, plan.H, plan.W), np.int64)
    w3 = _window_weight(plan, mutant)
    for w in range(plan.NW):
        at = _place(plan, w, mutant)
        if at is not None:
            t, y, x = at
            s[t:t + plan.L, y:y + plan.fs, x:x + plan.fs] += w3
    return s


def blend(tiles, plan, nc, chunk=None, mutant=None):
    """tiles NW x (L nc) x fs x fs (the net's output rows) -> F x nc x H x W float32, accumulated chunk by chunk"""
    assert tiles.shape == (plan.NW, plan.L * nc, plan.fs, plan.fs) and tiles.dtype == F32
    chunk = plan.NW if chunk is None else chunk
    acc = np.zeros((plan.F, nc, plan.H, plan.W), F32)
    for w0 in range(0, plan.NW, chunk):
        accumulate(acc, tiles[w0:w0 + chunk], plan, nc, w0, mutant)
    if mutant in (None, "k_mod_L"):
        s = plan.weight_sum()
        assert s.min() > 0
    else:
        s = mutant_weight_sum(plan, mutant)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = acc / s.astype(F32)[:, None]                                 # IEEE float32 division, the integer exact
    return np.where(s[:, None] > 0, out, F32(0)).astype(F32)


def finish(out, frames, mask):
    """out, frames F x nc x H x W in [-1,1]; mask nc x H x W uint8 -> (outImages, inpaintImages, fullImages) in [0,1]:
    inpaint = out where the mask is set, the frame elsewhere; then add(1):mul(0.5) on all three"""
    inp = np.where(mask[None] != 0, out, frames).astype(F32)
    return tuple(((a + F32(1)) * F32(0.5)).astype(F32) for a in (out, inp, frames))


def inpaint(net, frames, mask, L, fs, stride, stride_t=None, chunk=None, mutant=None):
    """The whole driver on the host.  net: window batch n x (L nc) x fs x fs -> the same shape, row by row independent."""
    frames = np.asarray(frames, F32)
    F, nc, H, W = frames.shape
    plan = Plan(F, H, W, L, fs, stride, stride_t)
    tiles = np.asarray(net(gather(frames, plan)), F32)
    return finish(blend(tiles, plan, nc, chunk, mutant), frames, np.asarray(mask))
