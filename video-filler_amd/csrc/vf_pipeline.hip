// vf_pipeline.hip — the data formats either side of the hot path, as HBM-bound byte movers:
//   * batch preparation the reference does on the host per sample before the closures run
//     (train.lua:284-298 centre hole; datavid/donkey_folder.lua:135-189 crop / mask / fill / hflip / [0,1] -> [-1,1]),
//     written straight into the NHWC buffers the kernels read;
//   * the whole-image inference tile loop of test_vid_wholeim.lua:159-205 (gather fineSize tiles of the padded
//     planar clip into ONE NHWC batch, scatter the net's output tiles back), incl. its per-tile vertical-flip rule;
//   * the same loop for clips of any size and length: overlapped windows in y, x and t, gathered in chunks and blended
//     with integer weights in a fixed order.
// Every kernel is one pass: each output element is written once, each input element read at most once per output
// that needs it.  Threads run along the NHWC channel axis (fastest) so the stores are fully coalesced; the planar
// side is read in C strided streams that stay in L2 (the planes are a few MB).
#include "vf_common.h"

namespace {

inline int pgrid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(vf_cdiv(n, 256), 1 << 20)); }

// ---------------------------------------------------------------------------------------------------------------
// train.lua:284-298.  batch: B x C x fs x fs planar in [-1,1] (the loader's tensor).
//   center = batch[:, :, fs/4 : 3fs/4, fs/4 : 3fs/4]                  (clone BEFORE painting, :285)
//   ctx    = batch with [fs/4+ov, 3fs/4-ov)^2 of channel c set to fill[c]  (:287-289)
__global__ void k_center_prepare(const float* __restrict__ batch, float* __restrict__ ctx_out, float* __restrict__ center,
                                 const float* __restrict__ fill, int B, int C, int fs, int ov) {
  const int64_t n = (int64_t)B * fs * fs * C;
  const int lo = fs / 4, hi = fs / 2 + fs / 4, cs = fs / 2;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    int64_t t = i / C;
    const int x = (int)(t % fs);
    t /= fs;
    const int y = (int)(t % fs);
    const int b = (int)(t / fs);
    const float v = batch[(((int64_t)b * C + c) * fs + y) * fs + x];
    const bool hole = y >= lo + ov && y < hi - ov && x >= lo + ov && x < hi - ov;
    ctx_out[i] = hole ? fill[c] : v;
    if (y >= lo && y < hi && x >= lo && x < hi) center[(((int64_t)b * cs + (y - lo)) * cs + (x - lo)) * C + c] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// datavid/donkey_folder.lua:135-189 (trainHook with withMask) for ONE sample.
//   clip: C x iH x iW planar in [0,1] (decoded, scaled);  mask: iH x iW float (the scaled mask image, one channel)
//   crop (w1, h1) .. +fs (image.crop, :147);  maskout = crop(mask) expanded over C (:162-163)
//   mode 0: masked = out with maskout > 0 filled (maskedFill, :166 — Byte semantics: any non-zero value)
//   mode 1: randomBlockMask (:114-129): nblk square blocks of side bs at 1-based top-left (tlx, tly) are filled and
//           maskout = 1 there, 0 elsewhere
//   hflip (:178-183) mirrors all three;  out/masked -> 2x-1 (:185-187); maskout stays 0/1.
struct ClipPrep {
  const float* clip;
  const float* mask;
  float* full;      // fs x fs x C  NHWC, [-1,1]
  float* masked;    // fs x fs x C
  float* maskout;   // fs x fs x C  (0/1 as float: the trainers copy the Byte mask into a Float tensor, :394)
  int C, iH, iW, fs, w1, h1, flip, mode, nblk, bs;
  float mask_value;
  int tlx[10], tly[10];
};
__global__ void k_clip_prepare(const ClipPrep p) {
  const int64_t n = (int64_t)p.fs * p.fs * p.C;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % p.C);
    const int64_t t = i / p.C;
    const int x = (int)(t % p.fs), y = (int)(t / p.fs);
    const int sx = p.flip ? p.fs - 1 - x : x;          // column of the un-flipped crop
    const int gy = p.h1 + y, gx = p.w1 + sx;
    const float v = p.clip[((int64_t)c * p.iH + gy) * p.iW + gx];
    bool m;
    if (p.mode == 0) {
      m = p.mask[(int64_t)gy * p.iW + gx] != 0.f;
    } else {
      m = false;
      for (int k = 0; k < p.nblk; ++k) {
        const int bx = p.tlx[k] - 1, by = p.tly[k] - 1;   // 1-based Lua coordinates
        m = m || (sx >= bx && sx < bx + p.bs && y >= by && y < by + p.bs);
      }
    }
    p.full[i] = 2.f * v - 1.f;
    p.masked[i] = 2.f * (m ? p.mask_value : v) - 1.f;
    p.maskout[i] = m ? 1.f : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// test_vid_wholeim.lua:159-205.  full: (G*nc) x H x W planar (H, W multiples of fs).  Tile (ty, tx), group g ->
// batch row (ty*TX + tx)*G + g, NHWC fs x fs x nc.  vflip[t] != 0: the tile is flipped vertically on the way in
// (:167-170) and its output flipped back on the way out (:191-197).
__global__ void k_tiles_gather(const float* __restrict__ full, float* __restrict__ tiles, int G, int nc, int H, int W,
                               int fs, const unsigned char* __restrict__ vflip) {
  const int TX = W / fs;
  const int64_t n = (int64_t)(H / fs) * TX * G * fs * fs * nc;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % nc);
    int64_t t = i / nc;
    const int x = (int)(t % fs);
    t /= fs;
    const int y = (int)(t % fs);
    t /= fs;
    const int g = (int)(t % G);
    const int tile = (int)(t / G);
    const int ty = tile / TX, tx = tile - ty * TX;
    const int sy = (vflip && vflip[tile]) ? fs - 1 - y : y;
    tiles[i] = full[((int64_t)(g * nc + c) * H + ty * fs + sy) * W + tx * fs + x];
  }
}
__global__ void k_tiles_scatter(const float* __restrict__ tiles, float* __restrict__ out, int G, int nc, int H, int W,
                                int fs, const unsigned char* __restrict__ vflip) {
  const int TX = W / fs;
  const int64_t n = (int64_t)(H / fs) * TX * G * fs * fs * nc;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % nc);
    int64_t t = i / nc;
    const int x = (int)(t % fs);
    t /= fs;
    const int y = (int)(t % fs);
    t /= fs;
    const int g = (int)(t % G);
    const int tile = (int)(t / G);
    const int ty = tile / TX, tx = tile - ty * TX;
    const int dy = (vflip && vflip[tile]) ? fs - 1 - y : y;
    out[((int64_t)(g * nc + c) * H + ty * fs + dy) * W + tx * fs + x] = tiles[i];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Overlapped, blended inference windows (tests/window_blend_ref.py is the rule).  One axis of the plan:
// `count` windows of `size` samples over n samples, window i at min(i * stride, n - size) — regular origins and, where the
// last regular window ends before n, one clamped to the end.  The origins are this closed form of three integers the
// host has checked, so no table travels to the device and nothing unchecked is ever an address.  2 stride >= size: a sample
// has at most two regular covers and the clamped one.
struct WinAxis {
  int n, size, stride, count;
  __host__ __device__ int origin(int i) const { return i * stride < n - size ? i * stride : n - size; }
  // integer taper at local coordinate l: 1, 2, ... up to r + 1 = size - stride + 1, and down again
  __device__ int weight(int l) const { return min(min(l + 1, size - l), size - stride + 1); }
  // the windows [lo, hi] that hold sample p
  __device__ void cover(int p, int& lo, int& hi) const {
    hi = min(p / stride, count - 1);
    if (hi + 1 < count && origin(hi + 1) <= p) ++hi;      // the clamped last window starts inside its neighbour
    lo = hi;
    while (lo > 0 && origin(lo - 1) + size > p) --lo;
  }
  // sum of the weights of all covers of p: an integer of the geometry alone
  __device__ int weight_sum(int p) const {
    int lo, hi, s = 0;
    cover(p, lo, hi);
    for (int i = lo; i <= hi; ++i) s += weight(p - origin(i));
    return s;
  }
};
struct WinGeo {
  WinAxis t, y, x;     // t: F frames in windows of L;  y, x: H, W in windows of fs
  int nc;
};

// frames (F*nc) x H x W planar -> rows [w0, w0 + nw) of the window batch, NHWC nw x fs x fs x (L*nc): window
// (it, iy, ix) has number (it*NY + iy)*NX + ix, channel k of its row is frame origin_t + k / nc, colour k % nc.
__global__ void k_windows_gather(const float* __restrict__ frames, float* __restrict__ tiles, const WinGeo g, int w0, int nw) {
  const int fs = g.y.size, Ck = g.t.size * g.nc, H = g.y.n, W = g.x.n;
  const int64_t n = (int64_t)nw * fs * fs * Ck;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % Ck);
    int64_t r = i / Ck;
    const int x = (int)(r % fs);
    r /= fs;
    const int y = (int)(r % fs);
    const int w = w0 + (int)(r / fs);
    const int ix = w % g.x.count, iy = (w / g.x.count) % g.y.count, it = w / (g.x.count * g.y.count);
    const int f = g.t.origin(it) + k / g.nc, c = k % g.nc;
    tiles[i] = frames[((int64_t)(f * g.nc + c) * H + g.y.origin(iy) + y) * W + g.x.origin(ix) + x];
  }
}

// Gather form of the blend: one thread owns one sample (frame f0 + .., colour, row y0 + .., column) of the accumulator
// (F*nc) x H x W and adds the contributions of the windows [w0, w0 + nw) that hold it, in ascending window number:
// acc = fadd(acc, fmul(float(w), v)), two roundings.  Chunks are launched in ascending order on one stream, so every sample
// sees all its covers in ascending number whatever the chunk size.  No atomics.  The launch spans frames [f0, f0 + nf) and
// rows [y0, y0 + ny): what the chunk's windows can touch.  Threads run along colour, then x: the NHWC rows are read in
// whole runs of nc floats per pixel and each colour plane is touched in runs of blockDim / nc columns.
__global__ void k_windows_accumulate(const float* __restrict__ tiles, float* __restrict__ acc, const WinGeo g, int w0, int nw,
                                     int f0, int nf, int y0, int ny) {
  const int fs = g.y.size, nc = g.nc, Ck = g.t.size * nc, H = g.y.n, W = g.x.n;
  const int64_t n = (int64_t)nf * ny * W * nc;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % nc);
    int64_t r = i / nc;
    const int x = (int)(r % W);
    r /= W;
    const int y = y0 + (int)(r % ny);
    const int f = f0 + (int)(r / ny);
    int tl, th, yl, yh, xl, xh;
    g.t.cover(f, tl, th);
    g.y.cover(y, yl, yh);
    g.x.cover(x, xl, xh);
    float* dst = acc + ((int64_t)(f * nc + c) * H + y) * W + x;
    float a = 0.f;
    bool any = false;
    for (int it = tl; it <= th; ++it) {
      const int lt = f - g.t.origin(it), wt = g.t.weight(lt);
      for (int iy = yl; iy <= yh; ++iy) {
        const int ly = y - g.y.origin(iy), wy = wt * g.y.weight(ly);
        for (int ix = xl; ix <= xh; ++ix) {
          const int w = (it * g.y.count + iy) * g.x.count + ix - w0;
          if (w < 0 || w >= nw) continue;
          const int lx = x - g.x.origin(ix);
          if (!any) {
            a = *dst;
            any = true;
          }
          const float v = tiles[(((int64_t)w * fs + ly) * fs + lx) * Ck + lt * nc + c];
          a = __fadd_rn(a, __fmul_rn((float)(wy * g.x.weight(lx)), v));
        }
      }
    }
    if (any) *dst = a;
  }
}

// out = fdiv(acc, float(sum of weights)); then, with frames given, the masked paste of test_vid_wholeim.lua:214-220 (mask:
// nc x H x W Byte, non-zero = hole) and add(1):mul(0.5) (:222-224) on all three results, as vf_masked_compose and
// vf_scale_shift(0.5, 0.5) compute them.  Planar throughout, x fastest.
__global__ void k_windows_finish(const float* __restrict__ acc, const float* __restrict__ frames, const unsigned char* __restrict__ mask,
                                 float* __restrict__ out, float* __restrict__ inpaint, float* __restrict__ full, const WinGeo g) {
  const int nc = g.nc, H = g.y.n, W = g.x.n;
  const int64_t n = (int64_t)g.t.n * nc * H * W;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % W);
    int64_t r = i / W;
    const int y = (int)(r % H);
    r /= H;
    const int c = (int)(r % nc), f = (int)(r / nc);
    const int s = g.t.weight_sum(f) * g.y.weight_sum(y) * g.x.weight_sum(x);
    const float o = __fdiv_rn(acc[i], (float)s);
    if (!frames) {
      out[i] = o;
      continue;
    }
    const float fr = frames[i];
    const float p = mask[((int64_t)c * H + y) * W + x] != 0 ? o : fr;
    out[i] = __fadd_rn(__fmul_rn(o, 0.5f), 0.5f);
    inpaint[i] = __fadd_rn(__fmul_rn(p, 0.5f), 0.5f);
    full[i] = __fadd_rn(__fmul_rn(fr, 0.5f), 0.5f);
  }
}

}  // namespace

VF_API int vf_center_prepare(vf_ctx* ctx, const float* batch_nchw, float* ctx_nhwc, float* center_nhwc,
                             const float* fill, int B, int C, int fs, int overlapPred) {
  VF_REQUIRE(B > 0 && C > 0 && fs >= 4 && fs % 4 == 0, "vf_center_prepare: bad shape B=%d C=%d fineSize=%d", B, C, fs);
  VF_REQUIRE(overlapPred >= 0 && 2 * overlapPred < fs / 2, "vf_center_prepare: overlapPred=%d does not fit", overlapPred);
  const int64_t n = (int64_t)B * C * fs * fs;
  VfProf prof(ctx, "center_prepare", 0.0, 4.0 * (double)n * 2.25);
  hipLaunchKernelGGL(k_center_prepare, dim3(pgrid(n)), dim3(256), 0, ctx->stream, batch_nchw, ctx_nhwc, center_nhwc, fill,
                     B, C, fs, overlapPred);
  VF_LAUNCH_CHECK();
  return 0;
}

VF_API int vf_clip_prepare(vf_ctx* ctx, const float* clip, const float* mask, float* full, float* masked,
                           float* maskout, int C, int iH, int iW, int fs, int w1, int h1, int flip, float mask_value,
                           int nblocks, int block_size, const int* tlx, const int* tly) {
  VF_REQUIRE(C > 0 && fs > 0 && w1 >= 0 && h1 >= 0 && w1 + fs <= iW && h1 + fs <= iH,
             "vf_clip_prepare: crop (%d,%d)+%d outside the %dx%d clip", w1, h1, fs, iW, iH);
  VF_REQUIRE(nblocks >= 0 && nblocks <= 10, "vf_clip_prepare: at most 10 random blocks (donkey_folder.lua:121), got %d", nblocks);
  VF_REQUIRE(nblocks > 0 || mask != nullptr, "vf_clip_prepare: a mask image or random blocks are required");
  ClipPrep p;
  p.clip = clip; p.mask = mask; p.full = full; p.masked = masked; p.maskout = maskout;
  p.C = C; p.iH = iH; p.iW = iW; p.fs = fs; p.w1 = w1; p.h1 = h1; p.flip = flip ? 1 : 0;
  p.mode = nblocks > 0 ? 1 : 0; p.nblk = nblocks; p.bs = block_size; p.mask_value = mask_value;
  for (int k = 0; k < 10; ++k) {
    p.tlx[k] = k < nblocks ? tlx[k] : 0;     // host arrays
    p.tly[k] = k < nblocks ? tly[k] : 0;
    if (k < nblocks)
      VF_REQUIRE(p.tlx[k] >= 1 && p.tly[k] >= 1 && p.tlx[k] - 1 + block_size <= fs && p.tly[k] - 1 + block_size <= fs,
                 "vf_clip_prepare: block %d at (%d,%d) size %d leaves the %d crop", k, p.tlx[k], p.tly[k], block_size, fs);
  }
  const int64_t n = (int64_t)C * fs * fs;
  VfProf prof(ctx, "clip_prepare", 0.0, 4.0 * (double)n * 4);
  hipLaunchKernelGGL(k_clip_prepare, dim3(pgrid(n)), dim3(256), 0, ctx->stream, p);
  VF_LAUNCH_CHECK();
  return 0;
}

static int tiles_check(int G, int nc, int H, int W, int fs) {
  VF_REQUIRE(G > 0 && nc > 0 && fs > 0 && H > 0 && W > 0 && H % fs == 0 && W % fs == 0,
             "tile loop: the %dx%d clip must be padded to multiples of fineSize=%d (test_vid_wholeim.lua:108)", H, W, fs);
  return 0;
}
VF_API int vf_tiles_gather(vf_ctx* ctx, const float* full, float* tiles, int groups, int nc, int H, int W, int fs,
                           const unsigned char* vflip) {
  if (int e = tiles_check(groups, nc, H, W, fs)) return e;
  const int64_t n = (int64_t)groups * nc * H * W;
  VfProf prof(ctx, "tiles_gather", 0.0, 8.0 * (double)n);
  hipLaunchKernelGGL(k_tiles_gather, dim3(pgrid(n)), dim3(256), 0, ctx->stream, full, tiles, groups, nc, H, W, fs, vflip);
  VF_LAUNCH_CHECK();
  return 0;
}
VF_API int vf_tiles_scatter(vf_ctx* ctx, const float* tiles, float* out, int groups, int nc, int H, int W, int fs,
                            const unsigned char* vflip) {
  if (int e = tiles_check(groups, nc, H, W, fs)) return e;
  const int64_t n = (int64_t)groups * nc * H * W;
  VfProf prof(ctx, "tiles_scatter", 0.0, 8.0 * (double)n);
  hipLaunchKernelGGL(k_tiles_scatter, dim3(pgrid(n)), dim3(256), 0, ctx->stream, tiles, out, groups, nc, H, W, fs, vflip);
  VF_LAUNCH_CHECK();
  return 0;
}

// One axis of a window plan, checked: n >= size, 1 <= stride <= size, 2 stride >= size.  nname, sname and stname are the caller's
// names of n, size and stride, for the message.
static int windows_axis(const char* who, const char* nname, const char* sname, const char* stname, int n, int size, int stride,
                        WinAxis* a) {
  VF_REQUIRE(size >= 1, "%s: %s=%d must be >= 1", who, sname, size);
  VF_REQUIRE(n >= size, "%s: %s=%d is smaller than a window (%s=%d); nothing is padded", who, nname, n, sname, size);
  VF_REQUIRE(stride >= 1 && stride <= size, "%s: %s=%d must lie in [1, %s=%d]", who, stname, stride, sname, size);
  VF_REQUIRE(2 * (int64_t)stride >= size, "%s: %s=%d: 2 %s must be >= %s=%d (an overlap of at most half a window)", who, stname,
             stride, stname, sname, size);
  a->n = n; a->size = size; a->stride = stride;
  a->count = (n - size) / stride + 1 + ((n - size) % stride != 0 ? 1 : 0);
  return 0;
}
static int windows_geo(const char* who, int F, int nc, int H, int W, int L, int fs, int stride, int stride_t, WinGeo* g) {
  VF_REQUIRE(nc >= 1, "%s: nc=%d must be >= 1", who, nc);
  if (int e = windows_axis(who, "F", "inputLen", "stride_t", F, L, stride_t, &g->t)) return e;
  if (int e = windows_axis(who, "H", "fineSize", "stride", H, fs, stride, &g->y)) return e;
  if (int e = windows_axis(who, "W", "fineSize", "stride", W, fs, stride, &g->x)) return e;
  g->nc = nc;
  // a sample has at most 3 covers per axis, each of weight <= r + 1: weights and their sums stay exact in float
  const int64_t bound = 27 * (int64_t)(fs - stride + 1) * (fs - stride + 1) * (L - stride_t + 1);
  VF_REQUIRE(bound < (1 << 24), "%s: stride=%d, stride_t=%d: weight sums up to %lld are not exact in float", who, stride, stride_t,
             (long long)bound);
  VF_REQUIRE((int64_t)g->t.count * g->y.count * g->x.count < INT32_MAX && (int64_t)F * nc < INT32_MAX && (int64_t)L * nc < INT32_MAX,
             "%s: the clip (F=%d, nc=%d, inputLen=%d) has too many windows or planes to number in 32 bits", who, F, nc, L);
  return 0;
}
static int windows_chunk(const char* who, const WinGeo& g, int w0, int nw) {
  const int64_t NW = (int64_t)g.t.count * g.y.count * g.x.count;
  VF_REQUIRE(w0 >= 0 && nw >= 1 && (int64_t)w0 + nw <= NW, "%s: windows [w0=%d, +nw=%d) leave the plan's %lld", who, w0, nw, (long long)NW);
  return 0;
}
VF_API int vf_windows_gather(vf_ctx* ctx, const float* frames, float* tiles, int F, int nc, int H, int W, int inputLen, int fs,
                             int stride, int stride_t, int w0, int nw) {
  WinGeo g;
  if (int e = windows_geo("vf_windows_gather", F, nc, H, W, inputLen, fs, stride, stride_t, &g)) return e;
  if (int e = windows_chunk("vf_windows_gather", g, w0, nw)) return e;
  VF_REQUIRE(frames && tiles, "vf_windows_gather: frames and tiles are required");
  const int64_t n = (int64_t)nw * inputLen * nc * fs * fs;
  VfProf prof(ctx, "windows_gather", 0.0, 8.0 * (double)n);
  hipLaunchKernelGGL(k_windows_gather, dim3(pgrid(n)), dim3(256), 0, ctx->stream, frames, tiles, g, w0, nw);
  VF_LAUNCH_CHECK();
  return 0;
}
VF_API int vf_windows_accumulate(vf_ctx* ctx, const float* tiles, float* acc, int F, int nc, int H, int W, int inputLen, int fs,
                                 int stride, int stride_t, int w0, int nw) {
  WinGeo g;
  if (int e = windows_geo("vf_windows_accumulate", F, nc, H, W, inputLen, fs, stride, stride_t, &g)) return e;
  if (int e = windows_chunk("vf_windows_accumulate", g, w0, nw)) return e;
  VF_REQUIRE(tiles && acc, "vf_windows_accumulate: tiles and acc are required");
  // the frames, and for a chunk inside one temporal window the rows, that the chunk's windows touch
  const int per_t = g.y.count * g.x.count, w1 = w0 + nw - 1;
  const int it0 = w0 / per_t, it1 = w1 / per_t;
  const int f0 = g.t.origin(it0), nf = g.t.origin(it1) + inputLen - f0;
  int y0 = 0, ny = H;
  if (it0 == it1) {
    y0 = g.y.origin((w0 % per_t) / g.x.count);
    ny = g.y.origin((w1 % per_t) / g.x.count) + fs - y0;
  }
  const int64_t n = (int64_t)nf * nc * ny * W;
  VfProf prof(ctx, "windows_accumulate", 0.0, 4.0 * (double)nw * inputLen * nc * fs * fs + 8.0 * (double)n);
  hipLaunchKernelGGL(k_windows_accumulate, dim3(pgrid(n)), dim3(256), 0, ctx->stream, tiles, acc, g, w0, nw, f0, nf, y0, ny);
  VF_LAUNCH_CHECK();
  return 0;
}
VF_API int vf_windows_finish(vf_ctx* ctx, const float* acc, const float* frames, const unsigned char* mask, float* out,
                             float* inpaint, float* full, int F, int nc, int H, int W, int inputLen, int fs, int stride,
                             int stride_t) {
  WinGeo g;
  if (int e = windows_geo("vf_windows_finish", F, nc, H, W, inputLen, fs, stride, stride_t, &g)) return e;
  VF_REQUIRE(acc && out, "vf_windows_finish: acc and out are required");
  VF_REQUIRE(frames ? (mask && inpaint && full) : (!mask && !inpaint && !full),
             "vf_windows_finish: frames, mask, inpaint and full go together (all for the paste and the [0,1] mapping, or none)");
  const int64_t n = (int64_t)F * nc * H * W;
  VfProf prof(ctx, "windows_finish", 0.0, (frames ? 21.0 : 8.0) * (double)n);
  hipLaunchKernelGGL(k_windows_finish, dim3(pgrid(n)), dim3(256), 0, ctx->stream, acc, frames, mask, out, inpaint, full, g);
  VF_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------ table modules, noise
// nn.JoinTable(2) forward / backward in the NHWC layout: dst[p][c_dst + c] = src[p][c_src + c], c < Cc.
__global__ void k_channel_copy(const float* __restrict__ src, int Cs, int cs0, float* __restrict__ dst, int Cd, int cd0, int Cc,
                               int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = i / Cc;
    const int c = (int)(i - p * Cc);
    dst[p * Cd + cd0 + c] = src[p * Cs + cs0 + c];
  }
}
VF_API int vf_channel_copy(vf_ctx* ctx, const float* src, int Csrc, int c_src, float* dst, int Cdst, int c_dst, int Ccopy,
                           int64_t npix) {
  VF_REQUIRE(Ccopy > 0 && c_src >= 0 && c_dst >= 0 && c_src + Ccopy <= Csrc && c_dst + Ccopy <= Cdst && npix > 0,
             "vf_channel_copy: channels [%d,+%d) of %d -> [%d,+%d) of %d", c_src, Ccopy, Csrc, c_dst, Ccopy, Cdst);
  const int64_t n = npix * Ccopy;
  VfProf prof(ctx, "channel_copy", 0.0, 8.0 * (double)n);
  hipLaunchKernelGGL(k_channel_copy, dim3(pgrid(n)), dim3(256), 0, ctx->stream, src, Csrc, c_src, dst, Cdst, c_dst, Ccopy, n);
  VF_LAUNCH_CHECK();
  return 0;
}

// noise:uniform(-1, 1) / noise:normal(0, 1) (train.lua:319-323).  Torch7's Mersenne-Twister stream cannot be reproduced;
// element i of draw `counter` is a pure function of (seed, counter, i): splitmix64 of the 64-bit index, 24-bit
// uniforms, Box-Muller for the normal.  The oracle restates it (oracle.noise_fill).
__device__ __forceinline__ uint64_t vf_splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__global__ void k_noise_fill(float* __restrict__ out, int64_t n, uint64_t seed, const int32_t* __restrict__ counter_dev,
                             uint64_t counter, int normal) {
  const uint64_t ctr = counter_dev ? (uint64_t)(uint32_t)counter_dev[0] : counter;
  const uint64_t base = vf_splitmix64(seed ^ vf_splitmix64(ctr));
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t z = vf_splitmix64(base + (uint64_t)i * 0xD1342543DE82EF95ull);
    const float u1 = (float)((z >> 40) + 1) * 5.9604644775390625e-8f;            // (0, 1]
    const float u2 = (float)((z >> 16) & 0xFFFFFF) * 5.9604644775390625e-8f;     // [0, 1)
    out[i] = normal ? sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2) : 2.f * u2 - 1.f;
  }
}
VF_API int vf_noise_fill(vf_ctx* ctx, float* out, int64_t n, uint64_t seed, const int32_t* counter_dev, uint64_t counter,
                         int normal) {
  VF_REQUIRE(n > 0, "vf_noise_fill: empty tensor");
  VfProf prof(ctx, "noise_fill", 0.0, 4.0 * (double)n);
  hipLaunchKernelGGL(k_noise_fill, dim3(pgrid(n)), dim3(256), 0, ctx->stream, out, n, seed, counter_dev, counter, normal);
  VF_LAUNCH_CHECK();
  return 0;
}
