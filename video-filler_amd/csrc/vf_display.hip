// vf_display.hip — the contact sheets of the inference scripts:
//   * image.toDisplayTensor of a packed N x C x h x w float tensor, C in {1, 3} (test.lua:129, demo.lua:96,
//     test_vid.lua:149): the images laid out on a grid filled with the pack's maximum, then image.minmax over the grid —
//     or over every image before the layout (scaleeach).  The `image` package is not part of the reference; the rule is
//     restated from memory in tests/display_ref.py, and these kernels equal that file bit for bit.
//   * the tail of test.lua / demo.lua (test.lua:98-128 = demo.lua:73-95): paste the prediction into the context, map
//     [-1,1] -> [0,1], paint the input's hole white, interleave the two into pretty_output.
// Two launches for a sheet.  k_display_minmax leaves (min, max) partials of the pack — of every image with scaleeach —
// in the workspace; k_display_layout reduces the few partials it needs in every block and writes the normalised grid,
// one cell (image + its padding) per blockIdx.y, threads along the grid's rows.  min / max do not depend on the order
// of their operands (inputs are finite), so the grid is the same on every run; there are no atomics.
#include "vf_common.h"

namespace {

constexpr int DISP_SLICE = 8192;      // elements of one reduction block's slice, at least
constexpr int DISP_PMAX = 256;        // partials of the whole pack: one per thread of a layout block
constexpr int DISP_PMAX_EACH = 8;     // partials per image with scaleeach

struct DispNorm {
  double min, max;                    // the caller's bounds (has_min / has_max)
  int has_min, has_max, symmetric, saturate;
};

// image.minmax's decisions for a tensor whose extremes are (tmin, tmax)
struct DispMap {
  float shift, d;
  int add, div, sat;
  __device__ __forceinline__ float operator()(float v) const {
    if (add) v = v + shift;
    if (div) v = v / d;               // IEEE division, correctly rounded (the default; no reciprocal)
    if (sat) v = v > 1.f ? 1.f : (v < 0.f ? 0.f : v);
    return v;
  }
};
__device__ __forceinline__ DispMap disp_map(const DispNorm& a, float tmin, float tmax) {
  DispMap m;
  float fmin = 0.f;
  double mn;
  if (!a.has_min) {
    float mnf;
    if (a.symmetric) {
      fmin = fmaxf(fabsf(tmin), fabsf(tmax));
      mnf = -fmin;
    } else {
      mnf = tmin;
    }
    mn = (double)mnf;
    m.shift = -mnf;
    m.add = mnf != 0.f;
  } else {
    mn = a.min;
    m.shift = (float)(-a.min);        // tensor:add(-min): the Lua number reaches the Float tensor as one cast
    m.add = a.min != 0.0;
  }
  if (!a.has_max)
    m.d = a.symmetric ? (float)(2.0 * (double)fmin) : (m.add ? tmax + m.shift : tmax);   // else: the shifted tensor's max()
  else
    m.d = (float)(a.max - mn);        // max - min in double, cast once
  m.div = m.d != 0.f;
  m.sat = a.saturate && (a.has_min || a.has_max);
  return m;
}

__device__ __forceinline__ void wave_minmax(float& lo, float& hi) {
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_down(lo, o, 64));
    hi = fmaxf(hi, __shfl_down(hi, o, 64));
  }
}
// all 256 threads call; every thread returns with the block's (lo, hi)
__device__ __forceinline__ void block_minmax(float& lo, float& hi) {
  __shared__ float slo[4], shi[4];
  wave_minmax(lo, hi);
  __syncthreads();                    // the arrays may still be read from a call before
  if ((threadIdx.x & 63) == 0) {
    slo[threadIdx.x >> 6] = lo;
    shi[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  lo = fminf(fminf(slo[0], slo[1]), fminf(slo[2], slo[3]));
  hi = fmaxf(fmaxf(shi[0], shi[1]), fmaxf(shi[2], shi[3]));
}

// Block (p, g) reduces slice p of group g (the pack, or image g of it: n elements each, contiguous in either layout)
// into part[g * P + p].  16-byte loads over the aligned middle of the slice, scalars at its ends (vec == 0: all scalar).
__global__ __launch_bounds__(256) void k_display_minmax(const float* __restrict__ x, int64_t n, int64_t slice, int vec,
                                                        float2* __restrict__ part) {
  const int64_t base = (int64_t)blockIdx.y * n;
  const int64_t s0 = (int64_t)blockIdx.x * slice, s1 = s0 + slice;
  const int64_t lo_i = base + (s0 < n ? s0 : n), hi_i = base + (s1 < n ? s1 : n);
  const int64_t up = (lo_i + 3) & ~(int64_t)3;
  const int64_t a0 = vec && up < hi_i ? up : hi_i;
  const int64_t a1 = a0 + ((hi_i - a0) & ~(int64_t)3);
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t i = lo_i + threadIdx.x; i < a0; i += 256) {
    const float v = x[i];
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  const float4* x4 = reinterpret_cast<const float4*>(x);
  for (int64_t i = (a0 >> 2) + threadIdx.x; i < (a1 >> 2); i += 256) {
    const float4 v = x4[i];
    lo = fminf(fminf(lo, v.x), fminf(v.y, fminf(v.z, v.w)));
    hi = fmaxf(fmaxf(hi, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
  }
  for (int64_t i = a1 + threadIdx.x; i < hi_i; i += 256) {
    const float v = x[i];
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  block_minmax(lo, hi);
  if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = make_float2(lo, hi);
}

struct DispLayout {
  const float* x;          // the pack: planar N x C x h x w, or (nhwc) N x h x w x C
  float* grid;             // C x (ch * ymaps) x (cw * xmaps)
  const float2* part;      // [groups][P]; NULL: no block needs the extremes
  int N, C, h, w, nhwc;
  int pad, xmaps, ymaps, P, scaleeach;
  DispNorm norm;
};
// blockIdx.y: the cell; blockIdx.x strides over the cell's C x ch x cw elements, cw fastest — stores run along grid rows,
// loads along image rows (planar) or at a stride of C floats inside one (nhwc)
__global__ __launch_bounds__(256) void k_display_layout(const DispLayout p) {
  const int k = blockIdx.y;
  const int ch = p.h + p.pad, cw = p.w + p.pad, half = p.pad >> 1;
  const int cy = k / p.xmaps, cx = k - cy * p.xmaps;
  const bool image = k < p.N;
  DispMap own = {0.f, 0.f, 0, 0, 0};
  float fill = 0.f;
  if (p.part) {
    if (!p.scaleeach) {
      float lo = INFINITY, hi = -INFINITY;
      if ((int)threadIdx.x < p.P) {
        const float2 v = p.part[threadIdx.x];
        lo = v.x;
        hi = v.y;
      }
      block_minmax(lo, hi);
      own = disp_map(p.norm, lo, hi);
      fill = own(hi);                                   // grid:fill(packed:max()), then minmax over the grid
    } else {
      if (image) {
        float lo = INFINITY, hi = -INFINITY;
        for (int j = 0; j < p.P; ++j) {
          const float2 v = p.part[(int64_t)k * p.P + j];
          lo = fminf(lo, v.x);
          hi = fmaxf(hi, v.y);
        }
        own = disp_map(p.norm, lo, hi);
      }
      if (!image || p.pad > 0) {
        // the maximum of the scaled pack: every image's map is monotone (rising, or falling for a negative divisor), so
        // its largest scaled value is the scaled minimum or the scaled maximum
        float best = -INFINITY, unused = INFINITY;
        for (int i = threadIdx.x; i < p.N; i += 256) {
          float lo = INFINITY, hi = -INFINITY;
          for (int j = 0; j < p.P; ++j) {
            const float2 v = p.part[(int64_t)i * p.P + j];
            lo = fminf(lo, v.x);
            hi = fmaxf(hi, v.y);
          }
          const DispMap m = disp_map(p.norm, lo, hi);
          best = fmaxf(best, fmaxf(m(lo), m(hi)));
        }
        block_minmax(unused, best);
        fill = best;
      }
    }
  } else {
    own = disp_map(p.norm, 0.f, 0.f);                   // both bounds given: the extremes are not used
  }
  const int GW = cw * p.xmaps;
  const int64_t GH = (int64_t)ch * p.ymaps;
  const int n = p.C * ch * cw;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int e = (int)i;
    const int xx = e % cw;
    const int t = e / cw;
    const int yy = t % ch, c = t / ch;
    const int iy = yy - half, ix = xx - half;
    float v = fill;
    if (image && iy >= 0 && iy < p.h && ix >= 0 && ix < p.w) {
      const int64_t src = p.nhwc ? (((int64_t)k * p.h + iy) * p.w + ix) * p.C + c : (((int64_t)k * p.C + c) * p.h + iy) * p.w + ix;
      v = own(p.x[src]);
    }
    p.grid[((int64_t)c * GH + (int64_t)cy * ch + yy) * GW + (int64_t)cx * cw + xx] = v;
  }
}

struct DispPlan {
  int xmaps, ymaps, groups, P;
  int64_t n, slice;        // elements per group, per reduction block
  bool reduce;
};
// Shapes are checked by the callers.  The extremes are not needed when both bounds are given, nothing is scaled per image
// and the grid has no cell or band that keeps the fill value (which is the pack's maximum).
DispPlan disp_plan(int N, int C, int h, int w, int padding, int nrow, int scaleeach, int has_min, int has_max) {
  DispPlan pl;
  pl.xmaps = std::min(nrow, N);
  pl.ymaps = (N + pl.xmaps - 1) / pl.xmaps;
  pl.groups = scaleeach ? N : 1;
  pl.n = (int64_t)C * h * w * (scaleeach ? 1 : N);
  pl.P = (int)std::max<int64_t>(1, std::min<int64_t>(vf_cdiv(pl.n, DISP_SLICE), scaleeach ? DISP_PMAX_EACH : DISP_PMAX));
  pl.slice = (vf_cdiv(pl.n, pl.P) + 3) & ~(int64_t)3;
  pl.reduce = scaleeach || !(has_min && has_max) || padding > 0 || pl.xmaps * pl.ymaps != N;
  return pl;
}

int disp_check(int N, int C, int h, int w, int padding, int nrow) {
  VF_REQUIRE(N > 0 && h > 0 && w > 0 && (C == 1 || C == 3),
             "vf_display_tensor: a packed %d x %d x %d x %d tensor; only N x C x h x w with C = 1 or 3 is laid out", N, C, h, w);
  VF_REQUIRE(padding >= 0 && padding % 2 == 0, "vf_display_tensor: padding=%d must be even and >= 0 (images sit at padding/2)", padding);
  VF_REQUIRE(nrow >= 1, "vf_display_tensor: nrow=%d", nrow);
  const int xmaps = std::min(nrow, N), ymaps = (N + xmaps - 1) / xmaps;
  VF_REQUIRE((int64_t)C * (h + padding) * ymaps * (int64_t)(w + padding) * xmaps < ((int64_t)1 << 31) && (int64_t)xmaps * ymaps <= 65535,
             "vf_display_tensor: a grid of %d x %d cells of %d x %d x %d is too large", ymaps, xmaps, C, h + padding, w + padding);
  return 0;
}

// test.lua:98-128.  Threads run over the planar outputs (x fastest): every store is coalesced, the NHWC loads are C floats apart.
__global__ __launch_bounds__(256) void k_center_finish(const float* __restrict__ ctx, const float* __restrict__ pred,
                                                       float* __restrict__ pretty, float* __restrict__ pasted,
                                                       float* __restrict__ predm, int B, int C, int fs, int ov) {
  const int64_t n = (int64_t)B * C * fs * fs;
  const int lo = fs / 4, hi = fs / 2 + fs / 4, hs = fs / 2;
  const int64_t img = (int64_t)C * fs * fs;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % fs);
    int64_t t = i / fs;
    const int y = (int)(t % fs);
    t /= fs;
    const int c = (int)(t % C);
    const int b = (int)(t / C);
    const float v = ctx[(((int64_t)b * fs + y) * fs + x) * C + c];
    const bool hole = y >= lo + ov && y < hi - ov && x >= lo + ov && x < hi - ov;
    float pv = v;
    if (y >= lo && y < hi && x >= lo && x < hi) {
      const float q = pred[(((int64_t)b * hs + (y - lo)) * hs + (x - lo)) * C + c];
      if (predm) predm[(((int64_t)b * C + c) * hs + (y - lo)) * hs + (x - lo)] = (q + 1.f) * 0.5f;
      if (hole) pv = q;
    }
    const int64_t r = i - (int64_t)b * img;             // (c, y, x) inside one image
    const float pm = (pv + 1.f) * 0.5f;                  // add(1):mul(0.5)
    pretty[(int64_t)(2 * b) * img + r] = hole ? 1.f : (v + 1.f) * 0.5f;
    pretty[(int64_t)(2 * b + 1) * img + r] = pm;
    if (pasted) pasted[i] = pm;
  }
}

}  // namespace

VF_API int vf_display_workspace_bytes(int N, int C, int h, int w, int padding, int nrow, int scaleeach, int has_min, int has_max,
                                      size_t* ws_bytes) {
  if (int e = disp_check(N, C, h, w, padding, nrow)) return e;
  const DispPlan pl = disp_plan(N, C, h, w, padding, nrow, scaleeach, has_min, has_max);
  *ws_bytes = pl.reduce ? (size_t)pl.groups * pl.P * sizeof(float2) : 0;
  return 0;
}

VF_API int vf_display_tensor(vf_ctx* ctx, const float* packed, int src_layout, float* grid, int N, int C, int h, int w,
                             int padding, int nrow, int scaleeach, int has_min, double min, int has_max, double max,
                             int symmetric, int saturate) {
  if (int e = disp_check(N, C, h, w, padding, nrow)) return e;
  VF_REQUIRE(src_layout == 0 || src_layout == 1, "vf_display_tensor: src_layout=%d (0 planar, 1 NHWC)", src_layout);
  const DispPlan pl = disp_plan(N, C, h, w, padding, nrow, scaleeach, has_min, has_max);
  const size_t need = pl.reduce ? (size_t)pl.groups * pl.P * sizeof(float2) : 0;
  VF_REQUIRE(vf_ws_avail(ctx) >= need, "vf_display_tensor: the workspace holds %zu bytes, the (min, max) partials need %zu",
             vf_ws_avail(ctx), need);
  float2* part = pl.reduce ? (float2*)vf_ws_ptr(ctx) : nullptr;
  const int64_t total = (int64_t)N * C * h * w;
  const int ch = h + padding, cw = w + padding;
  VfProf prof(ctx, "display_tensor", 0.0, 4.0 * ((pl.reduce ? 2.0 : 1.0) * (double)total + (double)C * ch * pl.ymaps * cw * pl.xmaps));
  if (pl.reduce) {
    hipLaunchKernelGGL(k_display_minmax, dim3(pl.P, pl.groups), dim3(256), 0, ctx->stream, packed, pl.n, pl.slice,
                       vf_aligned16(packed) ? 1 : 0, part);
    VF_LAUNCH_CHECK();
  }
  DispLayout p;
  p.x = packed; p.grid = grid; p.part = part;
  p.N = N; p.C = C; p.h = h; p.w = w; p.nhwc = src_layout;
  p.pad = padding; p.xmaps = pl.xmaps; p.ymaps = pl.ymaps; p.P = pl.P; p.scaleeach = scaleeach ? 1 : 0;
  p.norm.min = has_min ? min : 0.0; p.norm.max = has_max ? max : 0.0;
  p.norm.has_min = has_min ? 1 : 0; p.norm.has_max = has_max ? 1 : 0;
  p.norm.symmetric = symmetric ? 1 : 0; p.norm.saturate = saturate ? 1 : 0;
  const int gx = (int)std::max<int64_t>(1, std::min<int64_t>(vf_cdiv((int64_t)C * ch * cw, 1024), 65535));
  hipLaunchKernelGGL(k_display_layout, dim3(gx, pl.xmaps * pl.ymaps), dim3(256), 0, ctx->stream, p);
  VF_LAUNCH_CHECK();
  return 0;
}

VF_API int vf_center_finish(vf_ctx* ctx, const float* ctx_nhwc, const float* pred_nhwc, float* pretty, float* pasted,
                            float* pred_mapped, int B, int C, int fs, int overlapPred) {
  VF_REQUIRE(B > 0 && C > 0 && fs >= 4 && fs % 4 == 0, "vf_center_finish: bad shape B=%d C=%d fineSize=%d (fineSize %% 4 must be 0)", B, C, fs);
  VF_REQUIRE(overlapPred >= 0 && fs / 2 - 2 * overlapPred > 0, "vf_center_finish: overlapPred=%d leaves no hole in fineSize=%d",
             overlapPred, fs);
  const int64_t n = (int64_t)B * C * fs * fs;
  VfProf prof(ctx, "center_finish", 0.0, 4.0 * (double)n * (1.25 + 2.0 + (pasted ? 1.0 : 0.0) + (pred_mapped ? 0.25 : 0.0)));
  const int g = (int)std::max<int64_t>(1, std::min<int64_t>(vf_cdiv(n, 256), 1 << 20));
  hipLaunchKernelGGL(k_center_finish, dim3(g), dim3(256), 0, ctx->stream, ctx_nhwc, pred_nhwc, pretty, pasted, pred_mapped, B, C, fs,
                     overlapPred);
  VF_LAUNCH_CHECK();
  return 0;
}
