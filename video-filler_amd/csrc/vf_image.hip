// vf_image.hip — Torch7's image.scale (bilinear mode) and the loaders built on it, on the device:
//   * vf_image_scale / vf_image_scale_u8: image.scale of N frames of one size (Float result; Byte -> Byte for masks);
//   * vf_image_hook2d: data/donkey_folder.lua:40-88 for ONE decoded image — resize, crop at (w1, h1), hflip, [0,1] -> [-1,1]
//     into one row of the loader batch, evaluating only the crop's pixels;
//   * vf_image_whole_frames: test_vid_wholeim.lua:109-141 — resize, maskedFill, pad bottom-right, [0,1] -> [-1,1];
//   * vf_crop_stats: the dark-crop mean and the mask test of datavid/donkey_folder.lua:148-165 as one device pair;
//   * vf_patch_array_prepare: datavid/donkey_wholeim.lua:141-215 for ONE decoded frame — resize, maskedFill, shift, hflip, the
//     arr_h x arr_w window array and its four output windows, [0,1] -> [-1,1], into one row of the three channels-last batch
//     tensors, with the dark test's sum.
// One fused kernel: every output pixel recomputes the few row-pass values (`tmp` of scaleBilinear) its column pass
// reads, so the scaled image is never materialised.  The arithmetic is the restatement's float32, one rounding per
// operation in its order (the library builds with -ffp-contract=off; IEEE division): results are bit-identical to
// tests/image_ref.py.  Threads run along the output row, so stores are coalesced; the sources stay in L2.
#include "vf_block.h"
#include "vf_common.h"

namespace {

inline int igrid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(vf_cdiv(n, 256), 1 << 20)); }

enum { SRC_F32_CHW = 0, SRC_U8_HWC = 1, SRC_U8_CHW = 2 };   // SRC_U8_CHW: the Byte path (Byte tmp, Byte result)

// image.c FromIntermediate: identity for Float; for Byte x += 0.5, clamp to [0, 255], truncate
template <bool BYTE>
__device__ __forceinline__ float vf_fi(float x) {
  if (!BYTE) return x;
  x = x + 0.5f;
  if (x <= 0.f) return 0.f;
  if (x >= 255.f) return 255.f;
  return (float)(int)x;
}

// scaleLinear_rowcol evaluated at ONE destination index k of a line of S source values -> D values.  get(i) is the
// source value at i.  The downscale branch carries (i0, f0) from one destination index to the next in the reference;
// they are recomputed here from k with the same operations (f32(k) * scale), so every k is independent.  The min()
// clamps never fire for the sizes the entry points accept (< 2^16): they only keep every read inside the line.
template <bool BYTE, class Get>
__device__ __forceinline__ float vf_rowcol_at(int k, int S, int D, Get get) {
  if (D > S) {
    if (k == D - 1) return get(S - 1);
    if (S == 1) return get(0);
    const float scale = (float)(S - 1) / (float)(D - 1);
    float f = (float)k * scale;
    const int i = min((int)f, S - 1);
    f = f - (float)i;
    return vf_fi<BYTE>((1.f - f) * get(i) + f * get(min(i + 1, S - 1)));
  }
  if (D < S) {
    const float scale = (float)S / (float)D;
    float f0 = (float)k * scale;
    const int i0 = min((int)f0, S - 1);
    f0 = f0 - (float)i0;
    float f1 = (float)(k + 1) * scale;
    const int i1 = (int)f1;
    f1 = f1 - (float)i1;
    float acc = (1.f - f0) * get(i0);
    float n = 1.f - f0;
    const int tend = min(i1, S);
    for (int t = i0 + 1; t < tend; ++t) {
      acc = acc + get(t);
      n = n + 1.f;
    }
    if (i1 < S) {
      acc = acc + f1 * get(i1);
      n = n + f1;
    }
    return vf_fi<BYTE>(acc / n);
  }
  return get(k);
}

// Output element (n, c, y, x) of an N x C x OH x OW planar tensor is pixel (y0 + y, x0 + x') of channel c of the
// scaled frame n (x' = OW-1-x when flipped); outside the h x w scaled frame it is 0 (padding).  fill_mask (C x h x w
// Byte, shared by the frames) replaces masked pixels by fill_value; affine maps v -> v * mul + add afterwards.
struct ScalePlace {
  const void* src;
  void* dst;
  const unsigned char* fill_mask;
  int N, C, H, W, h, w, OH, OW, y0, x0, flip, affine;
  float fill_value, mul, add;
};

template <int SRC>
__global__ void k_scale_place(const ScalePlace p) {
  constexpr bool BYTE = SRC == SRC_U8_CHW;
  const int64_t total = (int64_t)p.N * p.C * p.OH * p.OW;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(idx % p.OW);
    int64_t t = idx / p.OW;
    const int y = (int)(t % p.OH);
    t /= p.OH;
    const int c = (int)(t % p.C);
    const int n = (int)(t / p.C);
    const int sy = p.y0 + y, sx = p.x0 + (p.flip ? p.OW - 1 - x : x);
    float v = 0.f;
    if (sy < p.h && sx < p.w) {
      auto load = [&](int j, int i) -> float {
        if (SRC == SRC_F32_CHW) return ((const float*)p.src)[(((int64_t)n * p.C + c) * p.H + j) * p.W + i];
        if (SRC == SRC_U8_HWC)          // image.load(path, nc, 'float'): b / 255 in float
          return (float)((const unsigned char*)p.src)[(((int64_t)n * p.H + j) * p.W + i) * p.C + c] / 255.f;
        return (float)((const unsigned char*)p.src)[(((int64_t)n * p.C + c) * p.H + j) * p.W + i];
      };
      // rows first (width W -> w), then columns (height H -> h), as scaleBilinear does
      v = vf_rowcol_at<BYTE>(sy, p.H, p.h, [&](int j) { return vf_rowcol_at<BYTE>(sx, p.W, p.w, [&](int i) { return load(j, i); }); });
      if (p.fill_mask && p.fill_mask[((int64_t)c * p.h + sy) * p.w + sx]) v = p.fill_value;
    }
    if (p.affine) {
      v = v * p.mul;
      v = v + p.add;
    }
    if (BYTE) ((unsigned char*)p.dst)[idx] = (unsigned char)v;
    else ((float*)p.dst)[idx] = v;
  }
}

int launch_scale_place(vf_ctx* ctx, int layout, const ScalePlace& p, const char* name) {
  const int64_t n = (int64_t)p.N * p.C * p.OH * p.OW;
  VfProf prof(ctx, name, 0.0, (layout == SRC_F32_CHW ? 4.0 : 1.0) * (double)p.N * p.C * p.H * p.W + (layout == SRC_U8_CHW ? 1.0 : 4.0) * (double)n);
  if (layout == SRC_F32_CHW) hipLaunchKernelGGL(k_scale_place<SRC_F32_CHW>, dim3(igrid(n)), dim3(256), 0, ctx->stream, p);
  else if (layout == SRC_U8_HWC) hipLaunchKernelGGL(k_scale_place<SRC_U8_HWC>, dim3(igrid(n)), dim3(256), 0, ctx->stream, p);
  else hipLaunchKernelGGL(k_scale_place<SRC_U8_CHW>, dim3(igrid(n)), dim3(256), 0, ctx->stream, p);
  VF_LAUNCH_CHECK();
  return 0;
}

constexpr int kMaxSide = 1 << 16;

int scale_check(const char* fn, int N, int C, int H, int W, int height, int width) {
  VF_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && height > 0 && width > 0 && H < kMaxSide && W < kMaxSide && height < kMaxSide &&
                 width < kMaxSide,
             "%s: N=%d C=%d %dx%d -> %dx%d (sides must lie in [1, 65535])", fn, N, C, H, W, height, width);
  return 0;
}

ScalePlace plain(const void* src, void* dst, int N, int C, int H, int W, int height, int width) {
  ScalePlace p;
  p.src = src; p.dst = dst; p.fill_mask = nullptr;
  p.N = N; p.C = C; p.H = H; p.W = W; p.h = height; p.w = width; p.OH = height; p.OW = width;
  p.y0 = 0; p.x0 = 0; p.flip = 0; p.affine = 0;
  p.fill_value = 0.f; p.mul = 1.f; p.add = 0.f;
  return p;
}

// datavid/donkey_folder.lua:148,165: sum (double, as TH's meanall accumulates) of the C x fs x fs crop of the planar clip
// and the max of the same crop of the Byte mask (iH x iW, or NULL).  One block, fixed reduction order: deterministic.
__global__ void __launch_bounds__(256) k_crop_stats(const float* __restrict__ clip, const unsigned char* __restrict__ mask, int C, int iH,
                                                    int iW, int fs, int w1, int h1, double* __restrict__ out) {
  __shared__ double ssum[256];
  __shared__ int smax;
  if (threadIdx.x == 0) smax = 0;
  __syncthreads();
  double s = 0.0;
  int m = 0;
  const int64_t n = (int64_t)C * fs * fs;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
    const int x = (int)(i % fs);
    const int64_t t = i / fs;
    const int y = (int)(t % fs), c = (int)(t / fs);
    s += (double)clip[((int64_t)c * iH + h1 + y) * iW + w1 + x];
    if (mask && c == 0) m = max(m, (int)mask[(int64_t)(h1 + y) * iW + w1 + x]);
  }
  atomicMax(&smax, m);                        // a max does not depend on the order; the sum's barriers stand behind it
  const double total = vf_block_sum_f64<256>(s, ssum);
  if (threadIdx.x == 0) {
    out[0] = total;
    out[1] = (double)smax;
  }
}

// datavid/donkey_wholeim.lua:141-215 (trainHook of train_wholeim_input.lua's loader) for ONE frame, after its loadImage: the
// frame scaled to h x w is shifted up-left by (crop_h-1, crop_w-1) with ZERO bands bottom and right (the masked copy and the
// mask too), mirrored over the full width if flip, and cut into arr_h x arr_w windows of fs x fs, steph / stepw apart.
struct PatchArray {
  const void* src;
  const unsigned char* mask;   // h x w Byte, or NULL
  float *masked, *full, *maskout;
  double* part;                // [fs] row partials of the top-left window's sum
  int H, W, h, w, fs, arr_h, arr_w, steph, stepw, dy, dx, flip;   // dy = crop_h-1, dx = crop_w-1
  float mask_value;
};

// Block y writes output row y of every window.  Item i = x * P + p (P windows, p fastest): the three channels of pixel (y, x)
// of window p, so neighbouring threads store neighbouring 12-byte pieces of the fs x fs x 3P record array, and the (at most) four
// threads of a pixel that own an output window store its 48-byte records of `full` and `maskout`.  The scaled pixel is evaluated
// once per window.  Window 0 of the unmasked input, before the [-1,1] map, is the dark test's patch (:188-189): its sum is
// accumulated in double, per thread in item order, then over the block by vf_block_sum_f64 — the same bits on every run.
template <int SRC>
__global__ void __launch_bounds__(256) k_patch_array(const PatchArray p) {
  __shared__ double ssum[256];
  const int y = blockIdx.x, P = p.arr_h * p.arr_w, C3 = 3 * P;
  double s = 0.0;
  for (int i = threadIdx.x; i < p.fs * P; i += 256) {
    const int x = i / P, win = i - x * P;
    const int ih = win / p.arr_w, iw = win - ih * p.arr_w;
    const int X = iw * p.stepw + x;
    const int sy = ih * p.steph + y + p.dy, sx = (p.flip ? p.w - 1 - X : X) + p.dx;
    const bool in = sy < p.h && sx < p.w;
    const bool m = in && p.mask && p.mask[(int64_t)sy * p.w + sx];
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      v[c] = 0.f;
      if (in) {
        auto load = [&](int j, int k) -> float {
          if (SRC == SRC_F32_CHW) return ((const float*)p.src)[((int64_t)c * p.H + j) * p.W + k];
          return (float)((const unsigned char*)p.src)[((int64_t)j * p.W + k) * 3 + c] / 255.f;
        };
        v[c] = vf_rowcol_at<false>(sy, p.H, p.h, [&](int j) { return vf_rowcol_at<false>(sx, p.W, p.w, [&](int k) { return load(j, k); }); });
      }
    }
    if (win == 0) {
      s += (double)v[0];
      s += (double)v[1];
      s += (double)v[2];
    }
    const int64_t pix = (int64_t)y * p.fs + x;
    float* mo = p.masked + pix * C3 + 3 * win;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float t = (m ? p.mask_value : v[c]) * 2.f;
      mo[c] = t + -1.f;
    }
    if (ih <= 1 && iw <= 1) {                  // h1 = ih, w1 = iw for steps >= 2 (:201-203)
      const int64_t o = pix * 12 + 3 * (2 * ih + iw);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float t = v[c] * 2.f;
        p.full[o + c] = t + -1.f;
        p.maskout[o + c] = m ? 1.f : 0.f;
      }
    }
  }
  const double total = vf_block_sum_f64<256>(s, ssum);
  if (threadIdx.x == 0) p.part[y] = total;
}

// the n row partials of k_patch_array into out[0]: one block, fixed order
__global__ void __launch_bounds__(256) k_sum_partials(const double* __restrict__ part, int n, double* __restrict__ out) {
  __shared__ double ssum[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += part[i];
  const double total = vf_block_sum_f64<256>(s, ssum);
  if (threadIdx.x == 0) out[0] = total;
}

}  // namespace

VF_API int vf_image_scale(vf_ctx* ctx, const void* src, int src_layout, float* dst, int N, int C, int H, int W, int height,
                          int width) {
  if (int e = scale_check("vf_image_scale", N, C, H, W, height, width)) return e;
  VF_REQUIRE(src_layout == SRC_F32_CHW || src_layout == SRC_U8_HWC, "vf_image_scale: src_layout %d is not 0 (float CHW) or 1 (uint8 HWC)",
             src_layout);
  return launch_scale_place(ctx, src_layout, plain(src, dst, N, C, H, W, height, width), "image_scale");
}

VF_API int vf_image_scale_u8(vf_ctx* ctx, const unsigned char* src, unsigned char* dst, int N, int C, int H, int W, int height,
                             int width) {
  if (int e = scale_check("vf_image_scale_u8", N, C, H, W, height, width)) return e;
  return launch_scale_place(ctx, SRC_U8_CHW, plain(src, dst, N, C, H, W, height, width), "image_scale_u8");
}

VF_API int vf_image_hook2d(vf_ctx* ctx, const void* src, int src_layout, float* out, int C, int H, int W, int height, int width,
                           int fs, int w1, int h1, int flip) {
  if (int e = scale_check("vf_image_hook2d", 1, C, H, W, height, width)) return e;
  VF_REQUIRE(src_layout == SRC_F32_CHW || src_layout == SRC_U8_HWC, "vf_image_hook2d: src_layout %d is not 0 (float CHW) or 1 (uint8 HWC)",
             src_layout);
  VF_REQUIRE(fs > 0 && w1 >= 0 && h1 >= 0 && w1 + fs <= width && h1 + fs <= height,
             "vf_image_hook2d: crop (%d,%d)+%d outside the %dx%d scaled image", w1, h1, fs, width, height);
  ScalePlace p = plain(src, out, 1, C, H, W, height, width);
  p.OH = fs; p.OW = fs; p.y0 = h1; p.x0 = w1; p.flip = flip ? 1 : 0;
  p.affine = 1; p.mul = 2.f; p.add = -1.f;
  return launch_scale_place(ctx, src_layout, p, "image_hook2d");
}

VF_API int vf_image_whole_frames(vf_ctx* ctx, const void* src, int src_layout, float* out, int N, int C, int H, int W, int height,
                                 int width, int outh, int outw, const unsigned char* fill_mask, float fill_value) {
  if (int e = scale_check("vf_image_whole_frames", N, C, H, W, height, width)) return e;
  VF_REQUIRE(src_layout == SRC_F32_CHW || src_layout == SRC_U8_HWC,
             "vf_image_whole_frames: src_layout %d is not 0 (float CHW) or 1 (uint8 HWC)", src_layout);
  VF_REQUIRE(outh >= height && outw >= width && outh < kMaxSide && outw < kMaxSide,
             "vf_image_whole_frames: the %dx%d padded frame does not hold the %dx%d scaled one", outh, outw, height, width);
  ScalePlace p = plain(src, out, N, C, H, W, height, width);
  p.OH = outh; p.OW = outw; p.fill_mask = fill_mask; p.fill_value = fill_value;
  p.affine = 1; p.mul = 2.f; p.add = -1.f;
  return launch_scale_place(ctx, src_layout, p, "image_whole_frames");
}

VF_API int vf_crop_stats(vf_ctx* ctx, const float* clip, const unsigned char* mask, int C, int iH, int iW, int fs, int w1, int h1,
                         double* out) {
  VF_REQUIRE(C > 0 && fs > 0 && w1 >= 0 && h1 >= 0 && w1 + fs <= iW && h1 + fs <= iH,
             "vf_crop_stats: crop (%d,%d)+%d outside the %dx%d clip", w1, h1, fs, iW, iH);
  VfProf prof(ctx, "crop_stats", 0.0, 4.0 * (double)C * fs * fs);
  hipLaunchKernelGGL(k_crop_stats, dim3(1), dim3(256), 0, ctx->stream, clip, mask, C, iH, iW, fs, w1, h1, out);
  VF_LAUNCH_CHECK();
  return 0;
}

VF_API int vf_patch_array_prepare(vf_ctx* ctx, const void* src, int src_layout, const unsigned char* mask, float* masked, float* full,
                                  float* maskout, double* sum, int H, int W, int height, int width, int fs, int arr_h, int arr_w,
                                  int crop_w, int crop_h, int flip, float mask_value) {
  if (int e = scale_check("vf_patch_array_prepare", 1, 3, H, W, height, width)) return e;
  VF_REQUIRE(src_layout == SRC_F32_CHW || src_layout == SRC_U8_HWC,
             "vf_patch_array_prepare: src_layout %d is not 0 (float CHW) or 1 (uint8 HWC)", src_layout);
  VF_REQUIRE(fs > 0 && arr_h >= 2 && arr_w >= 2 && arr_h <= 64 && arr_w <= 64,
             "vf_patch_array_prepare: fineSize %d, a %dx%d patch array (needs fineSize > 0 and 2 to 64 windows a side)", fs, arr_h, arr_w);
  const int steph = height >= fs ? (height - fs) / (arr_h - 1) : 0, stepw = width >= fs ? (width - fs) / (arr_w - 1) : 0;
  VF_REQUIRE(steph >= 2 && stepw >= 2,
             "vf_patch_array_prepare: the %dx%d scaled frame and a %dx%d array of %d-pixel windows give steps %d and %d (both must be "
             ">= 2)", height, width, arr_h, arr_w, fs, steph, stepw);
  VF_REQUIRE((height - fs) / steph + 1 == arr_h && (width - fs) / stepw + 1 == arr_w,
             "vf_patch_array_prepare: steps %d and %d over the %dx%d scaled frame visit %dx%d windows of %d pixels, not the %dx%d of the "
             "array", steph, stepw, height, width, (height - fs) / steph + 1, (width - fs) / stepw + 1, fs, arr_h, arr_w);
  VF_REQUIRE(crop_h >= 1 && crop_w >= 1 && crop_h <= height && crop_w <= width,
             "vf_patch_array_prepare: crop (%d,%d) outside the %dx%d scaled frame (1-based, at most the frame's sides)", crop_w, crop_h,
             height, width);
  VF_REQUIRE(vf_ws_avail(ctx) >= (size_t)fs * sizeof(double), "vf_patch_array_prepare: the workspace holds %zu bytes, the row partials need %zu",
             vf_ws_avail(ctx), (size_t)fs * sizeof(double));
  PatchArray p;
  p.src = src; p.mask = mask; p.masked = masked; p.full = full; p.maskout = maskout;
  p.part = (double*)vf_ws_ptr(ctx);
  p.H = H; p.W = W; p.h = height; p.w = width; p.fs = fs; p.arr_h = arr_h; p.arr_w = arr_w; p.steph = steph; p.stepw = stepw;
  p.dy = crop_h - 1; p.dx = crop_w - 1; p.flip = flip ? 1 : 0; p.mask_value = mask_value;
  VfProf prof(ctx, "patch_array_prepare", 0.0,
              (src_layout == SRC_F32_CHW ? 12.0 : 3.0) * (double)H * W + (double)height * width + 4.0 * (double)fs * fs * (3 * arr_h * arr_w + 24));
  if (src_layout == SRC_F32_CHW) hipLaunchKernelGGL(k_patch_array<SRC_F32_CHW>, dim3(fs), dim3(256), 0, ctx->stream, p);
  else hipLaunchKernelGGL(k_patch_array<SRC_U8_HWC>, dim3(fs), dim3(256), 0, ctx->stream, p);
  VF_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, ctx->stream, (const double*)p.part, fs, sum);
  VF_LAUNCH_CHECK();
  return 0;
}
