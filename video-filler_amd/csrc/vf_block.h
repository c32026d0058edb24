// vf_block.h — block-wide primitives shared by the device-side I/O stages (vf_image, vf_jpeg, vf_jpeg_enc, vf_png, vf_gif;
// DESIGN.md 5).
// vf_device.h stays the header of the MFMA and bf16-plane helpers; nothing on the training path includes this one.
#pragma once
#include <hip/hip_runtime.h>

// Exclusive prefix sum of one v per thread over a block of THREADS threads (a multiple of 64): an inclusive shuffle scan inside
// each wave, then the THREADS / 64 wave totals through s_w (room for that many T).  T is int, unsigned or unsigned long long:
// integer sums, so the result does not depend on the order.  Every thread of the block calls it.  It begins with a barrier —
// back-to-back calls may reuse s_w, and what the block wrote to LDS before the call is visible after it — and `total`, the sum
// over the block, is valid in every thread on return.
template <class T, int THREADS>
__device__ __forceinline__ T vf_block_excl_scan(T v, T* s_w, T& total) {
  static_assert(THREADS % 64 == 0 && THREADS >= 64 && THREADS <= 1024, "whole waves of one block");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T inc = v;
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  __syncthreads();
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  T base = 0;
  for (int w = 0; w < wave; ++w) base += s_w[w];
  total = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) total += s_w[w];
  return base + inc - v;
}

// Sum of one double per thread over a block of THREADS threads (a power of two) in a FIXED order: a tree through ssum (room for
// THREADS doubles) that adds element t + off to element t, off = THREADS / 2, ..., 1.  The same bits on every run; the order is
// pinned by tests/patch_array_ref.py and must not change.  Ends with a barrier: the sum is valid in every thread.
template <int THREADS>
__device__ __forceinline__ double vf_block_sum_f64(double v, double* ssum) {
  ssum[threadIdx.x] = v;
  __syncthreads();
  for (int off = THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) ssum[threadIdx.x] += ssum[threadIdx.x + off];
    __syncthreads();
  }
  return ssum[0];
}

// image.savePNG on a float tensor: saturate to [0,1], times 255 in float32, then libpng's C cast, which
// truncates; NaN -> 0 (fmaxf returns the operand that is a number)
__device__ __forceinline__ unsigned vf_savepng_byte(float x) {
  const float v = fminf(fmaxf(x, 0.f), 1.f);
  return (unsigned)(int)(255.f * v);
}
