// vf_block.h — what the device-side I/O stages share on the device (vf_image, vf_jpeg, vf_jpeg_enc, vf_png, vf_png_decode, vf_gif,
// vf_metrics): the block-wide scan and fp64 sum, the file-offsets kernel of the encoders, image.savePNG's byte rule
// and the one reader of a batch of frames through it.
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

// One block of THREADS threads: offsets[f] = sum of the sizes before file f, f = 0 .. n (in: the sizes at [f + 1], as the stage's
// per-frame scan left them).  The last step of the PNG and JPEG encoders; vf_gif.hip's k_gif_offsets is this loop with every
// frame placed and a header term per file.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_vf_file_offsets(int64_t* offsets, int n) {
  __shared__ unsigned long long s_w[THREADS / 64];
  if (threadIdx.x == 0) offsets[0] = 0;
  unsigned long long run = 0;
  for (int base = 0; base < n; base += THREADS) {
    const int f = base + threadIdx.x;
    const unsigned long long v = f < n ? (unsigned long long)offsets[f + 1] : 0ull;
    unsigned long long total;
    const unsigned long long e = vf_block_excl_scan<unsigned long long, THREADS>(v, s_w, total);
    if (f < n) offsets[f + 1] = (int64_t)(run + e + v);
    run += total;
  }
}
template <int THREADS = 256>   // a template too: only the stages that call it hold the kernel
static inline void vf_launch_file_offsets(hipStream_t stream, int64_t* offsets, int n) {
  hipLaunchKernelGGL(k_vf_file_offsets<THREADS>, dim3(1), dim3(THREADS), 0, stream, offsets, n);
}

// image.savePNG on a float tensor: saturate to [0,1], times 255 in float32, then libpng's C cast, which
// truncates; NaN -> 0 (fmaxf returns the operand that is a number)
__device__ __forceinline__ unsigned vf_savepng_byte(float x) {
  const float v = fminf(fmaxf(x, 0.f), 1.f);
  return (unsigned)(int)(255.f * v);
}

// A batch of frames as the encoders and the scores take it, and byte (frame f, channel c, row y, column x) of it: float planar
// N x C x H x W through vf_savepng_byte (KIND 0), or uint8 interleaved N x H x W x C as it is (KIND 1).  64-bit arithmetic: f is.
struct VfFrames {
  const void* src;
  int H, W, C;
};
template <int KIND>
__device__ __forceinline__ unsigned vf_frame_byte(const VfFrames& fr, long long f, int c, int y, int x) {
  if constexpr (KIND == 1) return ((const unsigned char*)fr.src)[((f * fr.H + y) * fr.W + x) * fr.C + c];
  else return vf_savepng_byte(((const float*)fr.src)[((f * fr.C + c) * fr.H + y) * fr.W + x]);
}
