// vf_device.h — device-side helpers shared by the kernels: vector types, buffer loads, the XCD-aware block order, the bf16
// rounding and the exact three-plane split, the per-tile BatchNorm partial sums.  Every producer and consumer of bf16 planes
// (BatchNorm apply / backward, vf_planes_split, the weight-planes kernels, the thin conv, the in-kernel mode-3 and BF = 1
// staging, the fused-Adam prep, the small-M kernels) calls the ONE split and the ONE rounding below: their bit-identity is by
// construction.
#pragma once
#include "vf_common.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x3 __attribute__((ext_vector_type(3)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// Buffer loads with hardware range checking: an offset past num_records returns 0, so padding taps, ragged
// tile edges and split-K tails need neither a branch nor a select — the loads stay in flight across the MFMAs.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t vf_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}
__device__ __forceinline__ f32x4 vf_bload4(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0));
}
// 12 bytes, dword-aligned: one whole 3-channel pixel (buffer_load_dwordx3); element 3 of the result is 0
__device__ __forceinline__ f32x4 vf_bload3(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
  const f32x3 v = __builtin_bit_cast(f32x3, __builtin_amdgcn_raw_buffer_load_b96(r, byte_off, 0, 0));
  const f32x4 o = {v[0], v[1], v[2], 0.f};
  return o;
}
__device__ __forceinline__ float vf_bload1(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 0));
}

// XCD-aware block order.  The dispatcher deals consecutive workgroup ids round-robin over the 8 XCDs (each with its
// own 4 MiB L2), so neighbouring tiles — which share input halos (k_igemm) or the whole gathered operand (k_wgrad's
// column tiles) — land on different L2s and every one of them fetches the shared rows from the fabric again
// (measured with FETCH_SIZE: 3-5x the algorithmic bytes).  This bijective remap gives each XCD one contiguous run of
// logical tile ids instead; it only ever changes speed, never results.
__device__ __forceinline__ int vf_xcd_remap(int h, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = h & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (h >> 3);
}

// The bf16-operand mode (vf_ctx_set_mfma_mode 1; BASELINE configs[4]'s "bf16"): ONE plane, the operand rounded to nearest-even,
// (u + 0x7FFF + lsb) >> 16 — 2 bytes per element instead of 6, one MFMA per product instead of six.  vf_rne16: the 16-bit
// pattern; vf_rne: that bf16 value as a float; vf_round4: four of them packed for one 8-byte store.
__device__ __forceinline__ unsigned vf_rne16(float v) {
  const unsigned u = __float_as_uint(v);
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ float vf_rne(float v) { return __uint_as_float(vf_rne16(v) << 16); }
__device__ __forceinline__ f32x4 vf_rne(f32x4 v) {
  f32x4 o = {vf_rne(v[0]), vf_rne(v[1]), vf_rne(v[2]), vf_rne(v[3])};
  return o;
}
__device__ __forceinline__ u32x2 vf_round4(f32x4 v) {
  u32x2 o;
  o[0] = vf_rne16(v[0]) | (vf_rne16(v[1]) << 16);
  o[1] = vf_rne16(v[2]) | (vf_rne16(v[3]) << 16);
  return o;
}

// Exact three-way split of fp32 values into bf16 planes by TRUNCATION (mode 3): plane q holds the top 16 bits of the
// running residual, the residual loses exactly those bits (v - float(top16(v)) is exact), and after two steps at most 8
// significant bits are left, so hi + mid + lo == v bit for bit.  vf_trunc16 is one step on one element: it returns the top
// 16 bits and leaves the residual in r.  vf_split3 does four elements at once and needs no conversion instruction: a
// v_perm_b32 packs the top halves of two residuals into one bf16x2 word (6 perms + 8 ands + 8 subs per four elements; the
// round-to-nearest form through v_cvt_pk_bf16_f32 cost 30).
__device__ __forceinline__ unsigned vf_trunc16(float& r) {
  const unsigned u = __float_as_uint(r);
  r -= __uint_as_float(u & 0xffff0000u);
  return u >> 16;
}
__device__ __forceinline__ void vf_split3(f32x4 v, u32x2 (&o)[3]) {
  float r0 = v[0], r1 = v[1], r2 = v[2], r3 = v[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const unsigned u0 = __float_as_uint(r0), u1 = __float_as_uint(r1), u2 = __float_as_uint(r2), u3 = __float_as_uint(r3);
    o[q][0] = __builtin_amdgcn_perm(u1, u0, 0x07060302u);      // (u1 & 0xffff0000) | (u0 >> 16)
    o[q][1] = __builtin_amdgcn_perm(u3, u2, 0x07060302u);
    if (q < 2) {
      r0 -= __uint_as_float(u0 & 0xffff0000u);
      r1 -= __uint_as_float(u1 & 0xffff0000u);
      r2 -= __uint_as_float(u2 & 0xffff0000u);
      r3 -= __uint_as_float(u3 & 0xffff0000u);
    }
  }
}

// Per-channel partial sums of one block's output tile -> one partial row (see VfBnSt).  Lane l of a wave holds column
// l % 32 of its 32-wide fragments and 16 rows per fragment: the per-lane sums over those rows are combined across the two
// lane halves with a shuffle, across the waves stacked in M through LDS in a fixed order (deterministic), and the block
// writes doubles.  `red` = 2 * WAVES_M * BN floats of LDS that nothing else uses any more.
template <int NT, int WAVES_M, int BN>
__device__ __forceinline__ void vf_bn_tile_partials(const VfBnSt& st, float (&s1)[NT], float (&s2)[NT], float* red, int wave_m,
                                                    int wn, int lane, int tid, int n0, int N, int bx, int pz) {
  const int lr = lane & 31;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    s1[nt] += __shfl_xor(s1[nt], 32, 64);
    s2[nt] += __shfl_xor(s2[nt], 32, 64);
    if (lane < 32) {
      red[(wave_m * 2 + 0) * BN + wn + nt * 32 + lr] = s1[nt];
      red[(wave_m * 2 + 1) * BN + wn + nt * 32 + lr] = s2[nt];
    }
  }
  __syncthreads();
  if (tid < BN && n0 + tid < N) {
    double a = 0, b = 0;
#pragma unroll
    for (int w = 0; w < WAVES_M; ++w) {
      a += (double)red[(w * 2 + 0) * BN + tid];
      b += (double)red[(w * 2 + 1) * BN + tid];
    }
    const int g = bx / st.tiles_per_group, local = bx - g * st.tiles_per_group;
    double* o = st.part + ((int64_t)(g * st.rows_per_group + local * st.zpar + pz) * 2) * N;
    o[n0 + tid] = a;
    o[N + n0 + tid] = b;
  }
}
