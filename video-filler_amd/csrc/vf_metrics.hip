// vf_metrics.hip — scores of a batch of result frames against the truth: per frame and region (every valid
// pixel; the valid pixels under the hole mask) the integer sums behind PSNR, mean absolute error, SSIM (uniform 7 x 7,
// scikit-image's default form) and the flicker between consecutive frames, on the BYTES save_frames would write.
// Every column of the table is an integer sum, so the order of the additions does not matter: blocks add their partial
// sums with 64-bit atomics, and the table equals tests/metrics_ref.py exactly on every run.
// One launch.  Block (tx, ty, n) owns the MT x MT pixels at (ty * MT, tx * MT) of frame n: they are the pixels it counts and
// the window centres it scores, so every pixel and every window is counted once.  Per channel:
//   load    the tile with a halo of 3 of a and of b into LDS as bytes (the byte rule applied on the way; 0 outside the valid
//           rectangle, which no counted window reaches and which is never read from memory);
//   rows    thread (row r, run of 8 columns) forms the five 7-sums Sx, Sy, Sxx, Syy, Sxy of its 8 windows from 16 bytes of
//           each image, 8 packed uint4 out.  Each sum is two byte dot products (4 + 3 bytes), written as such: the first
//           form, running sums that add the entering product and subtract the leaving one, came out of the compiler's own
//           byte-dot matching with the leaving byte added instead of subtracted — right on the host, wrong on the device
//           wherever a non-zero byte left a window;
//   columns thread (column, run of 4 rows) slides the 7-row sums down its run (10 uint4 in), scores its 4 windows and
//           counts its 4 pixels; the flicker term loads the same pixels of frame n - 1 from memory (no block waits for
//           another).
// The counters stay in registers across the channels, are summed over the block by wave shuffles and four LDS slots, and
// the non-zero ones go to the frame's row of the table.
#include "vf_block.h"
#include "vf_common.h"

namespace {

constexpr int MT = 32;                // tile side (tests/test_gpu_metrics.py: TILE)
constexpr int MHALO = MT + 6;         // 38: the tile with 3 pixels on every side
constexpr int MPITCH = 44;            // bytes per LDS row of a byte tile: 11 dwords (odd), so the rows of one column lie on
                                      // different banks when the rows pass reads them with lanes along r
constexpr int MRS = MT + 1;           // uint4 per LDS row of row sums: lanes along r are then 33 * 16 B apart, 16 B mod 128
constexpr int MROW_THREADS = MHALO * (MT / 8);   // 152 threads of the rows pass

struct MetArgs {
  const void* a;
  const void* b;
  const unsigned char* mask;
  unsigned long long* table;          // [N][2][VF_METRICS_COLS]
  int N, C, H, W, vh, vw, clip;
};

// One window from its integer sums (n = 49).  10^4 C1 = 65025 and 10^4 C2 = 585225: the four factors are exact integers below
// 2^53, so their conversions are exact; two IEEE divisions, one multiplication (the library is built with -ffp-contract=off and
// without fast-math: nothing is fused or taken through a reciprocal), times 2^30 (exact), to nearest-even.
__device__ __forceinline__ long long met_ssim_q(int Sx, int Sy, int Sxx, int Syy, int Sxy) {
  const long long pxy = (long long)Sx * Sy, sx2 = (long long)Sx * Sx, sy2 = (long long)Sy * Sy;
  const long long vx = 49LL * Sxx - sx2, vy = 49LL * Syy - sy2, cxy = 49LL * Sxy - pxy;
  const long long N1 = 20000LL * pxy + 2401LL * 65025, D1 = 10000LL * (sx2 + sy2) + 2401LL * 65025;
  const long long N2 = 20000LL * cxy + 2352LL * 585225, D2 = 10000LL * (vx + vy) + 2352LL * 585225;
  const double s = ((double)N1 / (double)D1) * ((double)N2 / (double)D2);
  return llrint(s * 1073741824.0);
}

// the 4 bytes from byte k (0 .. 12) of 16 bytes held as 4 dwords, little-endian; k is a constant where this is called
__device__ __forceinline__ unsigned met_dw(const unsigned (&w)[4], int k) {
  const int d = k >> 2, sh = (k & 3) * 8;
  return sh ? (w[d] >> sh) | (w[d + 1] << (32 - sh)) : w[d];
}
// sum of the four byte products of a and b, plus c (v_dot4_u32_u8)
__device__ __forceinline__ unsigned met_dot(unsigned a, unsigned b, unsigned c) { return __builtin_amdgcn_udot4(a, b, c, false); }

template <int KIND>
__global__ __launch_bounds__(256) void k_frame_metrics(const MetArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char s_a[MHALO * MPITCH];
  __shared__ __attribute__((aligned(16))) unsigned char s_b[MHALO * MPITCH];
  __shared__ uint4 s_row[MHALO * MRS];
  __shared__ long long s_red[4][2 * VF_METRICS_COLS];
  const int t = threadIdx.x;
  const int n = blockIdx.z;
  const int y0 = blockIdx.y * MT, x0 = blockIdx.x * MT;
  // the columns pass: this thread's 4 pixels / window centres are (y0 + py + i, x0 + px), i < 4
  const int px = t & (MT - 1), py = (t >> 5) * 4;
  const int gx = x0 + px;
  const bool flick = p.clip && n > 0;
  const VfFrames fa{p.a, p.H, p.W, p.C}, fb{p.b, p.H, p.W, p.C};
  unsigned hole = 0;                  // bit i: pixel i is valid and under the mask
  if (p.mask && gx < p.vw)
    for (int i = 0; i < 4; ++i)
      if (y0 + py + i < p.vh && p.mask[(int64_t)(y0 + py + i) * p.W + gx]) hole |= 1u << i;
  // [region][n, sse, sae, ssim_n, flicker]: a thread adds at most 4 * 3 values below 2^16 to each
  unsigned cnt[2][5] = {};
  long long q[2] = {0, 0};
  for (int c = 0; c < p.C; ++c) {
    __syncthreads();                  // the passes of the channel before are done with the tiles
    for (int i = t; i < MHALO * MHALO; i += 256) {
      const int r = i / MHALO, col = i - r * MHALO;
      const int y = y0 - 3 + r, x = x0 - 3 + col;
      unsigned va = 0, vb = 0;
      if (y >= 0 && y < p.vh && x >= 0 && x < p.vw) {
        va = vf_frame_byte<KIND>(fa, n, c, y, x);
        vb = vf_frame_byte<KIND>(fb, n, c, y, x);
      }
      s_a[r * MPITCH + col] = (unsigned char)va;
      s_b[r * MPITCH + col] = (unsigned char)vb;
    }
    __syncthreads();
    if (t < MROW_THREADS) {
      const int r = t % MHALO, seg = t / MHALO;
      unsigned wa[4], wb[4];
      const unsigned* ra = reinterpret_cast<const unsigned*>(s_a + r * MPITCH + seg * 8);
      const unsigned* rb = reinterpret_cast<const unsigned*>(s_b + r * MPITCH + seg * 8);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        wa[k] = ra[k];
        wb[k] = rb[k];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        // the window's 7 bytes as 4 + 3; every sum is formed afresh (see the header: no running sums of products here)
        const unsigned a0 = met_dw(wa, j), a1 = met_dw(wa, j + 4) & 0xffffffu;
        const unsigned b0 = met_dw(wb, j), b1 = met_dw(wb, j + 4) & 0xffffffu;
        const unsigned sx = met_dot(a0, 0x01010101u, met_dot(a1, 0x01010101u, 0)), sy = met_dot(b0, 0x01010101u, met_dot(b1, 0x01010101u, 0));
        s_row[r * MRS + seg * 8 + j] = make_uint4(sx | (sy << 16), met_dot(a0, a0, met_dot(a1, a1, 0)), met_dot(b0, b0, met_dot(b1, b1, 0)),
                                                  met_dot(a0, b0, met_dot(a1, b1, 0)));                          // Sx, Sy <= 7 * 255
      }
    }
    __syncthreads();
    int Sx = 0, Sy = 0, Sxx = 0, Syy = 0, Sxy = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const uint4 v = s_row[(py + k) * MRS + px];
      Sx += v.x & 0xffff; Sy += v.x >> 16; Sxx += v.y; Syy += v.z; Sxy += v.w;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint4 v = s_row[(py + i + 6) * MRS + px];
      Sx += v.x & 0xffff; Sy += v.x >> 16; Sxx += v.y; Syy += v.z; Sxy += v.w;
      const int gy = y0 + py + i;
      const bool in_hole = (hole >> i) & 1u;
      if (gy >= 3 && gy + 3 < p.vh && gx >= 3 && gx + 3 < p.vw) {                         // the window lies in the valid rectangle
        const long long s = met_ssim_q(Sx, Sy, Sxx, Syy, Sxy);
        q[0] += s;
        cnt[0][3] += 1;
        if (in_hole) {
          q[1] += s;
          cnt[1][3] += 1;
        }
      }
      if (gy < p.vh && gx < p.vw) {
        const int a = s_a[(py + i + 3) * MPITCH + px + 3], b = s_b[(py + i + 3) * MPITCH + px + 3];
        const int d = a - b;
        const unsigned ad = (unsigned)(d < 0 ? -d : d);
        unsigned fl = 0;
        if (flick) {
          const int e = d - ((int)vf_frame_byte<KIND>(fa, n - 1, c, gy, gx) - (int)vf_frame_byte<KIND>(fb, n - 1, c, gy, gx));
          fl = (unsigned)(e < 0 ? -e : e);
        }
        for (int reg = 0; reg < (in_hole ? 2 : 1); ++reg) {
          cnt[reg][0] += 1;
          cnt[reg][1] += (unsigned)(d * d);
          cnt[reg][2] += ad;
          cnt[reg][4] += fl;
        }
      }
      const uint4 u = s_row[(py + i) * MRS + px];
      Sx -= u.x & 0xffff; Sy -= u.x >> 16; Sxx -= u.y; Syy -= u.z; Sxy -= u.w;
    }
  }
  // the block's sums: a wave's 32-bit counters stay below 64 * 12 * 65025 < 2^26
  const int lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int reg = 0; reg < 2; ++reg) {
#pragma unroll
    for (int k = 0; k < 5; ++k)
      for (int o = 32; o > 0; o >>= 1) cnt[reg][k] += __shfl_down(cnt[reg][k], o, 64);
    for (int o = 32; o > 0; o >>= 1) q[reg] += __shfl_down(q[reg], o, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int reg = 0; reg < 2; ++reg) {
      long long* d = s_red[wave] + reg * VF_METRICS_COLS;
      d[VF_METRICS_N] = cnt[reg][0];
      d[VF_METRICS_SSE] = cnt[reg][1];
      d[VF_METRICS_SAE] = cnt[reg][2];
      d[VF_METRICS_SSIM_Q] = q[reg];
      d[VF_METRICS_SSIM_N] = cnt[reg][3];
      d[VF_METRICS_FLICKER] = cnt[reg][4];
    }
  }
  __syncthreads();
  if (t < 2 * VF_METRICS_COLS) {
    const long long v = s_red[0][t] + s_red[1][t] + s_red[2][t] + s_red[3][t];
    // two's complement: the unsigned add is the signed one (SSIM_Q may be negative)
    if (v != 0) atomicAdd(p.table + (int64_t)n * 2 * VF_METRICS_COLS + t, (unsigned long long)v);
  }
}

}  // namespace

VF_API int vf_frame_metrics(vf_ctx* ctx, const void* a, const void* b, int kind, int N, int C, int H, int W, int vh, int vw,
                            const unsigned char* mask, int clip, int64_t* table) {
  VF_REQUIRE(kind == 0 || kind == 1, "vf_frame_metrics: kind=%d (0 float N x C x H x W, 1 uint8 N x H x W x C)", kind);
  VF_REQUIRE(N >= 1 && N <= 65535 && (C == 1 || C == 3) && H >= 1 && H <= 16384 && W >= 1 && W <= 16384,
             "vf_frame_metrics: %d frames of %d x %d x %d; frames have 1 or 3 channels, sides 1 to 16384, 1 to 65535 of them", N, C, H, W);
  VF_REQUIRE(vh >= 1 && vh <= H && vw >= 1 && vw <= W, "vf_frame_metrics: the valid rectangle %d x %d is outside 1..%d x 1..%d", vh, vw, H, W);
  VF_REQUIRE(a && b && table, "vf_frame_metrics: a, b and table must not be NULL");
  const size_t tbytes = (size_t)N * 2 * VF_METRICS_COLS * sizeof(int64_t);
  VF_CHECK_HIP(hipMemsetAsync(table, 0, tbytes, ctx->stream));
  MetArgs p;
  p.a = a; p.b = b; p.mask = mask; p.table = reinterpret_cast<unsigned long long*>(table);
  p.N = N; p.C = C; p.H = H; p.W = W; p.vh = vh; p.vw = vw; p.clip = clip ? 1 : 0;
  const dim3 grid((unsigned)vf_cdiv(vw, MT), (unsigned)vf_cdiv(vh, MT), (unsigned)N);
  // what the scores need: every valid sample of both batches once, and the mask (the flicker term's second look at frame
  // n - 1 is the kernel's own traffic)
  const double bytes = 2.0 * N * C * (double)vh * vw * (kind == 0 ? 4.0 : 1.0) + (mask ? (double)vh * vw : 0.0) + (double)tbytes;
  if (kind == 0)
    VF_LAUNCH_TIMED(ctx, "frame_metrics", 0.0, bytes, k_frame_metrics<0>, grid, dim3(256), p);
  else
    VF_LAUNCH_TIMED(ctx, "frame_metrics", 0.0, bytes, k_frame_metrics<1>, grid, dim3(256), p);
  VF_LAUNCH_CHECK();
  return 0;
}
