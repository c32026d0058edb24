// vf_conv.hip — 4x4 convolution / transposed convolution, forward + data-grad + weight-grad, for gfx950.
//
// Every pass is an implicit GEMM on the matrix cores.  Three product modes (vf_ctx_set_mfma_mode, template parameter MODE):
//   3 (default)  fp32 operands split exactly into three bf16 planes on their way into LDS (truncation by v_perm_b32), six
//                cross terms on v_mfma_f32_32x32x16_bf16, fp32 accumulators: fp32-grade results at 1.1-1.4x mode 0's speed;
//   0            v_mfma_f32_32x32x2_f32 on the fp32 operands (bit for bit a k-ordered fmaf chain);
//   1            operands rounded to bf16, one term (opt-in).
// Activations are NHWC, weights are the reference tensors in channels-last (see include/vf_hip.h), which makes a layer's
// three passes need only two kernels:
//
//   k_igemm  C[m][n] = sum_{tap,c} A(m,tap,c) * Wt(n,tap,c)
//            - conv forward            (reference: THNN SpatialConvolutionMM_updateOutput, train.lua:89)
//            - conv data-grad          (transposed conv, 4 output-parity classes, each a 2x2-tap GEMM)
//            - full-conv forward       (= conv data-grad; THNN SpatialFullConvolution_updateOutput, train.lua:134)
//            - full-conv data-grad     (= conv forward without bias)
//            - the 4x4 -> 1x1 bottleneck conv and 1x1 -> 4x4 full-conv (plain GEMMs, weight-bandwidth bound)
//   k_wgrad / k_wgrad_group  dW[n][tap][c] = sum_p U(p,n) * V(p,tap,c), split over pixels p
//            - conv / full-conv accGradParameters (the two differ only in which tensor is x and which is gy);
//              the group form runs the weight gradients of a whole backward walk as one launch (vf_wgrad_group_*)
//
// Since round 2 the forward / data-grad passes of layers with >= 1024 GEMM rows and >= 32 channels are served by the
// planes-fed kernels of vf_pgemm.hip (operands split once by their producer, LDS-DMA staging), and the 3-channel
// image-side forward by vf_conv_thin.hip; k_igemm keeps the small-row layers (4x4 maps, bottleneck), modes 0 / 1, the
// thin-output passes (V = 0 scalar gather + col2im) and the callers that bring no planes.
//
// k_igemm tiles: 256 threads = 4 waves of 32x32 MFMA tiles (64x64, 64x128 or 128x128 block tiles), BK = 16 (modes 0 / 1)
// or 32 channels per step (mode 3), LDS double-buffered, register-staged global->LDS copies through BUFFER loads with
// hardware range checking (an out-of-range offset returns zeros: padding taps, ragged tile edges and split-K tails need
// neither a branch nor a select), so every load of step k+1 stays in flight across the MFMAs of step k.  Grid.z carries
// output parity and split-K; blocks are remapped so that the tiles sharing an operand panel land on one XCD's L2.
// Split-K partial slabs are combined by k_slab_reduce* in a fixed order (deterministic; no float atomics); that pass — or
// the GEMM epilogue when there is no split — also leaves the per-tile BatchNorm partial sums of the output when the next
// module is a BatchNorm (vf_bn_fuse_next_fwd / _bwd: the separate statistics pass over the tensor disappears).
#include <algorithm>
#include <vector>
#include <cstdlib>

#include "vf_device.h"

// bf16 MFMA operand (32 rows x 16 k, 8 consecutive k per lane) out of a K-MAJOR bf16 tile [k][LD] in LDS, with gfx950's
// transposing read: per 16-lane group ds_read_b64_tr_b16 takes a 4(k) x 16(column) block and hands lane i column i's four
// k values, so tiles whose pieces arrive as "4 consecutive columns at one k" are stored with one 8-byte write and need
// no transposing pass.  Lane l ends up with column col0 + l%32 and k = k0 + 8*(l/32) .. +7, the 32x32x16 operand map.
// LD (bf16 elements) = columns + 32 keeps the four k rows of a block on disjoint bank quarters.  EXEC must be full.
template <int LD>
__device__ __forceinline__ bf16x8 vf_tr_frag(const __bf16* tile, int col0, int k0, int lane) {
  const int grp = lane >> 4, i = lane & 15;
  const __bf16* a = tile + (k0 + 8 * (grp >> 1) + (i >> 2)) * LD + col0 + 16 * (grp & 1) + 4 * (i & 3);
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)a);
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(a + 4 * LD));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// ------------------------------------------------------------------------------------------------
struct IGemm {
  const float* A;     // gathered activations [B][Hi][Wi][C]
  const float* Wt;    // weights
  const float* bias;  // [N] or null
  float* Y;           // output [B][outH][outW][N]
  float* slab;        // split-K partials, ksplit x (output-sized) ; null when ksplit == 1
  int64_t out_elems;  // B*outH*outW*N
  unsigned a_bytes, w_bytes;  // operand sizes for the buffer descriptors (< 2 GiB each)
  int M, lgMh, lgMw;  // GEMM rows = B << (lgMh+lgMw), decoded as (b, my, mx)
  int Hi, Wi, C;
  int N;
  int TH, TW;                      // taps walked by the K loop
  int sy, ty, oy0, sx, tx, ox0;    // iy = my*sy + th*ty + oy0 (+ph in parity mode)
  int kh0, khs, kw0, kws;          // filter tap (kh, kw) = (kh0 + th*khs, kw0 + tw*kws)
  int wsN, wsC, wsTap;             // weight offset = n*wsN + (kh*4+kw)*wsTap + c*wsC   (all tensors < 2^31 elements)
  int outH, outW, osy, ooy0, osx, oox0;  // output pixel = (my*osy + ooy0, mx*osx + oox0)
  int parity;                      // 1: z&3 = (ph<<1)|pw shifts oy0/ox0/ooy0/oox0 and selects kh0/kw0
  int gm, gn, gz;                  // logical grid (the launch is 1-D, remapped per XCD)
  int ksplit, nk, nq;              // K steps (of 32), number of splits, 16-wide chunks on the vector path
  int klin;                        // K order of the vector path: 1 = tap outer, channel chunk inner (see next_chunk)
  // always 0 / NULL (nothing sets them any more); the kernel still tests them — without those branches the compiler allocates
  // k_igemm differently (the double-buffered mode-3 form: 100 -> 101 VGPRs, scratch in others)
  int dbg;
  long long* stamps;
  int act;
  float slope;
  const float* dmask;              // optional: out = act'(dmask[same index]) * out — the backward of the in-place activation
  int dact;                        // that produced this pass's output tensor's forward twin (nn.LeakyReLU:updateGradInput)
  float dslope;
  VfBnSt st;                       // BatchNorm statistics of the output as a by-product of the epilogue (mode 0: none)
};

// V = 2: 16-byte loads for A and B (C % 16 == 0);  V = 1: 16-byte A, scalar B (k-major B with N % 4 != 0);
// V = 0: scalar loads with a flattened (tap, c) K index (first/last layers: C = 3, 12, 27 ...).
// BF = 1: bf16-operand mode (opt-in, vf_ctx_set_mfma_mode): the fp32 pieces are rounded to bf16 (RNE) on their way
// into LDS (row-major [row][k], 80-byte rows: conflict-free ds_read_b128; k-major operands: vf_tr_frag) and the
// products run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.
// BF = 3: fp32-grade products on the bf16 pipe: every operand element is split EXACTLY into three bf16 planes
// (x = hi + mid + lo: 3 x 8 = the 24 significand bits of an fp32) and the six largest cross terms are accumulated —
// what is dropped (mid*lo, lo*mid, lo*lo) is below 2^-24 of the product, the size of one fp32 rounding.
// Everything outside the LDS tile (addresses, loads, epilogue, split-K) is shared with the fp32 path.
// KLIN: K walked in memory order (tap outer, channel chunk inner) — the 1x1-output bottleneck layers (see next_chunk);
// a template parameter so that no other instantiation carries its counters.
// DB (mode 3, V = 2 only): double-buffered LDS with the split and the LDS writes of step k+1 issued between the MFMAs of
// step k and the global loads running two steps ahead in a second register set — for launches whose grid leaves at
// most two blocks per CU anyway (the 66 KB this needs costs no occupancy there; see launch_igemm).
template <int BM, int BN, int WM, int WN, bool BKM, int V, int BF = 0, bool KLIN = false, bool DB = false>
__global__ __launch_bounds__(256) void k_igemm(const IGemm p) {
  // One K step = 32 = two 16-wide chunks; each chunk has its own (tap, c0), so any C % 16 == 0 vectorises.
  constexpr int BK = 32, LDA = BK + 4;
  constexpr int LDB = BKM ? (BN + 4) : BK + 4;
  constexpr int MT = WM / 32, NT = WN / 32;
  constexpr int WAVES_N = BN / WN;
  static_assert((BM / WM) * WAVES_N == 4, "4 waves per block");
  constexpr int A_CH = (BM * 8 + 255) / 256;
  constexpr int B_CH = (BN * 8 + 255) / 256;
  constexpr int A_SZ = BM * LDA;
  constexpr int B_SZ = BKM ? BK * LDB : BN * LDB;
  // Row-major bf16 tiles (BF): 64-byte rows, NO padding, the four 16-byte k-octets of a row XOR-swizzled by
  // (row >> 2) & 3.  ds_read_b128 serves {0-3,12-15,20-27}-style 16-lane groups on a 256-byte bank row: the four
  // row-quads of a group get the four different swizzles, so their octets land on 16 distinct slots; ds_write_b64
  // serves 16 contiguous lanes (= two whole rows) on a 128-byte window, which two unpadded 64-byte rows fill exactly.
  // (The padded linear layout — 80-byte rows — kept the reads conflict-free but made every plane write 2-way:
  //  SQ_LDS_BANK_CONFLICT was a third of the LDS pipe's active cycles.)
  constexpr int LDH = BK;                              // bf16 elements per LDS row (BF)
  auto frag_off = [](int row, int octet) { return row * LDH + ((octet ^ ((row >> 2) & 3)) << 3); };        // 8 k of `row`
  auto piece_off = [](int row, int kq) { return row * LDH + (((kq >> 1) ^ ((row >> 2) & 3)) << 3) + ((kq & 1) << 2); };
  constexpr int LDN = BN + 32;                         // k-major bf16 B tile (BF && BKM): [k][LDN], transposing reads
  constexpr int AH_SZ = BM * LDH, BH_SZ = BKM ? BK * LDN : BN * LDH;    // bf16 elements per buffer (BF)
  constexpr int NP = BF > 0 ? BF : 1;                  // bf16 planes per operand
  static_assert(!DB || (BF == 3 && V == 2), "the double-buffered schedule is built for mode 3's vector path");
  constexpr int NBUF = (BF == 3 && !DB) ? 1 : 2;       // three planes: single-buffered LDS (capacity), loads still run ahead
  constexpr int PL_SZ = AH_SZ + BH_SZ;                 // one plane of (A, B), bf16 elements
  constexpr int SMEM_F = BF ? (NBUF * NP * PL_SZ + 1) / 2 : 2 * (A_SZ + B_SZ);
  __shared__ __attribute__((aligned(16))) float smem[SMEM_F];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave / WAVES_N) * WM, wn = (wave % WAVES_N) * WN;
  if (p.stamps && tid == 0) { p.stamps[8 * blockIdx.x + 0] = wall_clock64(); p.stamps[8 * blockIdx.x + 4] = (long long)__builtin_readcyclecounter(); }
  // logical tile id: output parity fastest (the 4 parity classes of a transposed pass read the same input rows),
  // then M tiles (halo sharing), then N tiles, then split-K
  int lid = vf_xcd_remap(blockIdx.x, p.gm * p.gn * p.gz);
  int ph = 0, pw = 0;
  if (p.parity) {
    ph = (lid >> 1) & 1;
    pw = lid & 1;
    lid >>= 2;
  }
  const int bx = lid % p.gm, byz = lid / p.gm;
  const int m0 = bx * BM, n0 = (byz % p.gn) * BN;
  const int z = byz / p.gn;
  const int ks = z;
  const int steps = (p.nk + p.ksplit - 1) / p.ksplit;
  const int kt0 = ks * steps;
  const int kt1 = min(p.nk, kt0 + steps);
  const int oy0 = p.oy0 + ph, ox0 = p.ox0 + pw;
  const int kh0 = p.parity ? (1 - ph) : p.kh0, kw0 = p.parity ? (1 - pw) : p.kw0;
  const int ooy0 = p.ooy0 + ph, oox0 = p.oox0 + pw;
  const int Mw = 1 << p.lgMw, Mh = 1 << p.lgMh;
  const int Ktot = p.TH * p.TW * p.C;

  // ---- per-thread A rows (fixed for the whole K loop)
  int a_iy0[A_CH], a_ix0[A_CH], a_boff[A_CH];
  bool a_ok[A_CH];
#pragma unroll
  for (int i = 0; i < A_CH; ++i) {
    const int id = tid + 256 * i;
    const int m = m0 + (id >> 3);
    a_ok[i] = (id < BM * 8) && m < p.M;
    const int mx = m & (Mw - 1), my = (m >> p.lgMw) & (Mh - 1), b = m >> (p.lgMw + p.lgMh);
    a_iy0[i] = my * p.sy + oy0;
    a_ix0[i] = mx * p.sx + ox0;
    a_boff[i] = b * p.Hi * p.Wi * p.C;
  }
  const int kq = tid & 7;          // 16-byte column of the 32-wide K step
  const int kh = kq >> 2, kl = kq & 3;  // chunk (0/1) and 16-byte column inside the chunk

  f32x4 ra[DB ? 2 : 1][A_CH], rb[DB ? 2 : 1][B_CH];      // operand pieces in flight (DB: two steps' worth)
  const __amdgpu_buffer_rsrc_t rsA = vf_rsrc(p.A, p.a_bytes), rsW = vf_rsrc(p.Wt, p.w_bytes);

  auto tap_index = [&](int tap) {
    const int th = tap / p.TW, tw = tap - th * p.TW;
    return (kh0 + th * p.khs) * 4 + (kw0 + tw * p.kws);
  };

  // ---- vector path (V >= 1): everything that depends on the K step is wave-uniform (SALU); a lane only adds a
  // per-step delta to byte offsets it computed once, and tests one bit of its per-row tap-validity mask.
  unsigned a_mask[A_CH];   // bit t: tap t of this row is inside the image
  unsigned a_byte[A_CH];   // byte offset of (tap (0,0), c = 4*kl) for this row (wraps for padding rows; masked)
  unsigned w_byte[B_CH];   // per-thread weight byte offset at (tap 0, c0 = 0)
  bool w_ok[B_CH];
  if constexpr (V >= 1) {
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
      a_byte[i] = 4u * (unsigned)(a_boff[i] + (a_iy0[i] * p.Wi + a_ix0[i]) * p.C + 4 * kl);
      // bit (th*TW + tw) = row th and column tw of the tap window are inside the image: an outer product of a row
      // mask and a column mask (TH, TW <= 4) — a loop over all taps with a division each cost 8 us of prologue
      unsigned ym = 0, xm = 0;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t < p.TH && (unsigned)(a_iy0[i] + t * p.ty) < (unsigned)p.Hi) ym |= 1u << t;
        if (t < p.TW && (unsigned)(a_ix0[i] + t * p.tx) < (unsigned)p.Wi) xm |= 1u << t;
      }
      unsigned mk = 0;
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if ((ym >> t) & 1u) mk |= xm << (t * p.TW);
      a_mask[i] = a_ok[i] ? mk : 0u;
    }
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
      const int id = tid + 256 * i;
      if constexpr (!BKM) {
        const int n = n0 + (id >> 3);
        w_ok[i] = id < BN * 8 && n < p.N;
        w_byte[i] = 4u * (unsigned)(n * p.wsN + 4 * kl);
      } else {
        const int kk = id / (BN / 4), nq = id - kk * (BN / 4);
        const int n = n0 + 4 * nq;
        w_ok[i] = id < BN * 8 && n < p.N;
        w_byte[i] = 4u * (unsigned)((kk & 15) * p.wsC + n);
      }
    }
  }
  // uniform description of one 16-wide chunk: (tap, byte delta for A, byte delta for W, in range).  The K loop walks
  // chunks in order, so (tap, c0) advance incrementally — no division in the loop (a wave issues ~1 instruction per
  // 4-5 cycles; every instruction that is not an MFMA shortens the time the matrix pipe is fed).
  struct Chunk { int tap; unsigned dA, dW; bool ok; };
  const int lgTW = p.TW == 4 ? 2 : (p.TW == 2 ? 1 : 0);
  const int sA_th = 4 * p.ty * p.Wi * p.C, sA_tw = 4 * p.tx * p.C;
  const int sW_th = 4 * p.khs * 4 * p.wsTap, sW_tw = 4 * p.kws * p.wsTap, sW_0 = 4 * (kh0 * 4 + kw0) * p.wsTap;
  const int sW_c = 4 * (BKM ? p.wsC : 1);
  int it_tap = 0, it_c0 = 0, it_q = 0;     // state of the NEXT chunk to be described
  // the memory-order walk (KLIN) keeps its OWN two counters and is selected at compile time: written as a runtime
  // branch with the mirror-image update of it_tap / it_c0, LLVM merges the two branches into a select of ADDRESSES,
  // the counters move to scratch memory, and every K step of EVERY kernel starts with a scratch_load +
  // s_waitcnt vmcnt(0) in front of the operand prefetches (measured: -5 % per step)
  int kl_tap = 0, kl_c0 = 0;
  const int ntaps = p.TH * p.TW;
  if constexpr (V >= 1) {
    // chunk order: channel chunk OUTER, tap INNER — the 16 taps of one channel chunk touch the same input window, so
    // the re-reads are temporally close (L1/L2 hits) instead of one full window sweep per tap
    it_q = 2 * kt0;
    it_c0 = (it_q / ntaps) << 4;
    it_tap = it_q % ntaps;
    if constexpr (KLIN) {
      // a 1x1 output map (the bottleneck layers) has no window overlap between taps to exploit; walking K in memory
      // order instead makes each weight row a single forward stream of 128-byte lines per block rather than 64-byte
      // pieces 2 KB apart (the 131 MB weight matrix is what this GEMM is bounded by)
      const int cpt = p.C >> 4;
      kl_tap = it_q / cpt;
      kl_c0 = (it_q - kl_tap * cpt) << 4;
    }
  }
  auto next_chunk = [&]() {
    Chunk c;
    const int tap = KLIN ? kl_tap : it_tap, c0 = KLIN ? kl_c0 : it_c0;
    const int th = tap >> lgTW, tw = tap & (p.TW - 1);
    c.tap = tap;
    c.dA = (unsigned)(th * sA_th + tw * sA_tw + 4 * c0);
    c.dW = (unsigned)(sW_0 + th * sW_th + tw * sW_tw + c0 * sW_c);
    c.ok = it_q < p.nq;
    ++it_q;
    if constexpr (KLIN) {
      kl_c0 += 16;
      if (kl_c0 >= p.C) {
        kl_c0 = 0;
        ++kl_tap;
      }
    } else {
      if (++it_tap >= ntaps) {
        it_tap = 0;
        it_c0 += 16;
      }
    }
    return c;
  };

  // One K step's operands arrive as A_CH + B_CH independent pieces (one 16-byte register each).  `begin_tile` does
  // the wave-uniform part once per step; the pieces are issued one at a time BETWEEN the MFMAs of the running step
  // (a contiguous block of ~60 address/load instructions would leave the matrix pipe empty: it queues one MFMA).
  Chunk tc0, tc1;
  int t_tapv = 0;
  unsigned t_dA = 0;
  bool t_okq = false;
  int t_kt = 0;
  int s_dy[4], s_dx[4], s_c[4], s_w[4];     // scalar path (V = 0): per-step decomposition of this thread's k
  bool s_kok[4];
  auto begin_tile = [&](int kt, bool live) {
    t_kt = kt;
    if constexpr (V >= 1) {
      tc0 = next_chunk();      // SALU; begin_tile is called with consecutive kt
      tc1 = next_chunk();
      tc0.ok = tc0.ok && live;
      tc1.ok = tc1.ok && live;
      t_tapv = kh ? tc1.tap : tc0.tap;
      t_dA = kh ? tc1.dA : tc0.dA;
      t_okq = kh ? tc1.ok : tc0.ok;
    } else {
      t_okq = live;
      // scalar path: the (tap, c) decomposition of this thread's four k depends on the step only, not on the row —
      // done once here instead of once per row and element (a runtime division each; the 3-channel first layer
      // spent most of its time on them)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = kt * BK + 4 * kq + j;
        const int tap = k / p.C, c = k - tap * p.C;
        const int th = tap / p.TW, tw = tap - th * p.TW;
        s_dy[j] = th * p.ty;
        s_dx[j] = tw * p.tx;
        s_c[j] = c;
        s_kok[j] = live && k < Ktot;
        s_w[j] = tap_index(tap) * p.wsTap + c * p.wsC;
      }
    }
  };
  auto load_piece = [&](int pc, auto SET) {
    constexpr int rs = decltype(SET)::value;
    const int kt = t_kt;
    if constexpr (V >= 1) {
      if (pc < A_CH) {
        // ---------------- A: lanes with kh = 0 / 1 fetch chunk 0 / 1
        const int i = pc;
        const bool ok = t_okq && ((a_mask[i] >> t_tapv) & 1u);
        ra[rs][i] = vf_bload4(rsA, ok ? a_byte[i] + t_dA : VF_OOB);
      } else {
        // ---------------- B
        const int i = pc - A_CH;
        bool hi;
        if constexpr (!BKM) {
          hi = kh;
        } else {
          hi = (((tid + 256 * i) / (BN / 4)) >> 4) & 1;
        }
        const unsigned dW = hi ? tc1.dW : tc0.dW;
        const bool ok = w_ok[i] && (hi ? tc1.ok : tc0.ok);
        if constexpr (V == 2) {
          rb[rs][i] = vf_bload4(rsW, ok ? w_byte[i] + dW : VF_OOB);
        } else {   // V == 1: k-major B whose N is not a multiple of 4 -> four scalar loads along n
          const int n = n0 + 4 * ((tid + 256 * i) % (BN / 4));
          f32x4 v;
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = vf_bload1(rsW, (ok && n + j < p.N) ? w_byte[i] + dW + 4u * j : VF_OOB);
          rb[rs][i] = v;
        }
      }
    } else {
      // ---------------- scalar path: flattened K index, per-element (tap, c)
      if (pc < A_CH) {
        const int i = pc;
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int iy = a_iy0[i] + s_dy[j], ix = a_ix0[i] + s_dx[j];
          const bool ok = s_kok[j] && a_ok[i] && (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi;
          v[j] = vf_bload1(rsA, ok ? 4u * (unsigned)(a_boff[i] + (iy * p.Wi + ix) * p.C + s_c[j]) : VF_OOB);
        }
        ra[rs][i] = v;
      } else {
        const int i = pc - A_CH;
        const int id = tid + 256 * i;
        f32x4 v;
        if constexpr (!BKM) {
          const int n = n0 + (id >> 3);
          const bool okn = t_okq && id < BN * 8 && n < p.N;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            v[j] = vf_bload1(rsW, (okn && s_kok[j]) ? 4u * (unsigned)(n * p.wsN + s_w[j]) : VF_OOB);
        } else {
          const int kk = id / (BN / 4), nq = id - kk * (BN / 4);
          const int n = n0 + 4 * nq;
          const int k = kt * BK + kk;
          const int tap = k / p.C, c = k - tap * p.C;
          const bool okk = t_okq && id < BN * 8 && k < Ktot;
          const int base = tap_index(tap) * p.wsTap + c * p.wsC;
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = vf_bload1(rsW, (okk && n + j < p.N) ? 4u * (unsigned)(base + n + j) : VF_OOB);
        }
        rb[rs][i] = v;
      }
    }
  };
  auto load_tile = [&](int kt) {
    begin_tile(kt, true);
#pragma unroll
    for (int pc = 0; pc < A_CH + B_CH; ++pc) load_piece(pc, VfIntC<0>{});
  };

  auto store_piece = [&](int buf, int pc, auto SET) {
    constexpr int rs = decltype(SET)::value;
    if constexpr (BF) {
      // mode 3: plane q = top 16 bits of the residual after the planes before it (vf_split3); mode 1: bf16(v), RNE
      __bf16* base = (__bf16*)smem + buf * (NP * PL_SZ);
      if (pc < A_CH) {
        const int i = pc, id = tid + 256 * i;
        if (256 * i + 255 < BM * 8 || id < BM * 8) {
          __bf16* dst = base + piece_off(id >> 3, kq);
          if constexpr (NP == 3) {
            u32x2 s3[3];
            vf_split3(ra[rs][i], s3);
#pragma unroll
            for (int q = 0; q < 3; ++q) *(u32x2*)(dst + q * PL_SZ) = s3[q];
          } else {
            *(bf16x4*)dst = __builtin_convertvector(ra[rs][i], bf16x4);
          }
        }
      } else {
        const int i = pc - A_CH, id = tid + 256 * i;
        if (256 * i + 255 < BN * 8 || id < BN * 8) {
          f32x4 v = rb[rs][i];
          int off;
          if constexpr (!BKM) {
            off = piece_off(id >> 3, kq);
          } else {      // the piece holds 4 consecutive n at one k: stored as it comes, transposed by the reads
            const int kk = id / (BN / 4), nq = id - kk * (BN / 4);
            off = kk * LDN + 4 * nq;
          }
          __bf16* dst = base + AH_SZ + off;
          if constexpr (NP == 3) {
            u32x2 s3[3];
            vf_split3(v, s3);
#pragma unroll
            for (int q = 0; q < 3; ++q) *(u32x2*)(dst + q * PL_SZ) = s3[q];
          } else {
            *(bf16x4*)dst = __builtin_convertvector(v, bf16x4);
          }
        }
      }
      return;
    }
    float* As = smem + buf * (A_SZ + B_SZ);
    float* Bs = As + A_SZ;
    if (pc < A_CH) {
      const int i = pc, id = tid + 256 * i;
      if (256 * i + 255 < BM * 8 || id < BM * 8) *(f32x4*)(As + (id >> 3) * LDA + 4 * kq) = ra[rs][i];
    } else {
      const int i = pc - A_CH, id = tid + 256 * i;
      if (256 * i + 255 < BN * 8 || id < BN * 8) {     // constant-true for full pieces: no exec-mask branch in the loop
        if constexpr (!BKM) {
          *(f32x4*)(Bs + (id >> 3) * LDB + 4 * kq) = rb[rs][i];
        } else {
          const int kk = id / (BN / 4), nq = id - kk * (BN / 4);
          *(f32x4*)(Bs + kk * LDB + 4 * nq) = rb[rs][i];
        }
      }
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int pc = 0; pc < A_CH + B_CH; ++pc) store_piece(buf, pc, VfIntC<0>{});
  };

  f32x16 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

  const int lr = lane & 31, lh = lane >> 5;

  if (kt0 < kt1) {
    load_tile(kt0);
    store_tile(0);
  }
  __syncthreads();
  if (p.stamps && tid == 0) p.stamps[8 * blockIdx.x + 1] = wall_clock64();
  if constexpr (DB) {
    // Step kt (register set S = parity of kt - kt0, LDS buffer S):
    //   MFMA slot i < NPC  is followed by operand piece i of step kt+2 (global -> register set S, whose previous
    //                      content — step kt — went to LDS during step kt-1);
    //   the last NPC slots are each followed by one piece of step kt+1 (register set S^1, loaded during step kt-1):
    //                      split into planes + three LDS writes into buffer S^1, in the shadow of the running MFMA;
    //   the fragments of the second 16-deep group are read right after the first MFMA.  One barrier per step.
    constexpr int NPC = A_CH + B_CH;
    constexpr int NMF = 6 * MT * NT;               // MFMAs per 16-deep group
    constexpr int SLOTS = (BK / 16) * NMF;
    static_assert(2 * NPC <= SLOTS, "loads and LDS writes of one K step must fit between its MFMAs");
    begin_tile(kt0 + 1, kt0 + 1 < kt1);
#pragma unroll
    for (int pc = 0; pc < NPC; ++pc) load_piece(pc, VfIntC<1>{});
    auto step = [&](int kt, auto SET) {
      constexpr int S = decltype(SET)::value;
      const __bf16* base = (const __bf16*)smem + S * (NP * PL_SZ);
      // nothing of this step may float above this point (left alone, the split of step kt+1's pieces is hoisted to the
      // top of the step, in front of the loads issued here, and waits for ALL outstanding loads there)
      __builtin_amdgcn_sched_barrier(0);
      begin_tile(kt + 2, kt + 2 < kt1);
      bf16x8 a[2][NP][MT], b[2][NP][NT];
      auto read_frag = [&](int g) {
#pragma unroll
        for (int q = 0; q < NP; ++q) {
          const __bf16* Ah = base + q * PL_SZ;
          const __bf16* Bh = Ah + AH_SZ;
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) a[g][q][mt] = *(const bf16x8*)(Ah + frag_off(wm + mt * 32 + lr, 2 * g + lh));
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            if constexpr (!BKM)
              b[g][q][nt] = *(const bf16x8*)(Bh + frag_off(wn + nt * 32 + lr, 2 * g + lh));
            else
              b[g][q][nt] = vf_tr_frag<LDN>(Bh, wn + nt * 32, 16 * g, lane);
          }
        }
      };
      read_frag(0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int g = 0; g < BK / 16; ++g) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int t = 0; t < 6; ++t) {       // smallest terms first
              constexpr int qa[6] = {1, 0, 2, 0, 1, 0}, qb[6] = {1, 2, 0, 1, 0, 0};
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[g][qa[t]][mt], b[g][qb[t]][nt], acc[mt][nt], 0, 0, 0);
              const int slot = g * NMF + (mt * NT + nt) * 6 + t;
              if (slot == 0 && BK / 16 > 1) read_frag(1);
              if (slot < NPC) load_piece(slot, SET);
              // (unconditional: on the last step this writes zeros into the buffer nobody reads again; a branch here
              //  makes the compiler drain every outstanding load at the top of each step)
              if (slot >= SLOTS - NPC) store_piece(S ^ 1, slot - (SLOTS - NPC), VfIntC<(S ^ 1)>{});
              __builtin_amdgcn_sched_barrier(0);
            }
      }
      __syncthreads();
    };
    for (int kt = kt0; kt < kt1; kt += 2) {
      step(kt, VfIntC<0>{});
      if (kt + 1 < kt1) step(kt + 1, VfIntC<1>{});
    }
  } else
  if constexpr (BF) {
    for (int kt = kt0; kt < kt1; ++kt) {
      const int buf = NBUF == 2 ? ((kt - kt0) & 1) : 0;
      const __bf16* base = (const __bf16*)smem + buf * (NP * PL_SZ);
      begin_tile(kt + 1, kt + 1 < kt1);
#pragma unroll
      for (int pc = 0; pc < A_CH + B_CH; ++pc) load_piece(pc, VfIntC<0>{});
#pragma unroll
      for (int g = 0; g < BK / 16; ++g) {
        bf16x8 a[NP][MT], b[NP][NT];
#pragma unroll
        for (int q = 0; q < NP; ++q) {
          const __bf16* Ah = base + q * PL_SZ;
          const __bf16* Bh = Ah + AH_SZ;
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) a[q][mt] = *(const bf16x8*)(Ah + frag_off(wm + mt * 32 + lr, 2 * g + lh));
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            if constexpr (!BKM)
              b[q][nt] = *(const bf16x8*)(Bh + frag_off(wn + nt * 32 + lr, 2 * g + lh));
            else
              b[q][nt] = vf_tr_frag<LDN>(Bh, wn + nt * 32, 16 * g, lane);
          }
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            if constexpr (NP == 3) {      // smallest terms first
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][mt], b[1][nt], acc[mt][nt], 0, 0, 0);
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][mt], b[2][nt], acc[mt][nt], 0, 0, 0);
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2][mt], b[0][nt], acc[mt][nt], 0, 0, 0);
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][mt], b[1][nt], acc[mt][nt], 0, 0, 0);
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][mt], b[0][nt], acc[mt][nt], 0, 0, 0);
            }
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][mt], b[0][nt], acc[mt][nt], 0, 0, 0);
          }
      }
      // keep the split of the next step's pieces below this step's MFMAs: hoisted above them (it depends on the loads
      // only) it makes the wave wait for a load it issued two MFMAs earlier
      if constexpr (NBUF == 1) __builtin_amdgcn_sched_barrier(0);
      if constexpr (NBUF == 1) __syncthreads();       // everyone has read the tile before it is overwritten
      store_tile(NBUF == 2 ? (buf ^ 1) : 0);
      __syncthreads();
    }
  } else {
  constexpr int NPC = A_CH + B_CH;             // operand pieces per K step
  constexpr int NMF = 4 * MT * NT;             // MFMAs per 8-wide sub-step
  constexpr int SLOTS = (BK / 8) * NMF;        // MFMA slots per K step
  static_assert(2 * NPC <= SLOTS, "loads and LDS writes of one K step must fit between its MFMAs");
  for (int kt = kt0; kt < kt1; ++kt) {
    const int buf = (kt - kt0) & 1;
    const float* As = smem + buf * (A_SZ + B_SZ);
    const float* Bs = As + A_SZ;
    // The step's schedule, pinned with scheduling barriers (left alone, the compiler gathers all loads at the top and
    // all LDS writes at the bottom, and the matrix pipe idles through both):
    //   fragment reads run one sub-step ahead of the MFMAs that consume them (two waves sharing a SIMD interleave
    //   their MFMAs one for one and finish a group together, so a read issued only then is latency nobody covers);
    //   MFMA slot i < NPC is followed by operand piece i of step kt+1 (global -> register);
    //   the last NPC slots are each followed by one register -> LDS write into the other buffer.
    auto read_frag = [&](int ss, f32x4 (&a)[MT], f32x4 (&b)[NT]) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) a[mt] = *(const f32x4*)(As + (wm + mt * 32 + lr) * LDA + 8 * ss + 4 * lh);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        if constexpr (!BKM) {
          b[nt] = *(const f32x4*)(Bs + (wn + nt * 32 + lr) * LDB + 8 * ss + 4 * lh);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) b[nt][j] = Bs[(8 * ss + 4 * lh + j) * LDB + wn + nt * 32 + lr];
        }
      }
    };
    const bool more = kt + 1 < kt1 && !(p.dbg & 1);
    begin_tile(kt + 1, more);
    f32x4 fa[2][MT], fb[2][NT];
    read_frag(0, fa[0], fb[0]);
#pragma unroll
    for (int ss = 0; ss < BK / 8; ++ss) {
      if (ss + 1 < BK / 8) read_frag(ss + 1, fa[(ss + 1) & 1], fb[(ss + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[ss & 1][mt][j], fb[ss & 1][nt][j], acc[mt][nt], 0, 0, 0);
            const int slot = ss * NMF + (j * MT + mt) * NT + nt;
            if (slot < NPC) load_piece(slot, VfIntC<0>{});
            if (slot >= SLOTS - NPC) store_piece(buf ^ 1, slot - (SLOTS - NPC), VfIntC<0>{});
            __builtin_amdgcn_sched_barrier(0);
          }
    }
    __syncthreads();
  }

  }
  if (p.stamps && tid == 0) p.stamps[8 * blockIdx.x + 2] = wall_clock64();
  // ---- epilogue: C/D layout col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
  float* out = p.ksplit > 1 ? p.slab + (int64_t)ks * p.out_elems : p.Y;
  const bool fin = p.ksplit == 1;
  const int stm = fin ? p.st.mode : 0;      // with split-K the statistics come out of the slab reduce instead
  float bv[NT], sv[NT], st1[NT], st2[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int n = n0 + wn + nt * 32 + lr;
    bv[nt] = (fin && p.bias && n < p.N) ? p.bias[n] : 0.f;
    // statistics: the shift (forward) or the saved mean of this row tile's batch group (backward)
    sv[nt] = (stm && n < p.N) ? p.st.vec[(stm == 2 ? (bx / p.st.tiles_per_group) * p.N : 0) + n] : 0.f;
    st1[nt] = 0.f;
    st2[nt] = 0.f;
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wm + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      const int m = m0 + row;
      if (m >= p.M) continue;
      const int mx = m & (Mw - 1), my = (m >> p.lgMw) & (Mh - 1), b = m >> (p.lgMw + p.lgMh);
      const int64_t pix = ((int64_t)b * p.outH + (my * p.osy + ooy0)) * p.outW + (mx * p.osx + oox0);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n = n0 + wn + nt * 32 + lr;
        if (n < p.N) {
          float v = acc[mt][nt][r];
          if (fin) {
            v = vf_act_apply(v + bv[nt], p.act, p.slope);
            if (p.dmask) v = vf_act_grad(p.dmask[pix * p.N + n], v, p.dact, p.dslope);
            if (stm == 1) {
              const float d = v - sv[nt];
              st1[nt] += d;
              st2[nt] += d * d;
            } else if (stm == 2) {
              st1[nt] += v;
              st2[nt] += v * (p.st.x[pix * p.N + n] - sv[nt]);
            }
          }
          out[pix * p.N + n] = v;
        }
      }
    }
  }
  if (stm)      // (uniform over the block; the K loop ended on a barrier, so the tile memory is free)
    vf_bn_tile_partials<NT, BM / WM, BN>(p.st, st1, st2, smem, wave / WAVES_N, wn, lane, tid, n0, p.N, bx,
                                         p.parity ? ((ph << 1) | pw) : 0);
  if (p.stamps && tid == 0) {
    __builtin_amdgcn_s_waitcnt(0);     // stores retired (vmcnt 0)
    p.stamps[8 * blockIdx.x + 3] = wall_clock64();
    p.stamps[8 * blockIdx.x + 5] = (long long)__builtin_readcyclecounter();
  }
}

// y = act(sum_s slab[s] + bias)  or  dst = beta*dst + sum_s slab[s]  (wgrad).  Scalar form (any total).
__global__ void k_slab_reduce(const float* __restrict__ slab, float* __restrict__ dst, const float* __restrict__ bias,
                              int64_t total, int N, int ksplit, int act, float slope, float beta,
                              const float* __restrict__ dmask = nullptr, int dact = 0, float dslope = 0.f) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int k = 0; k < ksplit; ++k) s += slab[(int64_t)k * total + i];
    if (bias) s += bias[i % N];
    if (beta != 0.f) s += beta * dst[i];
    s = vf_act_apply(s, act, slope);
    if (dmask) s = vf_act_grad(dmask[i], s, dact, dslope);
    dst[i] = s;
  }
}
// 16-byte form: COLS float4 columns x (256 / COLS) split lanes per block; lanes are combined in a fixed order.
// COLS = 64 is the workhorse; COLS = 16 (16 split lanes) serves small outputs with very deep splits (the image-side
// weight gradients: 48 x 64 outputs from 500+ slabs — twelve 64-column blocks walking 128 slabs each sat at 15 us).
template <int COLS>
__global__ __launch_bounds__(256) void k_slab_reduce4(const float* __restrict__ slab, float* __restrict__ dst,
                                                      const float* __restrict__ bias, int64_t total4, int N, int ksplit,
                                                      int act, float slope, float beta,
                                                      const float* __restrict__ dmask = nullptr, int dact = 0,
                                                      float dslope = 0.f) {
  constexpr int L = 256 / COLS;
  const int tx = threadIdx.x % COLS, sl = threadIdx.x / COLS;
  const int64_t i4 = (int64_t)blockIdx.x * COLS + tx;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (i4 < total4) {
#pragma unroll 4
    for (int k = sl; k < ksplit; k += L) s += ((const f32x4*)slab)[(int64_t)k * total4 + i4];
  }
  __shared__ f32x4 red[L][COLS];
  red[sl][tx] = s;
  __syncthreads();
  if (sl == 0 && i4 < total4) {
    f32x4 t = red[0][tx];
#pragma unroll
    for (int l = 1; l < L; ++l) t += red[l][tx];
    if (beta != 0.f) t += beta * ((const f32x4*)dst)[i4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = t[e];
      if (bias) v += bias[(i4 * 4 + e) % N];
      t[e] = vf_act_apply(v, act, slope);
    }
    if (dmask) {
      const f32x4 m = ((const f32x4*)dmask)[i4];
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] = vf_act_grad(m[e], t[e], dact, dslope);
    }
    ((f32x4*)dst)[i4] = t;
  }
}
// Split-K combine that also leaves BatchNorm statistics partials (VfBnSt): the output [M][N] is walked as units of 256
// consecutive floats (64 float4 lanes); a block owns one 256-wide column chunk (blockIdx.y; N <= 256: the unit holds 256 / N
// whole rows) and a run of `units_per_block` row units, 4 row lanes deep, every thread summing its element's slabs in
// slab order.  A thread always sees the same four channels, so its statistics stay in registers until the end; the lanes
// that alias a channel (4 row lanes; 256 / N column lanes when N < 256) meet in LDS in a fixed order.  Requires
// total % 256 == 0 and (256 % N == 0 or N % 256 == 0) — every layer the nets pair with a BatchNorm.
__global__ __launch_bounds__(256) void k_slab_reduce_st(const float* __restrict__ slab, float* __restrict__ dst,
                                                        const float* __restrict__ bias, int64_t total4, int N, int ksplit, int act,
                                                        float slope, const float* __restrict__ dmask, int dact, float dslope,
                                                        int units_per_block, int64_t row_units, int ncc, const VfBnSt st) {
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int cc = blockIdx.y;
  const int ch0 = (N <= 256 ? (tx * 4) % N : cc * 256 + tx * 4);      // first of this thread's four channels
  const int g = blockIdx.x / st.tiles_per_group;                        // batch group of this block's rows
  f32x4 bv = {0.f, 0.f, 0.f, 0.f}, sv = {0.f, 0.f, 0.f, 0.f};
  if (bias) bv = *(const f32x4*)(bias + ch0);
  if (st.mode) sv = *(const f32x4*)(st.vec + (st.mode == 2 ? g * N : 0) + ch0);
  f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
  const int64_t u0 = (int64_t)blockIdx.x * units_per_block, u1 = min(row_units, u0 + units_per_block);
  for (int64_t ru = u0 + ty; ru < u1; ru += 4) {
    const int64_t i4 = (ru * ncc + cc) * 64 + tx;
    f32x4 t = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k = 0; k < ksplit; ++k) t += ((const f32x4*)slab)[(int64_t)k * total4 + i4];
    t += bv;
#pragma unroll
    for (int e = 0; e < 4; ++e) t[e] = vf_act_apply(t[e], act, slope);
    if (dmask) {
      const f32x4 m = ((const f32x4*)dmask)[i4];
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] = vf_act_grad(m[e], t[e], dact, dslope);
    }
    if (st.mode == 1) {
      const f32x4 d = t - sv;
      s1 += d;
      s2 += d * d;
    } else if (st.mode == 2) {
      const f32x4 xv = ((const f32x4*)st.x)[i4];
      s1 += t;
      s2 += t * (xv - sv);
    }
    ((f32x4*)dst)[i4] = t;
  }
  if (!st.mode) return;
  __shared__ f32x4 red[2][256];
  red[0][threadIdx.x] = s1;
  red[1][threadIdx.x] = s2;
  __syncthreads();
  const int lanes = N <= 256 ? N / 4 : 64;        // distinct float4 channel columns in this block
  if ((int)threadIdx.x < lanes) {
    double a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
    for (int t = threadIdx.x; t < 256; t += lanes) {     // (t % 64) % lanes == threadIdx.x: same channels (lanes divides 64)
      const f32x4 u = red[0][t], w = red[1][t];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        a[e] += (double)u[e];
        b[e] += (double)w[e];
      }
    }
    const int local = blockIdx.x - g * st.tiles_per_group;
    double* o = st.part + ((int64_t)(g * st.rows_per_group + local) * 2) * N;
    const int c0 = (N <= 256 ? 0 : cc * 256) + threadIdx.x * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o[c0 + e] = a[e];
      o[N + c0 + e] = b[e];
    }
  }
}
// plan of that launch: (units_per_block, blocks per group); false: the shape does not fit (caller keeps the plain reduce)
static bool slab_st_plan(int64_t total, int N, int groups, int rows_cap, int* units_per_block, int* blocks_per_group, int* ncc_out,
                         int64_t* row_units_out) {
  if (total % 256 != 0 || N % 4 != 0 || !((N <= 256 && 256 % N == 0) || (N > 256 && N % 256 == 0))) return false;
  const int ncc = N <= 256 ? 1 : N / 256;
  const int64_t row_units = total / 256 / ncc;
  if (row_units % groups != 0) return false;
  const int64_t per_group = row_units / groups;
  // ~512 blocks over the whole launch, at least 4 row units (one per row lane) each, a divisor of the group's units
  int64_t upb = std::max<int64_t>(4, vf_cdiv(row_units * ncc, 512));
  while (upb < per_group && per_group % upb != 0) ++upb;
  if (upb > per_group) upb = per_group;
  if (per_group % upb != 0) return false;
  const int64_t bpg = per_group / upb;
  if (bpg > rows_cap) return false;
  *units_per_block = (int)upb;
  *blocks_per_group = (int)bpg;
  *ncc_out = ncc;
  *row_units_out = row_units;
  return true;
}
static int launch_slab_reduce(vf_ctx* ctx, const float* slab, float* dst, const float* bias, int64_t total, int N, int ksplit,
                              int act, float slope, float beta, const float* dmask = nullptr, int dact = 0,
                              float dslope = 0.f) {
  if (total % 4 == 0 && ((((uintptr_t)slab) | ((uintptr_t)dst) | ((uintptr_t)dmask)) & 15) == 0 && ksplit > 0) {
    const int64_t total4 = total / 4;
    if (total4 <= 8192 && ksplit >= 64)
      hipLaunchKernelGGL(k_slab_reduce4<16>, dim3((int)vf_cdiv(total4, 16)), dim3(256), 0, ctx->stream, slab, dst, bias, total4, N,
                         ksplit, act, slope, beta, dmask, dact, dslope);
    else
      hipLaunchKernelGGL(k_slab_reduce4<64>, dim3((int)vf_cdiv(total4, 64)), dim3(256), 0, ctx->stream, slab, dst, bias, total4, N,
                         ksplit, act, slope, beta, dmask, dact, dslope);
  } else {
    const int nb = (int)std::min<int64_t>(vf_cdiv(total, 256), 4096);
    hipLaunchKernelGGL(k_slab_reduce, dim3(nb), dim3(256), 0, ctx->stream, slab, dst, bias, total, N, ksplit, act, slope, beta,
                       dmask, dact, dslope);
  }
  VF_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
struct WGrad {
  const float* U;   // plain operand at the LOW-res pixel grid: [P][Nu]
  const float* V;   // gathered operand on the HIGH-res grid: [B][Hv][Wv][Cv]
  float* dW;        // [Nu][16][Cv]
  float* slab;
  unsigned u_bytes, v_bytes;
  int P, lgMh, lgMw;
  int Nu, Cv, Hv, Wv;
  int stride, pad;  // iy = my*stride - pad + kh
  int ntaps;        // 16 (4x4 gather) or 1 (V already holds one K-row per pixel)
  int gx, gy, gz;   // logical grid (1-D launch, remapped per XCD)
  int ksplit, nk;   // nk = ceil(P/16)
  float beta;
};

// how a thread fetches its piece of the gathered operand V
enum WgV {
  WGV_SCALAR,   // four columns (tap, c), each with its own address and range test: any Cv
  WGV_VEC16,    // one 16-byte load: Cv % 4 == 0
  WGV_PIX3      // Cv == 3: one 12-byte load of a whole pixel.  The block's columns are col4 = 4 * tap + c with c = 3 a phantom
                // channel that is always zero, so the 16 taps fill a 64-column tile (BN = 64) and a thread owns one (pixel row, tap):
                // one (iy, ix), one range test and one address per piece, where the scalar form spends four of each on a 128-column
                // tile of which 48 columns exist
};
// BM over n (64 or 128); BN columns (tap,c): 128, or the 64 of WGV_PIX3.  VU: 16-byte loads legal for U; VV: the form of V's loads.
// BF: bf16-operand mode — U and V go into LDS as k-major bf16 tiles (one 8-byte store per piece), the fragments come
// out through the transposing read (vf_tr_frag) and the products run on v_mfma_f32_32x32x16_bf16, fp32 accumulation.
template <int BM, bool VU, WgV VV, int BF = 0, int BN = 128>
__device__ __forceinline__ void wgrad_body(const WGrad& p, const int block_id) {
  static_assert(VV == WGV_PIX3 ? (BN == 64 && BF != 0) : BN == 128, "the whole-pixel form is a 64-column tile of the bf16 modes");
  constexpr int BK = BF ? 32 : 16;                // bf16 mode: two 16-deep MFMA groups per barrier
  constexpr int LDU = BM + 4, LDV = BN + 4;
  // four waves.  BN = 128: 64 x 32 each side by side (BM = 64) or 64 x 64 as 2 x 2 (BM = 128); BN = 64: 2 x 2 waves of 32 x 32
  // (BM = 64) or 64 x 32 (BM = 128) — no wave holds columns that do not exist
  constexpr int WN = (BM == 128 && BN == 128) ? 64 : 32;
  constexpr int NT = WN / 32;
  constexpr int WAVES_N = BN / WN;
  constexpr int WM = BM / (4 / WAVES_N);
  constexpr int MT = WM / 32;
  constexpr int CQ = BN / 4;                 // threads across a V row (4 columns each); 256 / CQ pixel rows per piece
  constexpr int U_CH = (BK * BM / 4) / 256;  // 2 (BM=128) or 1 (BM=64)
  constexpr int V_CH = (BK * BN / 4) / 256;  // 2
  constexpr int U_SZ = BK * LDU, V_SZ = BK * LDV;
  constexpr int LDMU = BM + 32, LDMV = BN + 32;        // bf16 elements per k row (BF): k-major tiles, transposing reads
  constexpr int UH_SZ = BK * LDMU, VH_SZ = BK * LDMV;
  constexpr int NP = BF > 0 ? BF : 1;                  // bf16 planes per operand (3: exact split of the fp32 operands)
  constexpr int NBUF = BF == 3 ? 1 : 2;
  constexpr int PL_SZ = UH_SZ + VH_SZ;
  constexpr int SMEM_F = BF ? (NBUF * NP * PL_SZ + 1) / 2 : 2 * (U_SZ + V_SZ);
  __shared__ __attribute__((aligned(16))) float smem[SMEM_F];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave / WAVES_N) * WM, wn = (wave % WAVES_N) * WN;
  const int lid = vf_xcd_remap(block_id, p.gx * p.gy * p.gz);
  const int n0 = ((lid / p.gx) % p.gy) * BM, j0 = (lid % p.gx) * BN;
  const int ks = lid / (p.gx * p.gy);
  const int steps = (p.nk + p.ksplit - 1) / p.ksplit;
  const int kt0 = ks * steps, kt1 = min(p.nk, kt0 + steps);
  const int Ncols = p.ntaps * p.Cv;
  const int Mw = 1 << p.lgMw, Mh = 1 << p.lgMh;

  // V columns owned by this thread: 4 consecutive columns starting at j0 + 4*cq
  const int cq = tid % CQ, vrow = tid / CQ;
  int v_dy[4], v_dx[4], v_c[4];
  bool v_okc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = j0 + 4 * cq + j;
    v_okc[j] = col < Ncols;
    const int tap = v_okc[j] ? col / p.Cv : 0;
    v_c[j] = v_okc[j] ? col - tap * p.Cv : 0;
    v_dy[j] = (tap >> 2) - p.pad;
    v_dx[j] = (tap & 3) - p.pad;
  }
  const int uq = tid % (BM / 4), ukk = tid / (BM / 4);  // U: 4 consecutive n at pixel row ukk (+ 1024/BM per chunk)
  const int un = n0 + 4 * uq;

  f32x4 ru[U_CH], rv[V_CH];
  const __amdgpu_buffer_rsrc_t rsU = vf_rsrc(p.U, p.u_bytes), rsV = vf_rsrc(p.V, p.v_bytes);

  // one K step = U_CH + V_CH operand pieces (one 16-byte register each); `live` false turns a piece into a no-op load
  auto load_piece = [&](int kt, int pc, bool live) {
    if (pc < U_CH) {
      const int i = pc;
      const int pp = kt * BK + ukk + i * (1024 / BM);
      const bool okp = live && pp < p.P;
      if constexpr (VU) {
        ru[i] = vf_bload4(rsU, (okp && un < p.Nu) ? 4u * (unsigned)(pp * p.Nu + un) : VF_OOB);
      } else {
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] = vf_bload1(rsU, (okp && un + j < p.Nu) ? 4u * (unsigned)(pp * p.Nu + un + j) : VF_OOB);
        }
        ru[i] = v;
      }
    } else {
      const int i = pc - U_CH;
      const int pp = kt * BK + vrow + (256 / CQ) * i;
      const bool okp = live && pp < p.P;
      const int mx = pp & (Mw - 1), my = (pp >> p.lgMw) & (Mh - 1), b = pp >> (p.lgMw + p.lgMh);
      const int boff = b * p.Hv * p.Wv * p.Cv;
      if constexpr (VV == WGV_PIX3) {
        const int iy = my * p.stride + (cq >> 2) - p.pad, ix = mx * p.stride + (cq & 3) - p.pad;      // cq is the tap
        const bool ok = okp && (unsigned)iy < (unsigned)p.Hv && (unsigned)ix < (unsigned)p.Wv;
        rv[i] = vf_bload3(rsV, ok ? 4u * (unsigned)(boff + (iy * p.Wv + ix) * 3) : VF_OOB);
      } else if constexpr (VV == WGV_VEC16) {
        const int iy = my * p.stride + v_dy[0], ix = mx * p.stride + v_dx[0];
        const bool ok = okp && v_okc[0] && (unsigned)iy < (unsigned)p.Hv && (unsigned)ix < (unsigned)p.Wv;
        rv[i] = vf_bload4(rsV, ok ? 4u * (unsigned)(boff + (iy * p.Wv + ix) * p.Cv + v_c[0]) : VF_OOB);
      } else {
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int iy = my * p.stride + v_dy[j], ix = mx * p.stride + v_dx[j];
          const bool ok = okp && v_okc[j] && (unsigned)iy < (unsigned)p.Hv && (unsigned)ix < (unsigned)p.Wv;
          v[j] = vf_bload1(rsV, ok ? 4u * (unsigned)(boff + (iy * p.Wv + ix) * p.Cv + v_c[j]) : VF_OOB);
        }
        rv[i] = v;
      }
    }
  };
  auto store_piece = [&](int buf, int pc) {
    if constexpr (BF) {
      __bf16* base = (__bf16*)smem + buf * (NP * PL_SZ);
      f32x4 v;
      int off;
      if (pc < U_CH) {
        v = ru[pc];
        off = (ukk + pc * (1024 / BM)) * LDMU + 4 * uq;
      } else {
        const int i = pc - U_CH;
        v = rv[i];
        off = UH_SZ + (vrow + (256 / CQ) * i) * LDMV + 4 * cq;
      }
      if constexpr (NP == 3) {
        u32x2 s3[3];
        vf_split3(v, s3);
#pragma unroll
        for (int q = 0; q < 3; ++q) *(u32x2*)(base + q * PL_SZ + off) = s3[q];
      } else {
        *(bf16x4*)(base + off) = __builtin_convertvector(v, bf16x4);
      }
      return;
    }
    float* Us = smem + buf * (U_SZ + V_SZ);
    float* Vs = Us + U_SZ;
    if (pc < U_CH) {
      *(f32x4*)(Us + (ukk + pc * (1024 / BM)) * LDU + 4 * uq) = ru[pc];
    } else {
      const int i = pc - U_CH;
      *(f32x4*)(Vs + (vrow + (256 / CQ) * i) * LDV + 4 * cq) = rv[i];
    }
  };
  constexpr int NPC = U_CH + V_CH;
  auto load_tile = [&](int kt) {
#pragma unroll
    for (int pc = 0; pc < NPC; ++pc) load_piece(kt, pc, true);
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int pc = 0; pc < NPC; ++pc) store_piece(buf, pc);
  };

  f32x16 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
  const int lr = lane & 31, lh = lane >> 5;

  if (kt0 < kt1) {
    load_tile(kt0);
    store_tile(0);
  }
  __syncthreads();
  if constexpr (BF) {
    for (int kt = kt0; kt < kt1; ++kt) {
      const int buf = NBUF == 2 ? ((kt - kt0) & 1) : 0;
      const bool more = kt + 1 < kt1;
      const __bf16* base = (const __bf16*)smem + buf * (NP * PL_SZ);
#pragma unroll
      for (int pc = 0; pc < NPC; ++pc) load_piece(kt + 1, pc, more);
#pragma unroll
      for (int g = 0; g < BK / 16; ++g) {
        bf16x8 a[NP][MT], b[NP][NT];
#pragma unroll
        for (int q = 0; q < NP; ++q) {
          const __bf16* Uh = base + q * PL_SZ;
          const __bf16* Vh = Uh + UH_SZ;
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) a[q][mt] = vf_tr_frag<LDMU>(Uh, wm + mt * 32, 16 * g, lane);
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) b[q][nt] = vf_tr_frag<LDMV>(Vh, wn + nt * 32, 16 * g, lane);
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            if constexpr (NP == 3) {
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][mt], b[1][nt], acc[mt][nt], 0, 0, 0);
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][mt], b[2][nt], acc[mt][nt], 0, 0, 0);
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2][mt], b[0][nt], acc[mt][nt], 0, 0, 0);
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][mt], b[1][nt], acc[mt][nt], 0, 0, 0);
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][mt], b[0][nt], acc[mt][nt], 0, 0, 0);
            }
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][mt], b[0][nt], acc[mt][nt], 0, 0, 0);
          }
      }
      if constexpr (NBUF == 1) __syncthreads();
      store_tile(NBUF == 2 ? (buf ^ 1) : 0);
      __syncthreads();
    }
  } else {
  static_assert(BF != 0 || MT == 2, "the fp32 schedule below is written for two row fragments per wave");
  constexpr int NMF = 4 * 2 * NT;              // MFMAs per 8-wide sub-step
  constexpr int SLOTS = 2 * NMF;               // MFMA slots per K step (BK = 16)
  static_assert(2 * NPC <= SLOTS, "loads and LDS writes of one K step must fit between its MFMAs");
  for (int kt = kt0; kt < kt1; ++kt) {
    const int buf = (kt - kt0) & 1;
    const bool more = kt + 1 < kt1;
    const float* Us = smem + buf * (U_SZ + V_SZ);
    const float* Vs = Us + U_SZ;
    // same pinned schedule as k_igemm: fragment reads one sub-step ahead; MFMA slot i < NPC is followed by operand
    // piece i of step kt+1, the last NPC slots by the register -> LDS writes into the other buffer
    auto read_frag = [&](int ss, float (&a)[2][4], float (&b)[NT][4]) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = 8 * ss + 4 * lh + j;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) a[mt][j] = Us[k * LDU + wm + mt * 32 + lr];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) b[nt][j] = Vs[k * LDV + wn + nt * 32 + lr];
      }
    };
    float fa[2][2][4], fb[2][NT][4];
    read_frag(0, fa[0], fb[0]);
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
      if (ss == 0) read_frag(1, fa[1], fb[1]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[ss][mt][j], fb[ss][nt][j], acc[mt][nt], 0, 0, 0);
            const int slot = ss * NMF + (j * 2 + mt) * NT + nt;
            if (slot < NPC) load_piece(kt + 1, slot, more);
            if (slot >= SLOTS - NPC) store_piece(buf ^ 1, slot - (SLOTS - NPC));
            __builtin_amdgcn_sched_barrier(0);
          }
    }
    __syncthreads();
  }

  }
  const int64_t total = (int64_t)p.Nu * Ncols;
  float* out = p.ksplit > 1 ? p.slab + (int64_t)ks * total : p.dW;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = n0 + wm + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (n >= p.Nu) continue;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        int col = j0 + wn + nt * 32 + lr;
        bool okc = col < Ncols;
        if constexpr (VV == WGV_PIX3) {      // col4 = 4 * tap + c -> 3 * tap + c; the phantom channel has no element
          okc = (col & 3) != 3;
          col = 3 * (col >> 2) + (col & 3);
        }
        if (okc) {
          const int64_t idx = (int64_t)n * Ncols + col;
          float v = acc[mt][nt][r];
          if (p.ksplit == 1 && p.beta != 0.f) v += p.beta * out[idx];
          out[idx] = v;
        }
      }
    }
}

template <int BM, bool VU, WgV VV, int BF = 0>
__global__ __launch_bounds__(256) void k_wgrad(const WGrad p) {
  wgrad_body<BM, VU, VV, BF, VV == WGV_PIX3 ? 64 : 128>(p, blockIdx.x);
}

// Every weight gradient of a backward walk in ONE launch: dW_l needs only (input_l, gradOutput_l), both of which stay in
// their modules' buffers until the walk is over, so the GEMMs are recorded during the walk and launched together —
// one ramp and one tail instead of one per layer (each 512-block launch is a single round of blocks), and the
// descriptor table travels by value in the kernel arguments (no device table, nothing to keep in sync under a graph).
#define VF_WG_GROUP_MAX 16
struct WGradGroup {
  int n;
  int blk_off[VF_WG_GROUP_MAX + 1];   // multiples of 8: the XCD-aware tile order of a layer assumes blockIdx % 8 == local id % 8
  WGrad d[VF_WG_GROUP_MAX];
};
static_assert(sizeof(WGradGroup) <= 3584, "kernel arguments are limited to 4 KB");
template <int BM, bool VU, WgV VV, int BF>
__global__ __launch_bounds__(256) void k_wgrad_group(const WGradGroup G) {
  int l = 0;
  while (l + 1 < G.n && (int)blockIdx.x >= G.blk_off[l + 1]) ++l;
  const int local = (int)blockIdx.x - G.blk_off[l];
  if (local >= G.d[l].gx * G.d[l].gy * G.d[l].gz) return;      // padding blocks (uniform exit)
  wgrad_body<BM, VU, VV, BF>(G.d[l], local);
}
struct SlabGroup {
  int n;
  int blk_off[VF_WG_GROUP_MAX + 1];
  struct { const float* slab; float* dst; int64_t total4; int ksplit; float beta; } d[VF_WG_GROUP_MAX];
};
__global__ __launch_bounds__(256) void k_slab_reduce4_group(const SlabGroup G) {
  int l = 0;
  while (l + 1 < G.n && (int)blockIdx.x >= G.blk_off[l + 1]) ++l;
  const int tx = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int64_t i4 = (int64_t)((int)blockIdx.x - G.blk_off[l]) * 64 + tx;
  const int64_t total4 = G.d[l].total4;
  const int ksplit = G.d[l].ksplit;
  const float* slab = G.d[l].slab;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (i4 < total4) {
#pragma unroll 4
    for (int k = sl; k < ksplit; k += 4) s += ((const f32x4*)slab)[(int64_t)k * total4 + i4];
  }
  __shared__ f32x4 red[4][64];
  red[sl][tx] = s;
  __syncthreads();
  if (sl == 0 && i4 < total4) {
    f32x4 t = ((red[0][tx] + red[1][tx]) + red[2][tx]) + red[3][tx];
    f32x4* dst = (f32x4*)G.d[l].dst;
    if (G.d[l].beta != 0.f) t += G.d[l].beta * dst[i4];
    dst[i4] = t;
  }
}

// ------------------------------------------------------------------------------------------------
// Cout == 1, 4x4 stride-1 conv on a 4x4 map (netD's last layer, train.lua:195): dot products.
__global__ __launch_bounds__(256) void k_dot_fwd(const float* __restrict__ x, const float* __restrict__ w,
                                                 const float* __restrict__ bias, float* __restrict__ y, int K, int act,
                                                 float slope) {
  // one block per sample: 16-byte loads, four independent partial sums per thread, wave shuffle tree, 4 waves via LDS
  const int b = blockIdx.x;
  const float* xb = x + (int64_t)b * K;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if ((K & 3) == 0) {
    for (int k = 4 * threadIdx.x; k < K; k += 1024) {
      const f32x4 xv = *(const f32x4*)(xb + k), wv = *(const f32x4*)(w + k);
      acc[0] += xv[0] * wv[0];
      acc[1] += xv[1] * wv[1];
      acc[2] += xv[2] * wv[2];
      acc[3] += xv[3] * wv[3];
    }
  } else {
    for (int k = threadIdx.x; k < K; k += 256) acc[0] += xb[k] * w[k];
  }
  float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) y[b] = vf_act_apply(((red[0] + red[1]) + (red[2] + red[3])) + (bias ? bias[0] : 0.f), act, slope);
}
// ya != NULL: gy is the gradient w.r.t. the ACTIVATED output ya (the Sigmoid fused into this conv): its derivative rides here
__global__ void k_dot_bwd_data(const float* __restrict__ gy, const float* __restrict__ w, float* __restrict__ gx, int B,
                               int K, const float* __restrict__ ya, int act, float slope) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < (int64_t)B * K) {
    const int64_t b = i / K;
    const float g = ya ? vf_act_grad(ya[b], gy[b], act, slope) : gy[b];
    gx[i] = g * w[i % K];
  }
}
// gw[k] = beta*gw[k] + sum_b gy[b]*x[b][k]: a block owns 64 columns; its 8 waves take every 8th sample (coalesced 256-byte rows),
// eight samples in flight per wave, partials meet in LDS in a fixed order.  The per-sample factor (gy, times the derivative of a
// fused activation: see k_dot_bwd_data) is formed once per block, in LDS.  (One thread per column walking all B samples was a 64-deep
// dependent load chain on 32 blocks: 19 us for 2 MB; four waves with two sums in flight each still took 22 us at batch 128 — every
// iteration waited for its row AND for two scalar loads in front of it.)
__global__ __launch_bounds__(512) void k_dot_bwd_weight(const float* __restrict__ x, const float* __restrict__ gy,
                                                        float* __restrict__ gw, float* __restrict__ gb, int B, int K,
                                                        float beta, const float* __restrict__ ya, int act, float slope) {
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int k = blockIdx.x * 64 + lane;
  __shared__ float g[1024];
  __shared__ float red[8][64];
  float acc = 0.f;
  for (int b0 = 0; b0 < B; b0 += 1024) {                 // (B <= 1024 in every net: one pass)
    const int nb = min(1024, B - b0);
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += 512) g[b] = ya ? vf_act_grad(ya[b0 + b], gy[b0 + b], act, slope) : gy[b0 + b];
    __syncthreads();
    if (k < K) {
      const float* xp = x + (int64_t)b0 * K + k;
      int b = grp;
      for (; b + 56 < nb; b += 64) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = xp[(int64_t)(b + 8 * j) * K];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += g[b + 8 * j] * v[j];
      }
      for (; b < nb; b += 8) acc += g[b] * xp[(int64_t)b * K];
    }
  }
  red[grp][lane] = acc;
  __syncthreads();
  if (grp == 0 && k < K) {
    const float t = ((red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane])) + ((red[4][lane] + red[5][lane]) + (red[6][lane] + red[7][lane]));
    gw[k] = (beta != 0.f ? beta * gw[k] : 0.f) + t;
  }
  if (gb && blockIdx.x == 0 && threadIdx.x == 0) {
    float t = 0.f;
    for (int b = 0; b < B; ++b) t += ya ? vf_act_grad(ya[b], gy[b], act, slope) : gy[b];
    gb[0] = (beta != 0.f ? beta * gb[0] : 0.f) + t;
  }
}

// ------------------------------------------------------------------------------------------------
// Thin-output transposed passes (image side of the nets: N = 3, 12 ...: netG's last full-conv, netD's first-layer
// data-grad).  A 32-wide MFMA tile would be >60% padding there, so the pass runs as a plain GEMM to a column matrix
//   cols[B*Hi*Wi][16*N] = A[pixel][:] . W[:][(kh,kw,n)]        (the [c][kh][kw][n] weights ARE that [C][16N] matrix)
// followed by k_col2im4x4, in which every output pixel gathers its 4 taps (+bias, activation).  Measured 98 -> 30 us.
// (The mirror-image trick for thin INPUTS — im2col then GEMM — was measured slower than the scalar-gather path of
// k_igemm<V=0> for these K = 48 problems and is not used.)
__global__ __launch_bounds__(256) void k_col2im4x4(const float* __restrict__ cols, const float* __restrict__ bias,
                                                   float* __restrict__ y, int B, int lgHi, int lgWi, int N, int act, float slope) {
  // stride 2, pad 1: output (oh, ow) = (2i-1+kh, 2j-1+kw)  =>  kh = (oh+1) & 1 + 2*th, i = (oh+1-kh)/2
  const int Hi = 1 << lgHi, Wi = 1 << lgWi;
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t total = ((int64_t)B << (lgHi + lgWi + 2)) * N;
  if (t >= total) return;
  const int n = (int)(t % N);
  const int64_t pix = t / N;
  const int ow = (int)(pix & (2 * Wi - 1)), oh = (int)((pix >> (lgWi + 1)) & (2 * Hi - 1)), b = (int)(pix >> (lgWi + lgHi + 2));
  float s = bias ? bias[n] : 0.f;
#pragma unroll
  for (int th = 0; th < 2; ++th) {
    const int kh = ((oh + 1) & 1) + 2 * th, i = (oh + 1 - kh) >> 1;
    if ((unsigned)i >= (unsigned)Hi) continue;
#pragma unroll
    for (int tw = 0; tw < 2; ++tw) {
      const int kw = ((ow + 1) & 1) + 2 * tw, j = (ow + 1 - kw) >> 1;
      if ((unsigned)j >= (unsigned)Wi) continue;
      s += cols[((((int64_t)b << lgHi) + i) * Wi + j) * (16 * N) + (kh * 4 + kw) * N + n];
    }
  }
  y[t] = vf_act_apply(s, act, slope);
}

// ================================================================================================ host
// ---- the plan of one k_igemm pass: vector form, tile, split over K, the kernel form that serves it, what the profiler is told.
// One enumerator per kernel form; DESIGN.md 4.1 is read from ig_plan() below.
enum IgRoute {
  IG_TILE,              // k_igemm on the planned tile
  IG_TILE_KLIN,         //   ... K walked in memory order: the 64 x 128 tile of the 1x1-output bottleneck layers
  IG_TILE_DB,           //   ... the double-buffered schedule: mode 3's 64 x 64 tile on grids of at most two blocks per CU
  IG_SMALLM_ROWS,       // the bottleneck GEMMs at a small batch: vf_smallm.hip's weight-streaming kernel, weight rows of K floats
  IG_SMALLM_KMAJOR      //   ... weights [C][N], N contiguous
};
struct IgPlan {
  bool bkm;                    // B operand k-major (the transposed passes)
  int64_t a_elems, w_elems;
  int v, nq, nk, Ktot;         // vector form (k_igemm's V), 16-wide chunks, K steps, K
  int bm, bn;                  // block tile
  int ksplit, gm, gn, gz;
  bool klin, db;
  IgRoute route;
  VfBnStPlan stats;             // BatchNorm statistics as a by-product: from the epilogue, or from the slab reduce under split-K
  dim3 grid;
  char name[64];               // one name per kernel symbol (what rocprofv3 lists): k_igemm<bm, bn, ., ., kmajorB, v, mode>
  double flops, bytes;
  bool in_range() const { return a_elems < ((int64_t)1 << 29) && w_elems < ((int64_t)1 << 29); }      // a buffer descriptor spans 2 GiB
  bool smallm() const { return route == IG_SMALLM_ROWS || route == IG_SMALLM_KMAJOR; }
};
// g: the geometry; vecA / vecB: 16-byte loads legal for the A / B operand; mode: the product mode; req: the pending BatchNorm
// request, or NULL.  Launches nothing and writes nothing: launch_igemm takes the plan into `g` and the caller's extras.
static IgPlan ig_plan(const IGemm& g, bool vecA, bool vecB, int mode, size_t ws_avail, const VfBnRequest* req) {
  IgPlan p;
  const int zpar = g.parity ? 4 : 1;
  p.bkm = g.wsN == 1 && g.wsC != 1;
  p.a_elems = (int64_t)(g.M >> (g.lgMh + g.lgMw)) * g.Hi * g.Wi * g.C;
  p.w_elems = p.bkm ? (int64_t)g.C * g.wsC : (int64_t)g.N * g.wsN;
  p.v = (vecA && vecB) ? 2 : ((vecA && p.bkm) ? 1 : 0);
  p.Ktot = g.TH * g.TW * g.C;
  p.nq = g.TH * g.TW * (g.C / 16);
  p.nk = p.v >= 1 ? (p.nq + 1) / 2 : (int)vf_cdiv(p.Ktot, 32);
  // ---- tile selection: the largest tile that still gives >= 2 blocks per CU, else the smallest + split-K
  struct Tile { int bm, bn; };
  Tile t;
  if (g.N <= 32) {
    t = {256, 32};
  } else if (g.M <= 64) {
    t = {64, 128};
  } else {
    const Tile cand[3] = {{128, 128}, {128, 64}, {64, 64}};
    // mode 3's single-buffered three-plane tiles hide their two barriers per K step with co-resident blocks: they want
    // twice the blocks (measured: +2 % per step at 1024 and above)
    const int min_blocks = mode == 3 ? 1024 : 512;
    int pick = 2;
    for (int i = 0; i < 3; ++i) {
      if (cand[i].bn > 64 && g.N <= 64) continue;
      // a short K loop (<= 8 steps: the 64-channel transposed passes) leaves a 128-row block mostly prologue and
      // epilogue; four 64x64 blocks per CU cover each other's ends better (E2 data-gradient: 122 -> 112 us)
      if (g.parity && p.nk <= 8 && cand[i].bm > 64) continue;
      const int64_t blocks = vf_cdiv(g.M, cand[i].bm) * vf_cdiv(g.N, cand[i].bn) * zpar;
      if (blocks >= min_blocks) {
        pick = i;
        break;
      }
    }
    t = cand[pick];
    // (tried: 256 x 64 tiles — four 64x64 wave tiles stacked in M, one block per CU — for the N = 64 layers: 153 us
    //  against 125 us for E2's data-gradient; one wave per SIMD does not cover its own LDS/global latency)
  }
  p.bm = t.bm; p.bn = t.bn;
  constexpr int split_blocks = 512;     // (768 for the M <= 64 GEMMs: a wash)
  p.gm = (int)vf_cdiv(g.M, t.bm);
  p.gn = (int)vf_cdiv(g.N, t.bn);
  const int64_t blocks = (int64_t)p.gm * p.gn * zpar;
  p.ksplit = vf_split_k(blocks, split_blocks, p.nk, 8, 4, (size_t)g.out_elems * sizeof(float), ws_avail, VF_K_EVEN_OUT);
  // ---- the bottleneck GEMMs at a small batch (M <= 8 rows against hundreds of MB of weights): a weight-streaming kernel instead
  // of a tile (vf_smallm.hip); it leaves split-K slabs, which the combine takes like the tiled kernel's
  int sm_form = -1;
  if (!g.parity && g.lgMh == 0 && g.lgMw == 0 && g.M <= 8 && p.v == 2) {
    if (!p.bkm && g.Hi == g.TH && g.Wi == g.TW && g.oy0 == 0 && g.ox0 == 0 && g.sy == 1 && g.sx == 1 && g.ty == 1 && g.tx == 1 && g.wsC == 1 &&
        g.wsTap == g.C && g.wsN == p.Ktot && g.kh0 == 0 && g.kw0 == 0 && g.khs == 1 && g.kws == 1)
      sm_form = 0;        // A rows and weight rows are K = taps * C contiguous floats
    else if (p.bkm && g.TH * g.TW == 1 && g.Hi == 1 && g.Wi == 1 && g.wsC == g.N)
      sm_form = 1;        // weights [C][N], N contiguous
    if (sm_form >= 0) {
      const int s = vf_internal_smallm_plan(sm_form, g.M, g.N, p.Ktot, ws_avail);
      if (s >= 2) p.ksplit = s;
      else sm_form = -1;
    }
  }
  p.stats = vf_plan_bn_stats(req, g, p.ksplit, t.bm, p.gm, zpar);
  p.klin = !g.parity && g.lgMh == 0 && g.lgMw == 0 && g.TH * g.TW > 1 && t.bm == 64 && t.bn == 128 && !p.bkm && p.v == 2;
  p.gz = zpar * p.ksplit;
  p.grid = dim3((unsigned)p.gm * p.gn * zpar * p.ksplit);
  // double-buffered schedule: where the grid leaves at most two blocks per CU anyway (its 66 KB tiles cost nothing then)
  p.db = mode == 3 && p.v == 2 && t.bm == 64 && t.bn == 64 && (int64_t)p.grid.x <= 2 * 256;
  p.route = sm_form == 0 ? IG_SMALLM_ROWS : sm_form == 1 ? IG_SMALLM_KMAJOR : p.db ? IG_TILE_DB : p.klin ? IG_TILE_KLIN : IG_TILE;
  snprintf(p.name, sizeof(p.name), "igemm_%dx%d_%s_v%d%s%s", t.bm, t.bn, p.bkm ? "kmajorB" : "rowB", p.v,
           mode == 3 ? "_bf16x3" : (mode ? "_bf16" : ""), p.db ? "_db" : "");
  p.flops = 2.0 * (double)g.M * g.N * p.Ktot * zpar;
  // algorithmic bytes: both operands and the output once (small-batch passes over the bottleneck weights are bounded by these,
  // not by the matrix pipe: bench.py prices a kernel against whichever of its two rooflines is the longer)
  p.bytes = 4.0 * (double)p.a_elems + 4.0 * (double)p.w_elems + 4.0 * (double)g.out_elems;
  return p;
}

// route -> kernel: every k_igemm instantiation the library holds, keyed by what ig_plan decides.  Per tile and product mode:
// row-major B at V = 2 / 0 and k-major B at V = 2 / 1 / 0; besides them the K-in-memory-order form of the 64 x 128 tile and the
// double-buffered form of mode 3's 64 x 64 tile.  (Wave tiles: four waves of 32 x 32 MFMA tiles per block.)
typedef void (*IgKernel)(IGemm);
struct IgEntry {
  int bm, bn, mode;
  IgRoute route;
  bool bkm;
  int v;
  IgKernel kernel;
};
#define IG_TILE_ROWS(BM, BN, WM, WN, BF)                                    \
  {BM, BN, BF, IG_TILE, false, 2, k_igemm<BM, BN, WM, WN, false, 2, BF>},   \
  {BM, BN, BF, IG_TILE, false, 0, k_igemm<BM, BN, WM, WN, false, 0, BF>},   \
  {BM, BN, BF, IG_TILE, true, 2, k_igemm<BM, BN, WM, WN, true, 2, BF>},     \
  {BM, BN, BF, IG_TILE, true, 1, k_igemm<BM, BN, WM, WN, true, 1, BF>},     \
  {BM, BN, BF, IG_TILE, true, 0, k_igemm<BM, BN, WM, WN, true, 0, BF>}
#define IG_KLIN_ROW(BF) {64, 128, BF, IG_TILE_KLIN, false, 2, k_igemm<64, 128, 64, 32, false, 2, BF, true>}
static const IgEntry ig_table[] = {
    IG_TILE_ROWS(256, 32, 64, 32, 3), IG_TILE_ROWS(256, 32, 64, 32, 1), IG_TILE_ROWS(256, 32, 64, 32, 0),
    IG_TILE_ROWS(128, 128, 64, 64, 3), IG_TILE_ROWS(128, 128, 64, 64, 1), IG_TILE_ROWS(128, 128, 64, 64, 0),
    IG_TILE_ROWS(128, 64, 64, 32, 3), IG_TILE_ROWS(128, 64, 64, 32, 1), IG_TILE_ROWS(128, 64, 64, 32, 0),
    IG_KLIN_ROW(3), IG_TILE_ROWS(64, 128, 64, 32, 3), IG_KLIN_ROW(1), IG_TILE_ROWS(64, 128, 64, 32, 1),
    IG_KLIN_ROW(0), IG_TILE_ROWS(64, 128, 64, 32, 0),
    {64, 64, 3, IG_TILE_DB, false, 2, k_igemm<64, 64, 32, 32, false, 2, 3, false, true>},
    {64, 64, 3, IG_TILE_DB, true, 2, k_igemm<64, 64, 32, 32, true, 2, 3, false, true>},
    IG_TILE_ROWS(64, 64, 32, 32, 3), IG_TILE_ROWS(64, 64, 32, 32, 1), IG_TILE_ROWS(64, 64, 32, 32, 0),
};
#undef IG_TILE_ROWS
#undef IG_KLIN_ROW
// NULL where the table holds no such row (a plan that ig_plan does not make): the launch then fails its check
static IgKernel ig_kernel(const IgPlan& p, int mode) {
  for (const IgEntry& e : ig_table)
    if (e.bm == p.bm && e.bn == p.bn && e.mode == (mode == 3 ? 3 : mode ? 1 : 0) && e.route == p.route && e.bkm == p.bkm && e.v == p.v)
      return e.kernel;
  return nullptr;
}

// ex: the extras of the pass whose output tensor this launch writes (BatchNorm statistics: vf_plan_bn_stats); NULL for an inner
// GEMM into a column buffer.
static int launch_igemm(vf_ctx* ctx, IGemm& g, bool vecA, bool vecB, VfConvExtras* ex) {
  const IgPlan p = ig_plan(g, vecA, vecB, ctx->mfma_bf16, vf_ws_avail(ctx), ex ? &ex->bn : nullptr);
  VF_REQUIRE(p.in_range(), "operand exceeds the 2 GiB buffer-descriptor range");
  g.a_bytes = (unsigned)(p.a_elems * 4);
  g.w_bytes = (unsigned)(p.w_elems * 4);
  g.nq = p.nq; g.nk = p.nk;
  g.ksplit = p.ksplit;
  g.slab = p.ksplit > 1 ? (float*)vf_ws_ptr(ctx) : nullptr;
  g.klin = p.klin;
  g.gm = p.gm; g.gn = p.gn; g.gz = p.gz;
  vf_take_bn_stats(p.stats, g, ex);
  if (p.smallm()) {
    if (int rc = vf_internal_smallm_launch(ctx, p.route == IG_SMALLM_ROWS ? 0 : 1, g.A, g.Wt, g.slab, g.M, g.N, p.Ktot, p.ksplit)) return rc;
  } else {
    VF_LAUNCH_TIMED(ctx, p.name, p.flops, p.bytes, ig_kernel(p, ctx->mfma_bf16), p.grid, dim3(256), g);
  }
  VF_LAUNCH_CHECK();
  return vf_combine_slabs(ctx, "igemm", g, p.stats.slab, p.stats.slab ? ex->bn.groups : 1);
}

// the split-K combine for vf_pgemm.hip's launches (plain, or leaving BatchNorm statistics partials)
bool vf_internal_slab_st_ok(int64_t total, int N, int groups, int rows_cap, int* blocks_per_group) {
  int upb = 0, ncc = 0;
  int64_t units = 0;
  return total % 4 == 0 && slab_st_plan(total, N, groups, rows_cap, &upb, blocks_per_group, &ncc, &units);
}
int vf_internal_slab_reduce(vf_ctx* ctx, const float* slab, float* dst, const float* bias, int64_t total, int N, int ksplit, int act,
                            float slope, const float* dmask, int dact, float dslope, const VfBnSt* st, int st_groups) {
  if (st) {
    int upb = 0, bpg = 0, ncc = 0;
    int64_t units = 0;
    VF_REQUIRE(total % 4 == 0 && slab_st_plan(total, N, st_groups, st->rows_per_group, &upb, &bpg, &ncc, &units) && bpg == st->rows_per_group,
               "vf_internal_slab_reduce: the statistics plan changed between the GEMM and its combine");
    hipLaunchKernelGGL(k_slab_reduce_st, dim3((unsigned)(bpg * st_groups), (unsigned)ncc), dim3(256), 0, ctx->stream, slab, dst, bias,
                       total / 4, N, ksplit, act, slope, dmask, dact, dslope, upb, units, ncc, *st);
    VF_LAUNCH_CHECK();
    return 0;
  }
  return launch_slab_reduce(ctx, slab, dst, bias, total, N, ksplit, act, slope, 0.f, dmask, dact, dslope);
}

// ---- BatchNorm statistics request (VfBnRequest).  The public protocol: vf_bn_fuse_next_* leave one in the context, the next
// forward / data-gradient entry point takes it, unconditionally (vf_take_pending), vf_bn_fuse_result reads what it made of it.
int vf_internal_bn_request_fwd(VfBnRequest* r, const float* shift, double* part, int part_rows_cap, int groups) {
  VF_REQUIRE(shift && part && part_rows_cap > 0 && groups >= 1 && groups <= 64, "vf_bn_fuse_next_fwd: bad arguments");
  *r = VfBnRequest();
  r->st.mode = 1;
  r->st.vec = shift;
  r->st.part = part;
  r->groups = groups;
  r->rows_cap = part_rows_cap / groups;
  return 0;
}
int vf_internal_bn_request_bwd(VfBnRequest* r, const float* x, const float* y_act, int act, float slope, const float* save_mean,
                               double* part, int part_rows_cap, int groups) {
  VF_REQUIRE(x && save_mean && part && part_rows_cap > 0 && groups >= 1 && groups <= 64, "vf_bn_fuse_next_bwd: bad arguments");
  VF_REQUIRE(act == VF_ACT_NONE || y_act != nullptr, "vf_bn_fuse_next_bwd: the activation derivative needs the activated output");
  *r = VfBnRequest();
  r->st.mode = 2;
  r->st.vec = save_mean;
  r->st.x = x;
  r->st.part = part;
  r->yact = act == VF_ACT_NONE ? nullptr : y_act;
  r->act = act;
  r->slope = slope;
  r->groups = groups;
  r->rows_cap = part_rows_cap / groups;
  return 0;
}
VF_API int vf_bn_fuse_next_fwd(vf_ctx* ctx, const float* shift, double* part, int part_rows_cap, int groups) {
  if (int rc = vf_internal_bn_request_fwd(&ctx->bn_pending, shift, part, part_rows_cap, groups)) return rc;
  ctx->bn_result_rows = 0;
  return 0;
}
VF_API int vf_bn_fuse_next_bwd(vf_ctx* ctx, const float* x, const float* y_act, int act, float slope, const float* save_mean,
                               double* part, int part_rows_cap, int groups) {
  if (int rc = vf_internal_bn_request_bwd(&ctx->bn_pending, x, y_act, act, slope, save_mean, part, part_rows_cap, groups)) return rc;
  ctx->bn_result_rows = 0;
  return 0;
}
VF_API int vf_bn_fuse_result(vf_ctx* ctx, int* rows_per_group) {
  VF_REQUIRE(rows_per_group != nullptr, "vf_bn_fuse_result: NULL");
  *rows_per_group = ctx->bn_result_rows;
  ctx->bn_result_rows = 0;
  ctx->bn_pending.st.mode = 0;      // a request no entry point took does not linger
  return 0;
}

static int check_conv_args(const VfConvShape& s) {
  VF_REQUIRE(s.k == 4, "only 4x4 kernels are built by the reference (got k=%d)", s.k);
  VF_REQUIRE((s.stride == 2 && s.pad == 1) || (s.stride == 1 && s.pad == 0), "unsupported stride/pad %d/%d", s.stride, s.pad);
  VF_REQUIRE(s.B > 0 && s.Cin > 0 && s.Cout > 0, "bad sizes B=%d Cin=%d Cout=%d", s.B, s.Cin, s.Cout);
  VF_REQUIRE(s.pow2_map(), "spatial sizes must be powers of two (got %dx%d)", s.H, s.W);
  if (s.stride == 1) VF_REQUIRE(s.H >= 4 && s.W >= 4, "4x4 stride-1 conv needs H,W >= 4");
  if (s.stride == 2) VF_REQUIRE(s.H >= 2 && s.W >= 2, "stride-2 conv needs H,W >= 2");
  VF_REQUIRE((int64_t)s.Cin * s.Cout * 16 < ((int64_t)1 << 31), "weight tensor too large for 32-bit element offsets");
  return 0;
}
static int check_full_conv_args(const VfConvShape& s) {
  VF_REQUIRE(s.main_net_taps(), "unsupported full-conv shape");
  VF_REQUIRE(s.pow2_map(), "spatial sizes must be powers of two");
  return 0;
}

// ---- which pass serves a layer in front of (or instead of) the GEMM.  The thin kernels (vf_conv_thin.hip) decline by return
// value (< 0): where `route` is one of them, `fallback` is what serves the pass if it declines (else fallback == route).
enum GaRoute {          // gather passes: conv forward, full-conv data-gradient
  GA_DOT_HEAD,          // the 512 -> 1 head on its 4 x 4 map: k_dot_fwd
  GA_THIN_IN,           // the 3-channel image side: vf_internal_conv_thin_fwd
  GA_GEMM               // k_igemm over the 16 taps
};
struct GaPlan {
  GaRoute route, fallback;
};
// s: the pass as a conv (k = 4); conv_entry: the conv forward entry (the only one the thin-input kernel serves); stats: a BatchNorm
// request is pending
static GaPlan ga_plan(const VfConvShape& s, bool conv_entry, bool stats) {
  GaPlan p;
  p.fallback = s.Cout == 1 && s.stride == 1 && s.H == 4 && s.W == 4 ? GA_DOT_HEAD : GA_GEMM;
  p.route = conv_entry && s.stride == 2 && s.Cin == 3 && !stats ? GA_THIN_IN : p.fallback;
  return p;
}
enum TrRoute {          // transposed passes: conv data-gradient, full-conv forward
  TR_DOT_HEAD,          // the data-gradient of the 512 -> 1 head: k_dot_bwd_data
  TR_THIN_OUT,          // the image side (at most 4 output channels): vf_internal_deconv_thin_out
  TR_COL2IM,            // thin output: a column-buffer GEMM in the workspace, then k_col2im4x4
  TR_PARITY_GEMM,       // k_igemm, four output-parity classes of 2 x 2 taps each
  TR_GEMM_1X1           // 1 x 1 -> 4 x 4: a plain GEMM, with a pointwise bias pass behind it where there is a bias
};
struct TrPlan {
  TrRoute route, fallback;
  size_t col_bytes;     // TR_COL2IM: the column buffer
};
// s: the pass as a full-conv (k = 4), A on its H x W map; vecA / alignedW: 16-byte loads of A are legal, w is 16-byte aligned;
// mask / stats: a derivative mask, a pending BatchNorm request; ws_front / ws_bytes: the workspace's held front and size;
// conv_grad: the pass is a conv's data-gradient (the head's among them: one gradOutput channel on a 1 x 1 map)
static TrPlan tr_plan(const VfConvShape& s, bool vecA, bool alignedW, bool mask, bool stats, size_t ws_front, size_t ws_bytes,
                      bool conv_grad) {
  TrPlan p;
  p.col_bytes = 0;
  if (conv_grad && s.stride == 1 && s.Cin == 1) {
    p.route = p.fallback = TR_DOT_HEAD;
    return p;
  }
  p.col_bytes = (size_t)s.B * s.H * s.W * 16 * s.Cout * sizeof(float);
  const bool cols = s.stride == 2 && s.Cout < 32 && vecA && alignedW && ws_front == 0 && p.col_bytes + ((size_t)32 << 20) <= ws_bytes;
  p.fallback = cols ? TR_COL2IM : s.stride == 2 ? TR_PARITY_GEMM : TR_GEMM_1X1;
  p.route = s.stride == 2 && s.pad == 1 && s.Cout <= 4 && !mask && !stats ? TR_THIN_OUT : p.fallback;
  return p;
}

// Generic "conv-like" pass: Y[b,oy,ox,n] = sum_{kh,kw,c} A[b, oy*s-pad+kh, ox*s-pad+kw, c] * Wt(n,kh,kw,c)
// (conv forward: A = x, n = Cout, weights [n][kh][kw][c];  full-conv data-grad: A = gy, n = Cin_full,
//  weights [n][kh][kw][c] as well — same physical layout by construction.)  s: the pass as a conv (k = 4), A on its H x W map.
static int conv_like_fwd(vf_ctx* ctx, const float* A, const float* w, const float* bias, float* Y, const VfConvShape& s, int act,
                         float slope, VfConvExtras* ex, bool conv_entry = false) {
  const int B = s.B, Hi = s.H, Wi = s.W, C = s.Cin, N = s.Cout, stride = s.stride, pad = s.pad, Ho = s.out_h(), Wo = s.out_w();
  const GaPlan r = ga_plan(s, conv_entry, ex->bn.st.mode != 0);
  if (r.route == GA_THIN_IN) {      // the image-side layers: direct convolution (vf_conv_thin.hip)
    const int rc = vf_internal_conv_thin_fwd(ctx, A, w, bias, Y, nullptr, s, act, slope, ex);
    if (rc >= 0) return rc;
  }
  VF_REQUIRE(vf_is_pow2(Ho) && vf_is_pow2(Wo), "output spatial sizes must be powers of two");
  switch (r.fallback) {
    case GA_DOT_HEAD:
      hipLaunchKernelGGL(k_dot_fwd, dim3(B), dim3(256), 0, ctx->stream, A, w, bias, Y, 16 * C, act, slope);
      VF_LAUNCH_CHECK();
      return 0;
    default: {
      IGemm g;
      memset(&g, 0, sizeof(g));
      g.A = A; g.Wt = w; g.bias = bias; g.Y = Y;
      g.lgMh = vf_ilog2(Ho); g.lgMw = vf_ilog2(Wo);
      g.M = B * Ho * Wo;
      g.Hi = Hi; g.Wi = Wi; g.C = C; g.N = N;
      g.TH = 4; g.TW = 4;
      g.sy = stride; g.ty = 1; g.oy0 = -pad; g.sx = stride; g.tx = 1; g.ox0 = -pad;
      g.kh0 = 0; g.khs = 1; g.kw0 = 0; g.kws = 1;
      g.wsN = 16 * C; g.wsC = 1; g.wsTap = C;
      g.outH = Ho; g.outW = Wo; g.osy = 1; g.osx = 1;
      g.out_elems = (int64_t)g.M * N;
      g.act = act; g.slope = slope;
      return launch_igemm(ctx, g, (C % 16 == 0) && vf_aligned16(A), (C % 16 == 0) && vf_aligned16(w), ex);
    }
  }
}

// TR_COL2IM: cols[pixel][(kh,kw,n)] = A[pixel][:] . W[:][(kh,kw,n)]  (columns contiguous in [c][kh][kw][n]), then every output
// pixel gathers its 4 taps.  The column buffer holds the front of the workspace around the inner GEMM only, whatever that returns.
static int tr_col2im(vf_ctx* ctx, const TrPlan& r, const float* A, const float* w, const float* bias, float* Y, const VfConvShape& s,
                     int act, float slope, const float* dmask, int dact, float dslope) {
  const int B = s.B, Hi = s.H, Wi = s.W, C = s.Cin, N = s.Cout;
  const int64_t Mi = (int64_t)B * Hi * Wi;
  float* cols = (float*)ctx->ws;
  IGemm q;
  memset(&q, 0, sizeof(q));
  q.A = A; q.Wt = w; q.bias = nullptr; q.Y = cols;
  q.M = (int)Mi; q.lgMh = 0; q.lgMw = 0;
  q.Hi = 1; q.Wi = 1; q.C = C; q.N = 16 * N;
  q.TH = 1; q.TW = 1; q.sy = 1; q.ty = 1; q.sx = 1; q.tx = 1; q.khs = 1; q.kws = 1;
  q.wsN = 1; q.wsC = 16 * N; q.wsTap = 0;
  q.outH = 1; q.outW = 1; q.osy = 1; q.osx = 1;
  q.out_elems = Mi * 16 * N;
  q.act = VF_ACT_NONE;
  ctx->ws_front = (r.col_bytes + 255) & ~(size_t)255;
  const int rc = launch_igemm(ctx, q, true, true, nullptr);
  ctx->ws_front = 0;
  if (rc) return rc;
  const int64_t total = Mi * 4 * N;
  VfProf prof(ctx, "col2im4x4", 0.0, 4.0 * ((double)Mi * 16 * N + (double)total));
  hipLaunchKernelGGL(k_col2im4x4, dim3((unsigned)vf_cdiv(total, 256)), dim3(256), 0, ctx->stream, (const float*)cols, bias, Y,
                     B, vf_ilog2(Hi), vf_ilog2(Wi), N, act, slope);
  VF_LAUNCH_CHECK();
  if (dmask) return vf_act_bwd(ctx, dmask, Y, Y, total, dact, dslope);      // thin path: one more pass
  return 0;
}

// Generic "transposed" pass: Y[b,oh,ow,n] = sum_{kh,kw,c : oh = 2i-1+kh ...} A[b,i,j,c] * Wt[c][kh][kw][n]
// (conv data-grad: A = gy, c = Cout, n = Cin;  full-conv forward: A = x, c = Cin_full, n = Cout_full.)  s: the pass as a
// full-conv (k = 4), A on its H x W map.
static int conv_like_bwd(vf_ctx* ctx, const float* A, const float* w, const float* bias, float* Y, const VfConvShape& s, int act,
                         float slope, VfConvExtras* ex, const float* dmask = nullptr, int dact = 0, float dslope = 0.f,
                         bool conv_grad = false) {
  const int B = s.B, Hi = s.H, Wi = s.W, C = s.Cin, N = s.Cout;
  const bool vecA = (C % 16 == 0) && vf_aligned16(A);
  const TrPlan r = tr_plan(s, vecA, vf_aligned16(w), dmask != nullptr, ex->bn.st.mode != 0, ctx->ws_front, ctx->ws_bytes, conv_grad);
  if (r.route == TR_DOT_HEAD) {      // with the derivative of the activation fused into that conv (VfConvExtras::dot_act_y)
    const int64_t n = (int64_t)B * 16 * N;
    hipLaunchKernelGGL(k_dot_bwd_data, dim3((int)vf_cdiv(n, 256)), dim3(256), 0, ctx->stream, A, w, Y, B, 16 * N, ex->dot_act_y,
                       ex->dot_act, ex->dot_act_slope);
    VF_LAUNCH_CHECK();
    return 0;
  }
  if (r.route == TR_THIN_OUT) {      // the image side: direct kernel, no column matrix
    const int rc = vf_internal_deconv_thin_out(ctx, A, w, bias, Y, s, act, slope);
    if (rc >= 0) return rc;
  }
  if (r.fallback == TR_COL2IM) return tr_col2im(ctx, r, A, w, bias, Y, s, act, slope, dmask, dact, dslope);
  IGemm g;
  memset(&g, 0, sizeof(g));
  g.A = A; g.Wt = w; g.bias = bias; g.Y = Y;
  g.dmask = dmask; g.dact = dact; g.dslope = dslope;
  g.Hi = Hi; g.Wi = Wi; g.C = C; g.N = N;
  g.wsN = 1; g.wsC = 16 * N; g.wsTap = N;
  g.act = act; g.slope = slope;
  switch (r.fallback) {
    case TR_PARITY_GEMM:
      // output (2*Hi) x (2*Wi); per parity class a 2x2-tap GEMM over the low-res grid
      g.lgMh = vf_ilog2(Hi); g.lgMw = vf_ilog2(Wi);
      g.M = B * Hi * Wi;
      g.TH = 2; g.TW = 2;
      g.sy = 1; g.ty = -1; g.oy0 = 0; g.sx = 1; g.tx = -1; g.ox0 = 0;  // iy = my + ph - th
      g.khs = 2; g.kws = 2;                                            // kh = (1-ph) + 2*th
      g.outH = 2 * Hi; g.outW = 2 * Wi; g.osy = 2; g.osx = 2;
      g.parity = 1;
      g.out_elems = (int64_t)B * g.outH * g.outW * N;
      VF_REQUIRE(!(dmask && bias), "activation-backward epilogue is for data-gradient passes (no bias)");
      return launch_igemm(ctx, g, vecA, (N % 4 == 0) && vf_aligned16(w), ex);
    default: {
      // stride 1, pad 0, low-res 1x1 -> 4x4: plain GEMM whose N' = (kh,kw,n) columns are contiguous in [c][kh][kw][n]
      VF_REQUIRE(Hi == 1 && Wi == 1, "stride-1 transposed pass is built for the 1x1 bottleneck only (got %dx%d)", Hi, Wi);
      g.lgMh = 0; g.lgMw = 0;
      g.M = B;
      g.TH = 1; g.TW = 1;
      g.sy = 1; g.ty = 1; g.sx = 1; g.tx = 1;
      g.N = 16 * N;
      g.wsC = 16 * N; g.wsTap = 0;
      g.outH = 1; g.outW = 1; g.osy = 1; g.osx = 1;
      g.out_elems = (int64_t)B * 16 * N;
      VF_REQUIRE(!(dmask && bias), "activation-backward epilogue is for data-gradient passes (no bias)");
      if (bias) {  // bias index = column % N: apply bias + activation in a pointwise pass
        g.bias = nullptr;
        g.act = VF_ACT_NONE;
      }
      // (the GEMM columns are (kh, kw, n): not one channel per column, so no statistics by-product here)
      if (int rc = launch_igemm(ctx, g, vecA, ((16 * N) % 4 == 0) && vf_aligned16(w), nullptr)) return rc;
      if (bias) {
        const int64_t total = (int64_t)B * 16 * N;
        const int nb = (int)std::min<int64_t>(vf_cdiv(total, 256), 4096);
        hipLaunchKernelGGL(k_slab_reduce, dim3(nb), dim3(256), 0, ctx->stream, (const float*)Y, Y, bias, total, N, 0, act, slope, 1.f);
        VF_LAUNCH_CHECK();
      }
      return 0;
    }
  }
}

// dW[n][kh][kw][c] = beta*dW + sum_p U[p][n] * V[b, my*s-pad+kh, mx*s-pad+kw, c]
// ---- the plan of one weight gradient: both sides of the layer, the kernel that serves it, its split over K
enum WgRoute {
  WG_SMALLK,        // the bottleneck pair: vf_wgrad_small.hip's kernel, where it takes the call (else fp32_route())
  WG_PLANES_128,    // operands as planes: k_pwgrad_group (vf_pgemm.hip), whole 128 x 128 x 32 tiles
  WG_PLANES_64,     //   ... its 64 x 128 x 32 tile form: ONE row tile of 64
  WG_FP32_GROUP,    // fp32 operands that a group launch can take (k_wgrad_group: 16-byte loads on both sides)
  WG_FP32_SINGLE    // fp32 operands, launched at once (k_wgrad)
};
struct WgPlan {
  int B, stride, pad;
  int P, Hl, Wl, Nu;      // U's side, the low-resolution map: pixels, map, channels
  int Hv, Wv, Cv;         // V's side
  bool vecU, vecV;        // 16-byte loads are legal
  bool pix3;              // V is fetched as whole 3-channel pixels (WGV_PIX3): the image-side layers, in the bf16 modes
  int nk;                // K steps of the kernel's BK
  int bm, gx, gy;         // tile rows (128 / 64), column tiles, row tiles
  int64_t total;          // dW elements
  int target, ksplit;     // split-K: the blocks per layer aimed at, the K ranges taken
  WgRoute route;
  bool rider;             // a bottleneck layer that can ride in a planes launch, in the fp32-fed form of its descriptor
  // the bottleneck pair (1x1 map on one side, 4x4 on the other): dW = U^T V with K = batch — write-bound
  bool is_bottleneck() const { return Hl == 1 && Wl == 1 && Hv == 4 && Wv == 4 && stride == 1 && pad == 0; }
  bool planes() const { return route == WG_PLANES_128 || route == WG_PLANES_64; }
  int64_t u_elems() const { return (int64_t)P * Nu; }
  int64_t v_elems() const { return (int64_t)B * Hv * Wv * Cv; }
  // both operands inside the 2 GiB a buffer descriptor spans, at `bytes` per element (4: fp32; 6: three bf16 planes)
  bool in_range(int bytes) const { return u_elems() * bytes < ((int64_t)1 << 31) && v_elems() * bytes < ((int64_t)1 << 31); }
  WgRoute fp32_route() const { return vecU && vecV && (ksplit == 1 || total % 4 == 0) ? WG_FP32_GROUP : WG_FP32_SINGLE; }
  int blocks() const { return gx * gy * ksplit; }
  size_t slab_bytes() const { return ksplit > 1 ? vf_up256((size_t)ksplit * total * sizeof(float)) : 0; }
  double flops() const { return 2.0 * (double)P * Nu * 16.0 * Cv; }
};
// s: the layer; U lives on its low-resolution map, V on the other (conv: gradOutput, input; full: input, gradOutput); Up / Vp: planes or NULL
static WgPlan wg_plan(vf_ctx* ctx, const VfConvShape& s, bool full, const float* U, const float* V, const void* Up, const void* Vp) {
  const int mode = ctx->mfma_bf16;
  WgPlan p;
  p.B = s.B; p.stride = s.stride; p.pad = s.pad;
  p.Hl = full ? s.H : s.out_h(); p.Wl = full ? s.W : s.out_w(); p.Nu = full ? s.Cin : s.Cout;
  p.Hv = full ? s.full_out_h() : s.H; p.Wv = full ? s.full_out_w() : s.W; p.Cv = full ? s.Cout : s.Cin;
  p.P = s.B * p.Hl * p.Wl;
  p.vecU = (p.Nu % 4 == 0) && vf_aligned16(U);
  p.vecV = (p.Cv % 4 == 0) && vf_aligned16(V);
  // the whole-pixel form needs dword alignment only, which every tensor has.  It changes the tile's columns (64, all of them taps,
  // instead of 48 of 128), not the grid (gx = 1 either way), the K walk or the split below: the same sums in the same order
  p.pix3 = p.Cv == 3 && p.vecU && mode != 0;
  p.nk =(int)vf_cdiv(p.P, mode ? 32 : 16);
  p.bm = p.Nu > 64 ? 128 : 64;
  p.gy = (int)vf_cdiv(p.Nu, p.bm);
  p.gx = (int)vf_cdiv(16 * (int64_t)p.Cv, 128);
  p.total = (int64_t)p.Nu * 16 * p.Cv;
  // operands that arrive as planes (vf_*_bwd_weight_planes): the LDS-DMA kernel of vf_pgemm.hip, whole 128 x 128 x 32 tiles only —
  // or, in the three-plane mode, ONE row tile of 64 (Nu == 64: its 64 x 128 x 32 tile form; the one-plane mode and every other
  // Nu % 128 == 64 stay on the fp32-fed kernels)
  const bool pw64 = p.Nu == 64 && mode == 3;
  const bool use_pw = Up && Vp && (mode == 3 || mode == 1) && s.stride == 2 && s.pad == 1 && (p.Nu % 128 == 0 || pw64) && p.Cv % 64 == 0 &&
                      p.P % 32 == 0 && p.in_range(6) && p.total % 4 == 0;
  // split-K target, blocks per layer.  The planes layers ride in ONE group launch of seven or more layers, which fills the chip as
  // a whole: half the splits per layer leave k_pwgrad_group's time where it was and halve the slabs it writes and the combine
  // reads (same-box: combine 2 x 37.4 -> 2 x 21.8 us); the fp32-fed thin layers' kernel wants the full 512 (62 -> 86 us at 256)
  // A 64-row tile is half a 128-row tile's work per K step: 512 of them per layer keep its blocks as long as the launch's others
  // (at 256, E2's blocks run 64 half steps against the 8 - 16 whole ones of its neighbours and end the launch alone: same-box, the
  // iteration 2.851 ms at 256, 2.813 at 512, 2.842 before the form existed) — and the split is then the fp32-fed kernel's own: same bits
  p.target = use_pw && !pw64 ? 256 : 512;
  const int64_t tiles = (int64_t)p.gx * p.gy;
  p.ksplit = vf_split_k(tiles, p.target, p.nk, 16, 8, (size_t)p.total * sizeof(float), vf_ws_avail(ctx), VF_K_EVEN_OUT);
  p.route = p.is_bottleneck() ? WG_SMALLK : use_pw ? (pw64 ? WG_PLANES_64 : WG_PLANES_128) : p.fp32_route();
  p.rider = p.is_bottleneck() && (mode == 3 || mode == 1) && p.bm == 128 && p.ksplit == 1 && (16 * p.Cv) % 128 == 0 && p.vecU && p.vecV;
  return p;
}
// ---- the three descriptor forms of a planned layer.  WGrad and VfPWGrad name what they share alike: wg_desc_base fills that
template <class D>
static D wg_desc_base(const WgPlan& p, float beta) {
  D d;
  memset(&d, 0, sizeof(d));
  d.P = p.P; d.lgMh = vf_ilog2(p.Hl); d.lgMw = vf_ilog2(p.Wl);
  d.Nu = p.Nu; d.Cv = p.Cv; d.Hv = p.Hv; d.Wv = p.Wv;
  d.gx = p.gx; d.gy = p.gy; d.gz = p.ksplit;
  d.ksplit = p.ksplit; d.nk = p.nk;
  d.beta = beta;
  return d;
}
// slab: the layer's split-K slabs (ksplit > 1) or NULL
static WGrad wg_desc(const WgPlan& p, const float* U, const float* V, float* dW, float* slab, float beta) {
  WGrad g = wg_desc_base<WGrad>(p, beta);
  g.U = U; g.V = V; g.dW = dW; g.slab = slab;
  g.u_bytes = (unsigned)(p.u_elems() * 4);
  g.v_bytes = (unsigned)(p.v_elems() * 4);
  g.stride = p.stride; g.pad = p.pad;
  g.ntaps = 16;
  return g;
}
static VfPWGrad wg_desc_planes(const WgPlan& p, const void* Up, const void* Vp, float* dW, float* slab, float beta) {
  VfPWGrad w = wg_desc_base<VfPWGrad>(p, beta);
  w.Up = Up; w.Vp = Vp;
  w.out = p.ksplit > 1 ? slab : dW;
  w.u_ps = (unsigned)(p.u_elems() * 2);
  w.v_ps = (unsigned)(p.v_elems() * 2);
  return w;
}
// the fp32-fed form a bottleneck layer (WgPlan::rider) carries: U [B][Nu], V [B][4][4][Cv] = [B][16 * Cv].  A rider is whole
// 128 x 128 tiles over one K range of 32-deep steps: the plan's grid is the planes kernel's
static VfPWGrad wg_desc_rider(const WgPlan& p, const float* U, const float* V, float* dW, float beta) {
  VfPWGrad w = wg_desc_base<VfPWGrad>(p, beta);
  w.Uf = U; w.Vf = V;
  w.out = dW;
  return w;
}

// ---- recorder of a weight-gradient group (see k_wgrad_group)
struct WgRec {
  WgPlan p;
  WGrad g;
  VfPWGrad pw;      // a planes layer's descriptor; p.rider: its fp32-fed form, used when the group has planes layers (else the layer
                    // stays with k_wgrad_group)
  int bf;           // the family it launches with: the matrix-core mode, or 4: k_pwgrad_group
};
struct WgRecorder {
  std::vector<WgRec> recs;
  size_t ws_used = 0;      // slab bytes of the workspace that are spoken for
  bool open = false;       // between vf_wgrad_group_begin and _end: weight gradients are recorded, not launched
  void clear() {
    recs.clear();
    ws_used = 0;
  }
  // `bytes` of slabs behind everything spoken for, in a workspace of `avail` bytes: their offset, or false — launch what is
  // recorded (wg_flush) first.  ws_used may exceed what the records hold: a partial end keeps it over an empty record list,
  // because later slabs must not land in regions that a launch in flight still reads.
  bool reserve(size_t bytes, size_t avail, size_t* off) {
    if (ws_used + bytes > avail) return false;
    *off = ws_used;
    ws_used += bytes;
    return true;
  }
};
static WgRecorder& wg_recorder(vf_ctx* ctx) {
  if (!ctx->wg) ctx->wg = new WgRecorder();
  return *ctx->wg;
}
void vf_internal_wg_free(vf_ctx* ctx) {
  delete ctx->wg;
  ctx->wg = nullptr;
}
// the run-time (tile rows, matrix-core mode) of a weight-gradient launch as constants: f(VfIntC<BM>{}, VfIntC<BF>{})
template <class F>
static void wg_dispatch(int bm, int bf, F&& f) {
  auto with_mode = [&](auto BM) {
    if (bf == 3) f(BM, VfIntC<3>{});
    else if (bf) f(BM, VfIntC<1>{});
    else f(BM, VfIntC<0>{});
  };
  if (bm == 128) with_mode(VfIntC<128>{});
  else with_mode(VfIntC<64>{});
}
// One family of a flush: the records `pick` accepts go into descriptor tables of CAP layers (by value in the kernel arguments),
// a launch per full table and one for the rest.  put(slot, record, work) fills a slot, adds the layer's flops or bytes to `work`
// and returns its blocks; every layer starts at a multiple of `align` blocks.  launch(table, blocks, work) -> error code.
template <class Table, int CAP, class Pick, class Put, class Launch>
static int wg_pack(const std::vector<WgRec>& recs, int align, Pick&& pick, Put&& put, Launch&& launch) {
  Table G;
  int blocks = 0;
  double work = 0;
  G.n = 0;
  auto fire = [&]() -> int {
    if (G.n == 0) return 0;
    G.blk_off[G.n] = blocks;
    const int rc = launch(G, blocks, work);
    G.n = 0;
    blocks = 0;
    work = 0;
    return rc;
  };
  for (const WgRec& r : recs) {
    if (!pick(r)) continue;
    G.blk_off[G.n] = blocks;
    blocks += (put(G.d[G.n], r, work) + align - 1) / align * align;
    if (++G.n == CAP)
      if (int rc = fire()) return rc;
  }
  return fire();
}
static int wg_flush(vf_ctx* ctx) {
  WgRecorder& R = wg_recorder(ctx);
  if (R.recs.empty()) return 0;
  // the layers whose operands came as planes: one k_pwgrad_group launch (vf_pgemm.hip).  The bottleneck layers of the same
  // walk go with them in their fp32-fed form: write-bound tiles (131 MB of dW from K = batch) that hide under the MFMA-bound
  // ones of the same launch, as they did in k_wgrad_group
  bool any_planes = false;
  for (const WgRec& r : R.recs) any_planes |= (r.bf == 4);
  if (any_planes)
    for (WgRec& r : R.recs)
      if (r.p.rider) r.bf = 4;
  // (blocks in multiples of 8: the XCD-aware tile order of a layer assumes blockIdx % 8 == local id % 8)
  const int rc = wg_pack<VfPWGradGroup, VF_PWG_MAX>(
      R.recs, 8, [](const WgRec& r) { return r.bf == 4; },
      [](VfPWGrad& d, const WgRec& r, double& fl) {
        d = r.pw;
        fl += r.p.flops();
        return d.gx * d.gy * d.gz;
      },
      [&](const VfPWGradGroup& G, int blocks, double fl) {
        // the label says which tile forms the launch holds (a planes layer with Nu == 64 runs the 64-row form)
        int n64 = 0;
        for (int i = 0; i < G.n; ++i) n64 += G.d[i].Up != nullptr && G.d[i].Nu == 64;
        const char* name = n64 == 0 ? "pwgrad_group_128x128x32" : (n64 == G.n ? "pwgrad_group_64x128x32" : "pwgrad_group_64+128x128x32");
        return vf_internal_pwgrad_group(ctx, G, blocks, name, fl);
      });
  if (rc) return rc;
  // one launch per (tile rows, mode) family, VF_WG_GROUP_MAX layers at a time
  for (int bm : {128, 64})
    for (int bf : {3, 1, 0})
      wg_pack<WGradGroup, VF_WG_GROUP_MAX>(
          R.recs, 8, [&](const WgRec& r) { return r.p.bm == bm && r.bf == bf; },
          [](WGrad& d, const WgRec& r, double& fl) {
            d = r.g;
            fl += r.p.flops();
            return r.p.blocks();
          },
          [&](const WGradGroup& G, int blocks, double fl) {
            char name[64];
            snprintf(name, sizeof(name), "wgrad_group_%dx128%s", bm, bf == 3 ? "_bf16x3" : (bf ? "_bf16" : ""));
            wg_dispatch(bm, bf, [&](auto BM, auto BF) {
              VF_LAUNCH_TIMED(ctx, name, fl, 0.0, (k_wgrad_group<decltype(BM)::value, true, WGV_VEC16, decltype(BF)::value>), dim3(blocks),
                              dim3(256), G);
            });
            return 0;
          });
  VF_LAUNCH_CHECK();
  // the split-K slabs of all layers: one launch per VF_WG_GROUP_MAX layers (64 float4 per block, no alignment between layers)
  wg_pack<SlabGroup, VF_WG_GROUP_MAX>(
      R.recs, 1, [](const WgRec& r) { return r.g.ksplit > 1; },
      [](auto& d, const WgRec& r, double& bytes) {
        d.slab = r.g.slab;
        d.dst = r.g.dW;
        d.total4 = r.p.total / 4;
        d.ksplit = r.g.ksplit;
        d.beta = r.g.beta;
        bytes += 4.0 * (double)r.p.total * (r.g.ksplit + 1);
        return (int)vf_cdiv(r.p.total / 4, 64);
      },
      [&](const SlabGroup& S, int blocks, double bytes) {
        VfProf prof(ctx, "slab_reduce_wgrad_group", 0.0, bytes);
        hipLaunchKernelGGL(k_slab_reduce4_group, dim3(blocks), dim3(256), 0, ctx->stream, S);
        return 0;
      });
  VF_LAUNCH_CHECK();
  R.clear();
  return 0;
}
VF_API int vf_wgrad_group_begin(vf_ctx* ctx) {
  WgRecorder& R = wg_recorder(ctx);
  if (R.open) R.clear();      // the previous walk was abandoned before its _end (a host-side error): drop what it recorded
  R.open = true;
  return 0;
}
VF_API int vf_wgrad_group_abort(vf_ctx* ctx) {
  WgRecorder& R = wg_recorder(ctx);
  R.clear();
  R.open = false;
  return 0;
}
VF_API int vf_wgrad_group_end(vf_ctx* ctx) {
  WgRecorder& R = wg_recorder(ctx);
  VF_REQUIRE(R.open, "vf_wgrad_group_end: no group is open");
  R.open = false;
  return wg_flush(ctx);
}

// weight gradients recorded so far in the open group (not yet launched)
VF_API int vf_wgrad_group_count(vf_ctx* ctx, int* count) {
  VF_REQUIRE(count != nullptr, "vf_wgrad_group_count: NULL");
  WgRecorder& R = wg_recorder(ctx);
  *count = R.open ? (int)R.recs.size() : 0;
  return 0;
}
// launch the FIRST `count` recorded weight gradients (record order = walk order: the layers nearest the net's output) as one
// group and keep the group open with the rest still recorded: a data-parallel host starts the exchange of the finished bucket
// and then ends the group — both launches sit at the END of the backward walk, none in the middle of its data-gradient chain
VF_API int vf_wgrad_group_end_partial(vf_ctx* ctx, int count) {
  WgRecorder& R = wg_recorder(ctx);
  VF_REQUIRE(R.open, "vf_wgrad_group_end_partial: no group is open");
  if (R.recs.empty() || count <= 0) return 0;
  std::vector<WgRec> rest;
  if (count < (int)R.recs.size()) {
    rest.assign(R.recs.begin() + count, R.recs.end());
    R.recs.resize((size_t)count);
  }
  const size_t used = R.ws_used;
  const int rc = wg_flush(ctx);
  R.recs = rest;
  R.ws_used = used;      // (see WgRecorder::reserve)
  return rc;
}

static int wgrad(vf_ctx* ctx, const float* U, const float* V, float* dW, const VfConvShape& s, bool full, float beta, const void* Up,
                 const void* Vp) {
  WgPlan p = wg_plan(ctx, s, full, U, V, Up, Vp);
  if (p.route == WG_SMALLK) {
    const int rc = vf_internal_wgrad_smallk(ctx, U, V, dW, p.B, p.Nu, 16 * p.Cv, beta);
    if (rc >= 0) return rc;
    p.route = p.fp32_route();
  }
  VF_REQUIRE(p.in_range(4), "operand exceeds the 2 GiB buffer-descriptor range");
  WgRecorder& R = wg_recorder(ctx);
  auto slab_at = [&](size_t off) { return p.ksplit > 1 ? (float*)(vf_ws_ptr(ctx) + off) : nullptr; };
  size_t off = 0;
  if (p.planes() || (R.open && p.route == WG_FP32_GROUP)) {
    // recorded, not launched: the group runs at vf_wgrad_group_end.  Every recorded layer keeps its own slab region.
    // A planes layer outside a group is a group of one, launched at once.
    if (!R.reserve(p.slab_bytes(), vf_ws_avail(ctx), &off)) {
      if (int rc = wg_flush(ctx)) return rc;
      R.clear();
      VF_REQUIRE(R.reserve(p.slab_bytes(), vf_ws_avail(ctx), &off), "workspace too small for this layer's split-K slabs");
    }
    WgRec r;
    r.p = p;
    r.g = wg_desc(p, U, V, dW, slab_at(off), beta);
    r.bf = p.planes() ? 4 : ctx->mfma_bf16;
    if (p.planes()) r.pw = wg_desc_planes(p, Up, Vp, dW, r.g.slab, beta);
    else if (p.rider) r.pw = wg_desc_rider(p, U, V, dW, beta);
    R.recs.push_back(r);
    return R.open ? 0 : wg_flush(ctx);
  }
  float* slab = slab_at(0);
  if (R.open) {
    // a launch outside the group must not overwrite recorded slabs: its own slabs go BEHIND them (the group stays recorded: a
    // thin-channel layer at the end of a walk no longer launches the group ahead of vf_wgrad_group_end / _end_partial); only if
    // the workspace cannot hold both is the group finished first
    if (R.reserve(p.slab_bytes(), vf_ws_avail(ctx), &off)) slab = slab_at(off);
    else if (int rc = wg_flush(ctx)) return rc;
  }
  const WGrad g = wg_desc(p, U, V, dW, slab, beta);
  const int bf = ctx->mfma_bf16;
  const char* wname = p.pix3 ? (p.bm == 128 ? (bf == 3 ? "wgrad_128x64_pix3_bf16x3" : "wgrad_128x64_pix3_bf16")
                                            : (bf == 3 ? "wgrad_64x64_pix3_bf16x3" : "wgrad_64x64_pix3_bf16"))
                      : p.bm == 128 ? (bf == 3 ? "wgrad_128x128_bf16x3" : bf ? "wgrad_128x128_bf16" : "wgrad_128x128")
                                    : (bf == 3 ? "wgrad_64x128_bf16x3" : bf ? "wgrad_64x128_bf16" : "wgrad_64x128");
  const double wfl = p.flops();
  const dim3 grid((unsigned)p.blocks()), block(256);
  wg_dispatch(p.bm, bf, [&](auto BM, auto BF) {
    constexpr int bm_ = decltype(BM)::value, bf_ = decltype(BF)::value;
    if constexpr (bf_ != 0) {
      if (p.pix3) {
        VF_LAUNCH_TIMED(ctx, wname, wfl, 0.0, (k_wgrad<bm_, true, WGV_PIX3, bf_>), grid, block, g);
        return;
      }
    }
    if (p.vecU && p.vecV) VF_LAUNCH_TIMED(ctx, wname, wfl, 0.0, (k_wgrad<bm_, true, WGV_VEC16, bf_>), grid, block, g);
    else if (p.vecU) VF_LAUNCH_TIMED(ctx, wname, wfl, 0.0, (k_wgrad<bm_, true, WGV_SCALAR, bf_>), grid, block, g);
    else if (p.vecV) VF_LAUNCH_TIMED(ctx, wname, wfl, 0.0, (k_wgrad<bm_, false, WGV_VEC16, bf_>), grid, block, g);
    else VF_LAUNCH_TIMED(ctx, wname, wfl, 0.0, (k_wgrad<bm_, false, WGV_SCALAR, bf_>), grid, block, g);
  });
  VF_LAUNCH_CHECK();
  if (p.ksplit > 1) {
    VfProf prof(ctx, "slab_reduce_wgrad", 0.0, 4.0 * (double)p.total * (p.ksplit + 1));
    return launch_slab_reduce(ctx, g.slab, dW, nullptr, p.total, 1, p.ksplit, VF_ACT_NONE, 0.f, beta);
  }
  return 0;
}

// ----------------------------------------- C ABI: every entry builds its VfConvShape and calls the internal form
// 1 if this geometry runs on the matrix-core kernels, 0 if vf_conv_generic.hip serves it (include/vf_hip.h, "Shapes")
VF_API int vf_conv_is_fast(int H, int W, int k, int stride, int pad) { return VfConvShape{0, H, W, 0, 0, k, stride, pad}.matrix_core_conv(); }

int vf_internal_conv2d_fwd(vf_ctx* ctx, const float* x, const float* w, const float* bias, float* y, const VfConvShape& s, int act,
                           float slope, VfConvExtras* ex) {
  if (!s.matrix_core_conv()) return vf_internal_gconv_fwd(ctx, x, w, bias, y, s, act, slope);
  if (int rc = check_conv_args(s)) return rc;
  return conv_like_fwd(ctx, x, w, bias, y, s, act, slope, ex, true);
}
VF_API int vf_conv2d_fwd(vf_ctx* ctx, const float* x, const float* w, const float* bias, float* y, int B, int H, int W,
                         int Cin, int Cout, int k, int stride, int pad, int act, float slope) {
  const VfConvShape s{B, H, W, Cin, Cout, k, stride, pad};
  return vf_take_pending(ctx, [&](VfConvExtras* ex) { return vf_internal_conv2d_fwd(ctx, x, w, bias, y, s, act, slope, ex); });
}

int vf_internal_conv2d_bwd_data(vf_ctx* ctx, const float* gy, const float* w, float* gx, const VfConvShape& s, VfConvExtras* ex) {
  if (!s.matrix_core_conv()) return vf_internal_gconv_bwd_data(ctx, gy, w, gx, s);
  if (int rc = check_conv_args(s)) return rc;
  if (s.stride == 1) VF_REQUIRE(s.H == 4 && s.W == 4, "stride-1 conv data-grad is built for the 4x4 bottleneck input only");
  return conv_like_bwd(ctx, gy, w, nullptr, gx, s.gradient_of_conv(), VF_ACT_NONE, 0.f, ex, nullptr, 0, 0.f, true);
}
VF_API int vf_conv2d_bwd_data(vf_ctx* ctx, const float* gy, const float* w, float* gx, int B, int H, int W, int Cin,
                              int Cout, int k, int stride, int pad) {
  const VfConvShape s{B, H, W, Cin, Cout, k, stride, pad};
  return vf_take_pending(ctx, [&](VfConvExtras* ex) { return vf_internal_conv2d_bwd_data(ctx, gy, w, gx, s, ex); });
}

int vf_internal_conv2d_bwd_data_act(vf_ctx* ctx, const float* gy, const float* w, float* gx, const float* x_act, int act, float slope,
                                    const VfConvShape& s, VfConvExtras* ex) {
  if (int rc = check_conv_args(s)) return rc;
  VF_REQUIRE(x_act != nullptr && (act == VF_ACT_LRELU || act == VF_ACT_RELU),
             "vf_conv2d_bwd_data_act: needs the activated input and a (leaky) ReLU");
  VF_REQUIRE(s.stride == 2, "vf_conv2d_bwd_data_act: only the stride-2 layers follow a bare conv + activation pair");
  return conv_like_bwd(ctx, gy, w, nullptr, gx, s.gradient_of_conv(), VF_ACT_NONE, 0.f, ex, x_act, act, slope);
}
VF_API int vf_conv2d_bwd_data_act(vf_ctx* ctx, const float* gy, const float* w, float* gx, const float* x_act, int act,
                                  float slope, int B, int H, int W, int Cin, int Cout, int k, int stride, int pad) {
  const VfConvShape s{B, H, W, Cin, Cout, k, stride, pad};
  return vf_take_pending(ctx, [&](VfConvExtras* ex) { return vf_internal_conv2d_bwd_data_act(ctx, gy, w, gx, x_act, act, slope, s, ex); });
}

// The weight-gradient entry points leave a pending BatchNorm request alone.  x_planes / gy_planes: the bf16 planes of both
// operands (vf_planes_split layout), or NULL: the weight gradient runs on the planes-fed kernel where they are at hand and its
// shape allows (whole 128 x 128 x 32 tiles), on the fp32 operands otherwise.  ex (NULL: plain): the 512 -> 1 head's dot_act_y
int vf_internal_conv2d_bwd_weight(vf_ctx* ctx, const float* x, const float* gy, const void* x_planes, const void* gy_planes, float* gw,
                                  float* gb, const VfConvShape& s, float beta, const VfConvExtras* ex) {
  if (!s.matrix_core_conv()) return vf_internal_gconv_bwd_weight(ctx, x, gy, gw, gb, s, beta);
  if (int rc = check_conv_args(s)) return rc;
  if (s.Cout == 1 && s.stride == 1 && s.H == 4 && s.W == 4) {
    const VfConvExtras plain;
    if (!ex) ex = &plain;
    hipLaunchKernelGGL(k_dot_bwd_weight, dim3((int)vf_cdiv(16 * s.Cin, 64)), dim3(512), 0, ctx->stream, x, gy, gw, gb, s.B,
                       16 * s.Cin, beta, ex->dot_act_y, ex->dot_act, ex->dot_act_slope);
    VF_LAUNCH_CHECK();
    return 0;
  }
  // (tried: the bias gradient as a by-product of this kernel's own gy fragments — the waves that carried it made
  //  their blocks the slowest of every launch: +0.25 ms per step against the 0.19 ms of the separate column sums)
  if (int rc = wgrad(ctx, gy, x, gw, s, false, beta, gy_planes, x_planes)) return rc;
  if (gb) return vf_internal_colsum(ctx, gy, gb, (int64_t)s.B * s.out_h() * s.out_w(), s.Cout, beta);
  return 0;
}
VF_API int vf_conv2d_bwd_weight(vf_ctx* ctx, const float* x, const float* gy, float* gw, float* gb, int B, int H, int W,
                                int Cin, int Cout, int k, int stride, int pad, float beta) {
  return vf_conv2d_bwd_weight_planes(ctx, x, gy, nullptr, nullptr, gw, gb, B, H, W, Cin, Cout, k, stride, pad, beta);
}
VF_API int vf_conv2d_bwd_weight_planes(vf_ctx* ctx, const float* x, const float* gy, const void* x_planes, const void* gy_planes,
                                       float* gw, float* gb, int B, int H, int W, int Cin, int Cout, int k, int stride, int pad,
                                       float beta) {
  return vf_internal_conv2d_bwd_weight(ctx, x, gy, x_planes, gy_planes, gw, gb, VfConvShape{B, H, W, Cin, Cout, k, stride, pad}, beta, nullptr);
}

int vf_internal_deconv2d_fwd(vf_ctx* ctx, const float* x, const float* w, const float* bias, float* y, const VfConvShape& s, int act,
                             float slope, VfConvExtras* ex) {
  if (int rc = check_full_conv_args(s)) return rc;
  return conv_like_bwd(ctx, x, w, bias, y, s, act, slope, ex);
}
VF_API int vf_deconv2d_fwd(vf_ctx* ctx, const float* x, const float* w, const float* bias, float* y, int B, int H, int W,
                           int Cin, int Cout, int k, int stride, int pad, int act, float slope) {
  const VfConvShape s{B, H, W, Cin, Cout, k, stride, pad};
  return vf_take_pending(ctx, [&](VfConvExtras* ex) { return vf_internal_deconv2d_fwd(ctx, x, w, bias, y, s, act, slope, ex); });
}

int vf_internal_deconv2d_bwd_data(vf_ctx* ctx, const float* gy, const float* w, float* gx, const VfConvShape& s, VfConvExtras* ex) {
  if (int rc = check_full_conv_args(s)) return rc;
  // conv of gy (its output map, Cout channels) with weights [Cin][kh][kw][Cout] -> gx (H x W, Cin channels)
  return conv_like_fwd(ctx, gy, w, nullptr, gx, s.gradient_of_full(), VF_ACT_NONE, 0.f, ex);
}
VF_API int vf_deconv2d_bwd_data(vf_ctx* ctx, const float* gy, const float* w, float* gx, int B, int H, int W, int Cin,
                                int Cout, int k, int stride, int pad) {
  const VfConvShape s{B, H, W, Cin, Cout, k, stride, pad};
  return vf_take_pending(ctx, [&](VfConvExtras* ex) { return vf_internal_deconv2d_bwd_data(ctx, gy, w, gx, s, ex); });
}

int vf_internal_deconv2d_bwd_weight(vf_ctx* ctx, const float* x, const float* gy, const void* x_planes, const void* gy_planes, float* gw,
                                    float* gb, const VfConvShape& s, float beta) {
  if (int rc = check_full_conv_args(s)) return rc;
  // gw[ci][kh][kw][co] = sum_{b,i,j} x[b,i,j,ci] * gy[b, i*s-pad+kh, j*s-pad+kw, co]
  if (int rc = wgrad(ctx, x, gy, gw, s, true, beta, x_planes, gy_planes)) return rc;
  if (gb) return vf_internal_colsum(ctx, gy, gb, (int64_t)s.B * s.full_out_h() * s.full_out_w(), s.Cout, beta);
  return 0;
}
VF_API int vf_deconv2d_bwd_weight(vf_ctx* ctx, const float* x, const float* gy, float* gw, float* gb, int B, int H, int W,
                                  int Cin, int Cout, int k, int stride, int pad, float beta) {
  return vf_internal_deconv2d_bwd_weight(ctx, x, gy, nullptr, nullptr, gw, gb, VfConvShape{B, H, W, Cin, Cout, k, stride, pad}, beta);
}
VF_API int vf_deconv2d_bwd_weight_planes(vf_ctx* ctx, const float* x, const float* gy, const void* x_planes, const void* gy_planes,
                                         float* gw, float* gb, int B, int H, int W, int Cin, int Cout, int k, int stride, int pad,
                                         float beta) {
  return vf_internal_deconv2d_bwd_weight(ctx, x, gy, x_planes, gy_planes, gw, gb, VfConvShape{B, H, W, Cin, Cout, k, stride, pad}, beta);
}
