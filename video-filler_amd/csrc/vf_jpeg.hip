// vf_jpeg.hip — batched JPEG decode on the device, byte for byte libjpeg's default decompression.
// One pipeline, three rules (JpgRule) for which files it takes and how its errors are worded:
//   baseline     vf_jpeg_inspect, vf_jpeg_workspace_bytes, vf_jpeg_decode: SOF0 / SOF1 files of ONE scan, 4:4:4 / 4:2:2 /
//                4:2:0 or grey.  The workspace query reads the headers only (upper bounds), so the scan data is walked once;
//   progressive  vf_jpeg_scans_inspect, vf_jpeg_prog_*: SOF2 files;
//   layouts      vf_jpeg_inspect_layouts, vf_jpeg_layouts_*, vf_jpeg_decode_layouts: both kinds, any whole-number sampling,
//                RGB, sequential files of several scans ("layouts").
// Each decode entry turns N files into N uint8 H x W x C images at caller-given offsets of one buffer.  The launch count
// does not depend on N: the host parses the headers, walks every scan for its restart segments and stuffed bytes, builds
// the Huffman decode tables (9-bit lookahead + max-code fallback) and the natural-order dequantisation tables, and packs
// them with every scan's bytes into one staging buffer -> one upload.  Then
//   k_jpeg_unstuff     one wave per 4 KiB chunk drops the stuffed 0x00 bytes; the host found every 0xFF
//                      while it parsed, so each chunk's output offset is known and the chunks are independent;
//   k_jpeg_prog_first  one block per (image, first scan, restart segment): parallel Huffman decoding by
//                      self-synchronisation (Weißenberger & Schmidt, ICPP 2018) over fixed-size subsequences, then the
//                      write pass (de-zigzagged int16 coefficients) and the DC prediction as a segmented scan per
//                      component.  A sequential scan is a first scan whose lanes read a DC symbol and then AC symbols per
//                      block (prog_first_lane<WRITE, SEQ>); a baseline file is one such scan;
//   k_jpeg_prog_scan   one launch per further scan level (progressive refinements): one lane per (image, scan, segment);
//   k_jpeg_idct        one thread per 8x8 block: dequantise, jpeg_idct_islow, range-limit into uint8 component planes,
//                      each block placed by its component's own factors;
//   k_jpeg_color       one thread per output pixel: fancy upsampling, ycc_rgb_convert, crop into H x W x C
//                      (k_jpeg_color_layouts under the layouts rule: every component by its own upsampler, RGB copied).
// Everything is integer arithmetic.  vf_jpeg_prog_coefficients_host and vf_jpeg_layouts_coefficients_host assemble the
// coefficients on the host with the same lane functions.
#include <algorithm>
#include <string>
#include <vector>

#include "vf_block.h"
#include "vf_common.h"

namespace {

constexpr int kJpgMaxSide = 16384;
constexpr int kHuffThreads = 1024;                        // one block per restart segment (the lanes loop over its subsequences)
constexpr int kChunk = 4096;                              // stuffed bytes per unstuffing wave
constexpr int kLook = 9;                                  // lookahead bits of the fast Huffman table
enum { ST_OK = VF_JPEG_OK, ST_BAD = VF_JPEG_BAD_CODE, ST_SHORT = VF_JPEG_SHORT_DATA };
constexpr uint64_t kDead = ~0ull;                         // decoder state of a lane that stopped on an invalid code / overrun

// one Huffman table in decode form (jdhuff.c jpeg_make_d_derived_tbl, with a 9-bit lookahead)
struct JpgHuff {
  uint16_t look[1 << kLook];   // (length << 8) | symbol for codes of <= kLook bits; 0: longer code
  int32_t maxcode[18];         // largest code of each length, -1 if none; [17]: sentinel
  int32_t valoff[18];          // symbol index = code + valoff[length]
  uint8_t val[256];
};

struct JpgImage {
  int64_t coef_base;           // first 8x8 block of the image in the coefficient array
  int64_t plane_base[3];       // first byte of each component plane
  int64_t out_off;             // first byte of the H x W x C output
  int32_t W, H, ncomp, channels;
  int32_t mcux, mcuy, bpm, nblocks;
  int32_t pw[3], ph[3];        // padded plane sizes (whole MCUs)
  int32_t cw[3], ch[3];        // real component sizes: ceil(W * h / hmax), ceil(H * v / vmax)
  int32_t hs, vs;              // the frame's largest sampling factors (1, 1 for grayscale)
  int32_t hc[3], vc[3];        // per component: its sampling factors (1, 1 for grayscale)
  int32_t up[3];               // per component: its upsampler, UP_* (layouts)
  int32_t rgb;                 // 1: the three planes are R, G, B and are copied (layouts)
  int32_t bcomp[10], bx[10], by[10];   // per block of the MCU: component, block offset in it
  int32_t q[3][64];            // natural-order quantisation values per component
};

// a piece of one segment's stuffed bytes and where its kept bytes go
struct JpgChunk {
  int64_t src, dst;
  int32_t n, keep;             // stuffed bytes, kept bytes
  int32_t lo;                  // 1: the segment goes on before the chunk (the byte before it may be read)
};

struct JpgBatch {
  const JpgImage* img;
  const JpgChunk* chunk;
  const JpgHuff* huff;
  const uint8_t* scan;         // stuffed bytes (uploaded)
  uint8_t* bits;               // compacted bytes
  uint64_t* E;                 // per subsequence: entry state
  uint64_t* X;                 //                  exit state
  int32_t* Nb;                 //                  DC symbols decoded (then: exclusive prefix)
  uint8_t* D;                  //                  re-decode flag
  int16_t* coef;
  uint8_t* planes;
  uint8_t* out;
  int32_t* status;
  int32_t* rounds;
  int nchunk, sub_bits;
};

__host__ __device__ constexpr int zz_natural(int k) {
  // jpeg_natural_order: zig-zag index -> natural (row-major) index
  constexpr int8_t t[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return t[k];
}
[[maybe_unused]] __constant__ int8_t c_natural[80] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33,
                                     40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36,
                                     29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                                     47, 55, 62, 63,
                                     // extra entries for safety in decoder, as jutils.c: k > 63 lands on 63
                                     63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63};

#define VF_HD __host__ __device__ __forceinline__

// jpeg_natural_order[k] with k > 63 landing on 63, as jutils.c pads it for corrupt run lengths
VF_HD int natural(int k) {
#ifdef __HIP_DEVICE_COMPILE__
  return c_natural[k];
#else
  return k > 63 ? 63 : zz_natural(k);
#endif
}

__device__ __forceinline__ uint64_t st_pack(uint32_t p, int b, int k) { return ((uint64_t)p << 16) | ((uint64_t)b << 8) | (uint64_t)k; }

// ---- bit reader over one compacted segment (16-byte aligned, 16 bytes of slack behind it): a 64-bit window plus the next
// dword, loaded one dword ahead of use.  Positions only move forward, by at most 31 bits per symbol; the decoder checks
// every symbol against the segment's length, so the slack bytes (whatever they hold) never decide a result.
struct BitWin {
  const uint32_t* s;
  uint32_t wbyte;   // byte index of w's first byte (a multiple of 4)
  uint64_t w;       // bytes [wbyte, wbyte + 8), big-endian
  uint32_t nxt;     // bytes [wbyte + 8, wbyte + 12), big-endian
  VF_HD static uint32_t be(uint32_t v) { return __builtin_bswap32(v); }
  VF_HD void seek(uint32_t p) {
    wbyte = (p >> 3) & ~3u;
    const uint32_t d = wbyte >> 2;
    w = ((uint64_t)be(s[d]) << 32) | be(s[d + 1]);
    nxt = be(s[d + 2]);
  }
  // 32 bits starting at bit p (p at most 62 bits past the window start)
  VF_HD uint32_t peek(uint32_t p) {
    uint32_t o = p - 8u * wbyte;
    if (o >= 32) {
      w = (w << 32) | nxt;
      wbyte += 4;
      nxt = be(s[(wbyte >> 2) + 2]);
      o -= 32;
    }
    return (uint32_t)((w << o) >> 32);
  }
};

// one Huffman symbol at the top of `bits` (32-bit window): length (0: invalid code) and symbol
VF_HD int huff_decode(const JpgHuff& t, uint32_t bits, int& sym) {
  const uint32_t e = t.look[bits >> (32 - kLook)];
  if (e) {
    sym = e & 0xff;
    return (int)(e >> 8);
  }
  for (int l = kLook + 1; l <= 16; ++l) {
    const int code = (int)(bits >> (32 - l));
    if (code <= t.maxcode[l]) {
      sym = t.val[(code + t.valoff[l]) & 0xff];
      return l;
    }
  }
  return 0;
}

VF_HD int huff_extend(uint32_t r, int s) {  // HUFF_EXTEND
  return (int)r - ((r < (1u << (s - 1))) ? (1 << s) - 1 : 0);
}

enum { LANE_END = 0, LANE_DONE = 1, LANE_BAD = 2, LANE_SHORT = 3 };

// one wave per chunk: keep every byte but the 0x00 after a 0xFF (stuffing)
__global__ void k_jpeg_unstuff(const JpgBatch B) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (c >= B.nchunk) return;
  const JpgChunk ck = B.chunk[c];
  const uint8_t* in = B.scan + ck.src;
  uint8_t* out = B.bits + ck.dst;
  int base = 0;
  for (int c0 = 0; c0 < ck.n; c0 += 64) {
    const int i = c0 + lane;
    bool keep = false;
    uint8_t v = 0;
    if (i < ck.n) {
      v = in[i];
      keep = !(v == 0 && (i > 0 || ck.lo) && in[i - 1] == 0xFF);
    }
    const uint64_t m = __ballot(keep);
    const int pos = base + (int)__popcll(m & ((1ull << lane) - 1));
    if (keep && pos < ck.keep) out[pos] = v;
    base += (int)__popcll(m);
  }
}

// ---- jidctint.c jpeg_idct_islow
constexpr int CONST_BITS = 13, PASS1_BITS = 2;
constexpr int32_t FIX_0_298631336 = 2446, FIX_0_390180644 = 3196, FIX_0_541196100 = 4433, FIX_0_765366865 = 6270,
                  FIX_0_899976223 = 7373, FIX_1_175875602 = 9633, FIX_1_501321110 = 12299, FIX_1_847759065 = 15137,
                  FIX_1_961570560 = 16069, FIX_2_053119869 = 16819, FIX_2_562915447 = 20995, FIX_3_072711026 = 25172;

VF_HD int32_t descale(int32_t x, int n) { return (x + (1 << (n - 1))) >> n; }

// idct_range_limit[x & 1023] of jdmaster.c prepare_range_limit_table (the +128 level shift is part of the table)
VF_HD uint8_t idct_limit(int32_t x) {
  const int j = x & 1023;
  return (uint8_t)(j < 128 ? j + 128 : j < 512 ? 255 : j < 896 ? 0 : j - 896);
}

// one 1-D pass of the islow IDCT over in[0], in[s], ..., in[7s] -> o0..o7 before the descale
struct Idct8 {
  int32_t t10, t11, t12, t13, t0, t1, t2, t3;
  VF_HD void run(int32_t i0, int32_t i1, int32_t i2, int32_t i3, int32_t i4, int32_t i5, int32_t i6,
                                      int32_t i7) {
    int32_t z2 = i2, z3 = i6;
    int32_t z1 = (z2 + z3) * FIX_0_541196100;
    int32_t tmp2 = z1 + z3 * (-FIX_1_847759065);
    int32_t tmp3 = z1 + z2 * FIX_0_765366865;
    z2 = i0;
    z3 = i4;
    int32_t tmp0 = (z2 + z3) * (1 << CONST_BITS);
    int32_t tmp1 = (z2 - z3) * (1 << CONST_BITS);
    t10 = tmp0 + tmp3;
    t13 = tmp0 - tmp3;
    t11 = tmp1 + tmp2;
    t12 = tmp1 - tmp2;
    tmp0 = i7;
    tmp1 = i5;
    tmp2 = i3;
    tmp3 = i1;
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    int32_t z4 = tmp1 + tmp3;
    const int32_t z5 = (z3 + z4) * FIX_1_175875602;
    tmp0 = tmp0 * FIX_0_298631336;
    tmp1 = tmp1 * FIX_2_053119869;
    tmp2 = tmp2 * FIX_3_072711026;
    tmp3 = tmp3 * FIX_1_501321110;
    z1 = z1 * (-FIX_0_899976223);
    z2 = z2 * (-FIX_2_562915447);
    z3 = z3 * (-FIX_1_961570560);
    z4 = z4 * (-FIX_0_390180644);
    z3 += z5;
    z4 += z5;
    t0 = tmp0 + z1 + z3;
    t1 = tmp1 + z2 + z4;
    t2 = tmp2 + z2 + z3;
    t3 = tmp3 + z1 + z4;
  }
};

// one 8x8 block: dequantise (natural order), jpeg_idct_islow, range-limit into dst (row stride `stride`)
VF_HD void idct_islow(const int16_t* cf, const int32_t* q, uint8_t* dst, int stride) {
  int32_t ws[64];
  // pass 1: columns (the all-zero-AC shortcut of jidctint.c gives the same values, so it is not taken separately)
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    Idct8 d;
    d.run(cf[c] * q[c], cf[8 + c] * q[8 + c], cf[16 + c] * q[16 + c], cf[24 + c] * q[24 + c], cf[32 + c] * q[32 + c],
          cf[40 + c] * q[40 + c], cf[48 + c] * q[48 + c], cf[56 + c] * q[56 + c]);
    constexpr int n = CONST_BITS - PASS1_BITS;
    ws[c] = descale(d.t10 + d.t3, n);
    ws[56 + c] = descale(d.t10 - d.t3, n);
    ws[8 + c] = descale(d.t11 + d.t2, n);
    ws[48 + c] = descale(d.t11 - d.t2, n);
    ws[16 + c] = descale(d.t12 + d.t1, n);
    ws[40 + c] = descale(d.t12 - d.t1, n);
    ws[24 + c] = descale(d.t13 + d.t0, n);
    ws[32 + c] = descale(d.t13 - d.t0, n);
  }
  // pass 2: rows
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int32_t* w = ws + 8 * r;
    Idct8 d;
    d.run(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]);
    constexpr int n = CONST_BITS + PASS1_BITS + 3;
    uint8_t o[8];
    o[0] = idct_limit(descale(d.t10 + d.t3, n));
    o[7] = idct_limit(descale(d.t10 - d.t3, n));
    o[1] = idct_limit(descale(d.t11 + d.t2, n));
    o[6] = idct_limit(descale(d.t11 - d.t2, n));
    o[2] = idct_limit(descale(d.t12 + d.t1, n));
    o[5] = idct_limit(descale(d.t12 - d.t1, n));
    o[3] = idct_limit(descale(d.t13 + d.t0, n));
    o[4] = idct_limit(descale(d.t13 - d.t0, n));
    uint8_t* row = dst + (int64_t)r * stride;
    for (int x = 0; x < 8; ++x) row[x] = o[x];
  }
}

__global__ void k_jpeg_idct(const JpgBatch B) {
  const JpgImage& im = B.img[blockIdx.y];
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < im.nblocks; j += (int64_t)gridDim.x * blockDim.x) {
    const int m = (int)(j / im.bpm), b = (int)(j % im.bpm);
    const int ci = im.bcomp[b];
    const int bx = (m % im.mcux) * im.hc[ci] + im.bx[b], by = (m / im.mcux) * im.vc[ci] + im.by[b];
    idct_islow(B.coef + (im.coef_base + j) * 64, im.q[ci], B.planes + im.plane_base[ci] + (int64_t)by * 8 * im.pw[ci] + bx * 8,
               im.pw[ci]);
  }
}

// ---- jdsample.c (fancy upsampling) and jdcolor.c ycc_rgb_convert
VF_HD uint8_t clamp255(int v) { return (uint8_t)min(255, max(0, v)); }

// chroma sample of component ci at full-resolution (x, y)
VF_HD int chroma_at(const JpgBatch& B, const JpgImage& im, int ci, int x, int y) {
  const uint8_t* pl = B.planes + im.plane_base[ci];
  const int pw = im.pw[ci], cw = im.cw[ci], ch = im.ch[ci];
  if (im.hs == 1) return pl[(int64_t)y * pw + x];                       // 4:4:4 (vs == 1 with hs == 1)
  const int i = x >> 1;
  if (cw <= 2) return pl[(int64_t)(im.vs == 2 ? y >> 1 : y) * pw + i];  // h2v1_upsample / h2v2_upsample (box)
  if (im.vs == 1) {                                                     // h2v1_fancy_upsample
    const uint8_t* in = pl + (int64_t)y * pw;
    const int v3 = 3 * in[i];
    if (x & 1) return i == cw - 1 ? in[i] : (v3 + in[i + 1] + 2) >> 2;
    return i == 0 ? in[0] : (v3 + in[i - 1] + 1) >> 2;
  }
  // h2v2_fancy_upsample: the nearer row weighs 3, the farther 1; the rows beyond the edges replicate the edge rows
  const int r0 = y >> 1;
  const int r1 = (y & 1) ? min(r0 + 1, ch - 1) : max(r0 - 1, 0);
  const uint8_t* in0 = pl + (int64_t)r0 * pw;
  const uint8_t* in1 = pl + (int64_t)r1 * pw;
  auto cs = [&](int c) { return 3 * in0[c] + in1[c]; };
  const int c0 = cs(i);
  if (x & 1) return i == cw - 1 ? (4 * c0 + 7) >> 4 : (3 * c0 + cs(i + 1) + 7) >> 4;
  return i == 0 ? (4 * c0 + 8) >> 4 : (3 * c0 + cs(i - 1) + 8) >> 4;
}

// ---- layouts: jdsample.c jinit_upsampler's choice per component, made on the host
enum { UP_COPY = 0, UP_H2V1 = 1, UP_H2V2 = 2, UP_H1V2 = 3, UP_INT = 4 };

// sample of component ci at full-resolution (x, y), by the component's own upsampler
__device__ __forceinline__ int sample_at(const JpgBatch& B, const JpgImage& im, int ci, int x, int y) {
  const uint8_t* pl = B.planes + im.plane_base[ci];
  const int pw = im.pw[ci], cw = im.cw[ci], ch = im.ch[ci];
  switch (im.up[ci]) {
    case UP_COPY: return pl[(int64_t)y * pw + x];
    case UP_H2V1: {                                                     // h2v1_fancy_upsample (cw > 2)
      const uint8_t* in = pl + (int64_t)y * pw;
      const int i = x >> 1, v3 = 3 * in[i];
      if (x & 1) return i == cw - 1 ? in[i] : (v3 + in[i + 1] + 2) >> 2;
      return i == 0 ? in[0] : (v3 + in[i - 1] + 1) >> 2;
    }
    case UP_H2V2: {                                                     // h2v2_fancy_upsample (cw > 2)
      const int i = x >> 1, r0 = y >> 1;
      const int r1 = (y & 1) ? min(r0 + 1, ch - 1) : max(r0 - 1, 0);
      const uint8_t* in0 = pl + (int64_t)r0 * pw;
      const uint8_t* in1 = pl + (int64_t)r1 * pw;
      const int c0 = 3 * in0[i] + in1[i];
      if (x & 1) return i == cw - 1 ? (4 * c0 + 7) >> 4 : (3 * c0 + 3 * in0[i + 1] + in1[i + 1] + 7) >> 4;
      return i == 0 ? (4 * c0 + 8) >> 4 : (3 * c0 + 3 * in0[i - 1] + in1[i - 1] + 8) >> 4;
    }
    case UP_H1V2: {                                                     // h1v2_fancy_upsample: per column, any width
      const int r0 = y >> 1;
      const int r1 = (y & 1) ? min(r0 + 1, ch - 1) : max(r0 - 1, 0);
      return (3 * pl[(int64_t)r0 * pw + x] + pl[(int64_t)r1 * pw + x] + ((y & 1) ? 2 : 1)) >> 2;
    }
    default:                                                            // int_upsample: replicate
      return pl[(int64_t)(y / (im.vs / im.vc[ci])) * pw + x / (im.hs / im.hc[ci])];
  }
}

// k_jpeg_color for the layouts entry: every component through its own upsampler (luma may be the subsampled one), then
// ycc_rgb_convert, a copy (RGB) or the grey plane replicated.  A kernel of its own, so that the old entries' kernel is
// the one it was; `up` and `rgb` are the image's, so the branches are uniform per block.
__global__ void k_jpeg_color_layouts(const JpgBatch B) {
  const JpgImage& im = B.img[blockIdx.y];
  const int64_t npix = (int64_t)im.W * im.H;
  uint8_t* out = B.out + im.out_off;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / im.W), x = (int)(i % im.W);
    const int Y = sample_at(B, im, 0, x, y);
    if (im.ncomp == 1) {
      for (int c = 0; c < im.channels; ++c) out[i * im.channels + c] = (uint8_t)Y;
      continue;
    }
    const int c1 = sample_at(B, im, 1, x, y), c2 = sample_at(B, im, 2, x, y);
    if (im.rgb) {
      out[i * 3 + 0] = (uint8_t)Y;
      out[i * 3 + 1] = (uint8_t)c1;
      out[i * 3 + 2] = (uint8_t)c2;
      continue;
    }
    const int cb = c1 - 128, cr = c2 - 128;
    constexpr int SCALEBITS = 16, ONE_HALF = 1 << 15;
    out[i * 3 + 0] = clamp255(Y + ((91881 * cr + ONE_HALF) >> SCALEBITS));
    out[i * 3 + 1] = clamp255(Y + ((-22554 * cb + ONE_HALF + -46802 * cr) >> SCALEBITS));
    out[i * 3 + 2] = clamp255(Y + ((116130 * cb + ONE_HALF) >> SCALEBITS));
  }
}

__global__ void k_jpeg_color(const JpgBatch B) {
  const JpgImage& im = B.img[blockIdx.y];
  const int64_t npix = (int64_t)im.W * im.H;
  uint8_t* out = B.out + im.out_off;
  const uint8_t* yp = B.planes + im.plane_base[0];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / im.W), x = (int)(i % im.W);
    const int Y = yp[(int64_t)y * im.pw[0] + x];
    if (im.ncomp == 1) {
      for (int c = 0; c < im.channels; ++c) out[i * im.channels + c] = (uint8_t)Y;
      continue;
    }
    const int cb = chroma_at(B, im, 1, x, y) - 128, cr = chroma_at(B, im, 2, x, y) - 128;
    constexpr int SCALEBITS = 16, ONE_HALF = 1 << 15;
    const int r = Y + ((91881 * cr + ONE_HALF) >> SCALEBITS);
    const int g = Y + ((-22554 * cb + ONE_HALF + -46802 * cr) >> SCALEBITS);
    const int bl = Y + ((116130 * cb + ONE_HALF) >> SCALEBITS);
    out[i * 3 + 0] = clamp255(r);
    out[i * 3 + 1] = clamp255(g);
    out[i * 3 + 2] = clamp255(bl);
  }
}

// ================================================================================================ host side: parsing
struct RawHuff {
  uint8_t bits[17];
  uint8_t val[256];
  int nval;
  bool present;
  bool fits;   // the canonical codes fit their lengths, none all ones (jdhuff.c: else JERR_BAD_HUFF_TABLE)
};

// jpeg_make_d_derived_tbl's check: after the codes of length l, the next code must still fit in l bits
inline bool huff_fits(const uint8_t* bits) {
  int64_t code = 0;
  for (int l = 1; l <= 16; ++l) {
    code += bits[l];
    if (code >= ((int64_t)1 << l)) return false;
    code <<= 1;
  }
  return true;
}

// What a file must be for an entry to take it, and how the entry words its errors.  On the device it decides nothing but
// the colour kernel.
//   BASELINE     SOF0 / SOF1 files of one scan, 4:4:4 / 4:2:2 / 4:2:0 or grey, two Huffman slots per class;
//   PROGRESSIVE  SOF2 files of the same samplings; SOF2 is no reason, and the scan checks are jpg_prog_parse's;
//   LAYOUTS      SOF0 / SOF1 / SOF2, any whole-number sampling, RGB, sequential files of several scans.
enum JpgKind { BASELINE, PROGRESSIVE, LAYOUTS };
struct JpgRule {
  JpgKind kind;
  const char* who;       // what the messages about the batch's files start with
  const char* upload;    // profiling labels of the upload range and of the first scans' launch
  const char* entropy;
};
constexpr JpgRule kBaselineRule = {BASELINE, "vf_jpeg", "jpeg_upload", "jpeg_huffman"};
constexpr JpgRule kProgressiveRule = {PROGRESSIVE, "vf_jpeg_prog", "jpeg_prog_upload", "jpeg_prog_first"};
constexpr JpgRule kLayoutsRule = {LAYOUTS, "vf_jpeg_layouts", "jpeg_prog_upload", "jpeg_prog_first"};

struct JpgParsed {
  int W = 0, H = 0, ncomp = 0, prec = 0, sof = -1, ri = 0, hmax = 1, vmax = 1;
  int cid[4] = {}, hf[4] = {}, vf[4] = {}, tq[4] = {};
  int ns = 0, scomp[4] = {}, td[4] = {}, ta[4] = {};
  int ss = 0, se = 63, ahal = 0;
  bool jfif = false, adobe = false;
  bool rgb = false;         // layouts: the components are R, G, B (jdapimin.c default_decompress_parms)
  int adobe_transform = -1;
  int64_t scan_begin = 0;   // of the scan whose SOS was read last
  bool supported = false;
  std::string why;
  uint16_t qt[4][64] = {};   // natural order
  bool qt_ok[4] = {};
  RawHuff hdc[4] = {}, hac[4] = {};
};

// one restart segment of a scan: its stuffed bytes [begin, end) of the file and how many unstuffing keeps
struct JpgRestartSeg {
  int64_t begin, end, len;
};

inline int rd16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// the payloads of DHT, DQT and SOS (s: sl bytes behind the length) into P; non-zero with msg if malformed
int jpg_dht(const uint8_t* s, int sl, JpgParsed& P, std::string& msg) {
  int q = 0;
  while (q < sl) {
    if (q + 17 > sl) {
      msg = "truncated DHT";
      return 2;
    }
    const int tc = s[q] >> 4, th = s[q] & 15;
    int cnt = 0;
    for (int l = 1; l <= 16; ++l) cnt += s[q + l];
    if (q + 17 + cnt > sl || cnt > 256 || th > 3 || tc > 1) {
      msg = "malformed DHT";
      return 2;
    }
    RawHuff& h = tc ? P.hac[th] : P.hdc[th];
    h.bits[0] = 0;
    for (int l = 1; l <= 16; ++l) h.bits[l] = s[q + l];
    memcpy(h.val, s + q + 17, cnt);
    h.nval = cnt;
    h.present = true;
    h.fits = huff_fits(h.bits);
    q += 17 + cnt;
  }
  return 0;
}

int jpg_dqt(const uint8_t* s, int sl, JpgParsed& P, std::string& msg) {
  int q = 0;
  while (q < sl) {
    const int pq = s[q] >> 4, tqi = s[q] & 15;
    const int need = 1 + 64 * (pq ? 2 : 1);
    if (q + need > sl || tqi > 3 || pq > 1) {
      msg = "malformed DQT";
      return 2;
    }
    for (int k = 0; k < 64; ++k) P.qt[tqi][zz_natural(k)] = pq ? rd16(s + q + 1 + 2 * k) : s[q + 1 + k];
    P.qt_ok[tqi] = true;
    q += need;
  }
  return 0;
}

int jpg_sos(const uint8_t* s, int sl, JpgParsed& P, std::string& msg) {
  if (sl < 1) {
    msg = "truncated SOS";
    return 2;
  }
  P.ns = s[0];
  if (sl < 1 + 2 * P.ns + 3 || P.ns < 1 || P.ns > 4) {
    msg = "malformed SOS";
    return 2;
  }
  for (int i = 0; i < P.ns; ++i) {
    int f = -1;
    for (int c = 0; c < P.ncomp && c < 4; ++c)
      if (P.cid[c] == s[1 + 2 * i]) f = c;
    if (f < 0) {
      msg = "SOS names a component the frame does not have";
      return 2;
    }
    for (int j = 0; j < i; ++j)
      if (P.scomp[j] == f) {
        msg = "SOS names a component twice";
        return 2;
      }
    P.scomp[i] = f;
    P.td[i] = s[2 + 2 * i] >> 4;
    P.ta[i] = s[2 + 2 * i] & 15;
  }
  P.ss = s[1 + 2 * P.ns];
  P.se = s[2 + 2 * P.ns];
  P.ahal = s[3 + 2 * P.ns];
  return 0;
}

// One scan's entropy-coded data from byte `begin`: every 0xFF is stuffing (0xFF00), a restart marker, or the end of the
// scan.  -> its restart segments, the stuffed 0x00s' positions (appended to drops), its end and the marker there (-1:
// the data ran out)
int jpg_walk(const uint8_t* d, int64_t n, int64_t begin, std::vector<JpgRestartSeg>& segs, std::vector<int64_t>& drops,
             int64_t& scan_end, int& end_marker, std::string& msg) {
  int64_t q = begin, seg0 = q, drop = 0;
  int nrst = 0;
  end_marker = -1;
  drops.reserve(drops.size() + (size_t)(n - begin) / 200 + 16);   // entropy-coded bytes are 0xFF about once in 256
  for (;;) {
    const uint8_t* f = q < n ? (const uint8_t*)memchr(d + q, 0xFF, (size_t)(n - q)) : nullptr;
    if (!f) {
      scan_end = n;
      break;
    }
    const int64_t i = f - d;
    int64_t j = i + 1;
    while (j < n && d[j] == 0xFF) ++j;
    if (j >= n) {
      scan_end = i;
      break;
    }
    const int c = d[j];
    if (c == 0) {
      if (j - i > 1) {
        // fill bytes before a stuffed 0xFF: libjpeg-turbo's fast path reads them as a marker, its slow path (and
        // jpeg-6b) skips them, so the file has no one libjpeg result.  No encoder writes them.
        msg = "0xFF fill bytes inside the entropy-coded data at byte " + std::to_string(i);
        return 2;
      }
      ++drop;
      drops.push_back(j);   // the stuffed 0x00
      q = j + 1;
    } else if (c >= 0xD0 && c <= 0xD7) {
      if (c != 0xD0 + (nrst & 7)) {
        msg = "restart marker out of sequence";
        return 2;
      }
      ++nrst;
      segs.push_back({seg0, i, i - seg0 - drop});
      seg0 = j + 1;
      drop = 0;
      q = j + 1;
    } else {
      scan_end = i;
      end_marker = c;
      break;
    }
  }
  segs.push_back({seg0, scan_end, scan_end - seg0 - drop});
  return 0;
}

// The headers up to the first SOS.  0: parsed (P.supported says whether they let the rule take the file, P.why why not);
// else malformed (msg).  The entropy-coded data is jpg_prog_parse's.
int jpg_parse(const uint8_t* d, int64_t n, JpgParsed& P, std::string& msg, JpgKind kind) {
  const bool layouts = kind == LAYOUTS;
  auto unsupported = [&](const std::string& w) {
    if (P.why.empty()) P.why = w;
  };
  if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) {
    msg = "not a JPEG file (no SOI marker)";
    return 2;
  }
  int64_t p = 2;
  bool have_sos = false;
  for (;;) {
    // next marker: skip fill bytes
    if (p >= n) {
      msg = "truncated header (no SOS marker before the end of the data)";
      return 2;
    }
    if (d[p] != 0xFF) {
      msg = "malformed header: marker expected at byte " + std::to_string(p);
      return 2;
    }
    while (p < n && d[p] == 0xFF) ++p;
    if (p >= n) {
      msg = "truncated header";
      return 2;
    }
    const int m = d[p++];
    if (m == 0xD9) {
      msg = "no SOS marker (EOI before any scan)";
      return 2;
    }
    if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;   // no payload
    if (p + 2 > n) {
      msg = "truncated header";
      return 2;
    }
    const int L = rd16(d + p);
    if (L < 2 || p + L > n) {
      msg = "truncated header (marker 0x" + std::to_string(m) + " runs past the end of the data)";
      return 2;
    }
    const uint8_t* s = d + p + 2;
    const int sl = L - 2;
    if (m == 0xC0 || m == 0xC1 || m == 0xC2 || m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || (m >= 0xC9 && m <= 0xCB) ||
        (m >= 0xCD && m <= 0xCF)) {
      if (P.sof >= 0) {
        msg = "more than one SOF marker";
        return 2;
      }
      P.sof = m;
      if (sl < 6) {
        msg = "truncated SOF";
        return 2;
      }
      P.prec = s[0];
      P.H = rd16(s + 1);
      P.W = rd16(s + 3);
      P.ncomp = s[5];
      if (sl < 6 + 3 * P.ncomp) {
        msg = "truncated SOF";
        return 2;
      }
      for (int c = 0; c < P.ncomp && c < 4; ++c) {
        P.cid[c] = s[6 + 3 * c];
        P.hf[c] = s[7 + 3 * c] >> 4;
        P.vf[c] = s[7 + 3 * c] & 15;
        P.tq[c] = s[8 + 3 * c];
        P.hmax = std::max(P.hmax, P.hf[c]);
        P.vmax = std::max(P.vmax, P.vf[c]);
      }
      if ((m == 0xC2 && kind != BASELINE) || (layouts && (m == 0xC0 || m == 0xC1))) {
      } else if (m == 0xC2 || m == 0xC6 || m == 0xCA || m == 0xCE) unsupported("progressive");
      else if (m == 0xC3 || m == 0xC7 || m == 0xCB || m == 0xCF) unsupported("lossless");
      else if (m >= 0xC9) unsupported("arithmetic coding");
      else if (m >= 0xC5) unsupported("hierarchical (differential)");
      if (P.prec != 8) unsupported(std::to_string(P.prec) + "-bit samples");
      if (P.ncomp == 4) unsupported("4 components (CMYK / YCCK)");
      else if (P.ncomp != 1 && P.ncomp != 3) unsupported(std::to_string(P.ncomp) + " components");
      if (P.W <= 0 || P.H <= 0) unsupported("height or width 0 (DNL)");
      if (P.W > kJpgMaxSide || P.H > kJpgMaxSide) unsupported("larger than 16384 per side");
      if (P.ncomp == 3 && layouts) {
        // jdinput.c initial_setup / jdmaster.c: factors 1..4, whole-number ratios to the largest (libjpeg:
        // JERR_FRACT_SAMPLE_NOTIMPL), at most 10 blocks in an MCU (D_MAX_BLOCKS_IN_MCU, JERR_BAD_MCU_SIZE)
        const std::string f = std::to_string(P.hf[0]) + "x" + std::to_string(P.vf[0]) + "," + std::to_string(P.hf[1]) + "x" +
                              std::to_string(P.vf[1]) + "," + std::to_string(P.hf[2]) + "x" + std::to_string(P.vf[2]);
        int nb = 0;
        bool range = true, whole = true;
        for (int c = 0; c < 3; ++c) {
          range &= P.hf[c] >= 1 && P.hf[c] <= 4 && P.vf[c] >= 1 && P.vf[c] <= 4;
          nb += P.hf[c] * P.vf[c];
        }
        for (int c = 0; c < 3 && range; ++c) whole &= P.hmax % P.hf[c] == 0 && P.vmax % P.vf[c] == 0;
        if (!range) unsupported("sampling " + f + " (factors are 1 to 4)");
        else if (!whole) unsupported("sampling " + f + " (fractional ratio between components)");
        else if (nb > 10) unsupported("sampling " + f + " (" + std::to_string(nb) + " blocks in an MCU, 10 at most)");
      } else if (P.ncomp == 3) {
        const bool ok = P.hf[1] == 1 && P.vf[1] == 1 && P.hf[2] == 1 && P.vf[2] == 1 &&
                        ((P.hf[0] == 1 && P.vf[0] == 1) || (P.hf[0] == 2 && P.vf[0] == 1) || (P.hf[0] == 2 && P.vf[0] == 2));
        if (!ok)
          unsupported("sampling " + std::to_string(P.hf[0]) + "x" + std::to_string(P.vf[0]) + "," + std::to_string(P.hf[1]) +
                      "x" + std::to_string(P.vf[1]) + "," + std::to_string(P.hf[2]) + "x" + std::to_string(P.vf[2]) +
                      " (4:4:4, 4:2:2 and 4:2:0 only)");
      }
    } else if (m == 0xC4) {
      if (int e = jpg_dht(s, sl, P, msg)) return e;
    } else if (m == 0xDB) {
      if (int e = jpg_dqt(s, sl, P, msg)) return e;
    } else if (m == 0xDD) {   // DRI
      if (sl < 2) {
        msg = "truncated DRI";
        return 2;
      }
      P.ri = rd16(s);
    } else if (m == 0xE0) {
      if (sl >= 5 && !memcmp(s, "JFIF", 5)) P.jfif = true;
    } else if (m == 0xEE) {
      if (sl >= 12 && !memcmp(s, "Adobe", 5)) {
        P.adobe = true;
        P.adobe_transform = s[11];
      }
    } else if (m == 0xDA) {   // SOS
      if (P.sof < 0) {
        msg = "SOS before SOF";
        return 2;
      }
      if (int e = jpg_sos(s, sl, P, msg)) return e;
      P.scan_begin = p + L;
      have_sos = true;
    }
    p += L;
    if (have_sos) break;
  }
  // colour space (jdapimin.c default_decompress_parms) and the scan
  if (P.ncomp == 3) {
    if (P.jfif) {
    } else if (P.adobe) {
      if (P.adobe_transform == 0 && layouts) P.rgb = true;
      else if (P.adobe_transform == 0) unsupported("RGB colour transform (Adobe transform 0)");
      else if (P.adobe_transform != 1) unsupported("Adobe transform " + std::to_string(P.adobe_transform));
    } else if (P.cid[0] == 82 && P.cid[1] == 71 && P.cid[2] == 66) {
      if (layouts) P.rgb = true;
      else unsupported("RGB components");
    }
  }
  if (layouts || (kind == PROGRESSIVE && P.sof == 0xC2)) {   // every check of the scans is jpg_prog_parse's
    P.supported = P.why.empty();
    return 0;
  }
  // the one scan of a baseline file
  if (P.ns != P.ncomp && (P.ncomp == 1 || P.ncomp == 3)) unsupported("multi-scan sequential");
  if (P.ss != 0 || P.se != 63 || P.ahal != 0) unsupported("non-baseline scan parameters");
  for (int i = 0; i < P.ns && P.why.empty(); ++i) {
    const int f = P.scomp[i];
    if (P.tq[f] > 3 || !P.qt_ok[P.tq[f]]) unsupported("missing quantisation table");
    if (P.td[i] > 1 || P.ta[i] > 1 || !P.hdc[P.td[i]].present || !P.hac[P.ta[i]].present)
      unsupported("missing Huffman table (or one beyond baseline's two)");
    else {
      const RawHuff& h = P.hdc[P.td[i]];
      for (int v = 0; v < h.nval; ++v)
        if (h.val[v] > 15) unsupported("DC Huffman symbol above 15");
    }
  }
  for (int i = 0; i < P.ns; ++i) {
    // a table the scan uses whose codes overflow their lengths: libjpeg stops with JERR_BAD_HUFF_TABLE
    const RawHuff* used[2] = {P.td[i] <= 1 ? &P.hdc[P.td[i]] : nullptr, P.ta[i] <= 1 ? &P.hac[P.ta[i]] : nullptr};
    for (const RawHuff* h : used)
      if (h && h->present && !h->fits) {
        msg = "bad Huffman table: its code counts overflow the code lengths";
        return 2;
      }
  }
  P.supported = P.why.empty();
  return 0;
}

void build_huff(const RawHuff& r, JpgHuff& t) {
  memset(&t, 0, sizeof(t));
  if (!r.present || !r.fits) return;   // never used by a scan (jpg_parse rejects used ones); keeps `look` in bounds
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    t.valoff[l] = k - code;
    for (int i = 0; i < r.bits[l]; ++i, ++k, ++code) {
      if (l <= kLook) {
        const int lo = code << (kLook - l), hi = lo + (1 << (kLook - l));
        for (int e = lo; e < hi; ++e) t.look[e] = (uint16_t)((l << 8) | r.val[k]);
      }
    }
    t.maxcode[l] = r.bits[l] ? code - 1 : -1;
    code <<= 1;
  }
  t.maxcode[17] = 0x7fffffff;
  memcpy(t.val, r.val, 256);
}

inline int64_t seg_bits_bytes(int64_t len) { return ((len + 15) & ~(int64_t)15) + 16; }   // BitWin reads up to 11 bytes past the end

// ===================================================================== progressive (SOF2) files: DESIGN.md 5.9
// The entropy rule of jdphuff.c as four per-block functions (decode_mcu_DC_first, decode_mcu_AC_first,
// decode_mcu_DC_refine, decode_mcu_AC_refine), host and device alike, and one walker that takes a restart segment
// through them in order.  The scans of a batch are launched level by level (a scan's level is one more than the highest
// level among the earlier scans of its file that touch the same component and an overlapping band of coefficients):
// level 0 is every first scan (Ah = 0), decoded by self-synchronisation, a block per (image, scan, restart segment)
// (k_jpeg_prog_first); the levels behind are the refinement scans, where one lane walks one (image, scan, restart
// segment) in order (k_jpeg_prog_scan): what a block's bits mean depends on the coefficients it already has.
constexpr int kProgMaxScans = 64;
constexpr int kProgMaxMcuBlocks = 10;   // blocks of an interleaved MCU (libjpeg's D_MAX_BLOCKS_IN_MCU)

struct ProgScan {
  int32_t img;
  int32_t ss, se, ah, al;
  int32_t ns;                  // components
  int32_t interleaved;         // 1: a unit is an MCU of the frame's grid; 0: a unit is one real block of the one component
  int32_t nunit, nb;           // units in the scan; blocks per unit
  int32_t bw, h, v, b0;        // one component: real blocks per row, its sampling, its first block in the MCU
  int32_t boff[kProgMaxMcuBlocks];    // interleaved: each unit block's place in the frame's MCU ...
  int32_t bslot[kProgMaxMcuBlocks];   // ... and its component's place in the scan (DC predictor, table)
  int32_t tab[4];              // per scan component: its table in force at the SOS (DC for Ss = 0, else AC); -1: none
  // a scan of a sequential file (Ss = 0, Se = 63): every block is its DC symbol and then its AC symbols
  int32_t seq;
  int32_t ntab;                // its distinct tables: tab[0 .. ntab) when <= 4, else the ntab tables from tab[0] on
  int32_t dct[kProgMaxMcuBlocks], act[kProgMaxMcuBlocks];   // per unit block: its DC and AC table among those
};

struct ProgSeg {
  int64_t dst;                 // first byte in `bits` (compacted; 16-byte aligned, 16 bytes of slack behind)
  int32_t len;                 // compacted bytes
  int32_t scan;
  int32_t u0, nu;              // its units
  int32_t nsub;                // first scans: its subsequences, the first of them
  int64_t sub0;
};

// block j of unit u -> its place among the image's blocks (the baseline layout: MCU by MCU)
VF_HD int64_t prog_block(const JpgImage& im, const ProgScan& sc, int u, int j) {
  if (sc.interleaved) return (int64_t)u * im.bpm + sc.boff[j];
  const int by = u / sc.bw, bx = u % sc.bw;
  return ((int64_t)(by / sc.v) * im.mcux + bx / sc.h) * im.bpm + sc.b0 + (by % sc.v) * sc.h + bx % sc.h;
}

// Bits of one segment, in order.  Every read is checked against the segment's length first, so p never passes nbits
// and BitWin's loads stay inside the slack behind the segment.
struct ProgReader {
  BitWin bw;
  uint32_t p, nbits;
  // one Huffman symbol (0..255), or -ST_BAD / -ST_SHORT
  VF_HD int symbol(const JpgHuff& t) {
    int sym = 0;
    const int l = huff_decode(t, bw.peek(p), sym);
    if (!l) return -ST_BAD;
    if (p + (uint32_t)l > nbits) return -ST_SHORT;
    p += l;
    return sym;
  }
  // n (1..16) bits into v; ST_OK or ST_SHORT
  VF_HD int bits(int n, uint32_t& v) {
    if (p + (uint32_t)n > nbits) return ST_SHORT;
    v = bw.peek(p) >> (32 - n);
    p += n;
    return ST_OK;
  }
};

VF_HD int prog_dc_first(ProgReader& R, const JpgHuff& t, int al, int& pred, int16_t* blk) {
  const int s = R.symbol(t);
  if (s < 0) return -s;
  if (s > 15) return ST_BAD;
  uint32_t v = 0;
  if (s)
    if (int e = R.bits(s, v)) return e;
  pred = (int)((uint32_t)pred + (uint32_t)(s ? huff_extend(v, s) : 0));
  blk[0] = (int16_t)((uint32_t)pred << al);
  return ST_OK;
}

VF_HD int prog_dc_refine(ProgReader& R, int al, int16_t* blk) {
  uint32_t b;
  if (int e = R.bits(1, b)) return e;
  if (b) blk[0] = (int16_t)(blk[0] | (1 << al));
  return ST_OK;
}

VF_HD int prog_ac_first(ProgReader& R, const JpgHuff& t, int ss, int se, int al, int& eobrun, int16_t* blk) {
  if (eobrun > 0) {
    --eobrun;
    return ST_OK;
  }
  for (int k = ss; k <= se;) {
    const int rs = R.symbol(t);
    if (rs < 0) return -rs;
    const int r = rs >> 4, s = rs & 15;
    uint32_t v = 0;
    if (s) {
      k += r;
      if (k > se) return ST_BAD;
      if (int e = R.bits(s, v)) return e;
      blk[natural(k)] = (int16_t)(huff_extend(v, s) * (1 << al));
      ++k;
    } else if (r == 15) {
      k += 16;
    } else {
      if (r)
        if (int e = R.bits(r, v)) return e;
      eobrun = (1 << r) + (int)v - 1;
      break;
    }
  }
  return ST_OK;
}

// one correction bit of an already nonzero coefficient
VF_HD int prog_refine(ProgReader& R, int p1, int16_t* c) {
  uint32_t b;
  if (int e = R.bits(1, b)) return e;
  const int v = *c;
  if (b && (v & p1) == 0) *c = (int16_t)(v >= 0 ? v + p1 : v - p1);
  return ST_OK;
}

VF_HD int prog_ac_refine(ProgReader& R, const JpgHuff& t, int ss, int se, int al, int& eobrun, int16_t* blk) {
  const int p1 = 1 << al;
  int k = ss;
  if (eobrun == 0) {
    while (k <= se) {
      const int rs = R.symbol(t);
      if (rs < 0) return -rs;
      int r = rs >> 4, val = 0;
      const int s = rs & 15;
      uint32_t v = 0;
      if (s) {
        if (s != 1) return ST_BAD;
        if (int e = R.bits(1, v)) return e;
        val = v ? p1 : -p1;
      } else if (r != 15) {
        if (r)
          if (int e = R.bits(r, v)) return e;
        eobrun = (1 << r) + (int)v;
        break;
      }
      for (; k <= se; ++k) {
        int16_t* c = blk + natural(k);
        if (*c) {
          if (int e = prog_refine(R, p1, c)) return e;
        } else if (--r < 0) {
          break;
        }
      }
      if (val) {
        if (k > se) return ST_BAD;
        blk[natural(k)] = (int16_t)val;
      }
      ++k;
    }
  }
  if (eobrun > 0) {
    for (; k <= se; ++k) {
      int16_t* c = blk + natural(k);
      if (*c)
        if (int e = prog_refine(R, p1, c)) return e;
    }
    --eobrun;
  }
  return ST_OK;
}

// jdhuff.c decode_mcu for one block: the DC difference, then the AC symbols up to EOB or the 64th coefficient
VF_HD int seq_block(ProgReader& R, const JpgHuff& dct, const JpgHuff& act, int& pred, int16_t* blk) {
  if (int e = prog_dc_first(R, dct, 0, pred, blk)) return e;
  for (int k = 1; k < 64;) {
    const int rs = R.symbol(act);
    if (rs < 0) return -rs;
    const int r = rs >> 4, s = rs & 15;
    uint32_t v = 0;
    if (s) {
      k += r;
      if (int e = R.bits(s, v)) return e;
      blk[natural(k)] = (int16_t)huff_extend(v, s);
      ++k;
    } else if (r == 15) {
      k += 16;
    } else {
      break;
    }
  }
  return ST_OK;
}

// One restart segment of one scan, its units u0 .. u0 + nu in order; coef: the image's first coefficient.  The
// predictors and the EOB run start at 0 (process_restart); a run that outlasts the segment's blocks is bad data.
__host__ __device__ inline int prog_decode_segment(const JpgImage& im, const ProgScan& sc, const JpgHuff* huff, const uint32_t* bits,
                                                   uint32_t nbits, int u0, int nu, int16_t* coef) {
  ProgReader R{{bits, 0, 0, 0}, 0, nbits};
  R.bw.seek(0);
  int pred[4] = {0, 0, 0, 0};
  int eobrun = 0;
  for (int u = u0; u < u0 + nu; ++u)
    for (int j = 0; j < sc.nb; ++j) {
      int16_t* blk = coef + 64 * prog_block(im, sc, u, j);
      const int slot = sc.interleaved ? sc.bslot[j] : 0;
      int e;
      if (sc.seq) e = seq_block(R, huff[sc.tab[0] + sc.dct[j]], huff[sc.tab[0] + sc.act[j]], pred[slot], blk);
      else if (sc.ss == 0) e = sc.ah == 0 ? prog_dc_first(R, huff[sc.tab[slot]], sc.al, pred[slot], blk) : prog_dc_refine(R, sc.al, blk);
      else if (sc.ah == 0) e = prog_ac_first(R, huff[sc.tab[0]], sc.ss, sc.se, sc.al, eobrun, blk);
      else e = prog_ac_refine(R, huff[sc.tab[0]], sc.ss, sc.se, sc.al, eobrun, blk);
      if (e != ST_OK) return e;
    }
  return eobrun > 0 ? (int)ST_BAD : (int)ST_OK;
}

// ---- first scans (Ah = 0) by self-synchronisation (Weißenberger & Schmidt, ICPP 2018).  A lane's state is (p, j, k):
// the bit it is at, the block of the unit it is in (interleaved DC scans, sequential scans) and the zig-zag index (AC and
// sequential scans; Ss at the start of a block).
// An EOB run consumes no bits beyond its symbol, so it is taken whole where the symbol is read: it advances the block
// count by its length and never enters the state.
// Decode from (p, j, k) while the next symbol starts before pend.  g: the ordinal, among the segment's `total` blocks,
// of the block the lane is in (the exclusive scan of the counts; 0 when counting).  WRITE: store the coefficients (a DC
// value as its difference) and stop once `total` blocks are done; else count: g comes back as the blocks advanced,
// capped at total + 1.  Returns LANE_*.
// SEQ: the scan is a sequential file's (baseline, layouts), else a progressive first scan; the block picks the instance
// per scan.
template <bool WRITE, bool SEQ>
__host__ __device__ int prog_first_lane(const JpgImage& im, const ProgScan& sc, const JpgHuff* tabs, BitWin& bw, uint32_t nbits, uint32_t& p,
                                        int& j, int& k, uint32_t pend, int64_t& g, int64_t total, int u0, int16_t* coef) {
  const bool dc = sc.ss == 0;
  bw.seek(p);
  for (;;) {
    if (!WRITE && g > total) g = total + 1;
    // bits behind a sequential scan's last block are not the scan's (libjpeg skips them); an EOB run past it is bad data
    if (WRITE && SEQ && g >= total) return LANE_DONE;
    if (WRITE && (dc || k == sc.ss) && g >= total) return g > total ? LANE_BAD : LANE_DONE;
    if (p >= pend) return LANE_END;
    const uint32_t w = bw.peek(p);
    int sym;
    if constexpr (SEQ) {
      // a sequential scan: k = 0 is the block's DC symbol, j the block of the unit (its tables), g the block
      const int l = huff_decode(tabs[k == 0 ? sc.dct[j] : sc.act[j]], w, sym);
      if (!l || (k == 0 && sym > 15)) return LANE_BAD;
      const int r = k == 0 ? 0 : sym >> 4, s = k == 0 ? sym : sym & 15;
      if (p + (uint32_t)(l + s) > nbits) return LANE_SHORT;
      if (k > 0 && s == 0) {
        k = r == 15 ? k + 16 : 64;   // ZRL / EOB
      } else {
        k += r;
        if (WRITE)
          coef[64 * prog_block(im, sc, u0 + (int)(g / sc.nb), (int)(g % sc.nb)) + natural(k)] =
              (int16_t)(s ? huff_extend((w << l) >> (32 - s), s) : 0);
        ++k;
      }
      p += l + s;
      if (k >= 64) {
        k = 0;
        ++g;
        if (++j == sc.nb) j = 0;
      }
      continue;
    }
    if (dc) {
      const int l = huff_decode(tabs[sc.bslot[j]], w, sym);
      if (!l || sym > 15) return LANE_BAD;
      const int s = sym;
      if (p + (uint32_t)(l + s) > nbits) return LANE_SHORT;
      if (WRITE) coef[64 * prog_block(im, sc, u0 + (int)(g / sc.nb), (int)(g % sc.nb))] = (int16_t)(s ? huff_extend((w << l) >> (32 - s), s) : 0);
      p += l + s;
      ++g;
      if (++j == sc.nb) j = 0;
      continue;
    }
    const int l = huff_decode(tabs[0], w, sym);
    if (!l) return LANE_BAD;
    const int r = sym >> 4, s = sym & 15;
    if (s) {
      if (p + (uint32_t)(l + s) > nbits) return LANE_SHORT;
      k += r;
      if (k > sc.se) return LANE_BAD;
      if (WRITE) {
        if (g >= total) return LANE_BAD;   // a lane that starts inside a block the scan does not have
        coef[64 * prog_block(im, sc, u0 + (int)g, 0) + natural(k)] = (int16_t)(huff_extend((w << l) >> (32 - s), s) * (1 << sc.al));
      }
      ++k;
      p += l + s;
    } else if (r == 15) {
      if (p + (uint32_t)l > nbits) return LANE_SHORT;
      k += 16;
      p += l;
    } else {
      if (p + (uint32_t)(l + r) > nbits) return LANE_SHORT;
      g += (1 << r) + (int)(r ? (w << l) >> (32 - r) : 0);   // this block and the run's others
      p += l + r;
      k = sc.ss;
      continue;
    }
    if (k > sc.se) {
      ++g;
      k = sc.ss;
    }
  }
}

// the DC values of one unit's blocks: differences -> predictions, point-transformed.  run: each scan component's
// predictor before the unit
VF_HD void prog_dc_unit(const JpgImage& im, const ProgScan& sc, int u, unsigned* run, int16_t* coef) {
  for (int b = 0; b < sc.nb; ++b) {
    int16_t* dc = coef + 64 * prog_block(im, sc, u, b);
    run[sc.bslot[b]] += (unsigned)(int)*dc;
    *dc = (int16_t)(run[sc.bslot[b]] << sc.al);
  }
}

// one (image, first scan, restart segment) by its block.  SEQ as prog_first_lane; GT: the scan's tables are read from
// global memory (a sequential scan of three components may name six; the block has four slots), else from `tabs`.
// Both are template arguments so that each instance's table reads keep their address space.
template <bool SEQ, bool GT>
__device__ __forceinline__ void prog_first_block(const JpgBatch& B, const ProgSeg& sg, const ProgScan& sc, const JpgImage& im,
                                                 const JpgHuff* tabs, unsigned long long* s_w, int* changed) {
  const int t = threadIdx.x;
  const JpgHuff* T = GT ? B.huff + sc.tab[0] : tabs;
  const uint32_t nbits = 8u * (uint32_t)sg.len;
  const uint32_t sb = (uint32_t)B.sub_bits;
  const int nsub = sg.nsub;
  uint64_t* E = B.E + sg.sub0;
  uint64_t* X = B.X + sg.sub0;
  int32_t* Nb = B.Nb + sg.sub0;
  uint8_t* D = B.D + sg.sub0;
  const int64_t total = (int64_t)sg.nu * sc.nb;
  int16_t* coef = B.coef + im.coef_base * 64;
  BitWin bw{(const uint32_t*)(B.bits + sg.dst), 0, 0, 0};

  auto run = [&](int i, uint64_t e) {
    uint32_t p = (uint32_t)(e >> 16);
    int j = (int)((e >> 8) & 0xff), k = (int)(e & 0xff);
    int64_t g = 0;
    const uint32_t pend = min(nbits, (uint32_t)(i + 1) * sb);
    const int r = prog_first_lane<false, SEQ>(im, sc, T, bw, nbits, p, j, k, pend, g, total, sg.u0, nullptr);
    X[i] = r == LANE_END ? st_pack(p, j, k) : kDead;
    Nb[i] = (int32_t)g;
  };
  // speculative start of every subsequence at its first bit, at the start of a unit
  for (int i = t; i < nsub; i += kHuffThreads) {
    const uint64_t e = st_pack((uint32_t)i * sb, 0, sc.ss);
    E[i] = e;
    run(i, e);
  }
  // synchronise: a lane whose entry state differs from its predecessor's exit state decodes again from it.  A dead exit
  // (the predecessor stopped on an invalid code) is no information: the lane keeps its state, otherwise the dead state
  // would travel one lane per round to the end of the segment with the corrections behind it
  int nround = 0;
  for (;;) {
    if (t == 0) *changed = 0;
    __syncthreads();
    for (int i = t; i < nsub; i += kHuffThreads) {
      D[i] = 0;
      if (i == 0) continue;
      const uint64_t x = X[i - 1];
      if (x != E[i] && x != kDead) {
        E[i] = x;
        D[i] = 1;
        *changed = 1;
      }
    }
    __syncthreads();
    if (!*changed) break;
    ++nround;
    for (int i = t; i < nsub; i += kHuffThreads)
      if (D[i]) run(i, E[i]);
    __syncthreads();
  }
  if (t == 0) atomicMax(B.rounds, nround);
  // exclusive scan of the blocks each lane advances -> the block each lane starts in (capped: total + 1 is "beyond")
  {
    unsigned long long carry = 0;
    for (int c = 0; c < nsub; c += kHuffThreads) {
      const int i = c + t;
      const unsigned long long v = i < nsub ? (unsigned long long)Nb[i] : 0ull;
      unsigned long long tot;
      const unsigned long long pre = vf_block_excl_scan<unsigned long long, kHuffThreads>(v, s_w, tot);
      if (i < nsub) Nb[i] = (int32_t)min(carry + pre, (unsigned long long)total + 1);
      carry += tot;
    }
  }
  __syncthreads();
  // write pass from the synchronised states.  Behind a dead exit the chain is broken: that predecessor meets the invalid
  // code in its own write pass, and this lane writes nothing (an error only if it still owes blocks)
  int err = ST_OK;
  for (int i = t; i < nsub; i += kHuffThreads) {
    const uint64_t e = E[i];
    int64_t g = Nb[i];
    if (i > 0 && X[i - 1] == kDead) {
      if (g < total) err = ST_BAD;
      continue;
    }
    uint32_t p = (uint32_t)(e >> 16);
    int j = (int)((e >> 8) & 0xff), k = (int)(e & 0xff);
    const uint32_t pend = min(nbits, (uint32_t)(i + 1) * sb);
    const int r = prog_first_lane<true, SEQ>(im, sc, T, bw, nbits, p, j, k, pend, g, total, sg.u0, coef);
    if (r == LANE_BAD) err = ST_BAD;
    else if (r == LANE_SHORT || (r == LANE_END && i == nsub - 1)) err = max(err, (int)ST_SHORT);
  }
  if (err != ST_OK) atomicMax(B.status + sc.img, err);
  if (sc.ss != 0) return;
  __syncthreads();
  // DC prediction: per scan component, a running sum over the segment's units
  unsigned carry[4] = {0, 0, 0, 0};
  unsigned* s_u = (unsigned*)s_w;
  for (int c = 0; c < sg.nu; c += kHuffThreads) {
    const int m = c + t;
    unsigned sum[4] = {0, 0, 0, 0};
    if (m < sg.nu)
      for (int b = 0; b < sc.nb; ++b) sum[sc.bslot[b]] += (unsigned)(int)coef[64 * prog_block(im, sc, sg.u0 + m, b)];
    unsigned pre[4];
    for (int ci = 0; ci < 4; ++ci) {
      unsigned tot;
      pre[ci] = carry[ci] + vf_block_excl_scan<unsigned, kHuffThreads>(sum[ci], s_u, tot);
      carry[ci] += tot;
    }
    if (m < sg.nu) prog_dc_unit(im, sc, sg.u0 + m, pre, coef);
  }
}


__global__ __launch_bounds__(kHuffThreads) void k_jpeg_prog_first(const JpgBatch B, const ProgScan* scans, const ProgSeg* segs) {
  __shared__ JpgHuff tabs[4];
  __shared__ unsigned long long s_w[kHuffThreads / 64];
  __shared__ int changed;
  const int t = threadIdx.x;
  const ProgSeg sg = segs[blockIdx.x];
  const ProgScan& sc = scans[sg.scan];
  const JpgImage& im = B.img[sc.img];
  for (int c = 0; c < sc.ntab && sc.ntab <= 4; ++c) {
    const uint32_t* src = (const uint32_t*)(B.huff + sc.tab[c]);
    uint32_t* dst = (uint32_t*)(tabs + c);
    for (int i = t; i < (int)(sizeof(JpgHuff) / 4); i += kHuffThreads) dst[i] = src[i];
  }
  __syncthreads();
  if (!sc.seq) prog_first_block<false, false>(B, sg, sc, im, tabs, s_w, &changed);
  else if (sc.ntab <= 4) prog_first_block<true, false>(B, sg, sc, im, tabs, s_w, &changed);
  else prog_first_block<true, true>(B, sg, sc, im, tabs, s_w, &changed);
}

// the same on the host, lane after lane: what vf_jpeg_prog_coefficients_host runs the first scans through
inline int prog_first_segment_host(const JpgImage& im, const ProgScan& sc, const JpgHuff* huff, const uint32_t* bits, int len, int sub_bytes,
                                   int u0, int nu, int16_t* coef) {
  JpgHuff tabs[6];
  for (int c = 0; c < sc.ntab; ++c) tabs[c] = huff[sc.ntab > 4 ? sc.tab[0] + c : sc.tab[c]];
  const uint32_t nbits = 8u * (uint32_t)len, sb = 8u * (uint32_t)sub_bytes;
  const int nsub = (int)std::max<int64_t>(1, vf_cdiv(len, sub_bytes));
  const int64_t total = (int64_t)nu * sc.nb;
  std::vector<uint64_t> E(nsub), X(nsub);
  std::vector<int64_t> Nb(nsub);
  BitWin bw{bits, 0, 0, 0};
  auto state = [](uint32_t p, int j, int k) { return ((uint64_t)p << 16) | ((uint64_t)j << 8) | (uint64_t)k; };
  auto run = [&](int i) {
    uint32_t p = (uint32_t)(E[i] >> 16);
    int j = (int)((E[i] >> 8) & 0xff), k = (int)(E[i] & 0xff);
    int64_t g = 0;
    const uint32_t pend = std::min(nbits, (uint32_t)(i + 1) * sb);
    const int r = sc.seq ? prog_first_lane<false, true>(im, sc, tabs, bw, nbits, p, j, k, pend, g, total, u0, nullptr)
                         : prog_first_lane<false, false>(im, sc, tabs, bw, nbits, p, j, k, pend, g, total, u0, nullptr);
    X[i] = r == LANE_END ? state(p, j, k) : kDead;
    Nb[i] = g;
  };
  for (int i = 0; i < nsub; ++i) {
    E[i] = state((uint32_t)i * sb, 0, sc.ss);
    run(i);
  }
  for (bool changed = true; changed;) {
    changed = false;
    std::vector<int> again;
    for (int i = 1; i < nsub; ++i)
      if (X[i - 1] != E[i] && X[i - 1] != kDead) {
        E[i] = X[i - 1];
        again.push_back(i);
      }
    for (int i : again) run(i);   // after all the comparisons of the round, as the barrier has it
    changed = !again.empty();
  }
  int64_t at = 0;
  for (int i = 0; i < nsub; ++i) {
    const int64_t v = Nb[i];
    Nb[i] = std::min(at, total + 1);
    at += v;
  }
  int err = ST_OK;
  for (int i = 0; i < nsub; ++i) {
    int64_t g = Nb[i];
    if (i > 0 && X[i - 1] == kDead) {
      if (g < total) err = ST_BAD;
      continue;
    }
    uint32_t p = (uint32_t)(E[i] >> 16);
    int j = (int)((E[i] >> 8) & 0xff), k = (int)(E[i] & 0xff);
    const uint32_t pend = std::min(nbits, (uint32_t)(i + 1) * sb);
    const int r = sc.seq ? prog_first_lane<true, true>(im, sc, tabs, bw, nbits, p, j, k, pend, g, total, u0, coef)
                         : prog_first_lane<true, false>(im, sc, tabs, bw, nbits, p, j, k, pend, g, total, u0, coef);
    if (r == LANE_BAD) err = ST_BAD;
    else if (r == LANE_SHORT || (r == LANE_END && i == nsub - 1)) err = std::max(err, (int)ST_SHORT);
  }
  if (sc.ss == 0) {
    unsigned pred[4] = {0, 0, 0, 0};
    for (int u = u0; u < u0 + nu; ++u) prog_dc_unit(im, sc, u, pred, coef);
  }
  return err;
}

// one lane per (image, scan, restart segment) of one level
__global__ void k_jpeg_prog_scan(const JpgBatch B, const ProgScan* scans, const ProgSeg* segs, int first, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const ProgSeg sg = segs[first + i];
  const ProgScan& sc = scans[sg.scan];
  const JpgImage& im = B.img[sc.img];
  const int e = prog_decode_segment(im, sc, B.huff, (const uint32_t*)(B.bits + sg.dst), 8u * (uint32_t)sg.len, sg.u0, sg.nu,
                                    B.coef + im.coef_base * 64);
  if (e != ST_OK) atomicMax(B.status + sc.img, e);
}

// ---- host side
struct ProgScanHost {
  int ns = 0, scomp[4] = {}, ss = 0, se = 0, ah = 0, al = 0, ri = 0, level = 0;
  int tab[4] = {-1, -1, -1, -1};   // per scan component: its table among ProgParsed::tabs
  bool seq = false;                // a scan of a sequential file: tab[0] is the first of its ntab tables,
  int ntab = 0, dtab[4] = {}, atab[4] = {};   // dtab / atab each component's DC / AC table among them
  int64_t begin = 0, end = 0, nunit = 0;
  std::vector<JpgRestartSeg> segs;
  std::vector<int64_t> drops;   // positions of the bytes unstuffing drops, ascending
};

struct ProgParsed {
  JpgParsed P;                 // the frame: geometry, sampling, and the table state as the parse goes
  std::vector<ProgScanHost> scans;
  std::vector<RawHuff> tabs;   // every table a scan uses, as it stood at that SOS
  uint16_t q[3][64] = {};      // per component, latched at its first scan (jdinput.c latch_quant_tables)
  int nlevel = 0;
  bool gray() const { return P.ncomp == 1; }
  int h(int c) const { return gray() ? 1 : P.hf[c]; }
  int v(int c) const { return gray() ? 1 : P.vf[c]; }
  int hmax() const { return gray() ? 1 : P.hmax; }
  int vmax() const { return gray() ? 1 : P.vmax; }
  int64_t mcux() const { return vf_cdiv(P.W, 8 * hmax()); }
  int64_t mcuy() const { return vf_cdiv(P.H, 8 * vmax()); }
  int bpm() const { return gray() ? 1 : P.hf[0] * P.vf[0] + P.hf[1] * P.vf[1] + P.hf[2] * P.vf[2]; }
  int64_t nblocks() const { return mcux() * mcuy() * bpm(); }
};

// 0: parsed (P.supported / P.why as jpg_parse); else malformed (msg).  Walks every scan the rule takes: the one scan of a
// BASELINE file (a second SOS behind it is a reason, its data is not walked), the scans of a PROGRESSIVE file, and under
// LAYOUTS those of sequential files too (SOF0 / SOF1, any number of scans), with jpg_parse's wider samplings and RGB.
// walk false (BASELINE, whose headers say whether the file is taken): the headers only, no scan is recorded.
int jpg_prog_parse(const uint8_t* d, int64_t n, ProgParsed& G, std::string& msg, JpgKind kind, bool walk = true) {
  JpgParsed& P = G.P;
  if (int e = jpg_parse(d, n, P, msg, kind)) return e;
  if (!walk) return 0;
  P.supported = false;
  if (kind == PROGRESSIVE && P.sof != 0xC2 && P.why.empty()) P.why = "not progressive";
  if (!P.why.empty()) {
    if (kind == BASELINE) {   // vf_jpeg_inspect reports the extent of the first scan of a file it refuses, too
      ProgScanHost sc;
      sc.begin = P.scan_begin;
      int end_marker;
      if (int e = jpg_walk(d, n, sc.begin, sc.segs, sc.drops, sc.end, end_marker, msg)) return e;
      G.scans.push_back(std::move(sc));
    }
    return 0;
  }
  const bool seq = P.sof != 0xC2;
  G.tabs.reserve(6);           // what one scan of three components names at most
  int cov[3][64];              // the Al each coefficient was last coded at; -1: not yet
  for (auto& c : cov)
    for (int& k : c) k = -1;
  bool latched[3] = {false, false, false};
  int dc_at[4] = {-1, -1, -1, -1}, ac_at[4] = {-1, -1, -1, -1};   // the slots' places in G.tabs, -1 after a DHT
  for (;;) {
    // the scan whose SOS jpg_sos left in P
    if ((int)G.scans.size() == kProgMaxScans) {
      P.why = "more than " + std::to_string(kProgMaxScans) + " scans";
      return 0;
    }
    const std::string at = kind == BASELINE ? "" : "scan " + std::to_string(G.scans.size()) + ": ";   // a baseline file has the one
    ProgScanHost sc;
    sc.ns = P.ns;
    sc.ss = P.ss;
    sc.se = P.se;
    sc.ah = P.ahal >> 4;
    sc.al = P.ahal & 15;
    sc.ri = P.ri;
    sc.begin = P.scan_begin;
    sc.seq = seq;
    if (seq && (sc.ss != 0 || sc.se != 63 || P.ahal != 0)) {
      P.why = "non-baseline scan parameters";
      return 0;
    }
    bool bad = seq ? false : sc.ss > sc.se || sc.se > 63 || (sc.ss == 0 && sc.se != 0) || (sc.ss > 0 && sc.ns != 1) || sc.al > 13 ||
               (sc.ah != 0 && sc.al != sc.ah - 1) || sc.ns > P.ncomp;
    if (bad) {   // jdphuff.c start_pass_phuff_decoder: JERR_BAD_PROGRESSION
      msg = at + "bad progression parameters Ss=" + std::to_string(sc.ss) + " Se=" + std::to_string(sc.se) +
            " Ah=" + std::to_string(sc.ah) + " Al=" + std::to_string(sc.al) + " with " + std::to_string(sc.ns) + " components";
      return 2;
    }
    for (int i = 0; i < sc.ns && seq; ++i) {
      // the scan's tables as they stand at this SOS, side by side: DC and AC of each component, equal slots shared
      sc.scomp[i] = P.scomp[i];
      // baseline has two slots of each class; extended sequential four, which only the layouts rule takes
      const int top = kind == LAYOUTS && P.sof != 0xC0 ? 3 : 1;
      for (int ac = 0; ac < 2; ++ac) {
        const int slot = ac ? P.ta[i] : P.td[i];
        const RawHuff* h = slot <= top ? (ac ? &P.hac[slot] : &P.hdc[slot]) : nullptr;
        if (!h || !h->present) {
          P.why = "missing Huffman table (or one beyond baseline's two)";
          return 0;
        }
        if (!h->fits) {
          msg = at + "bad Huffman table: its code counts overflow the code lengths";
          return 2;
        }
        for (int v = 0; v < h->nval && !ac; ++v)
          if (h->val[v] > 15 && P.why.empty()) P.why = "DC Huffman symbol above 15";
        int found = -1;
        for (int j = 0; j < i; ++j)
          if ((ac ? P.ta[j] : P.td[j]) == slot) found = ac ? sc.atab[j] : sc.dtab[j];
        if (found < 0) {
          found = sc.ntab++;
          if (found == 0) sc.tab[0] = (int)G.tabs.size();
          G.tabs.push_back(*h);
        }
        (ac ? sc.atab[i] : sc.dtab[i]) = found;
      }
    }
    for (int i = 0; i < sc.ns && !seq; ++i) {
      sc.scomp[i] = P.scomp[i];
      if (sc.ss == 0 && sc.ah != 0) continue;   // DC refinement reads raw bits
      const bool dc = sc.ss == 0;
      const int slot = dc ? P.td[i] : P.ta[i];
      const RawHuff* h = slot <= 3 ? (dc ? &P.hdc[slot] : &P.hac[slot]) : nullptr;
      if (!h || !h->present) {
        msg = at + "names " + (dc ? "DC" : "AC") + " Huffman table " + std::to_string(slot) + ", which no DHT has defined";
        return 2;
      }
      if (!h->fits) {
        msg = at + "bad Huffman table: its code counts overflow the code lengths";
        return 2;
      }
      if (dc)
        for (int v = 0; v < h->nval; ++v)
          if (h->val[v] > 15 && P.why.empty()) P.why = "DC Huffman symbol above 15";
      int& where = dc ? dc_at[slot] : ac_at[slot];
      if (where < 0) {
        where = (int)G.tabs.size();
        G.tabs.push_back(*h);
      }
      sc.tab[i] = where;
    }
    // orderly: a first scan covers new ground, a refinement follows the Al before it, AC comes after the DC
    for (int i = 0; i < sc.ns && seq; ++i)
      if (cov[sc.scomp[i]][0] >= 0) {
        msg = at + "component " + std::to_string(sc.scomp[i]) + " is coded in two scans";
        return 2;
      }
    for (int i = 0; i < sc.ns && P.why.empty(); ++i) {
      const int c = sc.scomp[i];
      if (sc.ss > 0 && cov[c][0] < 0) P.why = "progression out of order";
      for (int k = sc.ss; k <= sc.se; ++k)
        if (sc.ah == 0 ? cov[c][k] >= 0 : cov[c][k] != sc.ah) P.why = "progression out of order";
      for (int k = sc.ss; k <= sc.se; ++k) cov[c][k] = sc.al;
      if (!latched[c]) {
        if (P.tq[c] > 3 || !P.qt_ok[P.tq[c]]) P.why = "missing quantisation table";
        else memcpy(G.q[c], P.qt[P.tq[c]], sizeof(G.q[c]));
        latched[c] = true;
      }
    }
    if (!P.why.empty()) return 0;
    if (sc.ns > 1) {
      sc.nunit = G.mcux() * G.mcuy();
      int nb = 0;
      for (int i = 0; i < sc.ns; ++i) nb += G.h(sc.scomp[i]) * G.v(sc.scomp[i]);
      if (nb > kProgMaxMcuBlocks) {
        msg = at + "more than 10 blocks in an MCU";
        return 2;
      }
    } else {
      const int c = sc.scomp[0];
      sc.nunit = vf_cdiv(vf_cdiv((int64_t)P.W * G.h(c), G.hmax()), 8) * vf_cdiv(vf_cdiv((int64_t)P.H * G.v(c), G.vmax()), 8);
    }
    for (size_t t = 0; t < G.scans.size(); ++t) {
      const ProgScanHost& o = G.scans[t];
      bool shares = false;
      for (int i = 0; i < sc.ns; ++i)
        for (int j = 0; j < o.ns; ++j) shares |= sc.scomp[i] == o.scomp[j];
      if (shares && o.ss <= sc.se && sc.ss <= o.se) sc.level = std::max(sc.level, o.level + 1);
    }
    G.nlevel = std::max(G.nlevel, sc.level + 1);
    int end_marker = -1;
    const int64_t want = sc.ri > 0 ? vf_cdiv(sc.nunit, sc.ri) : 1;
    sc.segs.reserve((size_t)std::min(want, n));
    if (int e = jpg_walk(d, n, sc.begin, sc.segs, sc.drops, sc.end, end_marker, msg)) {
      msg = at + msg;
      return e;
    }
    if ((int64_t)sc.segs.size() != want) {
      msg = at + "found " + std::to_string(sc.segs.size()) + " restart segments, the restart interval gives " + std::to_string(want);
      return 2;
    }
    for (const auto& sg : sc.segs)
      if (sg.end - sg.begin > (int64_t)1 << 28) P.why = "a restart segment above 256 MiB";
    int64_t p = sc.end;
    G.scans.push_back(std::move(sc));
    if (!P.why.empty()) return 0;
    // the markers up to the next SOS or EOI; data that just stops ends the file (libjpeg inserts an EOI)
    bool next = false;
    while (!next) {
      if (p >= n || d[p] != 0xFF) break;
      while (p < n && d[p] == 0xFF) ++p;
      if (p >= n) break;
      const int m = d[p++];
      if (m == 0xD9) break;
      if (kind == BASELINE) {   // a second SOS makes the file multi-scan; any other marker is skipped unread
        if (m == 0xDA) {
          P.why = "multi-scan sequential";
          return 0;
        }
        if (p + 2 > n) break;
        p += rd16(d + p);
        continue;
      }
      if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;
      if (p + 2 > n) break;
      const int L = rd16(d + p);
      if (L < 2 || p + L > n) {
        msg = "truncated marker 0x" + std::to_string(m) + " after " + at.substr(0, at.size() - 2);
        return 2;
      }
      const uint8_t* s = d + p + 2;
      const int sl = L - 2;
      if (m == 0xC4) {
        if (int e = jpg_dht(s, sl, P, msg)) return e;
        for (int t = 0; t < 4; ++t) dc_at[t] = ac_at[t] = -1;
      } else if (m == 0xDB) {
        if (int e = jpg_dqt(s, sl, P, msg)) return e;
      } else if (m == 0xDD) {
        if (sl < 2) {
          msg = "truncated DRI";
          return 2;
        }
        P.ri = rd16(s);
      } else if (m == 0xDA) {
        if (int e = jpg_sos(s, sl, P, msg)) return e;
        P.scan_begin = p + L;
        next = true;
      } else if (m >= 0xC0 && m <= 0xCF && m != 0xC8 && m != 0xCC) {
        msg = "more than one SOF marker";
        return 2;
      }
      p += L;
    }
    if (!next) break;
  }
  for (int c = 0; c < P.ncomp; ++c)
    for (int k = 0; k < 64; ++k)
      if (cov[c][k] != 0) P.why = seq ? "incomplete: component " + std::to_string(c) + " is in no scan" : "incomplete progression";
  P.supported = P.why.empty();
  return 0;
}

struct ProgPlan {
  std::vector<ProgParsed> G;
  int64_t nscan = 0, nseg = 0, nsub = 0, ntab = 0, nblk = 0, plane_bytes = 0, scan_bytes = 0, bits_bytes = 0, nchunk = 0;
  int64_t max_blocks = 0, max_pix = 0;
  std::vector<int64_t> level_segs;   // segments per level
  size_t o_img = 0, o_scans = 0, o_seg = 0, o_chunk = 0, o_huff = 0, o_scan = 0, stage = 0;
  size_t o_bits = 0, o_E = 0, o_X = 0, o_N = 0, o_D = 0, o_coef = 0, o_planes = 0, ws = 0;
};

// sub_bytes: the subsequence size of the first scans' decode (0: none of them is decoded that way).  bounds (the BASELINE
// rule's workspace query): upper bounds from the headers alone, so that a decode walks each file once.  A baseline file
// is one scan of at most four tables and as many segments as its restart interval gives; a segment's compacted length
// is at most its stuffed length, and the segments share the bytes from the scan's start to the end of the file.
int jpg_prog_plan(const JpgRule& rule, const uint8_t* data, const int64_t* offs, int n, int sub_bytes, ProgPlan& L, bool bounds = false) {
  const char* who = rule.who;
  VF_REQUIRE(n > 0 && data && offs, "%s: empty batch", who);
  VF_REQUIRE(sub_bytes == 0 || (sub_bytes >= 8 && sub_bytes <= (1 << 20)), "%s: subsequence size %d outside [8, 1 MiB]", who, sub_bytes);
  L.G.resize(n);
  for (int i = 0; i < n; ++i) {
    std::string msg;
    VF_REQUIRE(offs[i + 1] >= offs[i], "%s: offsets decrease at image %d", who, i);
    ProgParsed& G = L.G[i];
    if (jpg_prog_parse(data + offs[i], offs[i + 1] - offs[i], G, msg, rule.kind, !bounds)) {
      vf_set_error("%s: image %d: %s", who, i, msg.c_str());
      return 2;
    }
    if (!G.P.supported) {
      vf_set_error("%s: image %d: unsupported: %s", who, i, G.P.why.c_str());
      return 3;
    }
    L.nblk += G.nblocks();
    L.max_blocks = std::max(L.max_blocks, G.nblocks());
    L.max_pix = std::max(L.max_pix, (int64_t)G.P.W * G.P.H);
    L.plane_bytes = (int64_t)vf_up256((size_t)(L.plane_bytes + G.nblocks() * 64));
    if (bounds) {
      const int64_t nseg = G.P.ri > 0 ? vf_cdiv(G.mcux() * G.mcuy(), G.P.ri) : 1, sb = offs[i + 1] - offs[i] - G.P.scan_begin;
      L.nscan += 1;
      L.ntab += 4;
      L.nseg += nseg;
      L.nsub += vf_cdiv(sb, sub_bytes) + nseg;
      L.bits_bytes += sb + 32 * nseg;
      L.nchunk += vf_cdiv(sb, kChunk) + nseg;
      L.scan_bytes += (int64_t)vf_up256((size_t)sb + 8);
      continue;
    }
    L.nscan += (int64_t)G.scans.size();
    L.ntab += (int64_t)G.tabs.size();
    if ((int)L.level_segs.size() < G.nlevel) L.level_segs.resize(G.nlevel, 0);
    for (const auto& sc : G.scans) {
      L.nseg += (int64_t)sc.segs.size();
      L.level_segs[sc.level] += (int64_t)sc.segs.size();
      for (const auto& s : sc.segs) {
        L.bits_bytes += seg_bits_bytes(s.len);
        L.nchunk += vf_cdiv(s.end - s.begin, kChunk);
        if (sc.level == 0 && sub_bytes) L.nsub += std::max<int64_t>(1, vf_cdiv(s.len, sub_bytes));
      }
      L.scan_bytes += (int64_t)vf_up256((size_t)(sc.end - sc.begin) + 8);
    }
  }
  VF_REQUIRE(L.nseg < ((int64_t)1 << 31) && L.nchunk < ((int64_t)1 << 31), "%s: more than 2^31 restart segments or chunks", who);
  VfCarve ws;
  L.o_img = ws.take(sizeof(JpgImage) * n);
  L.o_scans = ws.take(sizeof(ProgScan) * L.nscan);
  L.o_seg = ws.take(sizeof(ProgSeg) * L.nseg);
  L.o_chunk = ws.take(sizeof(JpgChunk) * L.nchunk);
  L.o_huff = ws.take(sizeof(JpgHuff) * L.ntab);
  L.o_scan = ws.take((size_t)L.scan_bytes);
  L.stage = ws.at;
  L.o_bits = ws.take((size_t)L.bits_bytes);
  L.o_E = ws.take(8 * (size_t)L.nsub);
  L.o_X = ws.take(8 * (size_t)L.nsub);
  L.o_N = ws.take(4 * (size_t)L.nsub);
  L.o_D = ws.take((size_t)L.nsub);
  L.o_coef = ws.take(128 * (size_t)L.nblk);
  L.o_planes = ws.take((size_t)L.plane_bytes);
  L.ws = ws.at;
  return 0;
}

// fill the staging buffer; the segments lie level by level
// jdsample.c jinit_upsampler for a component that is 1 / rh by 1 / rv of the image and cw samples wide
int jpg_upsampler(int rh, int rv, int cw) {
  if (rh == 1 && rv == 1) return UP_COPY;
  if (rh == 2 && rv == 1 && cw > 2) return UP_H2V1;
  if (rh == 2 && rv == 2 && cw > 2) return UP_H2V2;
  if (rh == 1 && rv == 2) return UP_H1V2;
  return UP_INT;
}

void jpg_prog_pack(const uint8_t* data, const int64_t* offs, int n, int channels, int sub_bytes, const int64_t* out_offs, const ProgPlan& L,
                   uint8_t* st) {
  JpgImage* imgs = (JpgImage*)(st + L.o_img);
  ProgScan* scans = (ProgScan*)(st + L.o_scans);
  ProgSeg* segs = (ProgSeg*)(st + L.o_seg);
  JpgChunk* chunks = (JpgChunk*)(st + L.o_chunk);
  JpgHuff* huffs = (JpgHuff*)(st + L.o_huff);
  uint8_t* scan = st + L.o_scan;
  std::vector<int64_t> at(L.level_segs.size() + 1, 0);   // next free segment of each level
  for (size_t l = 0; l < L.level_segs.size(); ++l) at[l + 1] = at[l] + L.level_segs[l];
  int64_t coef = 0, plane = 0, sc_at = 0, dst = 0, sub = 0;
  int si = 0, ci = 0, ti = 0;
  for (int i = 0; i < n; ++i) {
    const ProgParsed& G = L.G[i];
    const JpgParsed& P = G.P;
    const uint8_t* d = data + offs[i];
    JpgImage& im = imgs[i];
    memset(&im, 0, sizeof(im));
    im.W = P.W;
    im.H = P.H;
    im.ncomp = P.ncomp;
    im.channels = channels;
    im.hs = G.hmax();
    im.vs = G.vmax();
    im.rgb = P.rgb;
    im.mcux = (int)G.mcux();
    im.mcuy = (int)G.mcuy();
    int cb0[3] = {0, 0, 0};   // each component's first block in the MCU (frame order)
    int b = 0;
    for (int c = 0; c < P.ncomp; ++c) {
      cb0[c] = b;
      for (int y = 0; y < G.v(c); ++y)
        for (int x = 0; x < G.h(c); ++x, ++b) {
          im.bcomp[b] = c;
          im.bx[b] = x;
          im.by[b] = y;
        }
    }
    im.bpm = b;
    im.nblocks = (int)G.nblocks();
    im.coef_base = coef;
    coef += im.nblocks;
    for (int c = 0; c < P.ncomp; ++c) {
      im.hc[c] = G.h(c);
      im.vc[c] = G.v(c);
      im.pw[c] = im.mcux * 8 * G.h(c);
      im.ph[c] = im.mcuy * 8 * G.v(c);
      im.cw[c] = (int)vf_cdiv((int64_t)P.W * G.h(c), G.hmax());
      im.ch[c] = (int)vf_cdiv((int64_t)P.H * G.v(c), G.vmax());
      im.up[c] = jpg_upsampler(G.hmax() / G.h(c), G.vmax() / G.v(c), im.cw[c]);
      im.plane_base[c] = plane;
      plane += (int64_t)im.pw[c] * im.ph[c];
      for (int k = 0; k < 64; ++k) im.q[c][k] = G.q[c][k];
    }
    plane = (int64_t)vf_up256((size_t)plane);
    im.out_off = out_offs[i];
    for (const RawHuff& r : G.tabs) build_huff(r, huffs[ti + (&r - G.tabs.data())]);
    for (const ProgScanHost& h : G.scans) {
      ProgScan& s = scans[si];
      memset(&s, 0, sizeof(s));
      s.img = i;
      s.ns = h.ns;
      s.ss = h.ss;
      s.se = h.se;
      s.ah = h.ah;
      s.al = h.al;
      s.nunit = (int32_t)h.nunit;
      s.interleaved = h.ns > 1;
      s.nb = 0;
      s.seq = h.seq;
      s.ntab = h.seq ? h.ntab : h.ns;
      for (int j = 0; j < h.ns; ++j) {
        const int c = h.scomp[j];
        s.tab[j] = h.tab[j] < 0 ? -1 : ti + h.tab[j];
        for (int y = 0; y < G.v(c); ++y)
          for (int x = 0; x < G.h(c); ++x, ++s.nb) {
            s.boff[s.nb] = cb0[c] + y * G.h(c) + x;
            s.bslot[s.nb] = j;
            s.dct[s.nb] = h.dtab[j];
            s.act[s.nb] = h.atab[j];
          }
      }
      for (int t = 0; t < 4 && h.seq; ++t) s.tab[t] = t < h.ntab ? ti + h.tab[0] + t : -1;
      if (!s.interleaved) {
        const int c = h.scomp[0];
        s.nb = 1;
        s.h = G.h(c);
        s.v = G.v(c);
        s.b0 = cb0[c];
        s.bw = (int32_t)vf_cdiv(vf_cdiv((int64_t)P.W * s.h, G.hmax()), 8);
      }
      const int64_t nbytes = h.end - h.begin;
      memcpy(scan + sc_at, d + h.begin, (size_t)nbytes);
      memset(scan + sc_at + nbytes, 0, vf_up256((size_t)nbytes + 8) - (size_t)nbytes);
      for (size_t k = 0; k < h.segs.size(); ++k) {
        const auto& g = h.segs[k];
        ProgSeg& o = segs[at[h.level]++];
        size_t di = std::lower_bound(h.drops.begin(), h.drops.end(), g.begin) - h.drops.begin();
        int64_t kept = 0;
        for (int64_t c0 = g.begin; c0 < g.end; c0 += kChunk, ++ci) {
          const int64_t c1 = std::min<int64_t>(c0 + kChunk, g.end);
          int64_t nd = 0;
          for (; di < h.drops.size() && h.drops[di] < c1; ++di) ++nd;
          JpgChunk& ck = chunks[ci];
          ck.src = sc_at + (c0 - h.begin);
          ck.dst = dst + kept;
          ck.n = (int32_t)(c1 - c0);
          ck.keep = (int32_t)(c1 - c0 - nd);
          ck.lo = c0 > g.begin;
          kept += ck.keep;
        }
        o.dst = dst;
        o.len = (int32_t)g.len;
        o.scan = si;
        o.u0 = (int32_t)(h.ri > 0 ? (int64_t)k * h.ri : 0);
        o.nu = (int32_t)(h.ri > 0 ? std::min<int64_t>(h.ri, h.nunit - o.u0) : h.nunit);
        o.nsub = h.level == 0 && sub_bytes ? (int32_t)std::max<int64_t>(1, vf_cdiv(g.len, sub_bytes)) : 0;
        o.sub0 = sub;
        sub += o.nsub;
        dst += seg_bits_bytes(g.len);
      }
      sc_at += (int64_t)vf_up256((size_t)nbytes + 8);
      ++si;
    }
    ti += (int)G.tabs.size();
  }
}

// k_jpeg_unstuff's rule for one chunk, on the host
void unstuff_host(const JpgChunk& ck, const uint8_t* scan, uint8_t* bits) {
  const uint8_t* in = scan + ck.src;
  uint8_t* out = bits + ck.dst;
  int pos = 0;
  for (int i = 0; i < ck.n; ++i) {
    const bool keep = !(in[i] == 0 && (i > 0 || ck.lo) && in[i - 1] == 0xFF);
    if (keep && pos < ck.keep) out[pos] = in[i];
    pos += keep;
  }
}

}  // namespace

VF_API int vf_jpeg_scans_inspect(const unsigned char* data, size_t len, int64_t* info, int64_t* scans, int scan_cap, char* reason,
                                 int reason_cap) {
  VF_REQUIRE(data && info, "vf_jpeg_scans_inspect: NULL argument");
  ProgParsed G;
  std::string msg;
  if (int rc = jpg_prog_parse(data, (int64_t)len, G, msg, PROGRESSIVE)) {
    vf_set_error("vf_jpeg_scans_inspect: %s", msg.c_str());
    return rc;
  }
  const JpgParsed& P = G.P;
  const bool geo = P.ncomp == 1 || P.ncomp == 3;
  info[0] = P.W;
  info[1] = P.H;
  info[2] = P.ncomp;
  info[3] = P.ncomp == 1 ? 1 : P.hf[0];
  info[4] = P.ncomp == 1 ? 1 : P.vf[0];
  info[5] = (int64_t)G.scans.size();
  info[6] = P.supported ? 1 : 0;
  info[7] = P.sof;
  info[8] = P.prec;
  info[9] = G.nlevel;
  info[10] = geo && P.W > 0 && P.H > 0 ? G.nblocks() : 0;
  info[11] = geo ? G.bpm() : 0;
  for (int i = 0; scans && i < scan_cap && i < (int)G.scans.size(); ++i) {
    const ProgScanHost& s = G.scans[i];
    int64_t* r = scans + 16 * i;
    r[0] = s.ns;
    for (int j = 0; j < 4; ++j) r[1 + j] = j < s.ns ? s.scomp[j] : -1;
    r[5] = s.ss;
    r[6] = s.se;
    r[7] = s.ah;
    r[8] = s.al;
    r[9] = s.ri;
    r[10] = s.begin;
    r[11] = s.end;
    r[12] = (int64_t)s.segs.size();
    r[13] = s.level;
    r[14] = s.nunit;
    r[15] = 0;
  }
  if (reason && reason_cap > 0) snprintf(reason, (size_t)reason_cap, "%s", P.why.c_str());
  return 0;
}

// the sizes of one batch under a rule: exact (every file is walked), or with bounds the header-only upper bounds
static int jpg_workspace_bytes(const JpgRule& rule, bool bounds, const unsigned char* data, const int64_t* offs, int n, int subseq_bytes,
                               size_t* ws_bytes, size_t* stage_bytes) {
  VF_REQUIRE(subseq_bytes != 0, "%s: subsequence size 0 outside [8, 1 MiB]", rule.who);
  ProgPlan L;
  if (int e = jpg_prog_plan(rule, data, offs, n, subseq_bytes, L, bounds)) return e;
  if (ws_bytes) *ws_bytes = L.ws;
  if (stage_bytes) *stage_bytes = L.stage;
  return 0;
}

VF_API int vf_jpeg_workspace_bytes(const unsigned char* data, const int64_t* offs, int n, int subseq_bytes, size_t* ws_bytes,
                                   size_t* stage_bytes) {
  return jpg_workspace_bytes(kBaselineRule, true, data, offs, n, subseq_bytes, ws_bytes, stage_bytes);
}

VF_API int vf_jpeg_prog_workspace_bytes(const unsigned char* data, const int64_t* offs, int n, int subseq_bytes, size_t* ws_bytes,
                                        size_t* stage_bytes) {
  return jpg_workspace_bytes(kProgressiveRule, false, data, offs, n, subseq_bytes, ws_bytes, stage_bytes);
}

VF_API int vf_jpeg_layouts_workspace_bytes(const unsigned char* data, const int64_t* offs, int n, int subseq_bytes, size_t* ws_bytes,
                                           size_t* stage_bytes) {
  return jpg_workspace_bytes(kLayoutsRule, false, data, offs, n, subseq_bytes, ws_bytes, stage_bytes);
}

// the assembled coefficients of one file on the host, under the progressive or the layouts rule
static int jpg_coefficients_host(const char* who, const JpgRule& rule, const unsigned char* data, size_t len, int subseq_bytes, int16_t* coef,
                                 size_t coef_blocks, int32_t* status) {
  VF_REQUIRE(data && coef && status, "%s: NULL argument", who);
  const int64_t offs[2] = {0, (int64_t)len}, out_offs[2] = {0, 0};
  ProgPlan L;
  if (int e = jpg_prog_plan(rule, data, offs, 1, subseq_bytes, L)) return e;
  VF_REQUIRE((int64_t)coef_blocks >= L.nblk, "%s: room for %zu blocks, the file has %lld", who, coef_blocks, (long long)L.nblk);
  std::vector<uint64_t> stage(L.stage / 8 + 1), bits((size_t)L.bits_bytes / 8 + 1, 0);
  uint8_t* st = (uint8_t*)stage.data();
  jpg_prog_pack(data, offs, 1, 3, subseq_bytes, out_offs, L, st);
  const JpgChunk* chunks = (const JpgChunk*)(st + L.o_chunk);
  for (int64_t c = 0; c < L.nchunk; ++c) unstuff_host(chunks[c], st + L.o_scan, (uint8_t*)bits.data());
  memset(coef, 0, 128 * (size_t)L.nblk);
  const JpgImage* im = (const JpgImage*)(st + L.o_img);
  const ProgScan* scans = (const ProgScan*)(st + L.o_scans);
  const ProgSeg* segs = (const ProgSeg*)(st + L.o_seg);
  *status = VF_JPEG_OK;
  for (int64_t s = 0; s < L.nseg; ++s) {   // level by level, as the device runs them
    const ProgSeg& sg = segs[s];
    const ProgScan& sc = scans[sg.scan];
    const JpgHuff* huff = (const JpgHuff*)(st + L.o_huff);
    const uint32_t* b = (const uint32_t*)((uint8_t*)bits.data() + sg.dst);
    const int e = sc.ah == 0 && subseq_bytes ? prog_first_segment_host(*im, sc, huff, b, sg.len, subseq_bytes, sg.u0, sg.nu, coef)
                                             : prog_decode_segment(*im, sc, huff, b, 8u * (uint32_t)sg.len, sg.u0, sg.nu, coef);
    *status = std::max(*status, e);
  }
  return 0;
}

VF_API int vf_jpeg_prog_coefficients_host(const unsigned char* data, size_t len, int subseq_bytes, int16_t* coef, size_t coef_blocks,
                                          int32_t* status) {
  return jpg_coefficients_host("vf_jpeg_prog_coefficients_host", kProgressiveRule, data, len, subseq_bytes, coef, coef_blocks, status);
}

VF_API int vf_jpeg_layouts_coefficients_host(const unsigned char* data, size_t len, int subseq_bytes, int16_t* coef, size_t coef_blocks,
                                             int32_t* status) {
  return jpg_coefficients_host("vf_jpeg_layouts_coefficients_host", kLayoutsRule, data, len, subseq_bytes, coef, coef_blocks, status);
}

// every entry's decode.  All first scans share level 0's launch: the one scan of a baseline file, the scans of a
// sequential file (layouts) and the first scans of a progressive one
static int jpg_scans_decode(const char* who, const JpgRule& rule, vf_ctx* ctx, const unsigned char* data, const int64_t* offs, int n, int channels,
                            int subseq_bytes, const int64_t* out_offs, unsigned char* out, void* stage, size_t stage_bytes, void* ws,
                            size_t ws_bytes, int32_t* status, int32_t* rounds, int32_t* levels) {
  VF_REQUIRE(channels == 1 || channels == 3, "%s: channels %d is not 1 or 3", who, channels);
  VF_REQUIRE(out && out_offs && stage && ws && status && rounds, "%s: NULL argument", who);
  VF_REQUIRE(subseq_bytes != 0, "%s: subsequence size 0 outside [8, 1 MiB]", rule.who);
  ProgPlan L;
  if (int e = jpg_prog_plan(rule, data, offs, n, subseq_bytes, L)) return e;
  VF_REQUIRE(stage_bytes >= L.stage && ws_bytes >= L.ws, "%s: staging %zu / workspace %zu bytes, need %zu / %zu", who, stage_bytes, ws_bytes,
             L.stage, L.ws);
  for (int i = 0; i < n; ++i)
    VF_REQUIRE(!(L.G[i].P.ncomp == 3 && channels == 1), "%s: image %d is %s; channels=1 takes grayscale files only", who, i,
               L.G[i].P.rgb ? "RGB" : "YCbCr");
  jpg_prog_pack(data, offs, n, channels, subseq_bytes, out_offs, L, (uint8_t*)stage);
  uint8_t* w = (uint8_t*)ws;
  JpgBatch B = {};
  B.img = (const JpgImage*)(w + L.o_img);
  B.chunk = (const JpgChunk*)(w + L.o_chunk);
  B.huff = (const JpgHuff*)(w + L.o_huff);
  B.scan = w + L.o_scan;
  B.bits = w + L.o_bits;
  B.E = (uint64_t*)(w + L.o_E);
  B.X = (uint64_t*)(w + L.o_X);
  B.Nb = (int32_t*)(w + L.o_N);
  B.D = w + L.o_D;
  B.coef = (int16_t*)(w + L.o_coef);
  B.planes = w + L.o_planes;
  B.out = out;
  B.status = status;
  B.rounds = rounds;
  B.nchunk = (int)L.nchunk;
  B.sub_bits = 8 * subseq_bytes;
  hipStream_t st = ctx->stream;
  {
    VfRange r(rule.upload);
    VF_CHECK_HIP(hipMemcpyAsync(w, stage, L.stage, hipMemcpyHostToDevice, st));
    VF_CHECK_HIP(hipMemsetAsync(w + L.o_coef, 0, (size_t)(128 * L.nblk), st));
    VF_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t) * n, st));
    VF_CHECK_HIP(hipMemsetAsync(rounds, 0, sizeof(int32_t), st));
  }
  const int64_t sb = L.scan_bytes;
  VF_LAUNCH_TIMED(ctx, "jpeg_unstuff", 0.0, 2.0 * sb, k_jpeg_unstuff, dim3((unsigned)std::max<int64_t>(1, vf_cdiv(L.nchunk, 4))), dim3(256), B);
  VF_LAUNCH_CHECK();
  // one launch per level: level 0 holds the first scans (a first scan covers new ground, so it waits for nothing), a
  // block each; the levels behind hold the refinements
  const ProgScan* d_scans = (const ProgScan*)(w + L.o_scans);
  const ProgSeg* d_segs = (const ProgSeg*)(w + L.o_seg);
  int64_t first = 0;
  for (size_t l = 0; l < L.level_segs.size(); ++l) {
    const int64_t cnt = L.level_segs[l];
    if (cnt > 0 && l == 0) {
      VF_LAUNCH_TIMED(ctx, rule.entropy, 0.0, 3.0 * sb / (double)L.level_segs.size(), k_jpeg_prog_first, dim3((unsigned)cnt), dim3(kHuffThreads),
                      B, d_scans, d_segs);
      VF_LAUNCH_CHECK();
    } else if (cnt > 0) {
      // A refinement level with few segments gives each its own wave (one lane's walk is not slowed by the divergent
      // walks of 63 others); many segments share waves
      const int lanes = (int)std::min<int64_t>(64, std::max<int64_t>(1, vf_cdiv(cnt, 8192)));
      VF_LAUNCH_TIMED(ctx, "jpeg_prog_refine", 0.0, 3.0 * sb / (double)L.level_segs.size(), k_jpeg_prog_scan, dim3((unsigned)vf_cdiv(cnt, lanes)),
                      dim3(lanes), B, d_scans, d_segs, (int)first, (int)cnt);
      VF_LAUNCH_CHECK();
    }
    first += cnt;
  }
  const unsigned gb = (unsigned)std::min<int64_t>(vf_cdiv(L.max_blocks, 256), 4096);
  VF_LAUNCH_TIMED(ctx, "jpeg_idct", 0.0, 192.0 * L.nblk, k_jpeg_idct, dim3(gb, n), dim3(256), B);
  VF_LAUNCH_CHECK();
  const unsigned gp = (unsigned)std::min<int64_t>(vf_cdiv(L.max_pix, 256), 4096);
  if (rule.kind == LAYOUTS) VF_LAUNCH_TIMED(ctx, "jpeg_color", 0.0, 2.0 * L.plane_bytes, k_jpeg_color_layouts, dim3(gp, n), dim3(256), B);
  else VF_LAUNCH_TIMED(ctx, "jpeg_color", 0.0, 2.0 * L.plane_bytes, k_jpeg_color, dim3(gp, n), dim3(256), B);
  VF_LAUNCH_CHECK();
  if (levels) *levels = (int32_t)L.level_segs.size();
  return 0;
}

VF_API int vf_jpeg_prog_decode(vf_ctx* ctx, const unsigned char* data, const int64_t* offs, int n, int channels, int subseq_bytes,
                               const int64_t* out_offs, unsigned char* out, void* stage, size_t stage_bytes, void* ws, size_t ws_bytes,
                               int32_t* status, int32_t* rounds, int32_t* levels) {
  return jpg_scans_decode("vf_jpeg_prog_decode", kProgressiveRule, ctx, data, offs, n, channels, subseq_bytes, out_offs, out, stage, stage_bytes, ws,
                          ws_bytes, status, rounds, levels);
}

VF_API int vf_jpeg_decode_layouts(vf_ctx* ctx, const unsigned char* data, const int64_t* offs, int n, int channels, int subseq_bytes,
                                  const int64_t* out_offs, unsigned char* out, void* stage, size_t stage_bytes, void* ws, size_t ws_bytes,
                                  int32_t* status, int32_t* rounds, int32_t* levels) {
  return jpg_scans_decode("vf_jpeg_decode_layouts", kLayoutsRule, ctx, data, offs, n, channels, subseq_bytes, out_offs, out, stage, stage_bytes, ws,
                          ws_bytes, status, rounds, levels);
}

// info (int64[20]) = {width, height, components, h0, v0, h1, v1, h2, v2, colour (0 grey, 1 YCbCr, 2 RGB), scans, supported,
// sof, precision, levels, blocks, blocks per MCU, 0, 0, 0}
VF_API int vf_jpeg_inspect_layouts(const unsigned char* data, size_t len, int64_t* info, char* reason, int reason_cap) {
  VF_REQUIRE(data && info, "vf_jpeg_inspect_layouts: NULL argument");
  ProgParsed G;
  std::string msg;
  if (int rc = jpg_prog_parse(data, (int64_t)len, G, msg, LAYOUTS)) {
    vf_set_error("vf_jpeg_inspect_layouts: %s", msg.c_str());
    return rc;
  }
  const JpgParsed& P = G.P;
  const bool geo = (P.ncomp == 1 || P.ncomp == 3) && P.W > 0 && P.H > 0 && P.supported;
  for (int i = 0; i < 20; ++i) info[i] = 0;
  info[0] = P.W;
  info[1] = P.H;
  info[2] = P.ncomp;
  for (int c = 0; c < 3 && c < P.ncomp; ++c) {
    info[3 + 2 * c] = P.hf[c];
    info[4 + 2 * c] = P.vf[c];
  }
  info[9] = P.ncomp == 1 ? 0 : P.rgb ? 2 : 1;
  info[10] = (int64_t)G.scans.size();
  info[11] = P.supported ? 1 : 0;
  info[12] = P.sof;
  info[13] = P.prec;
  info[14] = G.nlevel;
  info[15] = geo ? G.nblocks() : 0;
  info[16] = geo ? G.bpm() : 0;
  if (reason && reason_cap > 0) snprintf(reason, (size_t)reason_cap, "%s", P.why.c_str());
  return 0;
}

VF_API int vf_jpeg_inspect(const unsigned char* data, size_t len, int scan_walk, int64_t* info, char* reason, int reason_cap) {
  VF_REQUIRE(data && info, "vf_jpeg_inspect: NULL argument");
  ProgParsed G;
  std::string msg;
  if (int rc = jpg_prog_parse(data, (int64_t)len, G, msg, BASELINE, scan_walk != 0)) {
    vf_set_error("vf_jpeg_inspect: %s", msg.c_str());
    return rc;
  }
  const JpgParsed& P = G.P;
  const ProgScanHost* sc = G.scans.empty() ? nullptr : &G.scans[0];   // the first scan, when it was walked
  info[0] = P.W;
  info[1] = P.H;
  info[2] = P.ncomp;
  info[3] = P.ncomp == 1 ? 1 : P.hf[0];
  info[4] = P.ncomp == 1 ? 1 : P.vf[0];
  info[5] = P.ri;
  info[6] = P.scan_begin;
  info[7] = sc ? sc->end : -1;
  info[8] = P.supported ? 1 : 0;
  info[9] = P.sof;
  info[10] = sc ? (int64_t)sc->segs.size() : -1;
  info[11] = P.prec;
  if (reason && reason_cap > 0) snprintf(reason, (size_t)reason_cap, "%s", P.why.c_str());
  return 0;
}

VF_API int vf_jpeg_decode(vf_ctx* ctx, const unsigned char* data, const int64_t* offs, int n, int channels, int subseq_bytes,
                          const int64_t* out_offs, unsigned char* out, void* stage, size_t stage_bytes, void* ws, size_t ws_bytes,
                          int32_t* status, int32_t* rounds) {
  return jpg_scans_decode("vf_jpeg_decode", kBaselineRule, ctx, data, offs, n, channels, subseq_bytes, out_offs, out, stage, stage_bytes, ws,
                          ws_bytes, status, rounds, nullptr);
}

