// vf_jpeg_enc.hip — batched baseline JPEG encoder: frames on the device in, whole JFIF files out, byte for byte
// what libjpeg's default compression writes (tests/jpeg_enc_ref.py is the rule in numpy).
//   k_jenc_dct        one thread per 8x8 block in scan (MCU) order: the block's samples straight from the source (byte rule, colour
//                     conversion, edge replication, chroma downsampling), jfdctint's two passes, the quantiser; int16 zig-zag.
//   k_jenc_size       one thread per block: its code length in bits (the DC difference against the previous real block of its
//                     component), an exclusive scan inside the tile of 256 blocks, the tile's sum.
//   k_jenc_tile_scan  one workgroup per image: the tiles' bit offsets, the image's bit count.
//   k_jenc_clear      zeros under each image's stream, as far as it goes.
//   k_jenc_write      one thread per block: its codes at its bit offset into the zeroed stream.  A dword that lies wholly
//                     inside a block is stored, the dwords at a block's two ends are OR-ed in.
//   k_jenc_ff_count / k_jenc_ff_scan / k_vf_file_offsets (vf_block.h) / k_jenc_stuff   0xFF bytes per chunk of 4096 stream bytes,
//                     their prefix and the file sizes, the files' places, then header, stream with a 0x00 behind every 0xFF,
//                     1-padding, EOI.
// Nine launches whatever the batch; a file's bytes depend on its own frame, the quality and the sampling only.
//
// The options (vf_jpeg_encode_opts: restart intervals, optimised Huffman tables) run the same kernels as their OPTS instances,
// which leave the code above as it is when every option is off, and four kernels of their own:
//   k_jenc_hist       with optimize: one thread per block, its symbols counted per image and table (LDS first, then global).
//   k_jenc_table      with optimize: one workgroup per image and table: jpeg_gen_optimal_table (the two smallest counts by a
//                     reduction, a merge as one step of all threads), the limiting to 16 bits, the canonical codes into the image's
//                     LUT, the table's DHT segment.
//   k_jenc_seg_scan   one workgroup per image: every restart segment's byte start (its bits rounded up to a byte, summed), and
//                     what has to be added to the image-wide bit offset of its blocks.
//   k_jenc_write<1>   also pads a segment's last byte with 1-bits; k_jenc_stuff<1> puts RSTn behind a segment's last byte and the
//                     image's own header (prefix, its DHT segments, DRI, SOS) in front.
// Twelve launches and one memset with optimize, ten without; nothing synchronises.
//
// The progressive file (vf_jpeg_encode_prog: SOF2, libjpeg's ten or six scans) shares k_jenc_dct, jenc_gen_table, k_jenc_clear
// and k_jenc_ff_count with the above; its own kernels and their list stand at the end of this file.
#include "vf_block.h"
#include "vf_common.h"

namespace {

constexpr int JENC_MAX_SIDE = 16384;
constexpr int JENC_TILE = 256;            // blocks per workgroup of k_jenc_size / k_jenc_write: one per thread
constexpr int JENC_CHUNK = 4096;          // stream bytes per workgroup of the stuffing kernels: 16 per thread
constexpr int JENC_BLOCK_BITS = 64 * 27;  // the bound on a block's code (vf_hip.h has the derivation), a multiple of 32
constexpr int JENC_HDR_CAP = 624;         // the colour header is 623 bytes, the grey one 333
constexpr int JENC_HDR_BUF = 632;         // ... and DRI adds 6
constexpr int JENC_DHT_STRIDE = 288;      // a DHT segment is at most 2 + 2 + 1 + 16 + 256 bytes

// Annex K, read out of a file libjpeg wrote at quality 50 (there the scaled tables are the base tables).  Quantisation tables in
// the file's zig-zag order; Huffman tables as their DHT segments carry them: BITS[16], then HUFFVAL.
constexpr unsigned char K_QUANT[2][64] = {
    {16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51,
     56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101,
     103, 99},
    {17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
constexpr unsigned char K_DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr unsigned char K_DC_VAL[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr unsigned char K_AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr unsigned char K_AC_VAL[2][162] = {
    {1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240,
     36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73,
     74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132,
     133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178,
     179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217,
     218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
    {0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240,
     21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71,
     72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130,
     131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169,
     170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215,
     216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}};
// zig-zag position -> row-major position in the block
constexpr unsigned char K_ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// symbol -> code << 8 | length, the canonical codes of the four tables (jchuff.c's jpeg_make_c_derived_tbl)
struct JencLut {
  unsigned dc[2][12];
  unsigned ac[2][256];
};
constexpr JencLut jenc_make_lut() {
  JencLut t{};
  for (int s = 0; s < 2; ++s) {
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < K_DC_BITS[s][len - 1]; ++i) t.dc[s][K_DC_VAL[k++]] = code++ << 8 | (unsigned)len;
      code <<= 1;
    }
    code = 0;
    k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < K_AC_BITS[s][len - 1]; ++i) t.ac[s][K_AC_VAL[s][k++]] = code++ << 8 | (unsigned)len;
      code <<= 1;
    }
  }
  return t;
}
__constant__ JencLut c_jenc_lut = jenc_make_lut();

struct JencHdr {                 // everything in front of the entropy-coded data; the same for every file of a batch
  unsigned w[JENC_HDR_BUF / 4];  // bytes in memory order
  int len;
  int split;                     // with optimize the image's own DHT segments stand in front of byte `split`; else it is len
};

struct JencArgs {
  const void* src;
  short* coef;                   // [n][nb][64]: quantised coefficients, zig-zag, blocks in scan order (dummies are not written)
  unsigned* blk_off;             // [n][nb]: bit offset of the block inside its tile
  unsigned* tile_sum;            // [n][tiles]
  unsigned long long* tile_off;  // [n][tiles]: bit offset of the tile inside its image's stream
  unsigned long long* img_bits;  // [n]
  unsigned* stream;              // [n][cap_words]: the unstuffed stream, big-endian dwords (bit p is bit 31 - p % 32 of dword p / 32)
  unsigned* ff_cnt;              // [n][chunks]
  unsigned long long* ff_pref;   // [n][chunks]: 0xFF bytes in front of the chunk
  unsigned char* out;
  int64_t* offsets;              // [n + 1]
  long long cap_words;
  int n, H, W, C, hs, vs;        // luma sampling factors; chroma is 1 x 1
  int mcux, mcuy, bpm, nb;       // MCUs across and down, blocks per MCU, blocks per image
  int wb, hb;                    // real luma blocks across and down
  int tiles, chunks;
  unsigned short quant[2][64];   // zig-zag order, times 8: the divisors of jcdctmgr.c
  // the options (the OPTS instances of the kernels read these, the others never)
  int spb, nseg, optimize;       // blocks per restart segment (nb without restarts), segments per image, tables per image or 0
  unsigned long long* seg_start; // [n][nseg]: byte offset of the segment inside its image's (padded, unstuffed) stream
  long long* seg_shift;          // [n][nseg]: 8 * seg_start - the image-wide bit offset of the segment's first block
  unsigned* counts;              // [n][4][256]: symbol counts of table 2 * (luma 0 / chroma 1) + (DC 0 / AC 1)
  JencLut* lut;                  // [n]
  unsigned char* dht;            // [n][4][JENC_DHT_STRIDE]: the DHT segments
  int* dht_len;                  // [n][4]
};

// where block g of an image's scan lies
struct JencPos {
  int comp, X, Y;                // component, block column and row inside the component
  bool real;
};
__device__ __forceinline__ JencPos jenc_pos(const JencArgs& a, int g) {
  const int m = g / a.bpm, j = g - m * a.bpm, my = m / a.mcux, mx = m - my * a.mcux, luma = a.hs * a.vs;
  JencPos p;
  if (j < luma) {
    const int by = j / a.hs, bx = j - by * a.hs;
    p.comp = 0; p.X = mx * a.hs + bx; p.Y = my * a.vs + by;
    p.real = p.X < a.wb && p.Y < a.hb;
  } else {                       // a chroma component has as many blocks as there are MCUs: none is a dummy
    p.comp = j - luma + 1; p.X = mx; p.Y = my; p.real = true;
  }
  return p;
}

// ---------------------------------------------------------------------------------------------------- samples, FDCT, quantiser
// jccolor.c, SCALEBITS 16
template <int KIND>
__device__ __forceinline__ int jenc_comp(const JencArgs& a, long long f, int y, int x, int comp) {
  const VfFrames fr{a.src, a.H, a.W, a.C};
  if (a.C == 1) return (int)vf_frame_byte<KIND>(fr, f, 0, y, x);
  const int r = (int)vf_frame_byte<KIND>(fr, f, 0, y, x), g = (int)vf_frame_byte<KIND>(fr, f, 1, y, x);
  const int b = (int)vf_frame_byte<KIND>(fr, f, 2, y, x);
  if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}
// One sample of a component plane padded to whole MCUs (jcprepct.c, jcsample.c).  Columns: the source is replicated to the right.
// Rows: the source is replicated down to a multiple of the luma vertical factor, the component is downsampled, and then ITS last
// row is replicated down: row r of a chroma plane of ch rows comes from source rows vs * min(r, ch - 1) and the one below.
template <int KIND>
__device__ __forceinline__ int jenc_sample(const JencArgs& a, long long f, int comp, int r, int c) {
  if (comp == 0 || a.hs == 1) return jenc_comp<KIND>(a, f, min(r, a.H - 1), min(c, a.W - 1), comp);
  const int x0 = min(2 * c, a.W - 1), x1 = min(2 * c + 1, a.W - 1);
  if (a.vs == 1) {               // h2v1: bias 0, 1, 0, 1 ...
    const int y = min(r, a.H - 1);
    return (jenc_comp<KIND>(a, f, y, x0, comp) + jenc_comp<KIND>(a, f, y, x1, comp) + (c & 1)) >> 1;
  }
  const int rc = min(r, (a.H + 1) / 2 - 1), y0 = min(2 * rc, a.H - 1), y1 = min(2 * rc + 1, a.H - 1);
  return (jenc_comp<KIND>(a, f, y0, x0, comp) + jenc_comp<KIND>(a, f, y0, x1, comp) + jenc_comp<KIND>(a, f, y1, x0, comp) +
          jenc_comp<KIND>(a, f, y1, x1, comp) + 1 + (c & 1)) >> 2;   // h2v2: bias 1, 2, 1, 2 ...
}

__device__ __forceinline__ int jenc_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
// one pass of jfdctint.c over eight values; CONST_BITS 13, PASS1_BITS 2
template <bool FIRST>
__device__ __forceinline__ void jenc_fdct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
  constexpr int N = FIRST ? 13 - 2 : 13 + 2;
  int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  d0 = FIRST ? (t10 + t11) << 2 : jenc_descale(t10 + t11, 2);
  d4 = FIRST ? (t10 - t11) << 2 : jenc_descale(t10 - t11, 2);
  int z1 = (t12 + t13) * 4433;
  d2 = jenc_descale(z1 + t13 * 6270, N);
  d6 = jenc_descale(z1 - t12 * 15137, N);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299;
  z1 *= -7373; z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d7 = jenc_descale(t4 + z1 + z3, N);
  d5 = jenc_descale(t5 + z2 + z4, N);
  d3 = jenc_descale(t6 + z2 + z3, N);
  d1 = jenc_descale(t7 + z1 + z4, N);
}

// Threads take the blocks in scan order: the luma and chroma blocks of an MCU sit in neighbouring lanes and fetch the same pixels.
// (Luma blocks first and chroma after them, so that a wave's lanes do alike, measured 16 % slower: the pixels are fetched twice.)
template <int KIND>
__global__ __launch_bounds__(256) void k_jenc_dct(JencArgs a) {
  __shared__ int s_q[2][64];
  __shared__ float s_r[2][64];
  if (threadIdx.x < 128) {
    const int d = a.quant[threadIdx.x >> 6][threadIdx.x & 63];
    s_q[threadIdx.x >> 6][threadIdx.x & 63] = d;
    s_r[threadIdx.x >> 6][threadIdx.x & 63] = 1.f / (float)d;
  }
  __syncthreads();
  const int g = blockIdx.x * 256 + threadIdx.x;
  const long long f = blockIdx.y;
  if (g >= a.nb) return;
  const JencPos p = jenc_pos(a, g);
  if (!p.real) return;
  int v[64];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[8 * i + j] = jenc_sample<KIND>(a, f, p.comp, 8 * p.Y + i, 8 * p.X + j) - 128;
    jenc_fdct8<true>(v[8 * i], v[8 * i + 1], v[8 * i + 2], v[8 * i + 3], v[8 * i + 4], v[8 * i + 5], v[8 * i + 6], v[8 * i + 7]);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) jenc_fdct8<false>(v[j], v[8 + j], v[16 + j], v[24 + j], v[32 + j], v[40 + j], v[48 + j], v[56 + j]);
  const int* q = s_q[p.comp ? 1 : 0];
  const float* r = s_r[p.comp ? 1 : 0];
  unsigned w[32];
#pragma unroll
  for (int k = 0; k < 64; ++k) {                  // jcdctmgr.c: sign(c) * ((|c| + d / 2) / d)
    // the integer quotient through a float estimate: |c| + d / 2 < 2^17 and d < 2^11 are exact floats, the product of two correctly
    // rounded factors is off by less than one, and the two comparisons settle it
    const int c = v[K_ZZ[k]], d = q[k], num = abs(c) + (d >> 1);
    int m = (int)((float)num * r[k]);
    m -= m * d > num;
    m += (m + 1) * d <= num;
    const unsigned h = (unsigned)(c < 0 ? -m : m) & 0xFFFFu;
    if (k & 1) w[k >> 1] |= h << 16;
    else w[k >> 1] = h;
  }
  uint4* dst = (uint4*)(a.coef + (f * a.nb + g) * 64);
#pragma unroll
  for (int i = 0; i < 8; ++i) dst[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}

// ------------------------------------------------------------------------------------------------------------- entropy coding
template <bool OPTS>
__device__ __forceinline__ void jenc_load_lut(JencLut& s, const JencArgs& a, long long f) {   // the code tables into LDS: lanes look up different symbols
  const unsigned* src = (const unsigned*)&c_jenc_lut;
  if constexpr (OPTS)
    if (a.optimize) src = (const unsigned*)(a.lut + f);
  unsigned* dst = (unsigned*)&s;
  for (int i = threadIdx.x; i < (int)(sizeof(JencLut) / 4); i += 256) dst[i] = src[i];
  __syncthreads();
}

// The DC value the difference of real block g is taken against: the DC of the previous real block of g's component in scan order,
// 0 for the first.  A luma dummy keeps the predictor, so the walk steps over dummies (at most three) and over the chroma blocks.
// OPTS: a restart resets the predictors, so the walk stops at the first block of g's segment.
template <bool OPTS>
__device__ __forceinline__ int jenc_pred(const JencArgs& a, const short* coef, int g, const JencPos& p) {
  const int g0 = OPTS ? g / a.spb * a.spb : 0;
  if (p.comp) return g - a.bpm >= g0 ? coef[(long long)(g - a.bpm) * 64] : 0;
  const int luma = a.hs * a.vs;
  for (int q = g - 1; q >= g0; --q) {
    const int j = q % a.bpm;
    if (j >= luma) { q -= j - luma; continue; }   // on a chroma block: the loop's --q lands on the MCU's last luma block
    if (jenc_pos(a, q).real) return coef[(long long)q * 64];
  }
  return 0;
}

// jchuff.c's encode_one_block of block g: sym(class 0 DC / 1 AC, table 0 luma / 1 chroma, symbol, extra bits, their count)
// receives every symbol in the order of the stream
template <bool OPTS, class SYM>
__device__ __forceinline__ void jenc_block_syms(const JencArgs& a, const short* coef, int g, SYM&& sym) {
  const JencPos p = jenc_pos(a, g);
  const int t = p.comp ? 1 : 0;
  if (!p.real) {                                   // a dummy: DC difference 0, then EOB
    sym(0, t, 0, 0u, 0);
    sym(1, t, 0, 0u, 0);
    return;
  }
  const uint4* src = (const uint4*)(coef + (long long)g * 64);
  unsigned w[32];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint4 u = src[i];
    w[4 * i] = u.x; w[4 * i + 1] = u.y; w[4 * i + 2] = u.z; w[4 * i + 3] = u.w;
  }
  {
    const int diff = (int)(short)(w[0] & 0xFFFFu) - jenc_pred<OPTS>(a, coef, g, p);
    const int n = 32 - __clz(abs(diff));
    sym(0, t, n, (unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1u), n);
  }
  int run = 0;
#pragma unroll
  for (int k = 1; k < 64; ++k) {
    const int c = (int)(short)((k & 1) ? w[k >> 1] >> 16 : w[k >> 1] & 0xFFFFu);
    if (c == 0) { ++run; continue; }
    for (; run > 15; run -= 16) sym(1, t, 0xF0, 0u, 0);
    const int n = 32 - __clz(abs(c));
    sym(1, t, run << 4 | n, (unsigned)(c < 0 ? c - 1 : c) & ((1u << n) - 1u), n);
    run = 0;
  }
  if (run) sym(1, t, 0, 0u, 0);
}
// ... as codes: put(bits, count) receives every code with its extra bits behind it, at most 26 bits
template <bool OPTS, class PUT>
__device__ __forceinline__ void jenc_block_codes(const JencArgs& a, const JencLut& s, const short* coef, int g, PUT&& put) {
  jenc_block_syms<OPTS>(a, coef, g, [&](int cls, int t, int v, unsigned ext, int n) {
    const unsigned e = cls ? s.ac[t][v] : s.dc[t][v];
    put((e >> 8) << n | ext, (int)(e & 255) + n);
  });
}

template <bool OPTS>
__global__ __launch_bounds__(256) void k_jenc_size(JencArgs a) {
  __shared__ JencLut s;
  __shared__ unsigned s_w[4];
  const int g = blockIdx.x * JENC_TILE + threadIdx.x;
  const long long f = blockIdx.y;
  jenc_load_lut<OPTS>(s, a, f);
  unsigned bits = 0;
  if (g < a.nb) jenc_block_codes<OPTS>(a, s, a.coef + f * a.nb * 64, g, [&](unsigned, int count) { bits += (unsigned)count; });
  unsigned total;
  const unsigned at = vf_block_excl_scan<unsigned, 256>(bits, s_w, total);
  if (g < a.nb) a.blk_off[f * a.nb + g] = at;
  if (threadIdx.x == 0) a.tile_sum[f * a.tiles + blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_jenc_tile_scan(JencArgs a) {
  __shared__ unsigned long long s_w[4];
  const long long f = blockIdx.x;
  unsigned long long run = 0;
  for (int base = 0; base < a.tiles; base += 256) {
    const int t = base + threadIdx.x;
    const unsigned long long v = t < a.tiles ? a.tile_sum[f * a.tiles + t] : 0ull;
    unsigned long long total;
    const unsigned long long e = vf_block_excl_scan<unsigned long long, 256>(v, s_w, total);
    if (t < a.tiles) a.tile_off[f * a.tiles + t] = run + e;
    run += total;
  }
  if (threadIdx.x == 0) a.img_bits[f] = run;
}

// zeros under the image's stream and no further: the chunks (of the stuffing kernels) that hold any of its bits
__global__ __launch_bounds__(256) void k_jenc_clear(JencArgs a) {
  const long long f = blockIdx.y;
  const unsigned long long begin = (unsigned long long)blockIdx.x * JENC_CHUNK;
  if (begin >= (a.img_bits[f] + 7) >> 3) return;
  ((uint4*)(a.stream + f * a.cap_words + (long long)(begin >> 2)))[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
}

template <bool OPTS>
__global__ __launch_bounds__(256) void k_jenc_write(JencArgs a) {
  __shared__ JencLut s;
  const int g = blockIdx.x * JENC_TILE + threadIdx.x;
  const long long f = blockIdx.y;
  jenc_load_lut<OPTS>(s, a, f);
  if (g >= a.nb) return;
  unsigned long long at = a.tile_off[f * a.tiles + blockIdx.x] + a.blk_off[f * a.nb + g];
  if constexpr (OPTS) at = (unsigned long long)((long long)at + a.seg_shift[f * a.nseg + g / a.spb]);
  unsigned* dst = a.stream + f * a.cap_words + (long long)(at >> 5);
  // the bits in front of the block inside its first dword belong to earlier blocks: they enter as zeros, and that dword is OR-ed
  unsigned long long acc = 0;
  int cnt = (int)(at & 31);
  bool first = true;
  jenc_block_codes<OPTS>(a, s, a.coef + f * a.nb * 64, g, [&](unsigned bits, int count) {
    acc = acc << count | bits;
    cnt += count;
    if (cnt >= 32) {
      cnt -= 32;
      const unsigned word = (unsigned)(acc >> cnt);
      if (first) atomicOr(dst, word);
      else *dst = word;
      first = false;
      ++dst;
      acc &= (1ull << cnt) - 1ull;
    }
  });
  if constexpr (OPTS)                              // a segment's last block fills its last byte with 1-bits (cnt stays <= 32)
    if ((g + 1 == a.nb || (g + 1) % a.spb == 0) && (cnt & 7)) {
      const int k = 8 - (cnt & 7);
      acc = acc << k | ((1ull << k) - 1ull);
      cnt += k;
    }
  if (cnt) atomicOr(dst, (unsigned)(acc << (32 - cnt)));
}

// ------------------------------------------------------------------------------------------------------- the options' kernels
// the symbols of every block of the stream that will be written (DC differences against the segment-aware predictor), counted
__global__ __launch_bounds__(256) void k_jenc_hist(JencArgs a) {
  __shared__ unsigned s_h[4 * 256];
  for (int i = threadIdx.x; i < 4 * 256; i += 256) s_h[i] = 0;
  __syncthreads();
  const int g = blockIdx.x * JENC_TILE + threadIdx.x;
  const long long f = blockIdx.y;
  if (g < a.nb)
    jenc_block_syms<true>(a, a.coef + f * a.nb * 64, g, [&](int cls, int t, int v, unsigned, int) { atomicAdd(&s_h[(2 * t + cls) * 256 + v], 1u); });
  __syncthreads();
  for (int i = threadIdx.x; i < 4 * 256; i += 256)
    if (s_h[i]) atomicAdd(a.counts + f * (4 * 256) + i, s_h[i]);
}

// the two smallest of two ascending pairs of distinct keys
__device__ __forceinline__ void jenc_min2(unsigned long long& lo, unsigned long long& hi, unsigned long long lo2, unsigned long long hi2) {
  if (lo2 < lo) {
    hi = min(lo, hi2);
    lo = lo2;
  } else {
    hi = min(hi, lo2);
  }
}

// jpeg_gen_optimal_table.  Thread i owns symbol i, thread 256 the reserved code point (no
// real symbol gets the all-ones code).  libjpeg's `others` chain behind a tree's head is the set of that tree's leaves, so a merge
// is one step of all threads: the leaves of both trees grow by one bit and take the head's name.  The two smallest counts come
// from a reduction over keys count << 32 | 511 - symbol: the smallest count, and among equals the LARGEST symbol, as jchuff.c's
// `<=` scan finds them.  A code longer than 32 bits, which libjpeg refuses (it takes more than nine million symbols in Fibonacci
// proportions), is not told apart here; the counters of the lengths have room for any tree.
//
// jenc_gen_table is the table of one workgroup of JENC_TABLE_THREADS: 256 counts in, the canonical codes (symbol -> code << 8 |
// length) of the first lut_n symbols into lut, the DHT segment of class and id tc_th into d, its length into *d_len.
constexpr int JENC_TABLE_THREADS = 320;
__device__ __forceinline__ void jenc_gen_table(const unsigned* counts, unsigned* lut, int lut_n, unsigned char* d, int* d_len, int tc_th) {
  constexpr int WAVES = JENC_TABLE_THREADS / 64;
  constexpr unsigned long long NONE = ~0ull;
  __shared__ unsigned long long s_min[2][WAVES][2];
  __shared__ int s_size[256], s_bits[264], s_first[17], s_start[18];
  const int i = threadIdx.x, lane = i & 63, wave = i >> 6;
  unsigned freq = i < 256 ? counts[i] : i == 256 ? 1u : 0u;
  int head = i, size = 0;
  for (int it = 0;; ++it) {
    unsigned long long lo = freq ? (unsigned long long)freq << 32 | (unsigned)(511 - i) : NONE, hi = NONE;
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long lo2 = __shfl_xor(lo, o), hi2 = __shfl_xor(hi, o);
      jenc_min2(lo, hi, lo2, hi2);
    }
    if (lane == 0) {
      s_min[it & 1][wave][0] = lo;
      s_min[it & 1][wave][1] = hi;
    }
    __syncthreads();                               // one barrier a round: the next round writes the other half of s_min
    lo = hi = NONE;
    for (int w = 0; w < WAVES; ++w) jenc_min2(lo, hi, s_min[it & 1][w][0], s_min[it & 1][w][1]);
    if (hi == NONE) break;                         // one tree left (the same in every thread)
    const int c1 = 511 - (int)(unsigned)lo, c2 = 511 - (int)(unsigned)hi;
    if (i == c1) freq += (unsigned)(hi >> 32);
    if (i == c2) freq = 0;
    if (head == c1 || head == c2) {
      ++size;
      head = c1;
    }
  }
  if (i < 256) s_size[i] = size;
  if (i < 264) s_bits[i] = 0;
  __syncthreads();
  if (i <= 256 && size) atomicAdd(&s_bits[min(size, 263)], 1);
  __syncthreads();
  if (i == 0) {
    for (int l = 32; l > 16; --l)                  // the limiting to 16 bits of Annex K.2
      while (s_bits[l] > 0) {
        int j = l - 2;
        while (j > 0 && s_bits[j] == 0) --j;
        s_bits[l] -= 2;
        s_bits[l - 1] += 1;
        s_bits[j + 1] += 2;
        s_bits[j] -= 1;
      }
    int l = 16;
    while (l > 0 && s_bits[l] == 0) --l;
    s_bits[l] -= 1;                                // the reserved code point leaves
    int code = 0, at = 0;
    for (l = 1; l <= 16; ++l) {
      s_first[l] = code;
      s_start[l] = at;
      code = (code + s_bits[l]) << 1;
      at += s_bits[l];
    }
    s_start[17] = at;
  }
  __syncthreads();
  // HUFFVAL: the symbols by their UNLIMITED length, then by value; the limited lengths are dealt out along that order
  const int nsym = s_start[17];
  unsigned entry = 0;
  if (i < 256 && size) {
    int pos = 0;
    for (int j = 0; j < 256; ++j) {
      const int sj = s_size[j];
      pos += (sj && sj < size) || (sj == size && j < i);
    }
    int l = 1;
    while (l < 16 && pos >= s_start[l + 1]) ++l;
    entry = (unsigned)(s_first[l] + pos - s_start[l]) << 8 | (unsigned)l;
    d[21 + pos] = (unsigned char)i;
  }
  if (i < lut_n) lut[i] = entry;
  if (i < 16) d[5 + i] = (unsigned char)s_bits[i + 1];
  if (i == 0) {
    d[0] = 0xFF;
    d[1] = 0xC4;
    d[2] = (unsigned char)((19 + nsym) >> 8);
    d[3] = (unsigned char)((19 + nsym) & 255);
    d[4] = (unsigned char)tc_th;
    *d_len = 21 + nsym;
  }
}
// table blockIdx.x (2 * (luma 0 / chroma 1) + (DC 0 / AC 1)) of image blockIdx.y
__global__ __launch_bounds__(JENC_TABLE_THREADS) void k_jenc_table(JencArgs a) {
  const int k = blockIdx.x, cls = k & 1, t = k >> 1;
  const long long f = blockIdx.y;
  jenc_gen_table(a.counts + (f * 4 + k) * 256, cls ? a.lut[f].ac[t] : a.lut[f].dc[t], cls ? 256 : 12,   // a DC category is at most 11
                 a.dht + (f * 4 + k) * JENC_DHT_STRIDE, a.dht_len + f * 4 + k, cls << 4 | t);
}

// One workgroup per image.  The image-wide scan gave every block its bit offset as if there were no restarts; segment s is the
// bits between its first block and the next segment's, rounded up to a byte, and its blocks move by seg_shift.  The image's bit
// count becomes that of the padded stream, a whole number of bytes, for the kernels that follow.
__global__ __launch_bounds__(256) void k_jenc_seg_scan(JencArgs a) {
  __shared__ unsigned long long s_w[4];
  const long long f = blockIdx.x;
  const unsigned long long all = a.img_bits[f];    // read before the first barrier; thread 0 replaces it behind the last
  auto at = [&](long long g) { return a.tile_off[f * a.tiles + g / JENC_TILE] + a.blk_off[f * a.nb + g]; };
  unsigned long long run = 0;
  for (int base = 0; base < a.nseg; base += 256) {
    const int s = base + threadIdx.x;
    unsigned long long p0 = 0, v = 0;
    if (s < a.nseg) {
      p0 = at((long long)s * a.spb);
      v = ((s + 1 < a.nseg ? at((long long)(s + 1) * a.spb) : all) - p0 + 7) >> 3;
    }
    unsigned long long total;
    const unsigned long long e = vf_block_excl_scan<unsigned long long, 256>(v, s_w, total);
    if (s < a.nseg) {
      a.seg_start[f * a.nseg + s] = run + e;
      a.seg_shift[f * a.nseg + s] = (long long)(8 * (run + e)) - (long long)p0;
    }
    run += total;
  }
  if (threadIdx.x == 0) a.img_bits[f] = 8 * run;
}

// -------------------------------------------------------------------------------------------------------------- byte stuffing
// The 16 stream bytes of a thread, the last byte of the stream padded with 1-bits: -> how many of them exist, b[] their values
__device__ __forceinline__ int jenc_bytes16(const JencArgs& a, long long f, unsigned long long bits, unsigned long long pos, unsigned* b) {
  const unsigned long long nbytes = (bits + 7) >> 3;
  if (pos >= nbytes) return 0;
  const uint4 u = *(const uint4*)(a.stream + f * a.cap_words + (long long)(pos >> 2));
  const unsigned w[4] = {u.x, u.y, u.z, u.w};
  const int have = (int)min(16ull, nbytes - pos);
#pragma unroll
  for (int i = 0; i < 16; ++i) b[i] = (w[i >> 2] >> (24 - 8 * (i & 3))) & 255u;
  if (pos + have == nbytes && (bits & 7)) {
    const unsigned pad = (1u << (8 - (int)(bits & 7))) - 1u;
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (i == have - 1) b[i] |= pad;
  }
  return have;
}

__global__ __launch_bounds__(256) void k_jenc_ff_count(JencArgs a) {
  __shared__ unsigned s_w[4];
  const long long f = blockIdx.y;
  const unsigned long long bits = a.img_bits[f], begin = (unsigned long long)blockIdx.x * JENC_CHUNK;
  if (begin >= (bits + 7) >> 3) return;
  unsigned b[16];
  const int have = jenc_bytes16(a, f, bits, begin + threadIdx.x * 16, b);
  unsigned cnt = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) cnt += i < have && b[i] == 255u;
  unsigned total;
  vf_block_excl_scan<unsigned, 256>(cnt, s_w, total);
  if (threadIdx.x == 0) a.ff_cnt[f * a.chunks + blockIdx.x] = total;
}

// one workgroup per image: 0xFF bytes in front of every chunk, and the file's size at offsets[f + 1] (summed by k_vf_file_offsets)
// OPTS: the header is the image's own (its DHT segments), and two marker bytes stand behind every segment but the last
template <bool OPTS>
__device__ __forceinline__ int jenc_dht_bytes(const JencArgs& a, long long f) {
  int d = 0;
  if constexpr (OPTS)
    for (int k = 0; k < a.optimize; ++k) d += a.dht_len[f * 4 + k];
  return d;
}
template <bool OPTS>
__global__ __launch_bounds__(256) void k_jenc_ff_scan(JencArgs a, int hdr_len) {
  __shared__ unsigned long long s_w[4];
  const long long f = blockIdx.x;
  if constexpr (OPTS) hdr_len += jenc_dht_bytes<true>(a, f) + 2 * (a.nseg - 1);
  const unsigned long long nbytes = (a.img_bits[f] + 7) >> 3;
  const long long used = (long long)((nbytes + JENC_CHUNK - 1) / JENC_CHUNK);
  unsigned long long run = 0;
  for (long long base = 0; base < used; base += 256) {
    const long long c = base + threadIdx.x;
    const unsigned long long v = c < used ? a.ff_cnt[f * a.chunks + c] : 0ull;
    unsigned long long total;
    const unsigned long long e = vf_block_excl_scan<unsigned long long, 256>(v, s_w, total);
    if (c < used) a.ff_pref[f * a.chunks + c] = run + e;
    run += total;
  }
  if (threadIdx.x == 0) a.offsets[f + 1] = (int64_t)(hdr_len + nbytes + run + 2);
}

// OPTS: RSTn (not stuffed) behind the last byte of every segment but the last, so a byte of segment s stands 2 * s further on; the
// header is hdr's bytes with the image's DHT segments let in at hdr.split.
template <bool OPTS>
__global__ __launch_bounds__(256) void k_jenc_stuff(JencArgs a, JencHdr hdr) {
  __shared__ unsigned s_w[4];
  const long long f = blockIdx.y;
  const unsigned long long bits = a.img_bits[f], nbytes = (bits + 7) >> 3, begin = (unsigned long long)blockIdx.x * JENC_CHUNK;
  if (begin >= nbytes) return;
  unsigned char* file = a.out + a.offsets[f];
  unsigned b[16];
  const unsigned long long pos = begin + threadIdx.x * 16;
  const int have = jenc_bytes16(a, f, bits, pos, b);
  unsigned cnt = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) cnt += i < have && b[i] == 255u;
  unsigned total;
  const unsigned before = vf_block_excl_scan<unsigned, 256>(cnt, s_w, total);
  const int dht = jenc_dht_bytes<OPTS>(a, f);
  unsigned char* dst = file + hdr.len + dht + begin + a.ff_pref[f * a.chunks + blockIdx.x] + threadIdx.x * 16 + before;
  if constexpr (OPTS) {
    const unsigned long long* start = a.seg_start + f * a.nseg;
    int s = 0;                                     // the segment of the thread's first byte: the last that starts at or before it
    if (have)
      for (int hi = a.nseg - 1; s < hi;) {
        const int mid = (s + hi + 1) >> 1;
        if (start[mid] <= pos) s = mid;
        else hi = mid - 1;
      }
    dst += 2 * (long long)s;
    unsigned long long next = s + 1 < a.nseg ? start[s + 1] : ~0ull;
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (i < have) {
        *dst++ = (unsigned char)b[i];
        if (b[i] == 255u) *dst++ = 0;
        if (pos + i + 1 == next) {
          *dst++ = 0xFF;
          *dst++ = (unsigned char)(0xD0 + (s & 7));
          ++s;
          next = s + 1 < a.nseg ? start[s + 1] : ~0ull;
        }
      }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (i < have) {
        *dst++ = (unsigned char)b[i];
        if (b[i] == 255u) *dst++ = 0;
      }
  }
  if constexpr (OPTS) {
    if (blockIdx.x == 0)
      for (int i = threadIdx.x; i < hdr.len + dht; i += 256) {
        if (i >= hdr.split && i < hdr.split + dht) {
          int k = 0, j = i - hdr.split;
          for (; j >= a.dht_len[f * 4 + k]; ++k) j -= a.dht_len[f * 4 + k];
          file[i] = a.dht[(f * 4 + k) * JENC_DHT_STRIDE + j];
        } else {
          const int j = i < hdr.split ? i : i - dht;
          file[i] = (unsigned char)(hdr.w[j >> 2] >> (8 * (j & 3)));
        }
      }
  } else if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < hdr.len; i += 256) file[i] = (unsigned char)(hdr.w[i >> 2] >> (8 * (i & 3)));
  if (begin + JENC_CHUNK >= nbytes && threadIdx.x == 0) {
    const int64_t size = a.offsets[f + 1] - a.offsets[f];
    file[size - 2] = 0xFF;
    file[size - 1] = 0xD9;
  }
}

// ----------------------------------------------------------------------------------------------------------------------- host
struct JencPlan {
  int hs, vs, mcux, mcuy, bpm, nb, tiles, chunks;
  int interval, nseg, spb, tables;   // the options: MCUs per restart interval (0: none), segments, blocks per segment, optimised tables
  long long cap_bytes;           // an image's unstuffed stream, a whole number of chunks
  size_t o_coef, o_blk, o_tsum, o_toff, o_bits, o_stream, o_ffc, o_ffp, ws_bytes, out_bytes;
  size_t o_sstart, o_sshift, o_counts, o_lut, o_dht, o_dlen;
  bool opts() const { return interval || tables; }
};

int jenc_plan(const char* who, int n, int H, int W, int C, int subsampling, int restart_rows, int restart_blocks, int optimize,
              JencPlan* p) {
  VF_REQUIRE(C == 1 || C == 3, "%s: C = %d channels (a JPEG frame here is grey, 1 channel, or RGB, 3)", who, C);
  VF_REQUIRE(H >= 1 && H <= JENC_MAX_SIDE, "%s: H = %d (sides are 1 to %d)", who, H, JENC_MAX_SIDE);
  VF_REQUIRE(W >= 1 && W <= JENC_MAX_SIDE, "%s: W = %d (sides are 1 to %d)", who, W, JENC_MAX_SIDE);
  VF_REQUIRE(n >= 1 && n <= 65535, "%s: n = %d frames (1 to 65535)", who, n);
  VF_REQUIRE(C == 1 || (subsampling >= 0 && subsampling <= 2), "%s: subsampling = %d is not 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0)", who,
             subsampling);
  VF_REQUIRE(restart_rows >= 0 && restart_rows <= 65535, "%s: restart_rows = %d (0 to 65535 rows of MCUs)", who, restart_rows);
  VF_REQUIRE(restart_blocks >= 0 && restart_blocks <= 65535, "%s: restart_blocks = %d (0 to 65535 MCUs, what DRI can say)", who,
             restart_blocks);
  VF_REQUIRE(optimize == 0 || optimize == 1, "%s: optimize = %d is not 0 or 1", who, optimize);
  p->hs = C == 3 && subsampling >= 1 ? 2 : 1;
  p->vs = C == 3 && subsampling == 2 ? 2 : 1;
  p->mcux = (int)vf_cdiv(W, 8 * p->hs);
  p->mcuy = (int)vf_cdiv(H, 8 * p->vs);
  p->bpm = C == 3 ? p->hs * p->vs + 2 : 1;
  p->nb = p->mcux * p->mcuy * p->bpm;
  p->tiles = (int)vf_cdiv(p->nb, JENC_TILE);
  // jcmaster.c: rows of MCUs win over MCUs and are clamped to what DRI can say
  const int mcus = p->mcux * p->mcuy;
  p->interval = restart_rows > 0 ? (restart_rows * p->mcux < 65535 ? restart_rows * p->mcux : 65535) : restart_blocks;
  p->nseg = p->interval ? (int)vf_cdiv(mcus, p->interval) : 1;
  p->spb = p->interval && p->interval < mcus ? p->interval * p->bpm : p->nb;
  p->tables = optimize ? (C == 3 ? 4 : 2) : 0;
  // every segment but the last may end in a pad byte of its own
  p->cap_bytes = vf_cdiv((long long)p->nb * (JENC_BLOCK_BITS / 8) + (p->interval ? p->nseg : 0), JENC_CHUNK) * JENC_CHUNK;
  p->chunks = (int)(p->cap_bytes / JENC_CHUNK);
  const size_t blocks = (size_t)n * p->nb;
  VfCarve ws;
  p->o_coef = ws.take(blocks * 128);
  p->o_blk = ws.take(blocks * 4);
  p->o_tsum = ws.take((size_t)n * p->tiles * 4);
  p->o_toff = ws.take((size_t)n * p->tiles * 8);
  p->o_bits = ws.take((size_t)n * 8);
  p->o_stream = ws.take((size_t)n * p->cap_bytes);
  p->o_ffc = ws.take((size_t)n * p->chunks * 4);
  p->o_ffp = ws.take((size_t)n * p->chunks * 8);
  if (p->opts()) {
    p->o_sstart = ws.take((size_t)n * p->nseg * 8);
    p->o_sshift = ws.take((size_t)n * p->nseg * 8);
  }
  if (p->tables) {
    p->o_counts = ws.take((size_t)n * 4 * 256 * 4);
    p->o_lut = ws.take((size_t)n * sizeof(JencLut));
    p->o_dht = ws.take((size_t)n * 4 * JENC_DHT_STRIDE);
    p->o_dlen = ws.take((size_t)n * 4 * 4);
  }
  p->ws_bytes = ws.at;
  // every block at its bound, every stream byte stuffed; header and EOI.  With an interval: DRI, and per segment a pad byte, its
  // stuffing byte and two marker bytes.  An optimised code is at most 16 bits too, and its DHT segments are no longer than Annex K's.
  p->out_bytes = (size_t)n * ((size_t)p->nb * (JENC_BLOCK_BITS / 8) * 2 + JENC_HDR_CAP + 2 + (p->interval ? 4 * (size_t)p->nseg + 6 : 0));
  return 0;
}

struct JencHdrW {
  unsigned char b[JENC_HDR_BUF];
  int len = 0;
  void put(int v) { b[len++] = (unsigned char)v; }
  void put16(int v) { put(v >> 8); put(v & 255); }
};

// SOI, APP0 (JFIF 1.1, density 1:1), DQT per table, SOF0, DHT per table (with optimize: left out, the images bring their own),
// DRI for a non-zero interval, SOS; -> the divisors too
void jenc_header(int H, int W, int C, int quality, int hs, int vs, int interval, bool optimize, JencHdr* hdr, unsigned short quant[2][64]) {
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  unsigned char qt[2][64];
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 64; ++k) {
      const int v = (K_QUANT[t][k] * scale + 50) / 100;
      qt[t][k] = (unsigned char)(v < 1 ? 1 : v > 255 ? 255 : v);
      quant[t][k] = (unsigned short)(8 * qt[t][k]);
    }
  JencHdrW h;
  h.put(0xFF); h.put(0xD8);
  h.put(0xFF); h.put(0xE0); h.put16(16);
  for (const char c : {'J', 'F', 'I', 'F', '\0'}) h.put(c);
  h.put(1); h.put(1); h.put(0); h.put16(1); h.put16(1); h.put(0); h.put(0);
  for (int t = 0; t < (C == 3 ? 2 : 1); ++t) {
    h.put(0xFF); h.put(0xDB); h.put16(67); h.put(t);
    for (int k = 0; k < 64; ++k) h.put(qt[t][k]);
  }
  h.put(0xFF); h.put(0xC0); h.put16(8 + 3 * C); h.put(8); h.put16(H); h.put16(W); h.put(C);
  for (int c = 0; c < C; ++c) { h.put(c + 1); h.put(c == 0 ? hs << 4 | vs : 0x11); h.put(c == 0 ? 0 : 1); }
  for (int t = 0; t < (C == 3 ? 2 : 1) && !optimize; ++t) {
    h.put(0xFF); h.put(0xC4); h.put16(2 + 1 + 16 + 12); h.put(t);
    for (int i = 0; i < 16; ++i) h.put(K_DC_BITS[t][i]);
    for (int i = 0; i < 12; ++i) h.put(K_DC_VAL[i]);
    h.put(0xFF); h.put(0xC4); h.put16(2 + 1 + 16 + 162); h.put(0x10 | t);
    for (int i = 0; i < 16; ++i) h.put(K_AC_BITS[t][i]);
    for (int i = 0; i < 162; ++i) h.put(K_AC_VAL[t][i]);
  }
  hdr->split = h.len;
  if (interval) { h.put(0xFF); h.put(0xDD); h.put16(4); h.put16(interval); }
  h.put(0xFF); h.put(0xDA); h.put16(6 + 2 * C); h.put(C);
  for (int c = 0; c < C; ++c) { h.put(c + 1); h.put(c == 0 ? 0x00 : 0x11); }
  h.put(0); h.put(63); h.put(0);
  memset(hdr->w, 0, sizeof(hdr->w));
  memcpy(hdr->w, h.b, (size_t)h.len);
  hdr->len = h.len;
}

int jenc_workspace_bytes(const char* who, int n, int H, int W, int C, int subsampling, int restart_rows, int restart_blocks,
                         int optimize, size_t* ws_bytes, size_t* out_bytes) {
  JencPlan p;
  if (int e = jenc_plan(who, n, H, W, C, subsampling, restart_rows, restart_blocks, optimize, &p)) return e;
  if (ws_bytes) *ws_bytes = p.ws_bytes;
  if (out_bytes) *out_bytes = p.out_bytes;
  return 0;
}

// The launches of one call.  OPTS false is the default file's nine; OPTS true lets in the counts and the tables behind the DCT
// (optimize) and the segments' places behind the tile scan.
template <bool OPTS>
int jenc_launch(vf_ctx* ctx, const JencPlan& p, const JencArgs& a, const JencHdr& hdr, int kind) {
  const int n = a.n;
  const double px = (double)n * a.H * a.W * a.C, coef = (double)n * p.nb * 128;
  const dim3 per_tile((unsigned)p.tiles, n), per_chunk((unsigned)p.chunks, n);
  if (kind == 0) VF_LAUNCH_TIMED(ctx, "jpeg_enc_dct", 0.0, 4.0 * px + coef, k_jenc_dct<0>, per_tile, dim3(256), a);
  else VF_LAUNCH_TIMED(ctx, "jpeg_enc_dct", 0.0, px + coef, k_jenc_dct<1>, per_tile, dim3(256), a);
  VF_LAUNCH_CHECK();
  if constexpr (OPTS)
    if (p.tables) {
      VfProf prof(ctx, "jpeg_enc_tables", 0.0, coef);
      VF_CHECK_HIP(hipMemsetAsync(a.counts, 0, (size_t)n * 4 * 256 * 4, ctx->stream));
      hipLaunchKernelGGL(k_jenc_hist, per_tile, dim3(256), 0, ctx->stream, a);
      VF_LAUNCH_CHECK();
      hipLaunchKernelGGL(k_jenc_table, dim3(p.tables, n), dim3(JENC_TABLE_THREADS), 0, ctx->stream, a);
      VF_LAUNCH_CHECK();
    }
  VF_LAUNCH_TIMED(ctx, "jpeg_enc_size", 0.0, coef, k_jenc_size<OPTS>, per_tile, dim3(256), a);
  VF_LAUNCH_CHECK();
  VF_LAUNCH_TIMED(ctx, "jpeg_enc_scan", 0.0, 12.0 * n * p.tiles, k_jenc_tile_scan, dim3(n), dim3(256), a);
  VF_LAUNCH_CHECK();
  if constexpr (OPTS) {
    VF_LAUNCH_TIMED(ctx, "jpeg_enc_segments", 0.0, 28.0 * n * p.nseg, k_jenc_seg_scan, dim3(n), dim3(256), a);
    VF_LAUNCH_CHECK();
  }
  VF_LAUNCH_TIMED(ctx, "jpeg_enc_clear", 0.0, 0.0, k_jenc_clear, per_chunk, dim3(256), a);
  VF_LAUNCH_CHECK();
  VF_LAUNCH_TIMED(ctx, "jpeg_enc_write", 0.0, coef, k_jenc_write<OPTS>, per_tile, dim3(256), a);
  VF_LAUNCH_CHECK();
  {
    VfProf prof(ctx, "jpeg_enc_stuff", 0.0, 0.0);
    hipLaunchKernelGGL(k_jenc_ff_count, per_chunk, dim3(256), 0, ctx->stream, a);
    VF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_jenc_ff_scan<OPTS>, dim3(n), dim3(256), 0, ctx->stream, a, hdr.len);
    VF_LAUNCH_CHECK();
    vf_launch_file_offsets(ctx->stream, a.offsets, n);
    VF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_jenc_stuff<OPTS>, per_chunk, dim3(256), 0, ctx->stream, a, hdr);
    VF_LAUNCH_CHECK();
  }
  return 0;
}

int jenc_encode(const char* who, vf_ctx* ctx, const void* src, int kind, int n, int H, int W, int C, int quality, int subsampling,
                int restart_rows, int restart_blocks, int optimize, void* ws, size_t ws_bytes, unsigned char* out, size_t out_cap,
                int64_t* offsets) {
  JencPlan p;
  if (int e = jenc_plan(who, n, H, W, C, subsampling, restart_rows, restart_blocks, optimize, &p)) return e;
  VF_REQUIRE(quality >= 1 && quality <= 100, "%s: quality = %d (1 to 100)", who, quality);
  char batch[64];
  snprintf(batch, sizeof(batch), "%d frames of %dx%dx%d", n, H, W, C);
  if (int e = vf_check_encode_entry(who, kind, "C", batch, ws_bytes, p.ws_bytes, out_cap, p.out_bytes)) return e;
  JencArgs a;
  JencHdr hdr;
  jenc_header(H, W, C, quality, p.hs, p.vs, p.interval, p.tables != 0, &hdr, a.quant);
  char* w = (char*)ws;
  a.src = src;
  a.coef = (short*)(w + p.o_coef);
  a.blk_off = (unsigned*)(w + p.o_blk);
  a.tile_sum = (unsigned*)(w + p.o_tsum);
  a.tile_off = (unsigned long long*)(w + p.o_toff);
  a.img_bits = (unsigned long long*)(w + p.o_bits);
  a.stream = (unsigned*)(w + p.o_stream);
  a.ff_cnt = (unsigned*)(w + p.o_ffc);
  a.ff_pref = (unsigned long long*)(w + p.o_ffp);
  a.out = out;
  a.offsets = offsets;
  a.cap_words = p.cap_bytes / 4;
  a.n = n; a.H = H; a.W = W; a.C = C; a.hs = p.hs; a.vs = p.vs;
  a.mcux = p.mcux; a.mcuy = p.mcuy; a.bpm = p.bpm; a.nb = p.nb;
  a.wb = (int)vf_cdiv(W, 8); a.hb = (int)vf_cdiv(H, 8);
  a.tiles = p.tiles; a.chunks = p.chunks;
  a.spb = p.spb; a.nseg = p.nseg; a.optimize = p.tables;
  a.seg_start = p.opts() ? (unsigned long long*)(w + p.o_sstart) : nullptr;
  a.seg_shift = p.opts() ? (long long*)(w + p.o_sshift) : nullptr;
  a.counts = p.tables ? (unsigned*)(w + p.o_counts) : nullptr;
  a.lut = p.tables ? (JencLut*)(w + p.o_lut) : nullptr;
  a.dht = p.tables ? (unsigned char*)(w + p.o_dht) : nullptr;
  a.dht_len = p.tables ? (int*)(w + p.o_dlen) : nullptr;
  return p.opts() ? jenc_launch<true>(ctx, p, a, hdr, kind) : jenc_launch<false>(ctx, p, a, hdr, kind);
}

// ============================================================================================ the progressive encoder (SOF2)
// vf_jpeg_encode_prog: libjpeg's jpeg_simple_progression and jcphuff.c (tests/jpeg_enc_prog_ref.py is the rule in numpy).  The
// coefficients are k_jenc_dct's.  A scan walks its blocks (a DC scan every block of the interleaved order, an AC scan the real
// blocks of its component in raster order), and every kernel below takes all scans of all images in one launch, the scan in
// blockIdx.z (or .x where a workgroup owns a whole scan):
//   k_jprog_sum       one thread per block of a walk: its symbols counted (LDS first), and for an AC scan its summary: does it
//                     bring a symbol, does it end in zeros or correction bits and so join the EOB run, how many correction bits
//                     trail its last symbol.
//   k_jprog_runs      one wave per image and AC scan: jcphuff.c's EOBRUN and BE walked over the summaries, 64 blocks per step from
//                     two ballots.  A run is emitted behind its FIRST block's own symbols (nothing stands between that place and
//                     where libjpeg writes it), so the first block of a run receives the run's length and every other block 0,
//                     and the EOBn symbols are counted.
//   k_jprog_table     one workgroup per image and table: jenc_gen_table, two tables for the colour DC scan, none for a DC refinement.
//   k_jprog_size / k_jprog_tile_scan / k_jenc_clear / k_jprog_write   as the baseline's: a block's bits are its symbols, its run's
//                     EOBn code if it heads one, its trailing correction bits.  Every scan starts on a byte of the image's stream
//                     and its last block pads it with 1-bits.
//   k_jenc_ff_count / k_jprog_ff_scan / k_vf_file_offsets / k_jprog_stuff   the stuffing; the thread that holds a scan's first
//                     byte writes the image's DHT segments and the SOS of that scan in front of it.
// Twelve launches and two memsets whatever the batch and the scan count; nothing synchronises.
constexpr int JPROG_MAX_SCANS = 10;
constexpr int JPROG_BLOCK_BITS = 3968;    // the bound on a block's code over all scans (vf_hip.h has the derivation), a multiple of 32
constexpr int JPROG_PREFIX_CAP = 192;     // SOI, APP0, two DQT, SOF2: 177 bytes in colour
constexpr int JPROG_SOS_CAP = 14;
constexpr int JPROG_MAX_RUN = 0x7FFF;     // jcphuff.c: an EOB run is emitted when it reaches this length ...
constexpr int JPROG_MAX_BE = 937;         // ... or buffers more correction bits than MAX_CORR_BITS - DCTSIZE2 + 1

struct JprogScan {
  int comp;                      // the component of an AC scan; -1: all components interleaved (the DC scans)
  int ss, se, ah, al;
  int len, tiles;                // blocks of the walk, and their tiles of JENC_TILE
  int ntab;                      // tables of its own: 2 for the colour DC scan, 0 for a DC refinement, else 1
  unsigned char tc_th[2];        // their class << 4 | id
  unsigned char sos[JPROG_SOS_CAP];
  int sos_len;
};

struct JprogArgs {
  JencArgs e;                    // the geometry, coef, stream, img_bits, ff_cnt, ff_pref, out, offsets; tiles: of the longest walk;
                                 // blk_off [n][nscan][nb], tile_sum and tile_off [n][nscan][tiles]
  JprogScan scan[JPROG_MAX_SCANS];
  int nscan;
  unsigned char* sum;            // [n][nscan][nb]: trailing correction bits | joins << 6 | has a symbol << 7
  unsigned short* run;           // [n][nscan][nb]: the length of the EOB run this block heads, else 0
  unsigned* counts;              // [n][nscan][2][256]
  unsigned* lut;                 // [n][nscan][2][256]: symbol -> code << 8 | length
  unsigned char* dht;            // [n][nscan][2][JENC_DHT_STRIDE]
  int* dht_len;                  // [n][nscan][2]; 0 where the scan has no such table
  unsigned long long* scan_start;  // [n][nscan]: byte offset of the scan inside its image's unstuffed stream
  unsigned* hdr_before;          // [n][nscan]: the file's bytes in front of the scan's data that are not stream: prefix, DHTs, SOSs
  unsigned char prefix[JPROG_PREFIX_CAP];
  int prefix_len;
};

// block i of a scan's walk -> its place in the interleaved order of coef
__device__ __forceinline__ int jprog_block(const JencArgs& a, const JprogScan& sc, int i) {
  if (sc.comp < 0 || a.bpm == 1) return i;
  if (sc.comp > 0) return i * a.bpm + a.hs * a.vs + sc.comp - 1;   // a chroma component has one block per MCU, none a dummy
  const int Y = i / a.wb, X = i - Y * a.wb, my = Y / a.vs, mx = X / a.hs;
  return (my * a.mcux + mx) * a.bpm + (Y - my * a.vs) * a.hs + (X - mx * a.hs);
}

struct JprogSum {
  bool has, joins;
  int tail;
};

// jcphuff.c's encode_mcu_* of block i of the walk, in the order of the stream: sym(table 0 / 1 of the scan, symbol, extra bits,
// their count) for a code with its extra bits, raw(bits, count <= 63) for correction bits.  `run` is the length of the EOB run
// the block heads (0: none, and what the passes in front of k_jprog_runs give): its EOBn follows the block's own symbols.
template <class SYM, class RAW>
__device__ __forceinline__ JprogSum jprog_block_items(const JencArgs& a, const JprogScan& sc, const short* coef, int i, int run, SYM&& sym,
                                                      RAW&& raw) {
  const int g = jprog_block(a, sc, i);
  JprogSum r{false, false, 0};
  if (sc.se == 0) {
    // A dummy of the interleaved scan carries the DC of the previous real block of its component (jccoefct.c replicates it), the
    // value jenc_pred finds: its difference is 0 and its refinement bit is that block's.
    const JencPos p = jenc_pos(a, g);
    const int prev = jenc_pred<false>(a, coef, g, p), dc = p.real ? (int)coef[(long long)g * 64] : prev;
    if (sc.ah == 0) {
      const int diff = (dc >> sc.al) - (prev >> sc.al);        // arithmetic shifts, as jcphuff.c's
      const int n = 32 - __clz(abs(diff));
      sym(p.comp ? 1 : 0, n, (unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1u), n);
    } else {
      raw((unsigned long long)((dc >> sc.al) & 1), 1);
    }
    return r;
  }
  const uint4* src = (const uint4*)(coef + (long long)g * 64);
  unsigned w[32];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint4 u = src[j];
    w[4 * j] = u.x; w[4 * j + 1] = u.y; w[4 * j + 2] = u.z; w[4 * j + 3] = u.w;
  }
  auto at = [&](int k) { return (int)(short)((k & 1) ? w[k >> 1] >> 16 : w[k >> 1] & 0xFFFFu); };
  int zeros = 0, nbr = 0;
  unsigned long long br = 0;                       // the correction bits since the last symbol, oldest highest
  if (sc.ah == 0) {
#pragma unroll
    for (int k = 1; k < 64; ++k) {
      if (k < sc.ss || k > sc.se) continue;
      const int c = at(k), m = abs(c) >> sc.al;
      if (m == 0) { ++zeros; continue; }
      r.has = true;
      for (; zeros > 15; zeros -= 16) sym(0, 0xF0, 0u, 0);
      const int n = 32 - __clz(m);
      sym(0, zeros << 4 | n, (unsigned)(c < 0 ? ~m : m) & ((1u << n) - 1u), n);
      zeros = 0;
    }
  } else {
    int eob = 0;                                   // the last coefficient that becomes non-zero in this scan
#pragma unroll
    for (int k = 1; k < 64; ++k)
      if (k >= sc.ss && k <= sc.se && (abs(at(k)) >> sc.al) == 1) eob = k;
    r.has = eob != 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
      if (k < sc.ss || k > sc.se) continue;
      const int c = at(k), m = abs(c) >> sc.al;
      if (m == 0) { ++zeros; continue; }
      for (; zeros > 15 && k <= eob; zeros -= 16) {            // ZRL only while a symbol is still to come
        sym(0, 0xF0, 0u, 0);
        raw(br, nbr);
        br = 0; nbr = 0;
      }
      if (m > 1) {                                             // already non-zero: one correction bit
        br = br << 1 | (unsigned)(m & 1);
        ++nbr;
        continue;
      }
      sym(0, zeros << 4 | 1, c < 0 ? 0u : 1u, 1);
      raw(br, nbr);
      br = 0; nbr = 0; zeros = 0;
    }
  }
  r.joins = zeros > 0 || nbr > 0;
  r.tail = nbr;
  if (run) {
    const int n = 31 - __clz(run);
    sym(0, n << 4, (unsigned)run & ((1u << n) - 1u), n);
  }
  raw(br, nbr);
  return r;
}

__global__ __launch_bounds__(256) void k_jprog_sum(JprogArgs a) {
  __shared__ unsigned s_h[2 * 256];
  const int s = blockIdx.z;
  const JprogScan& sc = a.scan[s];
  if ((int)blockIdx.x >= sc.tiles || sc.ntab == 0) return;
  for (int i = threadIdx.x; i < 2 * 256; i += 256) s_h[i] = 0;
  __syncthreads();
  const int i = blockIdx.x * JENC_TILE + threadIdx.x;
  const long long f = blockIdx.y, fs = f * a.nscan + s;
  if (i < sc.len) {
    const JprogSum r = jprog_block_items(a.e, sc, a.e.coef + f * a.e.nb * 64, i, 0,
                                         [&](int t, int v, unsigned, int) { atomicAdd(&s_h[t * 256 + v], 1u); }, [](unsigned long long, int) {});
    a.sum[fs * a.e.nb + i] = (unsigned char)(r.tail | (r.joins ? 0x40 : 0) | (r.has ? 0x80 : 0));
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * 256; i += 256)
    if (s_h[i]) atomicAdd(a.counts + fs * 512 + i, s_h[i]);
}

// One wave per image and AC scan, the walk in steps of 64 blocks; every lane holds the same state (EOBRUN, BE, the open run's
// first block).  Every block has a symbol or joins the run (a block without a symbol ends in zeros or correction bits; one that
// does not join ends in a symbol), so the blocks with a symbol cut a step into runs: a block with a symbol that joins heads
// one, so does a block without a symbol behind one that does not join, and a run lasts up to the next block with a symbol.
//   The step in parallel: the open run takes the blocks in front of the first symbol, every lane that heads a run finds its
// end in the mask of the symbols, and the last run stays open; sums of trailing bits are popcounts of their six bit planes.
// That holds where no run can reach a limit inside the step: the open run's length + 64 < 0x7FFF, and its buffered bits + all
// trailing bits of the step <= 937.
//   The step in order: else the blocks one by one as jcphuff.c does.  This is the part of the run resolution that stays
// sequential: the 937-bit flush makes the cuts a greedy walk.  It costs 64 dependent iterations for a step that may hold a cut
// (DESIGN.md 5.8 has the measurement).
// Lane n counts the EOBn symbols; they enter the counts once at the end (k_jprog_sum counts no EOBn).
__global__ __launch_bounds__(64) void k_jprog_runs(JprogArgs a) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const JprogScan& sc = a.scan[s];
  if (sc.se == 0) return;
  const long long fs = (long long)blockIdx.y * a.nscan + s;
  const unsigned char* sum = a.sum + fs * a.e.nb;
  unsigned short* run = a.run + fs * a.e.nb;
  int len = 0, bits = 0, head = 0;
  unsigned eobn = 0;
  auto close = [&]() {
    if (lane == 0) run[head] = (unsigned short)len;
    if (lane == 31 - __clz(len)) ++eobn;
    len = 0;
    bits = 0;
  };
  unsigned ahead = lane < sc.len ? sum[lane] : 0u;  // the next step's summaries are on their way while this step is walked
  for (int base = 0; base < sc.len; base += 64) {
    const int i = base + lane, m = min(64, sc.len - base);
    const unsigned v = ahead;
    ahead = i + 64 < sc.len ? sum[i + 64] : 0u;
    const unsigned long long joins = __ballot((v & 0x40u) != 0), has = __ballot((v & 0x80u) != 0);
    const int tail = (int)(v & 63u);
    unsigned long long plane[6] = {0, 0, 0, 0, 0, 0};          // bit k of the trailing bits of every block: sums over blocks are
    if (sc.ah)                                                 // popcounts, scalar work (a first scan has no correction bits)
      for (int k = 0; k < 6; ++k) plane[k] = __ballot((tail >> k & 1) != 0);
    auto tails = [&](unsigned long long blocks) {
      int t = 0;
      for (int k = 0; k < 6; ++k) t += __popcll(plane[k] & blocks) << k;
      return t;
    };
    auto below = [](int b) { return b >= 64 ? ~0ull : (1ull << b) - 1ull; };
    const int p0 = has ? __ffsll((long long)has) - 1 : m;      // the first block with a symbol
    const bool sym = has >> lane & 1, join = joins >> lane & 1;
    const bool heads = lane < m && lane >= p0 && (sym ? join : lane > 0 && (has >> (lane - 1) & 1) && !(joins >> (lane - 1) & 1));
    const unsigned long long rest = has & ~((2ull << lane) - 1ull);                // the symbols behind this block
    const int end = rest ? __ffsll((long long)rest) - 1 : m;
    const int lead = tails(below(p0)), total = tails(~0ull);
    if (len + 64 < JPROG_MAX_RUN && bits + total <= JPROG_MAX_BE) {
      if (p0 > 0) {
        if (!len) head = base;
        len += p0;
        bits += lead;
      }
      if (len && p0 < m) close();
      const bool whole = heads && end < m;
      if (whole) run[i] = (unsigned short)(end - lane);
      const int n = whole ? 31 - __clz(end - lane) : -1;
      for (int k = 0; k < 6; ++k) {                // a run inside a step is shorter than 64
        const unsigned long long of_k = __ballot(n == k);
        if (lane == k) eobn += (unsigned)__popcll(of_k);
      }
      const unsigned long long open = __ballot(heads && end == m);                 // at most the last head
      if (open) {
        const int b = __ffsll((long long)open) - 1;
        head = base + b;
        len = m - b;
        bits = tails(~below(b));
      }
      continue;
    }
    for (int b = 0; b < m; ++b) {
      if ((has >> b & 1) && len) close();
      if (joins >> b & 1) {
        if (!len) head = base + b;
        ++len;
        bits += __builtin_amdgcn_readlane(tail, b);
        if (len == JPROG_MAX_RUN || bits > JPROG_MAX_BE) close();
      }
    }
  }
  if (len) close();
  if (lane < 15 && eobn) atomicAdd(a.counts + fs * 512 + (lane << 4), eobn);
}

__global__ __launch_bounds__(JENC_TABLE_THREADS) void k_jprog_table(JprogArgs a) {
  const int s = blockIdx.x >> 1, j = blockIdx.x & 1;
  const long long k = ((long long)blockIdx.y * a.nscan + s) * 2 + j;
  if (j >= a.scan[s].ntab) {
    if (threadIdx.x == 0) a.dht_len[k] = 0;
    return;
  }
  jenc_gen_table(a.counts + k * 256, a.lut + k * 256, 256, a.dht + k * JENC_DHT_STRIDE, a.dht_len + k, a.scan[s].tc_th[j]);
}

__device__ __forceinline__ void jprog_load_lut(unsigned (&s_lut)[2][256], const JprogArgs& a, long long fs) {
  for (int i = threadIdx.x; i < 512; i += 256) s_lut[i >> 8][i & 255] = a.lut[fs * 512 + i];
  __syncthreads();
}

__global__ __launch_bounds__(256) void k_jprog_size(JprogArgs a) {
  __shared__ unsigned s_lut[2][256];
  __shared__ unsigned s_w[4];
  const int s = blockIdx.z;
  const JprogScan& sc = a.scan[s];
  if ((int)blockIdx.x >= sc.tiles) return;
  const int i = blockIdx.x * JENC_TILE + threadIdx.x;
  const long long f = blockIdx.y, fs = f * a.nscan + s;
  jprog_load_lut(s_lut, a, fs);
  unsigned bits = 0;
  if (i < sc.len)
    jprog_block_items(a.e, sc, a.e.coef + f * a.e.nb * 64, i, sc.se ? (int)a.run[fs * a.e.nb + i] : 0,
                      [&](int t, int v, unsigned, int n) { bits += (s_lut[t][v] & 255u) + (unsigned)n; },
                      [&](unsigned long long, int n) { bits += (unsigned)n; });
  unsigned total;
  const unsigned at = vf_block_excl_scan<unsigned, 256>(bits, s_w, total);
  if (i < sc.len) a.e.blk_off[fs * a.e.nb + i] = at;
  if (threadIdx.x == 0) a.e.tile_sum[fs * a.e.tiles + blockIdx.x] = total;
}

// one workgroup per image: the tiles' bit offsets in the image's stream, scan behind scan, each from a byte boundary; the scans'
// byte offsets, the image's bit count (whole bytes), and what stands in front of every scan's data in the file
__global__ __launch_bounds__(256) void k_jprog_tile_scan(JprogArgs a) {
  __shared__ unsigned long long s_w[4];
  const long long f = blockIdx.x;
  unsigned long long run = 0;
  for (int s = 0; s < a.nscan; ++s) {
    const long long fs = f * a.nscan + s;
    run = (run + 7) & ~7ull;
    if (threadIdx.x == 0) a.scan_start[fs] = run >> 3;
    for (int base = 0; base < a.scan[s].tiles; base += 256) {
      const int t = base + threadIdx.x;
      const unsigned long long v = t < a.scan[s].tiles ? a.e.tile_sum[fs * a.e.tiles + t] : 0ull;
      unsigned long long total;
      const unsigned long long e = vf_block_excl_scan<unsigned long long, 256>(v, s_w, total);
      if (t < a.scan[s].tiles) a.e.tile_off[fs * a.e.tiles + t] = run + e;
      run += total;
    }
  }
  if (threadIdx.x == 0) {
    a.e.img_bits[f] = (run + 7) & ~7ull;
    unsigned h = (unsigned)a.prefix_len;
    for (int s = 0; s < a.nscan; ++s) {
      const long long fs = f * a.nscan + s;
      h += (unsigned)(a.dht_len[2 * fs] + a.dht_len[2 * fs + 1] + a.scan[s].sos_len);
      a.hdr_before[fs] = h;
    }
  }
}

__global__ __launch_bounds__(256) void k_jprog_write(JprogArgs a) {
  __shared__ unsigned s_lut[2][256];
  const int s = blockIdx.z;
  const JprogScan& sc = a.scan[s];
  if ((int)blockIdx.x >= sc.tiles) return;
  const int i = blockIdx.x * JENC_TILE + threadIdx.x;
  const long long f = blockIdx.y, fs = f * a.nscan + s;
  jprog_load_lut(s_lut, a, fs);
  if (i >= sc.len) return;
  const unsigned long long at = a.e.tile_off[fs * a.e.tiles + blockIdx.x] + a.e.blk_off[fs * a.e.nb + i];
  unsigned* dst = a.e.stream + f * a.e.cap_words + (long long)(at >> 5);
  // as k_jenc_write: the dword the block starts in and the one it ends in are OR-ed, those between are stored
  // ... and a block without a bit of its own (most blocks of a refinement scan over flat content) touches nothing
  unsigned long long acc = 0;
  int cnt = (int)(at & 31);
  bool first = true, fresh = false;                // fresh: acc holds bits that are not in memory yet
  auto put = [&](unsigned bits, int count) {       // count <= 32 on top of cnt < 32
    acc = acc << count | bits;
    cnt += count;
    fresh = true;
    if (cnt >= 32) {
      cnt -= 32;
      const unsigned word = (unsigned)(acc >> cnt);
      if (first) atomicOr(dst, word);
      else *dst = word;
      first = false;
      fresh = cnt > 0;
      ++dst;
      acc &= (1ull << cnt) - 1ull;
    }
  };
  jprog_block_items(a.e, sc, a.e.coef + f * a.e.nb * 64, i, sc.se ? (int)a.run[fs * a.e.nb + i] : 0,
                    [&](int t, int v, unsigned ext, int n) {
                      const unsigned e = s_lut[t][v];
                      put((e >> 8) << n | ext, (int)(e & 255u) + n);
                    },
                    [&](unsigned long long bits, int n) {
                      if (n > 32) {
                        put((unsigned)(bits >> 32), n - 32);
                        put((unsigned)bits, 32);
                      } else if (n) {
                        put((unsigned)bits, n);
                      }
                    });
  if (i + 1 == sc.len && (cnt & 7)) {              // the scan's last block fills its last byte with 1-bits
    const int k = 8 - (cnt & 7);
    acc = acc << k | ((1ull << k) - 1ull);
    cnt += k;
    fresh = true;
  }
  if (fresh) atomicOr(dst, (unsigned)(acc << (32 - cnt)));
}

__global__ __launch_bounds__(256) void k_jprog_ff_scan(JprogArgs a) {
  __shared__ unsigned long long s_w[4];
  const long long f = blockIdx.x;
  const unsigned long long nbytes = a.e.img_bits[f] >> 3;
  const long long used = (long long)((nbytes + JENC_CHUNK - 1) / JENC_CHUNK);
  unsigned long long run = 0;
  for (long long base = 0; base < used; base += 256) {
    const long long c = base + threadIdx.x;
    const unsigned long long v = c < used ? a.e.ff_cnt[f * a.e.chunks + c] : 0ull;
    unsigned long long total;
    const unsigned long long e = vf_block_excl_scan<unsigned long long, 256>(v, s_w, total);
    if (c < used) a.e.ff_pref[f * a.e.chunks + c] = run + e;
    run += total;
  }
  if (threadIdx.x == 0) a.e.offsets[f + 1] = (int64_t)(a.hdr_before[f * a.nscan + a.nscan - 1] + nbytes + run + 2);
}

// the DHT segments and the SOS of scan s of image f, ending at `end`
__device__ __forceinline__ void jprog_put_scan_header(const JprogArgs& a, long long f, int s, unsigned char* end) {
  const long long fs = f * a.nscan + s;
  const int d0 = a.dht_len[2 * fs], d1 = a.dht_len[2 * fs + 1], sos = a.scan[s].sos_len;
  unsigned char* p = end - (d0 + d1 + sos);
  for (int i = 0; i < d0; ++i) *p++ = a.dht[2 * fs * JENC_DHT_STRIDE + i];
  for (int i = 0; i < d1; ++i) *p++ = a.dht[(2 * fs + 1) * JENC_DHT_STRIDE + i];
  for (int i = 0; i < sos; ++i) *p++ = a.scan[s].sos[i];
}

__global__ __launch_bounds__(256) void k_jprog_stuff(JprogArgs a) {
  __shared__ unsigned s_w[4];
  const long long f = blockIdx.y;
  const unsigned long long bits = a.e.img_bits[f], nbytes = bits >> 3, begin = (unsigned long long)blockIdx.x * JENC_CHUNK;
  if (begin >= nbytes) return;
  unsigned char* file = a.e.out + a.e.offsets[f];
  unsigned b[16];
  const unsigned long long pos = begin + threadIdx.x * 16;
  const int have = jenc_bytes16(a.e, f, bits, pos, b);
  unsigned cnt = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) cnt += i < have && b[i] == 255u;
  unsigned total;
  const unsigned before = vf_block_excl_scan<unsigned, 256>(cnt, s_w, total);
  const unsigned long long* start = a.scan_start + f * a.nscan;
  const unsigned* hdr = a.hdr_before + f * a.nscan;
  if (have) {
    int s = 0;                                     // the scan of the thread's first byte: the last that starts at or before it
    while (s + 1 < a.nscan && start[s + 1] <= pos) ++s;
    unsigned char* dst = file + hdr[s] + begin + a.e.ff_pref[f * a.e.chunks + blockIdx.x] + threadIdx.x * 16 + before;
    if (start[s] == pos) jprog_put_scan_header(a, f, s, dst);
    unsigned long long next = s + 1 < a.nscan ? start[s + 1] : ~0ull;
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (i < have) {
        if (pos + i == next) {                     // the next scan begins with this byte: its header goes in front
          ++s;
          dst += hdr[s] - hdr[s - 1];
          jprog_put_scan_header(a, f, s, dst);
          next = s + 1 < a.nscan ? start[s + 1] : ~0ull;
        }
        *dst++ = (unsigned char)b[i];
        if (b[i] == 255u) *dst++ = 0;
      }
  }
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < a.prefix_len; i += 256) file[i] = a.prefix[i];
  if (begin + JENC_CHUNK >= nbytes && threadIdx.x == 0) {
    const int64_t size = a.e.offsets[f + 1] - a.e.offsets[f];
    file[size - 2] = 0xFF;
    file[size - 1] = 0xD9;
  }
}

struct JprogPlan {
  JencPlan b;                    // the geometry
  int nscan;
  long long cap_bytes;
  int chunks;
  size_t o_coef, o_blk, o_tsum, o_toff, o_bits, o_stream, o_ffc, o_ffp, o_sum, o_run, o_counts, o_lut, o_dht, o_dlen, o_sstart, o_hdr;
  size_t ws_bytes, out_bytes;
};

int jprog_plan(const char* who, int n, int H, int W, int C, int subsampling, JprogPlan* p) {
  if (int e = jenc_plan(who, n, H, W, C, subsampling, 0, 0, 0, &p->b)) return e;
  const int nb = p->b.nb, S = p->nscan = C == 3 ? 10 : 6;
  // every block at its bound, and a pad byte per scan
  p->cap_bytes = vf_cdiv((long long)nb * (JPROG_BLOCK_BITS / 8) + S, JENC_CHUNK) * JENC_CHUNK;
  p->chunks = (int)(p->cap_bytes / JENC_CHUNK);
  const size_t walks = (size_t)n * S * nb, tiles = (size_t)n * S * p->b.tiles, tables = (size_t)n * S * 2;
  VfCarve ws;
  p->o_coef = ws.take((size_t)n * nb * 128);
  p->o_blk = ws.take(walks * 4);
  p->o_tsum = ws.take(tiles * 4);
  p->o_toff = ws.take(tiles * 8);
  p->o_bits = ws.take((size_t)n * 8);
  p->o_stream = ws.take((size_t)n * p->cap_bytes);
  p->o_ffc = ws.take((size_t)n * p->chunks * 4);
  p->o_ffp = ws.take((size_t)n * p->chunks * 8);
  p->o_sum = ws.take(walks);
  p->o_run = ws.take(walks * 2);
  p->o_counts = ws.take(tables * 256 * 4);
  p->o_lut = ws.take(tables * 256 * 4);
  p->o_dht = ws.take(tables * JENC_DHT_STRIDE);
  p->o_dlen = ws.take(tables * 4);
  p->o_sstart = ws.take((size_t)n * S * 8);
  p->o_hdr = ws.take((size_t)n * S * 4);
  p->ws_bytes = ws.at;
  // every block at its bound and every scan's pad byte, every stream byte stuffed; the prefix, per scan two DHT segments and
  // the SOS, EOI
  p->out_bytes = (size_t)n * (((size_t)nb * (JPROG_BLOCK_BITS / 8) + S) * 2 + JPROG_PREFIX_CAP + (size_t)S * (2 * JENC_DHT_STRIDE + JPROG_SOS_CAP) + 2);
  return 0;
}

// jcparam.c's jpeg_simple_progression: (component or -1 for all, Ss, Se, Ah, Al)
constexpr int K_PROG_COLOUR[10][5] = {{-1, 0, 0, 0, 1}, {0, 1, 5, 0, 2},  {2, 1, 63, 0, 1}, {1, 1, 63, 0, 1}, {0, 6, 63, 0, 2},
                                      {0, 1, 63, 2, 1}, {-1, 0, 0, 1, 0}, {2, 1, 63, 1, 0}, {1, 1, 63, 1, 0}, {0, 1, 63, 1, 0}};
constexpr int K_PROG_GREY[6][5] = {{-1, 0, 0, 0, 1}, {0, 1, 5, 0, 2}, {0, 6, 63, 0, 2}, {0, 1, 63, 2, 1}, {-1, 0, 0, 1, 0}, {0, 1, 63, 1, 0}};

// the scans with their walks and SOS segments, and the prefix: jenc_header's bytes up to its first DHT, SOF0 turned into SOF2
void jprog_script(const JprogPlan& p, int H, int W, int C, int quality, JprogArgs* a) {
  JencHdr hdr;
  jenc_header(H, W, C, quality, p.b.hs, p.b.vs, 0, true, &hdr, a->e.quant);
  a->prefix_len = hdr.split;
  memcpy(a->prefix, hdr.w, (size_t)hdr.split);
  a->prefix[hdr.split - (8 + 3 * C) - 1] = 0xC2;
  a->nscan = p.nscan;
  for (int s = 0; s < p.nscan; ++s) {
    const int* k = C == 3 ? K_PROG_COLOUR[s] : K_PROG_GREY[s];
    JprogScan& sc = a->scan[s];
    sc.comp = k[0]; sc.ss = k[1]; sc.se = k[2]; sc.ah = k[3]; sc.al = k[4];
    const bool dc = sc.se == 0;
    sc.len = dc ? p.b.nb : sc.comp == 0 ? (int)(vf_cdiv(W, 8) * vf_cdiv(H, 8)) : p.b.mcux * p.b.mcuy;
    sc.tiles = (int)vf_cdiv(sc.len, JENC_TILE);
    sc.ntab = dc ? (sc.ah ? 0 : C == 3 ? 2 : 1) : 1;
    sc.tc_th[0] = (unsigned char)(dc ? 0x00 : 0x10 | (sc.comp > 0));
    sc.tc_th[1] = 0x01;
    // jcmarker.c: a DC scan names no AC table, a DC refinement no table at all, an AC scan no DC table
    const int comps = dc ? C : 1;
    unsigned char* b = sc.sos;
    *b++ = 0xFF; *b++ = 0xDA; *b++ = 0; *b++ = (unsigned char)(6 + 2 * comps); *b++ = (unsigned char)comps;
    for (int c = 0; c < comps; ++c) {
      const int id = dc ? c : sc.comp, t = id > 0;
      *b++ = (unsigned char)(id + 1);
      *b++ = (unsigned char)(dc ? (sc.ah ? 0 : t << 4) : t);
    }
    *b++ = (unsigned char)sc.ss; *b++ = (unsigned char)sc.se; *b++ = (unsigned char)(sc.ah << 4 | sc.al);
    sc.sos_len = (int)(b - sc.sos);
  }
}

int jprog_encode(const char* who, vf_ctx* ctx, const void* src, int kind, int n, int H, int W, int C, int quality, int subsampling,
                 void* ws, size_t ws_bytes, unsigned char* out, size_t out_cap, int64_t* offsets) {
  JprogPlan p;
  if (int e = jprog_plan(who, n, H, W, C, subsampling, &p)) return e;
  VF_REQUIRE(quality >= 1 && quality <= 100, "%s: quality = %d (1 to 100)", who, quality);
  char batch[64];
  snprintf(batch, sizeof(batch), "%d frames of %dx%dx%d", n, H, W, C);
  if (int e = vf_check_encode_entry(who, kind, "C", batch, ws_bytes, p.ws_bytes, out_cap, p.out_bytes)) return e;
  JprogArgs a;
  memset(&a, 0, sizeof(a));
  jprog_script(p, H, W, C, quality, &a);
  char* w = (char*)ws;
  JencArgs& e = a.e;
  e.src = src;
  e.coef = (short*)(w + p.o_coef);
  e.blk_off = (unsigned*)(w + p.o_blk);
  e.tile_sum = (unsigned*)(w + p.o_tsum);
  e.tile_off = (unsigned long long*)(w + p.o_toff);
  e.img_bits = (unsigned long long*)(w + p.o_bits);
  e.stream = (unsigned*)(w + p.o_stream);
  e.ff_cnt = (unsigned*)(w + p.o_ffc);
  e.ff_pref = (unsigned long long*)(w + p.o_ffp);
  e.out = out;
  e.offsets = offsets;
  e.cap_words = p.cap_bytes / 4;
  e.n = n; e.H = H; e.W = W; e.C = C; e.hs = p.b.hs; e.vs = p.b.vs;
  e.mcux = p.b.mcux; e.mcuy = p.b.mcuy; e.bpm = p.b.bpm; e.nb = p.b.nb;
  e.wb = (int)vf_cdiv(W, 8); e.hb = (int)vf_cdiv(H, 8);
  e.tiles = p.b.tiles; e.chunks = p.chunks;
  e.spb = p.b.nb; e.nseg = 1;
  a.sum = (unsigned char*)(w + p.o_sum);
  a.run = (unsigned short*)(w + p.o_run);
  a.counts = (unsigned*)(w + p.o_counts);
  a.lut = (unsigned*)(w + p.o_lut);
  a.dht = (unsigned char*)(w + p.o_dht);
  a.dht_len = (int*)(w + p.o_dlen);
  a.scan_start = (unsigned long long*)(w + p.o_sstart);
  a.hdr_before = (unsigned*)(w + p.o_hdr);
  const int S = p.nscan;
  const double px = (double)n * H * W * C, coef = (double)n * e.nb * 128;
  const dim3 per_tile((unsigned)e.tiles, n), per_walk((unsigned)e.tiles, n, S), per_chunk((unsigned)e.chunks, n);
  if (kind == 0) VF_LAUNCH_TIMED(ctx, "jpeg_prog_dct", 0.0, 4.0 * px + coef, k_jenc_dct<0>, per_tile, dim3(256), e);
  else VF_LAUNCH_TIMED(ctx, "jpeg_prog_dct", 0.0, px + coef, k_jenc_dct<1>, per_tile, dim3(256), e);
  VF_LAUNCH_CHECK();
  {
    VfProf prof(ctx, "jpeg_prog_sum", 0.0, coef * S / 2);
    VF_CHECK_HIP(hipMemsetAsync(a.counts, 0, (size_t)n * S * 2 * 256 * 4, ctx->stream));
    VF_CHECK_HIP(hipMemsetAsync(a.run, 0, (size_t)n * S * e.nb * 2, ctx->stream));
    hipLaunchKernelGGL(k_jprog_sum, per_walk, dim3(256), 0, ctx->stream, a);
    VF_LAUNCH_CHECK();
  }
  VF_LAUNCH_TIMED(ctx, "jpeg_prog_runs", 0.0, (double)n * S * e.nb, k_jprog_runs, dim3(S, n), dim3(64), a);
  VF_LAUNCH_CHECK();
  VF_LAUNCH_TIMED(ctx, "jpeg_prog_tables", 0.0, 0.0, k_jprog_table, dim3(2 * S, n), dim3(JENC_TABLE_THREADS), a);
  VF_LAUNCH_CHECK();
  VF_LAUNCH_TIMED(ctx, "jpeg_prog_size", 0.0, coef * S / 2, k_jprog_size, per_walk, dim3(256), a);
  VF_LAUNCH_CHECK();
  VF_LAUNCH_TIMED(ctx, "jpeg_prog_scan", 0.0, 12.0 * n * S * e.tiles, k_jprog_tile_scan, dim3(n), dim3(256), a);
  VF_LAUNCH_CHECK();
  VF_LAUNCH_TIMED(ctx, "jpeg_prog_clear", 0.0, 0.0, k_jenc_clear, per_chunk, dim3(256), e);
  VF_LAUNCH_CHECK();
  VF_LAUNCH_TIMED(ctx, "jpeg_prog_write", 0.0, coef * S / 2, k_jprog_write, per_walk, dim3(256), a);
  VF_LAUNCH_CHECK();
  {
    VfProf prof(ctx, "jpeg_prog_stuff", 0.0, 0.0);
    hipLaunchKernelGGL(k_jenc_ff_count, per_chunk, dim3(256), 0, ctx->stream, e);
    VF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_jprog_ff_scan, dim3(n), dim3(256), 0, ctx->stream, a);
    VF_LAUNCH_CHECK();
    vf_launch_file_offsets(ctx->stream, e.offsets, n);
    VF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_jprog_stuff, per_chunk, dim3(256), 0, ctx->stream, a);
    VF_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace

VF_API int vf_jpeg_encode_prog_workspace_bytes(int n, int H, int W, int C, int subsampling, size_t* ws_bytes, size_t* out_bytes) {
  JprogPlan p;
  if (int e = jprog_plan("vf_jpeg_encode_prog_workspace_bytes", n, H, W, C, subsampling, &p)) return e;
  if (ws_bytes) *ws_bytes = p.ws_bytes;
  if (out_bytes) *out_bytes = p.out_bytes;
  return 0;
}

VF_API int vf_jpeg_encode_prog(vf_ctx* ctx, const void* src, int kind, int n, int H, int W, int C, int quality, int subsampling,
                               void* ws, size_t ws_bytes, unsigned char* out, size_t out_cap, int64_t* offsets) {
  return jprog_encode("vf_jpeg_encode_prog", ctx, src, kind, n, H, W, C, quality, subsampling, ws, ws_bytes, out, out_cap, offsets);
}

VF_API int vf_jpeg_encode_workspace_bytes(int n, int H, int W, int C, int subsampling, size_t* ws_bytes, size_t* out_bytes) {
  return jenc_workspace_bytes("vf_jpeg_encode_workspace_bytes", n, H, W, C, subsampling, 0, 0, 0, ws_bytes, out_bytes);
}

VF_API int vf_jpeg_encode(vf_ctx* ctx, const void* src, int kind, int n, int H, int W, int C, int quality, int subsampling, void* ws,
                          size_t ws_bytes, unsigned char* out, size_t out_cap, int64_t* offsets) {
  return jenc_encode("vf_jpeg_encode", ctx, src, kind, n, H, W, C, quality, subsampling, 0, 0, 0, ws, ws_bytes, out, out_cap, offsets);
}

VF_API int vf_jpeg_encode_opts_workspace_bytes(int n, int H, int W, int C, int subsampling, int restart_rows, int restart_blocks,
                                               int optimize, size_t* ws_bytes, size_t* out_bytes) {
  return jenc_workspace_bytes("vf_jpeg_encode_opts_workspace_bytes", n, H, W, C, subsampling, restart_rows, restart_blocks, optimize,
                              ws_bytes, out_bytes);
}

VF_API int vf_jpeg_encode_opts(vf_ctx* ctx, const void* src, int kind, int n, int H, int W, int C, int quality, int subsampling,
                               int restart_rows, int restart_blocks, int optimize, void* ws, size_t ws_bytes, unsigned char* out,
                               size_t out_cap, int64_t* offsets) {
  return jenc_encode("vf_jpeg_encode_opts", ctx, src, kind, n, H, W, C, quality, subsampling, restart_rows, restart_blocks, optimize,
                     ws, ws_bytes, out, out_cap, offsets);
}
