// vf_png.hip — batched PNG encoder: frames on the device in, whole PNG files out.
//   k_png_filter    one block per row: the row's bytes (from float planar through vf_savepng_byte, or from interleaved bytes),
//                   the five PNG filters, libpng's minimum-sum-of-absolute-values choice, the filtered row.
//   k_png_deflate   one block per PNG_CHUNK bytes of a frame's filtered stream: LZ77 matches from an LDS hash table (resolved by
//                   position, so the result does not depend on which lane gets there first), a greedy parse, dynamic Huffman
//                   codes, the bits, or a stored block if that is not smaller; the chunk's IDAT with its CRC-32, its Adler sums.
//   k_png_frame_scan / k_vf_file_offsets (vf_block.h) / k_png_pack   chunk and file offsets, the Adler-32 of every frame, the
//                   files back to back.
//   k_png_deflate_dense   level 1's deflate stage in k_png_deflate's place: hash chains over the chunk and the 8 KiB of the same
//                   frame's stream before it, a lazy step, the same parse and coder; level 0's tokens where those code smaller.
// At level 0 no window crosses a chunk; at level 1 none crosses a frame.  A file's bytes depend on its own frame only.
#include "vf_block.h"
#include "vf_common.h"

namespace {

constexpr int PNG_CHUNK = 8192;          // filtered bytes per deflate block / IDAT chunk (backend.PNG_CHUNK mirrors it)
constexpr int PNG_SLOT = 8224;           // a chunk's IDAT in the workspace: 12 framing + 2 zlib header + 5 stored header + chunk + 4 Adler
constexpr int PNG_MAX_SIDE = 16384;
constexpr int HASH_BITS = 11;
constexpr int MAX_MATCH = 258, MIN_MATCH = 3;
constexpr unsigned CRC_POLY = 0xEDB88320u;
constexpr int CRC_SEG = 36;              // bytes per thread of the block-wide CRC: 256 * 36 >= the longest IDAT type + data
constexpr unsigned ADLER_MOD = 65521u;
constexpr int DIST0 = 288;               // the distance alphabet's place in the frequency / length / code arrays

struct PngArgs {
  const void* src;
  unsigned char* stream;   // [n][stream_len]: filter byte + filtered row, row after row
  unsigned char* slots;    // [n][nchunks][PNG_SLOT]
  unsigned* meta;          // [n][nchunks][4]: IDAT data bytes, Adler byte sum, Adler weighted sum, running CRC register
  unsigned* chunk_off;     // [n][nchunks]: offset of the chunk's IDAT behind the file's IHDR
  unsigned* adler;         // [n]
  unsigned char* out;
  int64_t* offsets;        // [n + 1]
  int n, H, W, C, rb, nchunks;
  long long stream_len;
};

// ------------------------------------------------------------------------------------------------------------- filter
template <int KIND>
__device__ __forceinline__ int png_px(const PngArgs& a, long long f, int y, int i) {   // byte i of row y
  // interleaved bytes are the row already: W * C pixels of one channel.  Planar floats: pixel i / C, channel i % C
  if (KIND == 1) return (int)vf_frame_byte<1>(VfFrames{a.src, a.H, a.rb, 1}, f, 0, y, i);
  const int x = a.C == 3 ? i / 3 : i, c = a.C == 3 ? i - 3 * x : 0;
  return (int)vf_frame_byte<0>(VfFrames{a.src, a.H, a.W, a.C}, f, c, y, x);
}

__device__ __forceinline__ int png_paeth(int a, int b, int c) {
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int png_filtered(int t, int x, int a, int b, int c) {
  switch (t) {
    case 0: return x & 255;
    case 1: return (x - a) & 255;
    case 2: return (x - b) & 255;
    case 3: return (x - ((a + b) >> 1)) & 255;
    default: return (x - png_paeth(a, b, c)) & 255;
  }
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <int KIND>
__global__ __launch_bounds__(256) void k_png_filter(PngArgs a) {
  __shared__ unsigned s_part[4][5];
  __shared__ int s_best;
  const int y = blockIdx.x, C = a.C, rb = a.rb;
  const long long f = blockIdx.y;
  unsigned s[5] = {0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < rb; i += 256) {
    const int x = png_px<KIND>(a, f, y, i), l = i >= C ? png_px<KIND>(a, f, y, i - C) : 0;
    const int u = y > 0 ? png_px<KIND>(a, f, y - 1, i) : 0, ul = (y > 0 && i >= C) ? png_px<KIND>(a, f, y - 1, i - C) : 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      const int v = png_filtered(t, x, l, u, ul);
      s[t] += v < 128 ? v : 256 - v;
    }
  }
#pragma unroll
  for (int t = 0; t < 5; ++t) {
    const unsigned w = wave_sum(s[t]);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6][t] = w;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int best = 0;
    unsigned mn = 0xFFFFFFFFu;
    for (int t = 0; t < 5; ++t) {                 // ties: the first of None, Sub, Up, Average, Paeth
      const unsigned v = s_part[0][t] + s_part[1][t] + s_part[2][t] + s_part[3][t];
      if (v < mn) { mn = v; best = t; }
    }
    s_best = best;
  }
  __syncthreads();
  const int best = s_best;
  unsigned char* dst = a.stream + f * a.stream_len + (long long)y * (rb + 1);
  if (threadIdx.x == 0) dst[0] = (unsigned char)best;
  for (int i = threadIdx.x; i < rb; i += 256) {
    const int x = png_px<KIND>(a, f, y, i), l = i >= C ? png_px<KIND>(a, f, y, i - C) : 0;
    const int u = y > 0 ? png_px<KIND>(a, f, y - 1, i) : 0, ul = (y > 0 && i >= C) ? png_px<KIND>(a, f, y - 1, i - C) : 0;
    dst[1 + i] = (unsigned char)png_filtered(best, x, l, u, ul);
  }
}

// ------------------------------------------------------------------------------------------------------------ deflate
__device__ __forceinline__ void len_code(int len, int& code, int& eb, int& ev) {   // RFC 1951 3.2.5
  const int l = len - MIN_MATCH;
  if (len == MAX_MATCH) { code = 285; eb = 0; ev = 0; }
  else if (l < 8) { code = 257 + l; eb = 0; ev = 0; }
  else { eb = (31 - __clz(l)) - 2; code = 261 + 4 * eb + ((l >> eb) & 3); ev = l & ((1 << eb) - 1); }
}
__device__ __forceinline__ void dist_code(int dist, int& code, int& eb, int& ev) {
  const int d = dist - 1;
  if (d < 4) { code = d; eb = 0; ev = 0; }
  else { eb = (31 - __clz(d)) - 1; code = 2 * eb + 2 + ((d >> eb) & 1); ev = d & ((1 << eb) - 1); }
}

constexpr int MATCH_GAIN = 16;           // 1/16 bit: a match must save a bit against its literals
__device__ __forceinline__ int match_cost(int len, int dist) {   // 1/16 bit
  int c, eb1, eb2, ev;
  len_code(len, c, eb1, ev);
  dist_code(dist, c, eb2, ev);
  return (8 + eb1 + 5 + eb2) * 16;
}

__device__ __forceinline__ unsigned crc_mulmod(unsigned a, unsigned b) {   // a * b mod the CRC-32 polynomial, reflected: bit 31 is x^0
  unsigned p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b & 1) ? (b >> 1) ^ CRC_POLY : b >> 1;
  }
  return p;
}
__device__ __forceinline__ unsigned crc_byte(unsigned c, unsigned byte) {
  c ^= byte;
  for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ CRC_POLY : c >> 1;
  return c;
}

// Code lengths of a Huffman code over the m used symbols sorted[0..m) (ascending frequency, ties by symbol), at most maxbits long.
// One thread.  The tree comes from the two-queue merge (leaves and internal nodes are both in non-decreasing weight order); depths
// beyond maxbits are cut to maxbits and the Kraft sum is repaired by moving one code at a time from the longest shorter length
// down, then the lengths go to the symbols by rank: the rarest get the longest.  lens[] must be zero on entry.  m >= 2.
__device__ void huff_lengths(const unsigned* freq, const unsigned short* sorted, int m, int maxbits, unsigned char* lens, unsigned* w,
                             unsigned short* par, unsigned char* depth) {
  // nodes 0..m-1: leaves in sorted order; m..2m-2: internal, in creation order; w[] holds internal weights only
  int li = 0, ii = 0, made = 0;
  for (; made < m - 1; ++made) {
    unsigned wsum = 0;
    for (int k = 0; k < 2; ++k) {
      const bool leaf = li < m && (ii >= made || freq[sorted[li]] <= w[ii]);
      if (leaf) { wsum += freq[sorted[li]]; par[li++] = (unsigned short)(m + made); }
      else { wsum += w[ii]; par[m + ii++] = (unsigned short)(m + made); }
    }
    w[made] = wsum;
  }
  unsigned cnt[16];
  for (int i = 0; i < 16; ++i) cnt[i] = 0;
  depth[m - 2] = 0;                                          // the root is internal node m - 2
  for (int i = m - 3; i >= 0; --i) depth[i] = (unsigned char)min(depth[par[m + i] - m] + 1, 40);
  for (int i = 0; i < m; ++i) cnt[min(depth[par[i] - m] + 1, maxbits)]++;
  unsigned total = 0;
  for (int l = 1; l <= maxbits; ++l) total += cnt[l] << (maxbits - l);
  while (total > (1u << maxbits)) {
    cnt[maxbits]--;
    for (int l = maxbits - 1; l > 0; --l)
      if (cnt[l]) { cnt[l]--; cnt[l + 1] += 2; break; }
    total--;
  }
  int idx = 0;
  for (int l = maxbits; l >= 1; --l)
    for (unsigned k = 0; k < cnt[l]; ++k) lens[sorted[idx++]] = (unsigned char)l;
}

__device__ __forceinline__ unsigned bit_reverse(unsigned code, int len) { return __brev(code) >> (32 - len); }

// the canonical code of symbol s in an alphabet of n lengths (RFC 1951 3.2.2), bit-reversed for the LSB-first stream
__device__ __forceinline__ unsigned canon_code(const unsigned char* lens, int n, int s) {
  const int len = lens[s];
  if (!len) return 0;
  unsigned code = 0;
  for (int t = 0; t < n; ++t) {
    const int lt = lens[t];
    if (lt && lt < len) code += 1u << (len - lt);
    else if (lt == len && t < s) code++;
  }
  return bit_reverse(code, len);
}

struct BitW {   // serial writer into a zeroed word buffer
  unsigned* buf;
  unsigned pos;
  __device__ void put(unsigned v, int nbits) {
    if (!nbits) return;
    const unsigned w = pos >> 5, o = pos & 31;
    buf[w] |= v << o;
    if (o + nbits > 32) buf[w + 1] |= v >> (32 - o);
    pos += nbits;
  }
};

// The header of a dynamic block (RFC 1951 3.2.7), by one thread, into the zeroed bit buffer: BFINAL, BTYPE 10, HLIT, HDIST,
// HCLEN, the code-length code (7 bits at most), the two length tables in 16 / 17 / 18 form.  lens: literal/length lengths at
// 0, distance lengths at DIST0; seq: room for 316 entries, symbol | extra << 8.  -> the bits written.
__device__ unsigned png_block_header(const unsigned char* lens, bool last, unsigned* buf, unsigned short* seq) {
  int hlit = 286, hdist = 30;
  while (hlit > 257 && !lens[hlit - 1]) --hlit;
  while (hdist > 1 && !lens[DIST0 + hdist - 1]) --hdist;
  const int total = hlit + hdist;
  int ns = 0;
  unsigned clf[19];
  for (int i = 0; i < 19; ++i) clf[i] = 0;
  for (int i = 0; i < total;) {
    const int v = i < hlit ? lens[i] : lens[DIST0 + i - hlit];
    int run = 1;
    while (i + run < total && (i + run < hlit ? lens[i + run] : lens[DIST0 + i + run - hlit]) == v) ++run;
    i += run;
    if (v == 0) {
      while (run >= 11) { const int r = min(run, 138); seq[ns++] = (unsigned short)(18 | ((r - 11) << 8)); clf[18]++; run -= r; }
      if (run >= 3) { seq[ns++] = (unsigned short)(17 | ((run - 3) << 8)); clf[17]++; run = 0; }
    } else {
      seq[ns++] = (unsigned short)v; clf[v]++; --run;
      while (run >= 3) { const int r = min(run, 6); seq[ns++] = (unsigned short)(16 | ((r - 3) << 8)); clf[16]++; run -= r; }
    }
    for (; run > 0; --run) { seq[ns++] = (unsigned short)v; clf[v]++; }
  }
  // the code-length code, 7 bits at most
  unsigned short srt[19];
  unsigned char cll[19];
  int m = 0;
  for (int i = 0; i < 19; ++i) {
    cll[i] = 0;
    if (!clf[i]) continue;
    int j = m++;
    for (; j > 0 && clf[srt[j - 1]] > clf[i]; --j) srt[j] = srt[j - 1];
    srt[j] = (unsigned short)i;
  }
  if (m == 1) cll[srt[0]] = cll[srt[0] ? 0 : 1] = 1;   // a complete code needs two
  else {
    unsigned w[19];
    unsigned short par[40];
    unsigned char dep[19];
    huff_lengths(clf, srt, m, 7, cll, w, par, dep);
  }
  const unsigned char order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  int hclen = 19;
  while (hclen > 4 && !cll[order[hclen - 1]]) --hclen;
  BitW bw{buf, 0};
  bw.put(last ? 1u : 0u, 1);
  bw.put(2u, 2);
  bw.put(hlit - 257, 5);
  bw.put(hdist - 1, 5);
  bw.put(hclen - 4, 4);
  for (int i = 0; i < hclen; ++i) bw.put(cll[order[i]], 3);
  for (int i = 0; i < ns; ++i) {
    const int sym = seq[i] & 255, ex = seq[i] >> 8;
    bw.put(canon_code(cll, 19, sym), cll[sym]);
    if (sym == 16) bw.put(ex, 2);
    else if (sym == 17) bw.put(ex, 3);
    else if (sym == 18) bw.put(ex, 7);
  }
  return bw.pos;
}

struct DeflateTables {                     // the small tables both deflate kernels keep beside their data, match words and scratch
  unsigned freq[320];
  unsigned crc[256];
  unsigned red[8];
  unsigned x[8];
  unsigned bits[1];                        // header bits
  int m[2];
  unsigned short sorted[320];
  unsigned short code[320];
  unsigned short cost[256];                // a literal's price, 1/16 bit
  unsigned short seq[320];                 // the two length tables in 16 / 17 / 18 form
  unsigned char len[320];
};

// The chunk's Adler sums, from every thread's partial sums over its bytes, to the chunk's meta words.  Ends without a barrier:
// the next stage's first one orders s_red.
__device__ __forceinline__ void png_chunk_adler(const PngArgs& a, DeflateTables& t, long long f, int k, unsigned ad_a, unsigned ad_b) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  ad_a = wave_sum(ad_a);
  ad_b = wave_sum(ad_b);
  if (lane == 0) { t.red[wave] = ad_a; t.red[4 + wave] = ad_b; }
  __syncthreads();
  if (tid == 0) {
    unsigned* mt = a.meta + (f * a.nchunks + k) * 4;
    mt[1] = (t.red[0] + t.red[1] + t.red[2] + t.red[3]) % ADLER_MOD;
    mt[2] = (t.red[4] + t.red[5] + t.red[6] + t.red[7]) % ADLER_MOD;
  }
}

// What a byte costs as a literal, in 1/16 bit: log2(n / count) from the chunk's byte histogram (the leading bit and four
// mantissa bits of the ratio), at least one bit.  A match is worth taking only where it beats that: in photographic rows
// three-byte repeats at long distances abound and cost more than the literals they replace.  freq[] is zero on entry and is
// cleared again; the caller's next barrier orders that.
__device__ __forceinline__ void png_literal_costs(DeflateTables& t, const unsigned char* s_data, int n) {
  const int tid = threadIdx.x;
  for (int p = tid; p < n; p += 256) atomicAdd(&t.freq[s_data[p]], 1u);
  __syncthreads();
  {
    const unsigned fr = t.freq[tid];
    unsigned c = 15 * 16;
    if (fr) {
      const unsigned r = ((unsigned)n << 8) / fr;
      const int e = 31 - __clz((int)r);
      c = min(max((unsigned)((e - 8) << 4) + ((r >> (e - 4)) & 15u), 16u), 15u * 16u);
    }
    t.cost[tid] = (unsigned short)c;
  }
  __syncthreads();
  for (int i = tid; i < 320; i += 256) t.freq[i] = 0;
}

// Greedy parse by one wave: 64 positions at a time, up to and including the first match
__device__ __forceinline__ void png_greedy_parse(unsigned* s_match, int n) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (wave == 0) {
    int pos = 0;
    while (pos < n) {
      const int p = pos + lane;
      const unsigned m = p < n ? s_match[p] : 0u;
      const unsigned long long mask = __ballot(m != 0);
      const int first = mask ? __ffsll((long long)mask) - 1 : 64;
      if (p < n && lane <= first) s_match[p] = m | 0x80000000u;
      if (first == 64) pos += 64;
      else pos += first + (int)(__shfl(m, first) & 0x1FFu);
    }
  }
  __syncthreads();
}

// Everything behind the tokens, for both kernels, in three steps.  png_code_tables: the histograms of the parsed tokens
// (s_match: length | distance << 16 | token start << 31 per chunk position; s_data: the chunk's n bytes), the two Huffman
// codes, the block header at the front of the zeroed bit buffer.  s_tab: PNG_CHUNK / 4 + 4 words of scratch (tree scratch,
// then the bit buffer).  freq[], len[] and code[] are zero on entry.
__device__ __forceinline__ void png_code_tables(DeflateTables& t, const unsigned char* s_data, const unsigned* s_match, unsigned* s_tab,
                                                int n, bool last) {
  auto& s_freq = t.freq;
  auto& s_sorted = t.sorted;
  auto& s_len = t.len;
  auto& s_code = t.code;
  auto& s_m = t.m;
  auto& s_bits = t.bits;
  auto& s_seq = t.seq;
  const int tid = threadIdx.x;

  // ---- histograms
  for (int p = tid; p < n; p += 256) {
    const unsigned m = s_match[p];
    if (m & 0x80000000u) {
      const int len = m & 0x1FF;
      if (len) {
        int c, eb, ev;
        len_code(len, c, eb, ev);
        atomicAdd(&s_freq[c], 1u);
        dist_code((m >> 16) & 0x7FFF, c, eb, ev);
        atomicAdd(&s_freq[DIST0 + c], 1u);
      } else {
        atomicAdd(&s_freq[s_data[p]], 1u);
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    s_freq[256] = 1;
    int used = 0;
    for (int i = 0; i < 30; ++i) used += s_freq[DIST0 + i] != 0;
    for (int i = 0; i < 30 && used < 2; ++i)       // at least two distance codes, as zlib sends
      if (!s_freq[DIST0 + i]) { s_freq[DIST0 + i] = 1; ++used; }
  }
  __syncthreads();

  // ---- rank sort of the used symbols of both alphabets
  for (int s = tid; s < 316; s += 256) {
    const int lo = s < 286 ? 0 : DIST0, cnt = s < 286 ? 286 : 30, me = s < 286 ? s : s - 286;
    const unsigned fr = s_freq[lo + me];
    if (fr) {
      int r = 0;
      for (int u = 0; u < cnt; ++u) {
        const unsigned ft = s_freq[lo + u];
        r += ft && (ft < fr || (ft == fr && u < me));
      }
      s_sorted[lo + r] = (unsigned short)me;
    }
  }
  if (tid == 64 || tid == 128) {
    const int lo = tid == 64 ? 0 : DIST0, cnt = tid == 64 ? 286 : 30;
    int m = 0;
    for (int u = 0; u < cnt; ++u) m += s_freq[lo + u] != 0;
    s_m[tid == 64 ? 0 : 1] = m;
  }
  __syncthreads();
  if (tid == 0 || tid == 64) {
    const int w = tid == 64;
    unsigned* scratch = s_tab + w * 700;             // 288 weights, 288 words of parents, 72 of depths
    huff_lengths(s_freq + (w ? DIST0 : 0), s_sorted + (w ? DIST0 : 0), s_m[w], 15, s_len + (w ? DIST0 : 0), scratch,
                 (unsigned short*)(scratch + 288), (unsigned char*)(scratch + 288 + 144 + 144));
  }
  __syncthreads();
  for (int i = tid; i < PNG_CHUNK / 4 + 4; i += 256) s_tab[i] = 0;
  for (int s = tid; s < 316; s += 256) {
    const int lo = s < 286 ? 0 : DIST0, cnt = s < 286 ? 286 : 30, me = s < 286 ? s : s - 286;
    s_code[lo + me] = (unsigned short)canon_code(s_len + lo, cnt, me);
  }
  __syncthreads();

  // ---- the block header
  if (tid == 0) s_bits[0] = png_block_header(s_len, last, s_tab, s_seq);
  __syncthreads();
}

// png_token_bits: each thread owns 32 consecutive positions -> the bits of all tokens; tok_at: those before this thread's.
__device__ __forceinline__ unsigned png_token_bits(DeflateTables& t, const unsigned char* s_data, const unsigned* s_match, int n,
                                                   unsigned& tok_at) {
  auto& s_len = t.len;
  const int tid = threadIdx.x;
  const int p0 = tid * (PNG_CHUNK / 256);
  unsigned mybits = 0;
  for (int p = p0; p < p0 + PNG_CHUNK / 256 && p < n; ++p) {
    const unsigned m = s_match[p];
    if (!(m & 0x80000000u)) continue;
    const int len = m & 0x1FF;
    if (len) {
      int c, eb, ev;
      len_code(len, c, eb, ev);
      mybits += s_len[c] + eb;
      dist_code((m >> 16) & 0x7FFF, c, eb, ev);
      mybits += s_len[DIST0 + c] + eb;
    } else {
      mybits += s_len[s_data[p]];
    }
  }
  unsigned tok_bits;
  tok_at = vf_block_excl_scan<unsigned, 256>(mybits, t.red, tok_bits);
  return tok_bits;
}

// the bytes of the chunk's block(s) as coded (header, tokens, end of block, the empty stored block that byte-aligns all but the
// last chunk); the chunk is coded if that is smaller than its n raw bytes, else stored in 5 + n
__device__ __forceinline__ unsigned png_coded_bytes(unsigned hdr_bits, unsigned tok_bits, unsigned eob_bits, bool last) {
  const unsigned body_bits = hdr_bits + tok_bits + eob_bits + (last ? 0u : 3u);   // + the empty stored block's header
  return ((body_bits + 7) >> 3) + (last ? 0u : 4u);
}

// png_write_chunk: the bits, or a stored block if that is not smaller; the chunk's IDAT with its CRC-32 in its slot, its size and
// CRC register in its meta words.
__device__ __forceinline__ void png_write_chunk(const PngArgs& a, DeflateTables& t, const unsigned char* s_data, const unsigned* s_match,
                                                unsigned* s_tab, long long f, int k, int n, bool last, unsigned tok_at, unsigned tok_bits) {
  auto& s_len = t.len;
  auto& s_code = t.code;
  auto& s_crc = t.crc;
  auto& s_x = t.x;
  const int tid = threadIdx.x;
  const int p0 = tid * (PNG_CHUNK / 256);
  const unsigned hdr_bits = t.bits[0];
  const unsigned coded_bytes = png_coded_bytes(hdr_bits, tok_bits, s_len[256], last);
  const unsigned body_bytes = coded_bytes - (last ? 0u : 4u);
  const bool coded = coded_bytes < (unsigned)n;        // not smaller than the raw bytes: stored
  const unsigned zh = k == 0 ? 2u : 0u;
  unsigned char* slot = a.slots + (f * a.nchunks + k) * (long long)PNG_SLOT;
  unsigned char* dat = slot + 8 + zh;
  unsigned dlen;
  if (coded) {
    unsigned bp = hdr_bits + tok_at;
    for (int p = p0; p < p0 + PNG_CHUNK / 256 && p < n; ++p) {
      const unsigned m = s_match[p];
      if (!(m & 0x80000000u)) continue;
      const int len = m & 0x1FF;
      unsigned long long v;
      int nb;
      if (len) {
        int c, eb, ev;
        len_code(len, c, eb, ev);
        v = s_code[c]; nb = s_len[c];
        v |= (unsigned long long)ev << nb; nb += eb;
        dist_code((m >> 16) & 0x7FFF, c, eb, ev);
        v |= (unsigned long long)s_code[DIST0 + c] << nb; nb += s_len[DIST0 + c];
        v |= (unsigned long long)ev << nb; nb += eb;
      } else {
        v = s_code[s_data[p]]; nb = s_len[s_data[p]];
      }
      const unsigned w = bp >> 5, o = bp & 31;
      atomicOr(&s_tab[w], (unsigned)(v << o));
      if (o + nb > 32) atomicOr(&s_tab[w + 1], (unsigned)(v >> (32 - o)));
      if (o + nb > 64) atomicOr(&s_tab[w + 2], (unsigned)(v >> (64 - o)));
      bp += nb;
    }
    if (tid == 255) {                                  // end of block
      const unsigned e = hdr_bits + tok_bits, w = e >> 5, o = e & 31;
      const unsigned v = s_code[256];
      atomicOr(&s_tab[w], v << o);
      if (o + s_len[256] > 32) atomicOr(&s_tab[w + 1], v >> (32 - o));
    }
    __syncthreads();
    for (unsigned i = tid; i < body_bytes; i += 256) dat[i] = (unsigned char)(s_tab[i >> 2] >> (8 * (i & 3)));
    if (!last && tid < 4) dat[body_bytes + tid] = tid < 2 ? 0x00 : 0xFF;       // LEN 0, NLEN ffff: ends on a byte boundary
    dlen = zh + coded_bytes;
  } else {
    if (tid == 0) {
      dat[0] = last ? 1 : 0;
      dat[1] = (unsigned char)(n & 255); dat[2] = (unsigned char)(n >> 8);
      dat[3] = (unsigned char)(~n & 255); dat[4] = (unsigned char)((~n >> 8) & 255);
    }
    for (int i = tid; i < n; i += 256) dat[5 + i] = s_data[i];
    dlen = zh + 5 + (unsigned)n;
  }
  if (tid == 0) {
    slot[4] = 'I'; slot[5] = 'D'; slot[6] = 'A'; slot[7] = 'T';
    if (zh) { slot[8] = 0x78; slot[9] = 0x9C; }
    const unsigned fl = dlen + (last ? 4u : 0u);       // the frame's last IDAT also carries the Adler-32 (k_png_pack)
    slot[0] = (unsigned char)(fl >> 24); slot[1] = (unsigned char)(fl >> 16); slot[2] = (unsigned char)(fl >> 8); slot[3] = (unsigned char)fl;
    unsigned x = 0x80000000u;                          // x^(8 * CRC_SEG) and its squares
    for (int i = 0; i < 8 * CRC_SEG; ++i) x = (x & 1) ? (x >> 1) ^ CRC_POLY : x >> 1;
    for (int l = 0; l < 8; ++l) { s_x[l] = x; x = crc_mulmod(x, x); }
  }
  __syncthreads();

  // ---- CRC-32 of type + data.  The register of a message is linear in the message once its first four bytes are complemented
  // (the all-ones preset), and leading zero bytes leave it at zero: the message is right-aligned in 256 segments of CRC_SEG bytes,
  // each thread takes one, and a tree folds them, the left half times x^(8 * bytes to its right).
  {
    const int L = 4 + (int)dlen, shift = 256 * CRC_SEG - L;
    unsigned c = 0;
    for (int j = 0; j < CRC_SEG; ++j) {
      const int r = tid * CRC_SEG + j - shift;
      if (r >= 0) c = crc_byte(c, (unsigned)slot[4 + r] ^ (r < 4 ? 0xFFu : 0u));
    }
    s_crc[tid] = c;
    __syncthreads();
    for (int l = 0; l < 8; ++l) {
      const int stride = 1 << l;
      if ((tid & (2 * stride - 1)) == 0) s_crc[tid] = crc_mulmod(s_crc[tid], s_x[l]) ^ s_crc[tid + stride];
      __syncthreads();
    }
    if (tid == 0) {
      unsigned* mt = a.meta + (f * a.nchunks + k) * 4;
      mt[0] = dlen;
      mt[3] = s_crc[0];
      if (!last) {
        const unsigned crc = ~s_crc[0];
        unsigned char* e = slot + 8 + dlen;
        e[0] = (unsigned char)(crc >> 24); e[1] = (unsigned char)(crc >> 16); e[2] = (unsigned char)(crc >> 8); e[3] = (unsigned char)crc;
      }
    }
  }
}

__device__ __forceinline__ void png_code_chunk(const PngArgs& a, DeflateTables& t, const unsigned char* s_data, unsigned* s_match,
                                               unsigned* s_tab, long long f, int k, int n, bool last) {
  png_code_tables(t, s_data, s_match, s_tab, n, last);
  unsigned tok_at;
  const unsigned tok_bits = png_token_bits(t, s_data, s_match, n, tok_at);
  png_write_chunk(a, t, s_data, s_match, s_tab, f, k, n, last, tok_at, tok_bits);
}

// Level 0's matches.  Positions go through the table 256 at a time: a position sees the latest earlier-batch position with its hash
// (atomicMax: by position, not by arrival), and its predecessor (runs).  Each is priced at 8 bits for the length symbol, 5 for
// the distance symbol and their extra bits; the one that saves more against the literals it covers wins, the nearer on a tie,
// and one that saves less than MATCH_GAIN is dropped.  s_tab: the hash table, 1 << HASH_BITS zeroed words; s_data: the chunk's
// bytes and two readable ones behind them.
__device__ __forceinline__ void png_match_fast(DeflateTables& t, const unsigned char* s_data, unsigned* s_match, unsigned* s_tab, int n) {
  auto& s_cost = t.cost;
  const int tid = threadIdx.x;
  for (int base = 0; base < n; base += 256) {
    const int p = base + tid;
    const bool h3 = p + 2 < n;
    unsigned h = 0, cand = 0;
    if (h3) {
      h = ((s_data[p] | (s_data[p + 1] << 8) | (s_data[p + 2] << 16)) * 0x9E3779B1u) >> (32 - HASH_BITS);
      cand = s_tab[h];
    }
    __syncthreads();
    if (h3) atomicMax(&s_tab[h], (unsigned)(p + 1));
    if (p < n) {
      const int maxl = min(MAX_MATCH, n - p);
      int l1 = 0, l2 = 0;
      if (cand) {
        const int q = (int)cand - 1;
        while (l1 < maxl && s_data[q + l1] == s_data[p + l1]) ++l1;
      }
      if (p >= 1)
        while (l2 < maxl && s_data[p - 1 + l2] == s_data[p + l2]) ++l2;
      int lit1 = 0, lit2 = 0, acc = 0;
      for (int i = 0; i < max(l1, l2); ++i) {
        acc += s_cost[s_data[p + i]];
        if (i + 1 == l1) lit1 = acc;
        if (i + 1 == l2) lit2 = acc;
      }
      int bl = 0, bd = 0, bg = 0;
      if (l1 >= MIN_MATCH) {
        const int g = lit1 - match_cost(l1, p + 1 - (int)cand);
        if (g >= MATCH_GAIN) { bg = g; bl = l1; bd = p + 1 - (int)cand; }
      }
      if (l2 >= MIN_MATCH) {
        const int g = lit2 - match_cost(l2, 1);
        if (g >= MATCH_GAIN && (!bl || g >= bg)) { bl = l2; bd = 1; }
      }
      s_match[p] = bl ? (unsigned)bl | ((unsigned)bd << 16) : 0u;
    }
    __syncthreads();
  }
}

struct DeflateLds {                        // all of k_png_deflate's LDS, in one place so that its size is checked
  unsigned match[PNG_CHUNK];               // length | distance << 16 | token start << 31
  unsigned tab[PNG_CHUNK / 4 + 4];         // hash table (position + 1), then tree scratch, then the bit buffer
  DeflateTables t;
  unsigned char data[PNG_CHUNK + 8];
};
// 54308 B: three blocks fit a CU's 160 KiB with 916 B to spare.  Anything added here must keep that.
static_assert(3 * sizeof(DeflateLds) <= 160 * 1024, "k_png_deflate: three blocks per CU no longer fit the LDS");

__global__ __launch_bounds__(256) void k_png_deflate(PngArgs a) {
  __shared__ DeflateLds lds;
  auto& s_data = lds.data;
  auto& s_match = lds.match;
  auto& s_tab = lds.tab;

  const int tid = threadIdx.x;
  const int k = blockIdx.x;
  const long long f = blockIdx.y;
  const long long begin = (long long)k * PNG_CHUNK;
  const int n = (int)min((long long)PNG_CHUNK, a.stream_len - begin);
  const bool last = k == a.nchunks - 1;
  const unsigned char* in = a.stream + f * a.stream_len + begin;

  // ---- load, Adler partial sums, clear
  unsigned ad_a = 0, ad_b = 0;
  for (int p = tid; p < PNG_CHUNK + 8; p += 256) {
    const unsigned d = p < n ? in[p] : 0;
    s_data[p] = (unsigned char)d;
    ad_a += d;
    if (p < n) ad_b = (ad_b + (unsigned)(n - p) * d) % ADLER_MOD;
  }
  for (int i = tid; i < PNG_CHUNK / 4 + 4; i += 256) s_tab[i] = 0;
  for (int i = tid; i < 320; i += 256) { lds.t.freq[i] = 0; lds.t.len[i] = 0; lds.t.code[i] = 0; }
  png_chunk_adler(a, lds.t, f, k, ad_a, ad_b);
  png_literal_costs(lds.t, s_data, n);

  png_match_fast(lds.t, s_data, s_match, s_tab, n);
  png_greedy_parse(s_match, n);
  png_code_chunk(a, lds.t, s_data, s_match, s_tab, f, k, n, last);
}

// ------------------------------------------------------------------------------------------------------ deflate, level 1
// k_png_deflate_dense: k_png_deflate's grid, slots and meta words, with a denser matcher and a lazy step in front of the same
// parse and coder (tests/png_dense_ref.py is its rule).  The block loads the chunk behind up to PNG_HIST bytes of the same
// frame's stream before it, the window; chunk 0 has none, and no window reaches into another frame.  Window positions are
// linked into hash chains: prev of a position is the nearest earlier window position with its hash.  The table goes 256
// positions at a time: a position takes the table's entry from the batches before (atomicMax: by position, not by arrival) or
// the nearest lower lane of its own batch with its hash, so the chains are a function of the bytes alone.  A chunk position
// then tries distance 1 and DENSE_CANDIDATES chain entries, nearest first; only a candidate longer than all before it is
// priced (k_png_deflate's prices), the best gain of at least MATCH_GAIN wins, and the walk ends at the longest possible length.
// Lazy step: a match is dropped if the next position holds a longer one.  The Adler sums and the CRC cover the chunk only.
// Prices are estimates, so these tokens can code larger than level 0's (photographic rows, by a fraction of a percent): the
// block first codes the chunk with level 0's matcher (png_match_fast), keeps that code's tables, header and size aside, and
// falls back to it where it is strictly smaller, so no chunk is larger than level 0's.
constexpr int PNG_HIST = 8192;             // window bytes in front of the chunk (tests/png_dense_ref.py HIST)
constexpr int DENSE_HASH_BITS = 12;
constexpr int DENSE_CANDIDATES = 64;
static_assert(PNG_HIST + PNG_CHUNK <= 32768 && PNG_HIST + PNG_CHUNK < 65535, "distances fit deflate's window, positions + 1 a chain link");

// The LDS plan.  One region of 48 KiB holds, in turn: level 0's hash table and scratch (at its front) and match words (its last
// 32 KiB); then the chain links (2 B a window position, the first 32 KiB) and the hash heads (the last 16 KiB); then the match
// words again (4 B a chunk position, the last 32 KiB), which grow over links that are done with: the match words of chunk
// position p lie on the links of chunk positions 2p and 2p + 1, chains only run backwards, and the chunk's positions are
// matched from its end, 256 at a time with a barrier between a batch's walks and its stores, so a store only covers links of
// positions at or behind its own batch.  Last, the front of the region is scratch and bit buffer again.
struct DenseLds {                          // all of k_png_deflate_dense's LDS
  unsigned region[(PNG_HIST + PNG_CHUNK) / 2 + PNG_CHUNK / 2];
  DeflateTables t;
  unsigned alt_hdr[144];                   // level 0's code of the chunk, kept for the fallback: the header's bits (4498 at most),
  unsigned alt_bits;                       // their number,
  unsigned short alt_code[320];            // the codes
  unsigned char alt_len[320];              // and their lengths
  unsigned short hb[256];                  // the hashes of the batch being linked
  unsigned char data[PNG_HIST + PNG_CHUNK + 8];
};
// 72 728 B: two blocks per CU (160 KiB).  With the match words beside the links (32 + 32 KiB, 89 112 B, one block per CU) the
// kernel took 118.1 ms for 120 frames of 384 x 512 x 3 on an MI355X; see DESIGN.md 5.3 for this layout's time.
static_assert(2 * sizeof(DenseLds) <= 160 * 1024, "k_png_deflate_dense: two blocks per CU no longer fit the LDS");
static_assert(PNG_HIST == PNG_CHUNK, "the overlay of match words and links assumes a history of 0 or PNG_CHUNK bytes");
static_assert((1 << DENSE_HASH_BITS) * 4 <= PNG_CHUNK * 2, "the hash heads live behind the links");

__global__ __launch_bounds__(256) void k_png_deflate_dense(PngArgs a) {
  __shared__ DenseLds lds;
  auto& s_cost = lds.t.cost;
  unsigned short* s_prev = (unsigned short*)lds.region;      // [PNG_HIST + PNG_CHUNK]
  unsigned* s_head = lds.region + (PNG_HIST + PNG_CHUNK) / 2;   // [1 << DENSE_HASH_BITS]
  unsigned* s_match = lds.region + PNG_CHUNK / 2;            // [PNG_CHUNK]
  unsigned* s_tab = lds.region;                              // [PNG_CHUNK / 4 + 4]

  const int tid = threadIdx.x;
  const int k = blockIdx.x;
  const long long f = blockIdx.y;
  const long long begin = (long long)k * PNG_CHUNK;
  const int n = (int)min((long long)PNG_CHUNK, a.stream_len - begin);
  const int h0 = (int)min((long long)PNG_HIST, begin);       // history bytes: the same frame's only
  const int m = h0 + n;                                      // window bytes
  const bool last = k == a.nchunks - 1;
  const unsigned char* in = a.stream + f * a.stream_len + begin - h0;
  unsigned char* s_win = lds.data;                           // the window
  unsigned char* s_data = lds.data + h0;                     // the chunk

  // ---- load, Adler partial sums over the chunk, clear
  unsigned ad_a = 0, ad_b = 0;
  for (int i = tid; i < PNG_HIST + PNG_CHUNK + 8; i += 256) {
    const unsigned d = i < m ? in[i] : 0;
    s_win[i] = (unsigned char)d;
    if (i >= h0 && i < m) {
      ad_a += d;
      ad_b = (ad_b + (unsigned)(m - i) * d) % ADLER_MOD;
    }
  }
  for (int i = tid; i < PNG_CHUNK / 4 + 4; i += 256) s_tab[i] = 0;
  for (int i = tid; i < 320; i += 256) { lds.t.freq[i] = 0; lds.t.len[i] = 0; lds.t.code[i] = 0; }
  png_chunk_adler(a, lds.t, f, k, ad_a, ad_b);
  png_literal_costs(lds.t, s_data, n);

  // ---- level 0's tokens and their code, kept aside
  png_match_fast(lds.t, s_data, s_match, s_tab, n);
  png_greedy_parse(s_match, n);
  png_code_tables(lds.t, s_data, s_match, s_tab, n, last);
  unsigned tok_at0;
  const unsigned tok_bits0 = png_token_bits(lds.t, s_data, s_match, n, tok_at0);
  const unsigned coded0 = png_coded_bytes(lds.t.bits[0], tok_bits0, lds.t.len[256], last);
  const unsigned bytes0 = coded0 < (unsigned)n ? coded0 : 5u + (unsigned)n;
  for (int i = tid; i < 144; i += 256) lds.alt_hdr[i] = s_tab[i];
  for (int i = tid; i < 320; i += 256) { lds.alt_code[i] = lds.t.code[i]; lds.alt_len[i] = lds.t.len[i]; }
  if (tid == 0) lds.alt_bits = lds.t.bits[0];
  __syncthreads();
  for (int i = tid; i < (int)(sizeof(lds.region) / 4); i += 256) lds.region[i] = 0;      // links: none; heads: none
  for (int i = tid; i < 320; i += 256) { lds.t.freq[i] = 0; lds.t.len[i] = 0; lds.t.code[i] = 0; }
  __syncthreads();

  // ---- chains over the window's hashed positions (those with two bytes behind them in the window)
  const int nh = m - 2;
  for (int base = 0; base < nh; base += 256) {
    const int i = base + tid;
    const bool on = i < nh;
    unsigned h = 0xFFFFu, link = 0;
    if (on) {
      h = ((s_win[i] | (s_win[i + 1] << 8) | (s_win[i + 2] << 16)) * 0x9E3779B1u) >> (32 - DENSE_HASH_BITS);
      link = s_head[h];
    }
    lds.hb[tid] = (unsigned short)h;
    __syncthreads();
    if (on) {
      atomicMax(&s_head[h], (unsigned)(i + 1));
      for (int j = tid - 1; j >= 0; j -= 8) {                // the nearest lower lane with this hash, eight lanes at a time
        unsigned hit = 0;
#pragma unroll
        for (int u = 7; u >= 0; --u)
          if (j - u >= 0 && lds.hb[j - u] == h) hit = (unsigned)(j - u + 1);
        if (hit) { link = (unsigned)base + hit; break; }
      }
      s_prev[i] = (unsigned short)link;
    }
    __syncthreads();
  }

  // ---- matches of the chunk's positions, 256 at a time from the chunk's end (see DenseLds)
  for (int base = (n - 1) & ~255; base >= 0; base -= 256) {
    const int p = base + tid;
    unsigned mw = 0;
    if (p < n) {
      const int i = h0 + p, maxl = min(MAX_MATCH, n - p);
      int bl = 0, bd = 0, bg = 0, longest = 0, acc = 0;      // acc: the price of the first `longest` bytes as literals
      unsigned link = s_prev[i];
      for (int c = 0; c <= DENSE_CANDIDATES; ++c) {
        int q;
        if (c == 0) {
          if (i < 1) continue;
          q = i - 1;
        } else {
          if (!link) break;
          q = (int)link - 1;
          link = s_prev[q];
        }
        if (s_win[q + longest] != s_win[i + longest]) continue;   // cannot be longer
        int l = 0;
        while (l < maxl && s_win[q + l] == s_win[i + l]) ++l;
        if (l <= longest) continue;
        for (int u = longest; u < l; ++u) acc += s_cost[s_win[i + u]];
        longest = l;
        if (l >= MIN_MATCH) {
          const int g = acc - match_cost(l, i - q);
          if (g >= MATCH_GAIN && g > bg) { bg = g; bl = l; bd = i - q; }
        }
        if (l >= maxl) break;
      }
      mw = bl ? (unsigned)bl | ((unsigned)bd << 16) : 0u;
    }
    __syncthreads();
    if (p < n) s_match[p] = mw;
  }
  __syncthreads();

  // ---- lazy step: thread t owns positions t, t + 256, ...; all are read before any is dropped
  unsigned drop = 0;
  for (int r = 0; r < PNG_CHUNK / 256; ++r) {
    const int p = r * 256 + tid;
    if (p + 1 < n) {
      const unsigned l0 = s_match[p] & 0x1FFu, l1 = s_match[p + 1] & 0x1FFu;
      if (l0 && l1 > l0) drop |= 1u << r;
    }
  }
  __syncthreads();
  for (int r = 0; r < PNG_CHUNK / 256; ++r)
    if (drop & (1u << r)) s_match[r * 256 + tid] = 0;
  __syncthreads();

  png_greedy_parse(s_match, n);
  png_code_tables(lds.t, s_data, s_match, s_tab, n, last);
  unsigned tok_at;
  unsigned tok_bits = png_token_bits(lds.t, s_data, s_match, n, tok_at);
  const unsigned coded1 = png_coded_bytes(lds.t.bits[0], tok_bits, lds.t.len[256], last);
  const unsigned bytes1 = coded1 < (unsigned)n ? coded1 : 5u + (unsigned)n;

  // ---- fallback (the same for the whole block): level 0's tokens again, behind the code kept aside
  if (bytes0 < bytes1) {
    __syncthreads();
    for (int i = tid; i < PNG_CHUNK / 4 + 4; i += 256) s_tab[i] = 0;
    __syncthreads();
    png_match_fast(lds.t, s_data, s_match, s_tab, n);
    png_greedy_parse(s_match, n);
    for (int i = tid; i < PNG_CHUNK / 4 + 4; i += 256) s_tab[i] = i < 144 ? lds.alt_hdr[i] : 0u;
    for (int i = tid; i < 320; i += 256) { lds.t.code[i] = lds.alt_code[i]; lds.t.len[i] = lds.alt_len[i]; }
    if (tid == 0) lds.t.bits[0] = lds.alt_bits;
    __syncthreads();
    tok_at = tok_at0;
    tok_bits = tok_bits0;
  }
  png_write_chunk(a, lds.t, s_data, s_match, s_tab, f, k, n, last, tok_at, tok_bits);
}

// --------------------------------------------------------------------------------------------------------------- pack
constexpr int PNG_HEAD = 8 + 25, PNG_TAIL = 12;   // signature + IHDR; IEND

// One frame, by its block: where each of its chunks goes behind the first (chunk_off; `framing` bytes of length, type, CRC and,
// in an APNG's fdAT, sequence number around each), the frame's Adler-32.  -> the bytes of all its chunks, in every thread.
__device__ __forceinline__ unsigned png_scan_frame(const PngArgs& a, long long f, unsigned framing) {
  __shared__ unsigned s_w[4];
  const unsigned* meta = a.meta + f * a.nchunks * 4;
  unsigned run = 0;
  for (int base = 0; base < a.nchunks; base += 256) {
    const int k = base + threadIdx.x;
    const unsigned v = k < a.nchunks ? framing + meta[4 * k] + (k == a.nchunks - 1 ? 4u : 0u) : 0u;
    unsigned total;
    const unsigned e = vf_block_excl_scan<unsigned, 256>(v, s_w, total);
    if (k < a.nchunks) a.chunk_off[f * a.nchunks + k] = run + e;
    run += total;
  }
  // The Adler-32: appending a piece (byte sum A, weighted sum B, length L) to sums (s1, s2) gives (s1 + A, s2 + L * s1 + B), and
  // that is associative.  Each thread folds a run of consecutive chunks from (0, 0), thread 0 folds the 256 runs from (1, 0): at
  // the largest frame (98 305 chunks) that is 385 + 256 dependent steps, not 98 305.
  __shared__ unsigned s_a[256], s_b[256];
  __shared__ unsigned long long s_l[256];
  {
    const int per = (a.nchunks + 255) / 256, k0 = min(threadIdx.x * per, (unsigned)a.nchunks), k1 = min(k0 + per, a.nchunks);
    unsigned long long s1 = 0, s2 = 0, tot = 0;
    for (int k = k0; k < k1; ++k) {
      const unsigned long long len = (unsigned long long)min((long long)PNG_CHUNK, a.stream_len - (long long)k * PNG_CHUNK);
      s2 = (s2 + len * s1 + meta[4 * k + 2]) % ADLER_MOD;
      s1 = (s1 + meta[4 * k + 1]) % ADLER_MOD;
      tot += len;
    }
    s_a[threadIdx.x] = (unsigned)s1; s_b[threadIdx.x] = (unsigned)s2; s_l[threadIdx.x] = tot;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s1 = 1, s2 = 0;
    for (int t = 0; t < 256; ++t) {
      s2 = (s2 + (s_l[t] % ADLER_MOD) * s1 + s_b[t]) % ADLER_MOD;
      s1 = (s1 + s_a[t]) % ADLER_MOD;
    }
    a.adler[f] = (unsigned)((s2 << 16) | s1);
  }
  return run;
}

// one block per frame: where each IDAT goes, the frame's Adler-32, the file's size (offsets[f + 1], summed by k_vf_file_offsets)
__global__ __launch_bounds__(256) void k_png_frame_scan(PngArgs a) {
  const long long f = blockIdx.x;
  const unsigned run = png_scan_frame(a, f, 12u);
  if (threadIdx.x == 0) a.offsets[f + 1] = (int64_t)PNG_HEAD + run + PNG_TAIL;
}

__device__ __forceinline__ void put_be32(unsigned char* p, unsigned v) {
  p[0] = (unsigned char)(v >> 24); p[1] = (unsigned char)(v >> 16); p[2] = (unsigned char)(v >> 8); p[3] = (unsigned char)v;
}

__global__ __launch_bounds__(256) void k_png_pack(PngArgs a) {
  const int k = blockIdx.x;
  const long long f = blockIdx.y;
  const bool last = k == a.nchunks - 1;
  const unsigned* mt = a.meta + (f * a.nchunks + k) * 4;
  const unsigned dlen = mt[0];
  const unsigned char* slot = a.slots + (f * a.nchunks + k) * (long long)PNG_SLOT;
  unsigned char* file = a.out + a.offsets[f];
  unsigned char* dst = file + PNG_HEAD + a.chunk_off[f * a.nchunks + k];
  const unsigned ncopy = 8 + dlen + (last ? 0u : 4u);
  for (unsigned i = threadIdx.x; i < ncopy; i += 256) dst[i] = slot[i];
  if (threadIdx.x == 0 && last) {                      // the Adler-32 goes through the chunk's CRC register, then IEND
    const unsigned ad = a.adler[f];
    unsigned c = mt[3];
    for (int i = 0; i < 4; ++i) c = crc_byte(c, (ad >> (24 - 8 * i)) & 255);
    put_be32(dst + 8 + dlen, ad);
    put_be32(dst + 12 + dlen, ~c);
    unsigned char* e = dst + 16 + dlen;
    const unsigned char iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    for (int i = 0; i < 12; ++i) e[i] = iend[i];
  }
  if (threadIdx.x == 64 && k == 0) {
    const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    for (int i = 0; i < 8; ++i) file[i] = sig[i];
    unsigned char* h = file + 8;
    put_be32(h, 13);
    h[4] = 'I'; h[5] = 'H'; h[6] = 'D'; h[7] = 'R';
    put_be32(h + 8, (unsigned)a.W);
    put_be32(h + 12, (unsigned)a.H);
    h[16] = 8; h[17] = a.C == 3 ? 2 : 0; h[18] = 0; h[19] = 0; h[20] = 0;
    unsigned c = 0xFFFFFFFFu;
    for (int i = 4; i < 21; ++i) c = crc_byte(c, h[i]);
    put_be32(h + 21, ~c);
  }
}

// --------------------------------------------------------------------------------------------------------------- APNG
// An animated PNG of a clip: signature, frame 0's IHDR, acTL; per frame an fcTL and the frame's own zlib stream,
// frame 0's as its IDATs, every later frame's as one fdAT (sequence number + the IDAT's payload) per IDAT; IEND.  The filter and
// deflate kernels above run over all frames of all clips; what follows places and frames their chunks.
constexpr int APNG_HEAD = PNG_HEAD + 20, APNG_FCTL = 38;   // signature + IHDR + acTL; an fcTL chunk
constexpr int APNG_SLICE = 65535;                          // frames per launch of the kernels with a frame per blockIdx.y

struct ApngArgs {
  PngArgs p;                      // offsets: [clips + 1]; the other arrays hold clips * frames frames, clip after clip
  unsigned* frame_len;            // [clips * frames]: bytes of the frame's chunks with their framing, behind its fcTL
  unsigned long long* frame_off;  // [clips * frames]: the frame's fcTL in its clip's file
  long long f0;                   // the first frame of this launch
  int frames;                     // per clip
  int delay, loop;
};

// one block per frame: k_png_frame_scan with 16 bytes around an fdAT's data, and the frame's size to frame_len
__global__ __launch_bounds__(256) void k_apng_frame_scan(ApngArgs g) {
  const long long f = g.f0 + blockIdx.x;
  const unsigned run = png_scan_frame(g.p, f, f % g.frames == 0 ? 12u : 16u);
  if (threadIdx.x == 0) g.frame_len[f] = run;
}

// one block per clip: where each frame's fcTL goes, the file's size (offsets[clip + 1], summed by k_vf_file_offsets)
__global__ __launch_bounds__(256) void k_apng_clip_scan(ApngArgs g) {
  __shared__ unsigned long long s_w[4];
  const long long clip = blockIdx.x, fb = clip * g.frames;
  unsigned long long run = APNG_HEAD;
  for (int base = 0; base < g.frames; base += 256) {
    const int j = base + threadIdx.x;
    const unsigned long long v = j < g.frames ? (unsigned long long)APNG_FCTL + g.frame_len[fb + j] : 0ull;
    unsigned long long total;
    const unsigned long long e = vf_block_excl_scan<unsigned long long, 256>(v, s_w, total);
    if (j < g.frames) g.frame_off[fb + j] = run + e;
    run += total;
  }
  if (threadIdx.x == 0) g.p.offsets[clip + 1] = (int64_t)(run + PNG_TAIL);
}

// length, type and dlen bytes of data are in place at h: the CRC-32 behind them, serially (the small chunks: acTL, fcTL)
__device__ __forceinline__ void apng_seal(unsigned char* h, int dlen) {
  unsigned c = 0xFFFFFFFFu;
  for (int i = 4; i < 8 + dlen; ++i) c = crc_byte(c, h[i]);
  put_be32(h + 8 + dlen, ~c);
}

// one block per chunk.  Frame 0 of a clip: k_png_pack's copy behind signature, IHDR, acTL and fcTL.  A later frame: the IDAT's
// data behind an fdAT's length, type and sequence number.  Its CRC comes from the IDAT's register r = S(F, 'IDAT' || data) the
// deflate kernel left (S: the raw register function, F: the all-ones preset): S is linear in its start value, so
//   S(F, 'fdAT' || seq || data) = r ^ (S(F, 'IDAT') ^ S(F, 'fdAT' || seq)) * x^(8 * dlen)   mod the CRC polynomial,
// the power by square and multiply; the frame's Adler-32 then goes through that register as in k_png_pack.
__global__ __launch_bounds__(256) void k_apng_pack(ApngArgs g) {
  const PngArgs& a = g.p;
  const int k = blockIdx.x;
  const long long f = g.f0 + blockIdx.y, clip = f / g.frames;
  const int j = (int)(f - clip * g.frames);
  const bool last = k == a.nchunks - 1;
  const unsigned* mt = a.meta + (f * a.nchunks + k) * 4;
  const unsigned dlen = mt[0];
  const unsigned char* slot = a.slots + (f * a.nchunks + k) * (long long)PNG_SLOT;
  unsigned char* file = a.out + a.offsets[clip];
  unsigned char* fctl = file + g.frame_off[f];
  unsigned char* dst = fctl + APNG_FCTL + a.chunk_off[f * a.nchunks + k];
  // sequence numbers: frame 0's fcTL has 0; frame j >= 1 takes nchunks + 1 from 1 + (j - 1) * (nchunks + 1) on
  const unsigned seq_fctl = j ? 1u + (unsigned)(j - 1) * (unsigned)(a.nchunks + 1) : 0u;
  const unsigned hd = j ? 12u : 8u;                    // bytes in front of the chunk's data
  if (j == 0) {
    const unsigned ncopy = 8 + dlen + (last ? 0u : 4u);
    for (unsigned i = threadIdx.x; i < ncopy; i += 256) dst[i] = slot[i];
  } else {
    for (unsigned i = threadIdx.x; i < dlen; i += 256) dst[12 + i] = slot[8 + i];
  }
  if (threadIdx.x == 0 && (j || last)) {
    unsigned c = mt[3];
    if (j) {
      const unsigned seq = seq_fctl + 1u + (unsigned)k;
      put_be32(dst, dlen + 4u + (last ? 4u : 0u));
      dst[4] = 'f'; dst[5] = 'd'; dst[6] = 'A'; dst[7] = 'T';
      put_be32(dst + 8, seq);
      unsigned r1 = 0xFFFFFFFFu, r2 = 0xFFFFFFFFu;
      for (int i = 4; i < 8; ++i) r1 = crc_byte(r1, slot[i]);
      for (int i = 4; i < 12; ++i) r2 = crc_byte(r2, dst[i]);
      unsigned xp = 0x80000000u, sq = 0x00800000u;     // 1 and x^8
      for (unsigned e = dlen; e; e >>= 1) {
        if (e & 1) xp = crc_mulmod(xp, sq);
        sq = crc_mulmod(sq, sq);
      }
      c ^= crc_mulmod(r1 ^ r2, xp);
    }
    unsigned char* t = dst + hd + dlen;
    if (last) {
      const unsigned ad = a.adler[f];
      for (int i = 0; i < 4; ++i) c = crc_byte(c, (ad >> (24 - 8 * i)) & 255);
      put_be32(t, ad);
      t += 4;
    }
    put_be32(t, ~c);
    if (last && j == g.frames - 1) {
      const unsigned char iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
      for (int i = 0; i < 12; ++i) t[4 + i] = iend[i];
    }
  }
  if (threadIdx.x == 64 && k == 0) {
    if (j == 0) {
      const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
      for (int i = 0; i < 8; ++i) file[i] = sig[i];
      unsigned char* h = file + 8;
      put_be32(h, 13);
      h[4] = 'I'; h[5] = 'H'; h[6] = 'D'; h[7] = 'R';
      put_be32(h + 8, (unsigned)a.W);
      put_be32(h + 12, (unsigned)a.H);
      h[16] = 8; h[17] = a.C == 3 ? 2 : 0; h[18] = 0; h[19] = 0; h[20] = 0;
      apng_seal(h, 13);
      h = file + PNG_HEAD;
      put_be32(h, 8);
      h[4] = 'a'; h[5] = 'c'; h[6] = 'T'; h[7] = 'L';
      put_be32(h + 8, (unsigned)g.frames);
      put_be32(h + 12, (unsigned)g.loop);
      apng_seal(h, 8);
    }
    unsigned char* h = fctl;
    put_be32(h, 26);
    h[4] = 'f'; h[5] = 'c'; h[6] = 'T'; h[7] = 'L';
    put_be32(h + 8, seq_fctl);
    put_be32(h + 12, (unsigned)a.W);
    put_be32(h + 16, (unsigned)a.H);
    put_be32(h + 20, 0);
    put_be32(h + 24, 0);
    h[28] = (unsigned char)(g.delay >> 8); h[29] = (unsigned char)g.delay;
    h[30] = 0; h[31] = 100;                             // delay_den: centiseconds
    h[32] = 0; h[33] = 0;                               // dispose NONE, blend SOURCE
    apng_seal(h, 26);
  }
}

struct PngPlan {
  long long rb, stream_len, nchunks;
  size_t o_stream, o_slots, o_meta, o_off, o_adler, ws_bytes, out_bytes;
};

int png_plan(const char* who, int n, int H, int W, int C, PngPlan* p) {
  VF_REQUIRE(C == 1 || C == 3, "%s: %d channels (a PNG frame here is grey, 1 channel, or RGB, 3)", who, C);
  VF_REQUIRE(H >= 1 && W >= 1 && H <= PNG_MAX_SIDE && W <= PNG_MAX_SIDE, "%s: a %dx%d frame (sides are 1 to %d)", who, H, W, PNG_MAX_SIDE);
  VF_REQUIRE(n >= 1 && n <= 65535, "%s: a batch of %d frames (1 to 65535)", who, n);
  p->rb = (long long)W * C;
  p->stream_len = (long long)H * (p->rb + 1);
  p->nchunks = vf_cdiv(p->stream_len, PNG_CHUNK);
  const size_t chunks = (size_t)n * p->nchunks;
  VfCarve ws;
  p->o_stream = ws.take((size_t)n * p->stream_len);
  p->o_slots = ws.take(chunks * PNG_SLOT);
  p->o_meta = ws.take(chunks * 16);
  p->o_off = ws.take(chunks * 4);
  p->o_adler = ws.take((size_t)n * 4);
  p->ws_bytes = ws.at;
  // every chunk stored: 5 bytes of block header and 12 of IDAT framing each; zlib header and Adler-32; signature, IHDR, IEND
  p->out_bytes = (size_t)n * ((size_t)p->stream_len + (size_t)p->nchunks * 17 + 6 + PNG_HEAD + PNG_TAIL);
  return 0;
}

struct ApngPlan {
  PngPlan png;               // the geometry of one frame; its offsets and bounds are not used
  long long frames_all;
  size_t o_stream, o_slots, o_meta, o_off, o_adler, o_flen, o_foff, ws_bytes, out_bytes;
};

int apng_plan(const char* who, int g, int n, int H, int W, int C, int delay, int loop, ApngPlan* p) {
  if (int e = png_plan(who, 1, H, W, C, &p->png)) return e;
  VF_REQUIRE(n >= 1 && n <= 65535, "%s: n: a clip of %d frames (1 to 65535)", who, n);
  VF_REQUIRE(g >= 1 && g <= 65535, "%s: g: a batch of %d clips (1 to 65535)", who, g);
  VF_REQUIRE(delay >= 0 && delay <= 65535, "%s: delay: %d centiseconds (0 to 65535)", who, delay);
  VF_REQUIRE(loop >= 0 && loop <= 65535, "%s: loop: %d plays (0 to 65535; 0 plays forever)", who, loop);
  VF_REQUIRE((long long)n * (p->png.nchunks + 1) < (1ll << 31),
             "%s: n: %d frames of %lld chunks (sequence numbers, frames * (chunks + 1), stay below 2^31)", who, n, p->png.nchunks);
  p->frames_all = (long long)g * n;
  const size_t frames = (size_t)p->frames_all, chunks = frames * (size_t)p->png.nchunks;
  VfCarve ws;
  p->o_stream = ws.take(frames * (size_t)p->png.stream_len);
  p->o_slots = ws.take(chunks * PNG_SLOT);
  p->o_meta = ws.take(chunks * 16);
  p->o_off = ws.take(chunks * 4);
  p->o_adler = ws.take(frames * 4);
  p->o_flen = ws.take(frames * 4);
  p->o_foff = ws.take(frames * 8);
  p->ws_bytes = ws.at;
  // every chunk stored: 5 bytes of block header and 16 of fdAT framing each; zlib header and Adler-32; an fcTL per frame;
  // signature, IHDR, acTL, IEND
  p->out_bytes = (size_t)g * ((size_t)n * ((size_t)p->png.stream_len + (size_t)p->png.nchunks * 21 + 6 + APNG_FCTL) + APNG_HEAD + PNG_TAIL);
  return 0;
}

}  // namespace

VF_API int vf_apng_workspace_bytes(int g, int n, int H, int W, int C, int delay, int loop, size_t* ws_bytes, size_t* out_bytes) {
  ApngPlan p;
  if (int e = apng_plan("vf_apng_workspace_bytes", g, n, H, W, C, delay, loop, &p)) return e;
  if (ws_bytes) *ws_bytes = p.ws_bytes;
  if (out_bytes) *out_bytes = p.out_bytes;
  return 0;
}

namespace {

// level 0: k_png_deflate; level 1: k_png_deflate_dense.  Every other stage is the same for both.
int png_check_level(const char* who, int level) {
  VF_REQUIRE(level == 0 || level == 1, "%s: level: %d (0: the fast matcher; 1: dense, chained matches over history)", who, level);
  return 0;
}

void png_launch_deflate(vf_ctx* ctx, int level, double stream, dim3 grid, const PngArgs& a) {
  if (level == 0) VF_LAUNCH_TIMED(ctx, "png_deflate", 0.0, 2.0 * stream, k_png_deflate, grid, dim3(256), a);
  else VF_LAUNCH_TIMED(ctx, "png_deflate_dense", 0.0, 3.0 * stream, k_png_deflate_dense, grid, dim3(256), a);
}

int apng_encode(const char* who, vf_ctx* ctx, const void* src, int kind, int g, int n, int H, int W, int C, int delay, int loop, int level,
                void* ws, size_t ws_bytes, unsigned char* out, size_t out_cap, int64_t* offsets) {
  ApngPlan p;
  if (int e = png_check_level(who, level)) return e;
  if (int e = apng_plan(who, g, n, H, W, C, delay, loop, &p)) return e;
  char batch[80];
  snprintf(batch, sizeof(batch), "%d clips of %d frames of %dx%dx%d", g, n, H, W, C);
  if (int e = vf_check_encode_entry(who, kind, "C", batch, ws_bytes, p.ws_bytes, out_cap, p.out_bytes)) return e;
  ApngArgs A;
  PngArgs& a = A.p;
  a.src = src;
  a.stream = (unsigned char*)ws + p.o_stream;
  a.slots = (unsigned char*)ws + p.o_slots;
  a.meta = (unsigned*)((char*)ws + p.o_meta);
  a.chunk_off = (unsigned*)((char*)ws + p.o_off);
  a.adler = (unsigned*)((char*)ws + p.o_adler);
  a.out = out;
  a.offsets = offsets;
  a.n = n; a.H = H; a.W = W; a.C = C; a.rb = (int)p.png.rb; a.nchunks = (int)p.png.nchunks;
  a.stream_len = p.png.stream_len;
  A.frame_len = (unsigned*)((char*)ws + p.o_flen);
  A.frame_off = (unsigned long long*)((char*)ws + p.o_foff);
  A.frames = n; A.delay = delay; A.loop = loop;
  const long long nchunks = p.png.nchunks;
  // the kernels of vf_png_encode as they are, a slice of at most APNG_SLICE frames (blockIdx.y) at a time: the slice's arrays
  for (long long f0 = 0; f0 < p.frames_all; f0 += APNG_SLICE) {
    const int m = (int)(p.frames_all - f0 < APNG_SLICE ? p.frames_all - f0 : APNG_SLICE);
    PngArgs s = a;
    s.src = (const char*)src + (size_t)f0 * H * W * C * (kind == 0 ? sizeof(float) : 1);
    s.stream = a.stream + f0 * a.stream_len;
    s.slots = a.slots + f0 * nchunks * PNG_SLOT;
    s.meta = a.meta + f0 * nchunks * 4;
    s.n = m;
    const double px = (double)m * H * W * C, stream = (double)m * a.stream_len;
    if (kind == 0) VF_LAUNCH_TIMED(ctx, "png_filter", 0.0, 8.0 * px + stream, k_png_filter<0>, dim3(H, m), dim3(256), s);
    else VF_LAUNCH_TIMED(ctx, "png_filter", 0.0, 2.0 * px + stream, k_png_filter<1>, dim3(H, m), dim3(256), s);
    VF_LAUNCH_CHECK();
    png_launch_deflate(ctx, level, stream, dim3((unsigned)nchunks, m), s);
    VF_LAUNCH_CHECK();
  }
  {
    VfProf prof(ctx, "apng_pack", 0.0, 2.0 * (double)p.frames_all * a.stream_len);
    for (long long f0 = 0; f0 < p.frames_all; f0 += APNG_SLICE) {
      const int m = (int)(p.frames_all - f0 < APNG_SLICE ? p.frames_all - f0 : APNG_SLICE);
      A.f0 = f0;
      hipLaunchKernelGGL(k_apng_frame_scan, dim3(m), dim3(256), 0, ctx->stream, A);
      VF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_apng_clip_scan, dim3(g), dim3(256), 0, ctx->stream, A);
    VF_LAUNCH_CHECK();
    vf_launch_file_offsets(ctx->stream, offsets, g);
    VF_LAUNCH_CHECK();
    for (long long f0 = 0; f0 < p.frames_all; f0 += APNG_SLICE) {
      const int m = (int)(p.frames_all - f0 < APNG_SLICE ? p.frames_all - f0 : APNG_SLICE);
      A.f0 = f0;
      hipLaunchKernelGGL(k_apng_pack, dim3((unsigned)nchunks, m), dim3(256), 0, ctx->stream, A);
      VF_LAUNCH_CHECK();
    }
  }
  return 0;
}

}  // namespace

VF_API int vf_apng_encode(vf_ctx* ctx, const void* src, int kind, int g, int n, int H, int W, int C, int delay, int loop, void* ws,
                          size_t ws_bytes, unsigned char* out, size_t out_cap, int64_t* offsets) {
  return apng_encode("vf_apng_encode", ctx, src, kind, g, n, H, W, C, delay, loop, 0, ws, ws_bytes, out, out_cap, offsets);
}

VF_API int vf_apng_encode_level(vf_ctx* ctx, const void* src, int kind, int g, int n, int H, int W, int C, int delay, int loop, int level,
                                void* ws, size_t ws_bytes, unsigned char* out, size_t out_cap, int64_t* offsets) {
  return apng_encode("vf_apng_encode_level", ctx, src, kind, g, n, H, W, C, delay, loop, level, ws, ws_bytes, out, out_cap, offsets);
}

VF_API int vf_png_workspace_bytes(int n, int H, int W, int C, size_t* ws_bytes, size_t* out_bytes) {
  PngPlan p;
  if (int e = png_plan("vf_png_workspace_bytes", n, H, W, C, &p)) return e;
  if (ws_bytes) *ws_bytes = p.ws_bytes;
  if (out_bytes) *out_bytes = p.out_bytes;
  return 0;
}

namespace {

int png_encode(const char* who, vf_ctx* ctx, const void* src, int kind, int n, int H, int W, int C, int level, void* ws, size_t ws_bytes,
               unsigned char* out, size_t out_cap, int64_t* offsets) {
  PngPlan p;
  if (int e = png_check_level(who, level)) return e;
  if (int e = png_plan(who, n, H, W, C, &p)) return e;
  char batch[64];
  snprintf(batch, sizeof(batch), "%d frames of %dx%dx%d", n, H, W, C);
  if (int e = vf_check_encode_entry(who, kind, "C", batch, ws_bytes, p.ws_bytes, out_cap, p.out_bytes)) return e;
  PngArgs a;
  a.src = src;
  a.stream = (unsigned char*)ws + p.o_stream;
  a.slots = (unsigned char*)ws + p.o_slots;
  a.meta = (unsigned*)((char*)ws + p.o_meta);
  a.chunk_off = (unsigned*)((char*)ws + p.o_off);
  a.adler = (unsigned*)((char*)ws + p.o_adler);
  a.out = out;
  a.offsets = offsets;
  a.n = n; a.H = H; a.W = W; a.C = C; a.rb = (int)p.rb; a.nchunks = (int)p.nchunks;
  a.stream_len = p.stream_len;
  const double px = (double)n * H * W * C, stream = (double)n * p.stream_len;
  if (kind == 0) VF_LAUNCH_TIMED(ctx, "png_filter", 0.0, 8.0 * px + stream, k_png_filter<0>, dim3(H, n), dim3(256), a);
  else VF_LAUNCH_TIMED(ctx, "png_filter", 0.0, 2.0 * px + stream, k_png_filter<1>, dim3(H, n), dim3(256), a);
  VF_LAUNCH_CHECK();
  png_launch_deflate(ctx, level, stream, dim3((unsigned)p.nchunks, n), a);
  VF_LAUNCH_CHECK();
  {
    VfProf prof(ctx, "png_pack", 0.0, 2.0 * stream);
    hipLaunchKernelGGL(k_png_frame_scan, dim3(n), dim3(256), 0, ctx->stream, a);
    VF_LAUNCH_CHECK();
    vf_launch_file_offsets(ctx->stream, offsets, n);
    VF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_png_pack, dim3((unsigned)p.nchunks, n), dim3(256), 0, ctx->stream, a);
    VF_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace

VF_API int vf_png_encode(vf_ctx* ctx, const void* src, int kind, int n, int H, int W, int C, void* ws, size_t ws_bytes,
                         unsigned char* out, size_t out_cap, int64_t* offsets) {
  return png_encode("vf_png_encode", ctx, src, kind, n, H, W, C, 0, ws, ws_bytes, out, out_cap, offsets);
}

VF_API int vf_png_encode_level(vf_ctx* ctx, const void* src, int kind, int n, int H, int W, int C, int level, void* ws, size_t ws_bytes,
                               unsigned char* out, size_t out_cap, int64_t* offsets) {
  return png_encode("vf_png_encode_level", ctx, src, kind, n, H, W, C, level, ws, ws_bytes, out, out_cap, offsets);
}
