// vf_gif.hip — batched animated-GIF encoder: clips of frames on the device in, whole GIF89a files out.
//   k_gif_table   one block per frame: the 5-bit-per-channel histogram in LDS (bytes from float planar through vf_savepng_byte,
//                 or interleaved bytes), then either the frame's <= 256 colours in ascending order (an LDS hash
//                 set of the 24-bit colours, sorted by rank) or the median cut of tests/gif_ref.py: up to 255 sequential splits,
//                 each a block-wide argmax, a marginal histogram and the extents of the two halves; the box means from a second
//                 walk over the pixels.  Integer counts and sums only: nothing depends on the order of arrival.
//   k_gif_map     the nearest table entry of every pixel (squared distance in 8-bit RGB, lowest index on a tie), table in LDS.
//   k_gif_lzw     one lane per GIF_CHUNK pixels: variable-width LZW from Clear to Clear with a private open-addressing dictionary
//                 in the workspace; the chunk's code bits go to a private slot, their number to a table.
//   k_gif_frame_scan / k_gif_offsets / k_gif_pack   bit offsets of the chunks, sizes and places of frames and files; every output
//                 byte gathers its bits from the one or two slots that cover it; sub-block lengths, headers, tables, trailers.
// A Clear after every GIF_CHUNK pixels keeps the dictionary below 4096 entries, so chunks are independent and a frame's bytes
// depend on that frame and the delay only.
#include "vf_block.h"
#include "vf_common.h"

namespace {

constexpr int GIF_CHUNK = 3824;          // pixels from Clear to Clear (backend.GIF_CHUNK mirrors it): 258 + GIF_CHUNK <= 4096
constexpr int GIF_MAX_SIDE = 16384, GIF_MAX_FRAMES = 65535, GIF_MAX_CLIPS = 65535, GIF_MAX_DELAY = 65535;
constexpr int GIF_CELLS = 32768;
constexpr int GIF_SET = 2048;            // slots of the colour set: 256 colours + one more from each of 1024 threads at most
constexpr int GIF_DICT = 8192;           // slots of a chunk's dictionary, at most GIF_CHUNK of them used
constexpr int GIF_MAX_BITS = 9 + 12 * GIF_CHUNK + 12;          // leading Clear of a frame, the codes, the Clear or EOI behind them
constexpr int GIF_SLOT_WORDS = (GIF_MAX_BITS + 31) / 32 + 1;   // + 1: k_gif_pack reads the word after the one a bit is in
constexpr int GIF_LANE_CAP = 32768;      // dictionaries in the workspace: 1 GiB at most; more chunks than that take turns
constexpr int GIF_FILE_HEAD = 13 + 19;   // header + logical screen descriptor; NETSCAPE2.0
constexpr int GIF_FRAME_HEAD = 8 + 10 + 768 + 1;               // graphic control extension, image descriptor, table, code size
constexpr unsigned GIF_EMPTY = 0xFFFFFFFFu;
static_assert(258 + GIF_CHUNK <= 4096 && GIF_CHUNK % 16 == 0, "a chunk never fills the dictionary and starts on a 16-byte boundary");

struct GifArgs {
  const void* src;
  unsigned char* idx;            // [F][px_stride]
  unsigned char* table;          // [F][768]
  unsigned* dict;                // [lanes][GIF_DICT]: (prefix << 8 | byte) << 12 | code
  unsigned* slots;               // [F][nchunks][GIF_SLOT_WORDS]
  unsigned* bitlen;              // [F][nchunks]
  unsigned long long* bitoff;    // [F][nchunks]: bits of the frame before the chunk
  unsigned long long* fpos;      // [F]: the frame's bytes (k_gif_frame_scan), then its place in out (k_gif_offsets)
  unsigned long long* dbytes;    // [F]: code bytes of the frame
  unsigned char* out;
  int64_t* offsets;              // [clips + 1]
  int clips, frames, H, W, delay, nchunks, lanes;
  long long npix, px_stride;
};

template <int KIND>
__device__ __forceinline__ unsigned gif_rgb(const GifArgs& a, long long f, long long p) {   // r << 16 | g << 8 | b
  // not through vf_frame_byte: a pixel is its index p here, never (y, x), and the three bytes of one share a base; the reader's
  // three separate indices cost k_gif_table 5 % (profiles/codec_host_isa_compare.txt).  The byte rule is the shared one.
  if (KIND == 1) {
    const unsigned char* s = (const unsigned char*)a.src + (f * a.npix + p) * 3;
    return ((unsigned)s[0] << 16) | ((unsigned)s[1] << 8) | s[2];
  }
  const float* s = (const float*)a.src + f * 3 * a.npix + p;
  return (vf_savepng_byte(s[0]) << 16) | (vf_savepng_byte(s[a.npix]) << 8) | vf_savepng_byte(s[2 * a.npix]);
}

__device__ __forceinline__ int gif_cell(unsigned rgb) { return (int)(((rgb >> 19) << 10) | (((rgb >> 11) & 31) << 5) | ((rgb >> 3) & 31)); }

// -------------------------------------------------------------------------------------------------------------- table
struct TableLds {                                 // all of k_gif_table's LDS: one block per CU
  unsigned cnt[GIF_CELLS];                        // pixels per cell; after the cut, the cell's box
  union {
    unsigned set[GIF_SET];                        // the frame's colours while they may be <= 256
    unsigned long long sum[256][3];               // channel sums of the boxes
  } u;
  unsigned pop[256], ncell[256];
  unsigned char box[256][6];                      // r0, r1, g0, g1, b0, b1, inclusive
  unsigned marg[32];
  int ext[2][6];                                  // extents of the two halves of a split (and of the frame: ext[0])
  unsigned hpop[2], hcell[2];
  unsigned ncol;
  int sel, axis, cut, nbox;
};
static_assert(sizeof(TableLds) <= 160 * 1024, "k_gif_table: the LDS of one CU");

// the occupied cells of box (lo/hi per axis) that thread tid of 1024 walks: f(cell, count, r, g, b)
template <class F>
__device__ __forceinline__ void gif_box_walk(const unsigned* cnt, const unsigned char* bx, F&& f) {
  const int er = bx[1] - bx[0] + 1, eg = bx[3] - bx[2] + 1, eb = bx[5] - bx[4] + 1;
  const int vol = er * eg * eb;
  for (int i = threadIdx.x; i < vol; i += 1024) {
    const int b = bx[4] + i % eb, g = bx[2] + (i / eb) % eg, r = bx[0] + i / (eb * eg);
    const int cell = (r << 10) | (g << 5) | b;
    const unsigned c = cnt[cell];
    if (c) f(cell, c, r, g, b);
  }
}

template <int KIND>
__global__ __launch_bounds__(1024) void k_gif_table(GifArgs a) {
  __shared__ TableLds s;
  const int tid = threadIdx.x;
  const long long f = (long long)blockIdx.y * a.frames + blockIdx.x;
  unsigned char* table = a.table + f * 768;

  // ---- histogram, occupied cells and their bounding box
  for (int i = tid; i < GIF_CELLS; i += 1024) s.cnt[i] = 0;
  if (tid < 6) s.ext[0][tid] = (tid & 1) ? -1 : 32;
  if (tid == 0) { s.hcell[0] = 0; s.ncol = 0; }
  __syncthreads();
  for (long long p = tid; p < a.npix; p += 1024) atomicAdd(&s.cnt[gif_cell(gif_rgb<KIND>(a, f, p))], 1u);
  __syncthreads();
  {
    int lo[3] = {32, 32, 32}, hi[3] = {-1, -1, -1};
    unsigned occ = 0;
    for (int cell = tid; cell < GIF_CELLS; cell += 1024) {
      if (!s.cnt[cell]) continue;
      const int c3[3] = {cell >> 10, (cell >> 5) & 31, cell & 31};
      ++occ;
#pragma unroll
      for (int x = 0; x < 3; ++x) { lo[x] = min(lo[x], c3[x]); hi[x] = max(hi[x], c3[x]); }
    }
    if (occ) {
      atomicAdd(&s.hcell[0], occ);
#pragma unroll
      for (int x = 0; x < 3; ++x) { atomicMin(&s.ext[0][2 * x], lo[x]); atomicMax(&s.ext[0][2 * x + 1], hi[x]); }
    }
  }
  for (int i = tid; i < GIF_SET; i += 1024) s.u.set[i] = GIF_EMPTY;
  __syncthreads();

  // ---- <= 256 colours?  They then lie in <= 256 cells.  A set of the 24-bit colours; every thread stops once 257 are in it.
  const unsigned occupied = s.hcell[0];
  if (occupied <= 256) {
    volatile unsigned* ncol = &s.ncol;
    for (long long p = tid; p < a.npix && *ncol <= 256; p += 1024) {
      const unsigned key = gif_rgb<KIND>(a, f, p);
      unsigned h = (key * 0x9E3779B1u) >> 21;
      for (;;) {
        const unsigned old = atomicCAS(&s.u.set[h], GIF_EMPTY, key);
        if (old == GIF_EMPTY) { atomicAdd(&s.ncol, 1u); break; }
        if (old == key) break;
        h = (h + 1) & (GIF_SET - 1);
      }
    }
    __syncthreads();
    if (s.ncol <= 256) {                          // the colours by rank, the rest zero
      const unsigned n = s.ncol;
      for (int i = tid; i < GIF_SET; i += 1024) {
        const unsigned key = s.u.set[i];
        if (key == GIF_EMPTY) continue;
        int r = 0;
        for (int j = 0; j < GIF_SET; ++j) r += s.u.set[j] < key;     // GIF_EMPTY is above every colour
        table[3 * r] = (unsigned char)(key >> 16); table[3 * r + 1] = (unsigned char)(key >> 8); table[3 * r + 2] = (unsigned char)key;
      }
      for (int i = 3 * (int)n + tid; i < 768; i += 1024) table[i] = 0;
      return;
    }
  }
  __syncthreads();

  // ---- median cut
  if (tid == 0) {
    for (int x = 0; x < 6; ++x) s.box[0][x] = (unsigned char)s.ext[0][x];
    s.pop[0] = (unsigned)a.npix;
    s.ncell[0] = occupied;
    s.nbox = 1;
  }
  __syncthreads();
  for (;;) {
    const int nbox = s.nbox;
    if (nbox >= 256) break;
    if (tid < 64) {                               // the box with the most pixels that can be split, the lowest number on a tie
      unsigned long long best = 0;
      for (int k = tid; k < nbox; k += 64)
        if (s.ncell[k] > 1) best = max(best, ((unsigned long long)s.pop[k] << 8) | (unsigned)(255 - k));
      for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o));
      if (tid == 0) {
        if (!best) s.sel = -1;
        else {
          const int k = 255 - (int)(best & 255);
          const unsigned char* bx = s.box[k];
          const int er = bx[1] - bx[0], eg = bx[3] - bx[2], eb = bx[5] - bx[4];
          s.sel = k;
          s.axis = (er >= eg && er >= eb) ? 0 : (eg >= eb ? 1 : 2);     // R, then G, then B on a tie
        }
      }
      if (tid < 32) s.marg[tid] = 0;
    }
    __syncthreads();
    const int k = s.sel;
    if (k < 0) break;
    const int axis = s.axis;
    const unsigned char* bx = s.box[k];
    gif_box_walk(s.cnt, bx, [&](int, unsigned c, int r, int g, int b) { atomicAdd(&s.marg[axis == 0 ? r : axis == 1 ? g : b], c); });
    __syncthreads();
    if (tid == 0) {
      const int lo = bx[2 * axis], hi = bx[2 * axis + 1];
      const unsigned long long pop = s.pop[k];
      unsigned long long cum = 0;
      int c = lo;
      for (; c < hi - 1; ++c) {
        cum += s.marg[c];
        if (2 * cum >= pop) break;
      }
      s.cut = c;                                  // the smallest c with 2 * (pixels at lo..c) >= pop, at most hi - 1
      for (int h = 0; h < 2; ++h) {
        for (int x = 0; x < 6; ++x) s.ext[h][x] = (x & 1) ? -1 : 32;
        s.hpop[h] = 0; s.hcell[h] = 0;
      }
    }
    __syncthreads();
    {
      const int cut = s.cut;
      int lo[2][3], hi[2][3];
      unsigned pp[2] = {0, 0}, nc[2] = {0, 0};
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int x = 0; x < 3; ++x) { lo[h][x] = 32; hi[h][x] = -1; }
      gif_box_walk(s.cnt, bx, [&](int, unsigned c, int r, int g, int b) {
        const int c3[3] = {r, g, b};
        const bool up = c3[axis] > cut;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if ((h == 1) != up) continue;
          pp[h] += c; ++nc[h];
#pragma unroll
          for (int x = 0; x < 3; ++x) { lo[h][x] = min(lo[h][x], c3[x]); hi[h][x] = max(hi[h][x], c3[x]); }
        }
      });
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (!nc[h]) continue;
        atomicAdd(&s.hpop[h], pp[h]);
        atomicAdd(&s.hcell[h], nc[h]);
#pragma unroll
        for (int x = 0; x < 3; ++x) { atomicMin(&s.ext[h][2 * x], lo[h][x]); atomicMax(&s.ext[h][2 * x + 1], hi[h][x]); }
      }
    }
    __syncthreads();
    if (tid < 2) {                                // the lower half keeps the number, the upper half takes the next free one
      const int dst = tid == 0 ? k : nbox;
      for (int x = 0; x < 6; ++x) s.box[dst][x] = (unsigned char)s.ext[tid][x];
      s.pop[dst] = s.hpop[tid];
      s.ncell[dst] = s.hcell[tid];
      if (tid == 1) s.nbox = nbox + 1;
    }
    __syncthreads();
  }

  // ---- the box of every occupied cell, then the channel sums of the boxes over the pixels
  const int nbox = s.nbox;
  for (int cell = tid; cell < GIF_CELLS; cell += 1024) {
    if (!s.cnt[cell]) continue;
    const int r = cell >> 10, g = (cell >> 5) & 31, b = cell & 31;
    int k = 0;
    for (; k < nbox - 1; ++k) {
      const unsigned char* bx = s.box[k];
      if (r >= bx[0] && r <= bx[1] && g >= bx[2] && g <= bx[3] && b >= bx[4] && b <= bx[5]) break;
    }
    s.cnt[cell] = (unsigned)k;
  }
  for (int i = tid; i < 768; i += 1024) s.u.sum[i / 3][i % 3] = 0;
  __syncthreads();
  {
    // a thread's pixels are 1024 apart (a wave reads neighbours); while they stay in one box (padding, masks, flat regions) they
    // are summed in registers and leave with one atomic per channel
    unsigned cur = GIF_EMPTY;
    unsigned long long sr = 0, sg = 0, sb = 0;
    const long long per = (a.npix + 1023) / 1024;
    for (long long i = 0; i < per; ++i) {
      const long long p = i * 1024 + tid;
      if (p >= a.npix) break;
      const unsigned rgb = gif_rgb<KIND>(a, f, p);
      const unsigned k = s.cnt[gif_cell(rgb)];
      if (k != cur) {
        if (cur != GIF_EMPTY) { atomicAdd(&s.u.sum[cur][0], sr); atomicAdd(&s.u.sum[cur][1], sg); atomicAdd(&s.u.sum[cur][2], sb); }
        cur = k; sr = sg = sb = 0;
      }
      sr += rgb >> 16; sg += (rgb >> 8) & 255; sb += rgb & 255;
    }
    if (cur != GIF_EMPTY) { atomicAdd(&s.u.sum[cur][0], sr); atomicAdd(&s.u.sum[cur][1], sg); atomicAdd(&s.u.sum[cur][2], sb); }
  }
  __syncthreads();
  for (int i = tid; i < 768; i += 1024) {
    const int k = i / 3;
    unsigned v = 0;
    if (k < nbox) {
      const unsigned long long n = s.pop[k];
      v = (unsigned)((2 * s.u.sum[k][i % 3] + n) / (2 * n));       // the mean, rounded to nearest
    }
    table[i] = (unsigned char)v;
  }
}

// ---------------------------------------------------------------------------------------------------------------- map
constexpr int MAP_PX = 4;                         // consecutive pixels of a thread: one that repeats its neighbour keeps the index

template <int KIND>
__global__ __launch_bounds__(256) void k_gif_map(GifArgs a) {
  __shared__ unsigned s_tab[256];
  const long long f = (long long)blockIdx.z * a.frames + blockIdx.y;
  const unsigned char* table = a.table + f * 768;
  s_tab[threadIdx.x] = ((unsigned)table[3 * threadIdx.x] << 16) | ((unsigned)table[3 * threadIdx.x + 1] << 8) | table[3 * threadIdx.x + 2];
  __syncthreads();
  const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * MAP_PX;
  unsigned char* dst = a.idx + f * a.px_stride;
  unsigned prev = GIF_EMPTY, best = 0;
  for (int j = 0; j < MAP_PX; ++j) {
    const long long p = p0 + j;
    if (p >= a.npix) break;
    const unsigned rgb = gif_rgb<KIND>(a, f, p);
    if (rgb != prev) {
      const int r = rgb >> 16, g = (rgb >> 8) & 255, b = rgb & 255;
      int bd = 0x7FFFFFFF;
#pragma unroll 8
      for (int k = 0; k < 256; ++k) {             // ascending and strict: the lowest index on a tie
        const unsigned t = s_tab[k];
        const int dr = r - (int)(t >> 16), dg = g - (int)((t >> 8) & 255), db = b - (int)(t & 255);
        const int d = dr * dr + dg * dg + db * db;
        if (d < bd) { bd = d; best = (unsigned)k; }
      }
      prev = rgb;
    }
    dst[p] = (unsigned char)best;
  }
}

// ---------------------------------------------------------------------------------------------------------------- LZW
__device__ __forceinline__ int gif_width(int m) { return max(9, 32 - __clz(256 + m)); }   // bits of the m-th code after a Clear

struct GifBits {                                  // serial LSB-first writer into a chunk's slot
  unsigned* w;
  unsigned long long acc;
  int nb;
  unsigned total;
  __device__ __forceinline__ void put(unsigned v, int n) {
    acc |= (unsigned long long)v << nb;
    nb += n;
    total += n;
    if (nb >= 32) { *w++ = (unsigned)acc; acc >>= 32; nb -= 32; }
  }
};

__global__ __launch_bounds__(64) void k_gif_lzw(GifArgs a) {
  const int lane = threadIdx.x;
  const long long frames_all = (long long)a.clips * a.frames, chunks_all = frames_all * a.nchunks;
  uint4* wave_dict = (uint4*)(a.dict + (size_t)blockIdx.x * 64 * GIF_DICT);
  unsigned* dict = a.dict + ((size_t)blockIdx.x * 64 + lane) * GIF_DICT;
  for (long long base = (long long)blockIdx.x * 64; base < chunks_all; base += a.lanes) {
    for (int i = lane; i < 64 * GIF_DICT / 4; i += 64) wave_dict[i] = make_uint4(GIF_EMPTY, GIF_EMPTY, GIF_EMPTY, GIF_EMPTY);
    __syncthreads();                              // the wave's 64 dictionaries are empty before any lane looks into its own
    const long long ch = base + lane;
    if (ch < chunks_all) {
      const long long f = ch / a.nchunks;
      const int k = (int)(ch - f * a.nchunks);
      const long long start = (long long)k * GIF_CHUNK;
      const int n = (int)min((long long)GIF_CHUNK, a.npix - start);
      const unsigned* px = (const unsigned*)(a.idx + f * a.px_stride + start);   // px_stride and GIF_CHUNK are multiples of 16
      GifBits bw{a.slots + (size_t)ch * GIF_SLOT_WORDS, 0ull, 0, 0u};
      if (k == 0) bw.put(256u, 9);
      unsigned word = px[0];
      unsigned prefix = word & 255;
      unsigned next = 258;
      int m = 0;
      for (int i = 1; i < n; ++i) {
        if ((i & 3) == 0) word = px[i >> 2];
        const unsigned b = (word >> (8 * (i & 3))) & 255;
        const unsigned key = (prefix << 8) | b;
        unsigned h = (key * 0x9E3779B1u) >> 19;
        unsigned e;
        while ((e = dict[h]) != GIF_EMPTY && (e >> 12) != key) h = (h + 1) & (GIF_DICT - 1);
        if (e != GIF_EMPTY) { prefix = e & 4095; continue; }
        bw.put(prefix, gif_width(++m));
        dict[h] = (key << 12) | next++;
        prefix = b;
      }
      bw.put(prefix, gif_width(++m));
      bw.put(k == a.nchunks - 1 ? 257u : 256u, gif_width(m + 1));   // EOI, or the next chunk's Clear at the width the decoder is at
      if (bw.nb) *bw.w = (unsigned)bw.acc;
      a.bitlen[ch] = bw.total;
    }
    __syncthreads();
  }
}

// --------------------------------------------------------------------------------------------------------------- pack
// one block per frame: the bits before every chunk, the frame's code bytes and its size in the file
__global__ __launch_bounds__(256) void k_gif_frame_scan(GifArgs a) {
  __shared__ unsigned long long s_w[4];
  const long long f = (long long)blockIdx.y * a.frames + blockIdx.x;
  const unsigned* len = a.bitlen + f * a.nchunks;
  unsigned long long run = 0;
  for (int base = 0; base < a.nchunks; base += 256) {
    const int k = base + threadIdx.x;
    unsigned long long total;
    const unsigned long long e = vf_block_excl_scan<unsigned long long, 256>(k < a.nchunks ? len[k] : 0u, s_w, total);
    if (k < a.nchunks) a.bitoff[f * a.nchunks + k] = run + e;
    run += total;
  }
  if (threadIdx.x == 0) {
    const unsigned long long d = (run + 7) >> 3;
    a.dbytes[f] = d;
    a.fpos[f] = GIF_FRAME_HEAD + d + (d + 254) / 255 + 1;          // + the sub-blocks' length bytes and the terminator
  }
}

// one block: fpos[f] becomes the place of frame f in out, offsets[c] the place of file c.  k_vf_file_offsets (vf_block.h) is the
// plain case, one frame per file and no header term; this one also places every frame inside its file.
__global__ __launch_bounds__(256) void k_gif_offsets(GifArgs a) {
  __shared__ unsigned long long s_w[4];
  const long long frames_all = (long long)a.clips * a.frames;
  unsigned long long run = 0;
  for (long long base = 0; base < frames_all; base += 256) {
    const long long f = base + threadIdx.x;
    unsigned long long total;
    const unsigned long long e = vf_block_excl_scan<unsigned long long, 256>(f < frames_all ? a.fpos[f] : 0ull, s_w, total);
    if (f < frames_all) {
      const long long c = f / a.frames;
      const unsigned long long file = run + e + (unsigned long long)c * (GIF_FILE_HEAD + 1);   // earlier files' headers and trailers
      a.fpos[f] = file + GIF_FILE_HEAD;
      if (f == c * a.frames) a.offsets[c] = (int64_t)file;
    }
    run += total;
  }
  if (threadIdx.x == 0) a.offsets[a.clips] = (int64_t)(run + (unsigned long long)a.clips * (GIF_FILE_HEAD + 1));
}

__device__ __forceinline__ unsigned gif_slot_bits(const unsigned* slot, unsigned q, int n) {   // n <= 8 bits from bit q
  const unsigned w = q >> 5, o = q & 31;
  const unsigned long long v = slot[w] | ((unsigned long long)slot[w + 1] << 32);
  return (unsigned)(v >> o) & ((1u << n) - 1);
}

__global__ __launch_bounds__(256) void k_gif_pack(GifArgs a) {
  const int fi = blockIdx.y;
  const long long f = (long long)blockIdx.z * a.frames + fi;
  const unsigned long long D = a.dbytes[f];
  unsigned char* fr = a.out + a.fpos[f];
  unsigned char* data = fr + GIF_FRAME_HEAD;
  const unsigned long long* off = a.bitoff + f * a.nchunks;
  const unsigned* len = a.bitlen + f * a.nchunks;
  const unsigned* slots = a.slots + (size_t)f * a.nchunks * GIF_SLOT_WORDS;
  for (unsigned long long j = (unsigned long long)blockIdx.x * 256 + threadIdx.x; j < D; j += (unsigned long long)gridDim.x * 256) {
    const unsigned long long p = 8 * j;
    int lo = 0, hi = a.nchunks - 1;               // the last chunk that starts at or before bit p
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    const unsigned q = (unsigned)(p - off[lo]);
    const int avail = (int)min(8u, len[lo] - q);
    unsigned v = gif_slot_bits(slots + (size_t)lo * GIF_SLOT_WORDS, q, avail);
    if (avail < 8 && lo + 1 < a.nchunks)          // a chunk holds 18 bits at least: a byte takes from two at most
      v |= gif_slot_bits(slots + (size_t)(lo + 1) * GIF_SLOT_WORDS, 0, 8 - avail) << avail;
    const unsigned long long at = j + j / 255 + 1;
    data[at] = (unsigned char)v;
    if (j % 255 == 0) data[at - 1] = (unsigned char)min(255ull, D - j);
  }
  if (blockIdx.x != 0) return;
  const int t = threadIdx.x;
  for (int i = t; i < 768; i += 256) fr[18 + i] = a.table[f * 768 + i];
  if (t == 0) {
    const unsigned char head[18] = {0x21, 0xF9, 0x04, 0x00, (unsigned char)(a.delay & 255), (unsigned char)(a.delay >> 8), 0x00, 0x00,
                                    0x2C, 0, 0, 0, 0, (unsigned char)(a.W & 255), (unsigned char)(a.W >> 8), (unsigned char)(a.H & 255),
                                    (unsigned char)(a.H >> 8), 0x87};
    for (int i = 0; i < 18; ++i) fr[i] = head[i];
    fr[18 + 768] = 0x08;
    data[D + (D + 254) / 255] = 0x00;
  }
  if (t == 64 && fi == 0) {
    unsigned char* file = fr - GIF_FILE_HEAD;
    const unsigned char head[GIF_FILE_HEAD] = {'G', 'I', 'F', '8', '9', 'a', (unsigned char)(a.W & 255), (unsigned char)(a.W >> 8),
                                               (unsigned char)(a.H & 255), (unsigned char)(a.H >> 8), 0x70, 0x00, 0x00,
                                               0x21, 0xFF, 0x0B, 'N', 'E', 'T', 'S', 'C', 'A', 'P', 'E', '2', '.', '0', 0x03, 0x01, 0x00, 0x00, 0x00};
    for (int i = 0; i < GIF_FILE_HEAD; ++i) file[i] = head[i];
  }
  if (t == 128 && fi == a.frames - 1) data[D + (D + 254) / 255 + 1] = 0x3B;
}

struct GifPlan {
  long long npix, px_stride, nchunks, frames_all, chunks_all, lanes;
  size_t o_idx, o_table, o_dict, o_slots, o_len, o_off, o_fpos, o_dbytes, ws_bytes, out_bytes;
};

int gif_plan(const char* who, int clips, int frames, int H, int W, GifPlan* p) {
  VF_REQUIRE(H >= 1 && W >= 1 && H <= GIF_MAX_SIDE && W <= GIF_MAX_SIDE, "%s: a %dx%d frame (sides are 1 to %d)", who, H, W, GIF_MAX_SIDE);
  VF_REQUIRE(frames >= 1 && frames <= GIF_MAX_FRAMES, "%s: a clip of %d frames (1 to %d)", who, frames, GIF_MAX_FRAMES);
  VF_REQUIRE(clips >= 1 && clips <= GIF_MAX_CLIPS, "%s: a batch of %d clips (1 to %d)", who, clips, GIF_MAX_CLIPS);
  p->npix = (long long)H * W;
  p->px_stride = (p->npix + 15) & ~15ll;
  p->nchunks = vf_cdiv(p->npix, GIF_CHUNK);
  p->frames_all = (long long)clips * frames;
  VF_REQUIRE(p->frames_all * p->npix <= (1ll << 38), "%s: a batch of %d clips of %d frames of %dx%d (2^38 pixels at most in one call)", who,
             clips, frames, H, W);
  p->chunks_all = p->frames_all * p->nchunks;
  p->lanes = (p->chunks_all < GIF_LANE_CAP ? p->chunks_all + 63 : GIF_LANE_CAP) / 64 * 64;
  VfCarve ws;
  p->o_idx = ws.take((size_t)p->frames_all * p->px_stride);
  p->o_table = ws.take((size_t)p->frames_all * 768);
  p->o_dict = ws.take((size_t)p->lanes * GIF_DICT * 4);
  p->o_slots = ws.take((size_t)p->chunks_all * GIF_SLOT_WORDS * 4);
  p->o_len = ws.take((size_t)p->chunks_all * 4);
  p->o_off = ws.take((size_t)p->chunks_all * 8);
  p->o_fpos = ws.take((size_t)p->frames_all * 8);
  p->o_dbytes = ws.take((size_t)p->frames_all * 8);
  p->ws_bytes = ws.at;
  // every pixel a 12-bit code of its own, a 12-bit Clear or EOI behind every chunk, the leading Clear
  const size_t d = ((size_t)p->npix * 12 + (size_t)p->nchunks * 12 + 9 + 7) / 8;
  p->out_bytes = (size_t)clips * (GIF_FILE_HEAD + 1 + (size_t)frames * (GIF_FRAME_HEAD + d + (d + 254) / 255 + 1));
  return 0;
}

}  // namespace

VF_API int vf_gif_workspace_bytes(int clips, int frames, int H, int W, size_t* ws_bytes, size_t* out_bytes) {
  GifPlan p;
  if (int e = gif_plan("vf_gif_workspace_bytes", clips, frames, H, W, &p)) return e;
  if (ws_bytes) *ws_bytes = p.ws_bytes;
  if (out_bytes) *out_bytes = p.out_bytes;
  return 0;
}

VF_API int vf_gif_encode(vf_ctx* ctx, const void* src, int kind, int clips, int frames, int H, int W, int delay_cs, void* ws,
                         size_t ws_bytes, unsigned char* out, size_t out_cap, int64_t* offsets) {
  GifPlan p;
  if (int e = gif_plan("vf_gif_encode", clips, frames, H, W, &p)) return e;
  VF_REQUIRE(delay_cs >= 0 && delay_cs <= GIF_MAX_DELAY, "vf_gif_encode: a delay of %d centiseconds (0 to %d)", delay_cs, GIF_MAX_DELAY);
  char batch[64];
  snprintf(batch, sizeof(batch), "%d clips of %d frames of %dx%d", clips, frames, H, W);
  if (int e = vf_check_encode_entry("vf_gif_encode", kind, "3", batch, ws_bytes, p.ws_bytes, out_cap, p.out_bytes)) return e;
  GifArgs a;
  char* w = (char*)ws;
  a.src = src;
  a.idx = (unsigned char*)(w + p.o_idx);
  a.table = (unsigned char*)(w + p.o_table);
  a.dict = (unsigned*)(w + p.o_dict);
  a.slots = (unsigned*)(w + p.o_slots);
  a.bitlen = (unsigned*)(w + p.o_len);
  a.bitoff = (unsigned long long*)(w + p.o_off);
  a.fpos = (unsigned long long*)(w + p.o_fpos);
  a.dbytes = (unsigned long long*)(w + p.o_dbytes);
  a.out = out;
  a.offsets = offsets;
  a.clips = clips; a.frames = frames; a.H = H; a.W = W; a.delay = delay_cs;
  a.nchunks = (int)p.nchunks; a.lanes = (int)p.lanes;
  a.npix = p.npix; a.px_stride = p.px_stride;
  const double px = (double)p.frames_all * p.npix, in_b = kind == 0 ? 12.0 : 3.0;
  const dim3 per_frame(frames, clips);
  const dim3 map_grid((unsigned)vf_cdiv(p.npix, 256 * MAP_PX), frames, clips);
  if (kind == 0) {
    VF_LAUNCH_TIMED(ctx, "gif_table", 0.0, 2.0 * in_b * px, k_gif_table<0>, per_frame, dim3(1024), a);
    VF_LAUNCH_CHECK();
    VF_LAUNCH_TIMED(ctx, "gif_map", 0.0, (in_b + 1.0) * px, k_gif_map<0>, map_grid, dim3(256), a);
  } else {
    VF_LAUNCH_TIMED(ctx, "gif_table", 0.0, 2.0 * in_b * px, k_gif_table<1>, per_frame, dim3(1024), a);
    VF_LAUNCH_CHECK();
    VF_LAUNCH_TIMED(ctx, "gif_map", 0.0, (in_b + 1.0) * px, k_gif_map<1>, map_grid, dim3(256), a);
  }
  VF_LAUNCH_CHECK();
  VF_LAUNCH_TIMED(ctx, "gif_lzw", 0.0, 3.0 * px, k_gif_lzw, dim3((unsigned)(p.lanes / 64)), dim3(64), a);
  VF_LAUNCH_CHECK();
  {
    VfProf prof(ctx, "gif_pack", 0.0, 3.0 * px);
    hipLaunchKernelGGL(k_gif_frame_scan, per_frame, dim3(256), 0, ctx->stream, a);
    VF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_gif_offsets, dim3(1), dim3(256), 0, ctx->stream, a);
    VF_LAUNCH_CHECK();
    const long long dmax = (p.npix * 12 + p.nchunks * 12 + 9 + 7) / 8;
    const unsigned xb = (unsigned)(vf_cdiv(dmax, 256) < 4096 ? vf_cdiv(dmax, 256) : 4096);
    hipLaunchKernelGGL(k_gif_pack, dim3(xb, frames, clips), dim3(256), 0, ctx->stream, a);
    VF_LAUNCH_CHECK();
  }
  return 0;
}
