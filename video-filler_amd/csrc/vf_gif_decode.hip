// vf_gif_decode.hip — batched animated-GIF decode on the device: LZW, interlace, compositing.
//   * vf_gif_inspect (host only): the walk of one GIF87a / GIF89a file, its frames, supported or why not;
//   * vf_gif_decode_workspace_bytes: device workspace and host staging sizes of one batch;
//   * vf_gif_decode: n files -> n uint8 N_i x H_i x W_i x (3 | 4) stacks of composited frames at caller-given offsets.
// Pipeline (two launches, whatever n and the frame counts): the host walks every file (vf_gif_parse.h), puts each frame's
// sub-blocks behind one another and packs them with one colour table and one descriptor per frame into one staging buffer
// -> one upload.  Then
//   k_gifd_lzw      one 256-thread block per frame.  When a code is read, the string it adds to the dictionary is the
//                   previous code's output plus one byte — which is the first byte of what this code puts out right behind
//                   it.  So an entry is a place in the frame's OWN output and a length, a non-root code is a copy from an
//                   earlier place (KwKwK: the copy that overlaps its own first byte), and the rest is k_pngd_inflate's
//                   scheme: thread 0 turns codes into (source, length) tokens, all threads resolve a batch of them (pointer
//                   doubling for sources inside it) and store it;
//   k_gifd_compose  one thread per canvas pixel of a file: the frames in order, the RGBA canvas value and the disposal-3
//                   copy in registers; rectangle test, interlace row, index, transparency, table, store, disposal.
// Everything is integer arithmetic.  A corrupt stream ends in the file's status word: every read of the code bytes is
// bounded by the stream's length, every store by the rectangle's size.
#include <algorithm>
#include <string>
#include <vector>

#include "vf_block.h"
#include "vf_common.h"
#include "vf_gif_parse.h"

namespace {

constexpr int kLzwThreads = 256;
constexpr int kDict = 4096;                          // codes are 12 bits at most
constexpr int kCap = 8192;                           // indices per token batch (uint16 places, two blocks per CU)
constexpr int kMaxStr = 4096;                        // no string is longer: an entry is one index longer than an older one
constexpr int kTok = 1984;                           // tokens per batch (what two blocks per CU leave room for)
constexpr int kWin = 4096;                           // code bytes held in LDS: kTok codes of 12 bits and slack
constexpr int kWinSlack = 16;
constexpr int kRounds = 13;                          // ceil(log2 kCap): pointer-doubling rounds at most
constexpr uint32_t kLit = 0x80000000u;               // a token that is one root index
static_assert((1 << kRounds) >= kCap, "a chain inside a batch has fewer than kCap links");
static_assert(kTok * 12 / 8 + kWinSlack + 8 <= kWin, "a batch's codes fit the window");
static_assert(kCap >= 2 * kMaxStr, "a batch takes at least one string after the room check");

#define VF_HD __device__ __forceinline__

struct GifdCtl {
  uint32_t bp;                 // bit position of the reader in the stream
  uint32_t nbits;              // 8 * slen
  uint32_t wbase;              // byte position of the window's first byte (a multiple of 4)
  int32_t next;                // the next free code
  int32_t width;               // bits of the next code
  int32_t prev_pos, prev_len;  // where the previous code's string stands in the output; length 0: there is none (after a Clear)
  int32_t out_pos;             // indices written before this batch
  int32_t nout, ntok;          // this batch
  int32_t done, status;
};

struct LzwLds {
  uint32_t win[kWin / 4 + 4];
  uint32_t dpos[kDict];        // entry: first index of the string in the frame's output ...
  uint16_t dlen[kDict];        // ... and its length
  uint16_t idx[2][kCap];       // per index of the batch: itself (value known) or the earlier one of the batch it copies
  uint8_t val[kCap];
  uint16_t tok_off[kTok + 1];  // first index of each token in the batch
  uint32_t tok_src[kTok];      // kLit | root, or the source's place in the frame's output
  GifdCtl c;
};
// 256 bytes of slack: __syncthreads_or takes LDS of its own
static_assert(2 * (sizeof(LzwLds) + 256) <= 160 * 1024, "k_gifd_lzw: two blocks per CU (160 KiB of LDS)");

struct GifdBatch {
  const gifd::File* files;
  const gifd::Frame* frames;
  const uint32_t* tables;      // 256 words (r | g << 8 | b << 16) per frame
  const uint8_t* streams;
  uint8_t* idx;
  uint8_t* out;
  int32_t* status;
};

// 32 bits of the stream starting at bit bp, least significant first (the window holds bytes [wbase, wbase + kWin + 16),
// zeros past the stream's end)
VF_HD uint32_t gifd_peek(const LzwLds& L, uint32_t bp) {
  const uint32_t o = (bp >> 3) - L.c.wbase;
  const uint32_t d = o >> 2, sh = (o & 3) * 8 + (bp & 7);
  return (uint32_t)((((uint64_t)L.win[d + 1] << 32) | L.win[d]) >> sh);
}

// thread 0: codes into tokens until the token buffer, the batch's room or the window is used up, the rectangle is full or
// the stream fails.  Every iteration consumes one code or ends the loop.
VF_HD void gifd_tokens(LzwLds& L, int mincode, int npix) {
  GifdCtl& c = L.c;
  const int clear = 1 << mincode, eoi = clear + 1;
  uint32_t bp = c.bp;
  int ntok = 0, nout = 0, next = c.next, width = c.width, prev_pos = c.prev_pos, prev_len = c.prev_len;
  int status = 0, done = 0;
  const uint32_t stop = 8u * (c.wbase + kWin - kWinSlack);
  while (ntok < kTok && nout + kMaxStr <= kCap && bp <= stop) {
    if (bp + (uint32_t)width > c.nbits) {
      status = VF_GIF_SHORT_DATA;
      break;
    }
    const int code = (int)(gifd_peek(L, bp) & ((1u << width) - 1));
    bp += (uint32_t)width;
    if (code == clear) {
      next = eoi + 1;
      width = mincode + 1;
      prev_len = 0;
      continue;
    }
    if (code == eoi) {
      status = VF_GIF_SHORT_DATA;                              // the rectangle is not full, or the loop had ended
      break;
    }
    uint32_t src;
    int len;
    if (prev_len == 0) {
      if (code > eoi) {
        status = VF_GIF_BAD_CODE;
        break;
      }
      src = kLit | (uint32_t)code;
      len = 1;
    } else {
      if (code > next) {                                       // next <= 4096 and code <= 4095: a full dictionary passes
        status = VF_GIF_BAD_CODE;
        break;
      }
      if (next < kDict) {
        L.dpos[next] = (uint32_t)prev_pos;
        L.dlen[next] = (uint16_t)(prev_len + 1);
        ++next;
        if (next == (1 << width) && width < 12) ++width;
      }
      if (code < clear) {
        src = kLit | (uint32_t)code;
        len = 1;
      } else {
        src = L.dpos[code];                                    // eoi < code < next: written since the last Clear
        len = L.dlen[code];
      }
    }
    const int start = c.out_pos + nout;
    prev_pos = start;
    prev_len = len;
    if (start + len >= npix) {
      len = npix - start;
      done = 1;
    }
    L.tok_off[ntok] = (uint16_t)nout;
    L.tok_src[ntok] = src;
    ++ntok;
    nout += len;
    if (done) break;
  }
  L.tok_off[ntok] = (uint16_t)nout;
  c.bp = bp;
  c.next = next;
  c.width = width;
  c.prev_pos = prev_pos;
  c.prev_len = prev_len;
  c.ntok = ntok;
  c.nout = nout;
  c.done = done;
  c.status = status;
}

// every thread: the batch's indices that are known at once (roots, copies from before the batch) and, for the others, the
// earlier index of the batch they repeat.  prev: the frame's indices written so far
VF_HD void gifd_resolve_init(LzwLds& L, const uint8_t* prev, int t, int nt) {
  const GifdCtl& c = L.c;
  for (int p = t; p < c.nout; p += nt) {
    int lo = 0, hi = c.ntok - 1;                               // the last token that starts at or before p
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (L.tok_off[mid] <= p) lo = mid;
      else hi = mid - 1;
    }
    const uint32_t v = L.tok_src[lo];
    int from = p;
    if (v & kLit) {
      L.val[p] = (uint8_t)v;
    } else {
      // an entry stands before the token that uses it: q < out_pos + tok_off[lo] + (p - tok_off[lo]) = out_pos + p
      const int q = (int)v + (p - (int)L.tok_off[lo]);
      if (q < c.out_pos) L.val[p] = prev[q];
      else from = q - c.out_pos;
    }
    L.idx[0][p] = (uint16_t)from;
  }
}

// every thread: one pointer-doubling round from idx[k] into idx[1 - k]; whether anything moved
VF_HD int gifd_double(LzwLds& L, int k, int t, int nt) {
  int moved = 0;
  for (int p = t; p < L.c.nout; p += nt) {
    const uint16_t a = L.idx[k][p], b = L.idx[k][a];
    L.idx[1 - k][p] = b;
    moved |= a != b;
  }
  return moved;
}

// one block per frame
__global__ __launch_bounds__(kLzwThreads) void k_gifd_lzw(const GifdBatch B) {
  __shared__ LzwLds L;
  const int t = threadIdx.x;
  const gifd::Frame& fr = B.frames[blockIdx.x];
  const uint32_t* src32 = (const uint32_t*)(B.streams + fr.src);
  const uint32_t ndw = ((uint32_t)fr.slen + 3) >> 2;
  uint8_t* dst = B.idx + fr.idx_off;
  const int npix = fr.npix, mincode = fr.mincode;
  if (t == 0) {
    GifdCtl& c = L.c;
    c.bp = 0;
    c.nbits = 8u * (uint32_t)fr.slen;
    c.wbase = 0;
    c.next = (1 << mincode) + 2;                               // a stream without a leading Clear starts as behind one
    c.width = mincode + 1;
    c.prev_pos = c.prev_len = 0;
    c.out_pos = c.nout = c.ntok = 0;
    c.done = c.status = 0;
  }
  __syncthreads();
  // every batch consumes at least one code of 3 bits or more, or ends the loop
  const uint32_t max_batches = 8u * (uint32_t)fr.slen / 3u + 4u;
  for (uint32_t it = 0; it < max_batches; ++it) {
    if (t == 0) L.c.wbase = (L.c.bp >> 3) & ~3u;
    __syncthreads();
    const uint32_t g0 = L.c.wbase >> 2;
    for (int i = t; i < kWin / 4 + 4; i += kLzwThreads) L.win[i] = g0 + (uint32_t)i < ndw ? src32[g0 + i] : 0u;
    __syncthreads();
    if (t == 0) gifd_tokens(L, mincode, npix);
    __syncthreads();
    if (L.c.ntok > 0) {
      gifd_resolve_init(L, dst, t, kLzwThreads);
      __syncthreads();
      int k = 0;
      for (int r = 0; r < kRounds; ++r) {
        const int moved = gifd_double(L, k, t, kLzwThreads);
        k = 1 - k;
        if (!__syncthreads_or(moved)) break;
      }
      const int out_pos = L.c.out_pos;
      for (int p = t; p < L.c.nout; p += kLzwThreads) {        // out_pos + nout <= npix: gifd_tokens cut the last string
        const int r = L.idx[k][p];
        dst[out_pos + p] = L.val[r];                           // a root's value was written by gifd_resolve_init alone
      }
    }
    __syncthreads();                                           // the batch is in memory before a later one copies from it
    const bool stop = L.c.status || L.c.done;
    __syncthreads();                                           // every thread has read the batch's end before thread 0 goes on
    if (stop) break;
    if (t == 0) L.c.out_pos += L.c.nout;
  }
  if (t == 0) {
    int st = L.c.status;
    if (!st && !L.c.done) st = VF_GIF_SHORT_DATA;              // the batch bound ran out: cannot happen, and is no fault
    if (st) atomicMax(B.status + fr.file, st);                 // a maximum: the same word in any order
  }
}

// the place in the stream's row order of display row r of an interlaced frame of h rows
VF_HD int gifd_lace_row(int r, int h) {
  const int n1 = (h + 7) >> 3, n2 = (h + 3) >> 3, n3 = (h + 1) >> 2;
  if ((r & 7) == 0) return r >> 3;
  if ((r & 7) == 4) return n1 + (r >> 3);
  if ((r & 3) == 2) return n1 + n2 + (r >> 2);
  return n1 + n2 + n3 + (r >> 1);
}

// one thread per canvas pixel of a file; blockIdx.y: the file.  Frame descriptors are the same for every lane.
__global__ __launch_bounds__(256) void k_gifd_compose(const GifdBatch B) {
  const gifd::File& fl = B.files[blockIdx.y];
  if (B.status[blockIdx.y] != 0 && B.status[blockIdx.y] != VF_GIF_BAD_INDEX) return;   // a frame's indices are not all there
  const int W = fl.W, H = fl.H, oc = fl.oc, nf = fl.nframes;
  const int64_t npix = (int64_t)W * H;
  uint8_t* out = B.out + fl.out_off;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / W), x = (int)(i % W);
    uint32_t canvas = 0, saved = 0;                            // r | g << 8 | b << 16 | a << 24
    bool bad = false;
    for (int k = 0; k < nf; ++k) {
      const gifd::Frame& fr = B.frames[fl.first + k];
      if (fr.disposal == 3) saved = canvas;
      const int rx = x - fr.x, ry = y - fr.y;
      const bool inside = rx >= 0 && rx < fr.w && ry >= 0 && ry < fr.h;
      if (inside) {
        const int row = fr.interlace ? gifd_lace_row(ry, fr.h) : ry;
        const int ix = B.idx[fr.idx_off + (int64_t)row * fr.w + rx];
        if (ix != fr.trans) {
          if (ix >= fr.tsize) bad = true;
          else canvas = B.tables[(int64_t)fr.table * 256 + ix] | 0xff000000u;
        }
      }
      uint8_t* o = out + ((int64_t)k * npix + i) * oc;
      o[0] = (uint8_t)canvas;
      o[1] = (uint8_t)(canvas >> 8);
      o[2] = (uint8_t)(canvas >> 16);
      if (oc == 4) o[3] = (uint8_t)(canvas >> 24);
      if (fr.disposal == 2 && inside) canvas = 0;
      else if (fr.disposal == 3) canvas = saved;
    }
    if (bad) atomicMax(B.status + blockIdx.y, (int)VF_GIF_BAD_INDEX);
  }
}

int gifd_plan(const char* who, const unsigned char* data, const int64_t* offs, int n, int alpha, gifd::Plan& L) {
  std::string msg;
  const int rc = gifd::plan(data, offs, n, alpha, L, msg);
  if (rc) vf_set_error("%s: %s", who, msg.c_str());
  return rc;
}

}  // namespace

VF_API int vf_gif_inspect(const unsigned char* data, size_t len, int64_t* info, int64_t* frames, int frame_cap, char* reason,
                          int reason_cap) {
  VF_REQUIRE(data && info && frame_cap >= 0, "vf_gif_inspect: NULL argument or negative frame_cap");
  gifd::Parsed P;
  std::string msg;
  const int rc = gifd::parse(data, (int64_t)len, P, msg);
  if (rc) {
    vf_set_error("vf_gif_inspect: %s", msg.c_str());
    return rc;
  }
  info[0] = P.W;
  info[1] = P.H;
  info[2] = (int64_t)P.frames.size();
  info[3] = P.loop;
  info[4] = P.supported ? 1 : 0;
  info[5] = P.gsize;
  info[6] = P.version;
  info[7] = P.rect_pix;
  if (frames) {
    const size_t rows = std::min(P.frames.size(), (size_t)frame_cap);
    for (size_t k = 0; k < rows; ++k) {
      const gifd::ParsedFrame& f = P.frames[k];
      int64_t* r = frames + 12 * k;
      r[0] = f.delay;
      r[1] = f.disposal;
      r[2] = f.x;
      r[3] = f.y;
      r[4] = f.w;
      r[5] = f.h;
      r[6] = f.interlace;
      r[7] = f.trans;
      r[8] = f.tsize;
      r[9] = f.local;
      r[10] = f.mincode;
      r[11] = f.data_bytes;
    }
  }
  if (reason && reason_cap > 0) snprintf(reason, (size_t)reason_cap, "%s", P.why.c_str());
  return 0;
}

VF_API int vf_gif_decode_workspace_bytes(const unsigned char* data, const int64_t* offs, int n, int alpha, size_t* ws_bytes,
                                         size_t* stage_bytes) {
  gifd::Plan L;
  if (int e = gifd_plan("vf_gif_decode_workspace_bytes", data, offs, n, alpha, L)) return e;
  if (ws_bytes) *ws_bytes = L.ws;
  if (stage_bytes) *stage_bytes = L.stage;
  return 0;
}

VF_API int vf_gif_decode(vf_ctx* ctx, const unsigned char* data, const int64_t* offs, int n, int alpha, const int64_t* out_offs,
                         unsigned char* out, void* stage, size_t stage_bytes, void* ws, size_t ws_bytes, int32_t* status) {
  VF_REQUIRE(out && out_offs && stage && ws && status, "vf_gif_decode: NULL argument");
  gifd::Plan L;
  if (int e = gifd_plan("vf_gif_decode", data, offs, n, alpha, L)) return e;
  VF_REQUIRE(stage_bytes >= L.stage && ws_bytes >= L.ws, "vf_gif_decode: staging %zu / workspace %zu bytes, need %zu / %zu", stage_bytes,
             ws_bytes, L.stage, L.ws);
  gifd::pack(data, offs, n, alpha, out_offs, L, (uint8_t*)stage);
  uint8_t* w = (uint8_t*)ws;
  GifdBatch B;
  B.files = (const gifd::File*)(w + L.o_files);
  B.frames = (const gifd::Frame*)(w + L.o_frames);
  B.tables = (const uint32_t*)(w + L.o_tables);
  B.streams = w + L.o_streams;
  B.idx = w + L.o_idx;
  B.out = out;
  B.status = status;
  hipStream_t st = ctx->stream;
  {
    VfRange r("gifd_upload");
    VF_CHECK_HIP(hipMemcpyAsync(w, stage, L.stage, hipMemcpyHostToDevice, st));
    VF_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t) * n, st));
  }
  VF_LAUNCH_TIMED(ctx, "gifd_lzw", 0.0, (double)L.stream_bytes + (double)L.idx_bytes, k_gifd_lzw, dim3((unsigned)L.nframes),
                  dim3(kLzwThreads), B);
  VF_LAUNCH_CHECK();
  const unsigned gp = (unsigned)std::min<int64_t>(std::max<int64_t>(1, vf_cdiv(L.max_pix, 256)), 4096);
  VF_LAUNCH_TIMED(ctx, "gifd_compose", 0.0, (double)L.idx_bytes + (double)L.out_bytes, k_gifd_compose, dim3(gp, n), dim3(256), B);
  VF_LAUNCH_CHECK();
  return 0;
}
