// vf_png_decode.hip — batched PNG decode on the device: inflate, unfilter, expand.
// One pipeline, two rules (PngRule) for which files it takes, how its messages begin and what its launches are called:
//   default  vf_png_inspect (host only: chunks, IHDR, PLTE / tRNS, the zlib header, supported or why not),
//            vf_png_decode_workspace_bytes (device workspace and host staging sizes of one batch), vf_png_decode (N files ->
//            N uint8 H x W x C images at caller-given offsets of one buffer): files of 8 bits or fewer without interlace;
//   full     vf_png_inspect_full, vf_png_decode_full_workspace_bytes, vf_png_decode_full: Adam7-interlaced and 16-bit files
//            too, written as uint8 or float32.
// An image is up to seven passes, each a sub-image with its own rows; a file without interlace is the one-pass case (pass 1
// = the image), and the default rule's files are that case at 8 bits or fewer, written as uint8.
// Pipeline (three launches, whatever N): the host walks the chunks, checks the CRCs, concatenates every file's IDAT
// payloads behind one another (minus the two zlib header bytes) and packs them with PLTE / tRNS and one descriptor per
// image (PngdImage: the file, then its passes' sizes and places) into one staging buffer -> one upload.  Then
//   k_pngd_inflate   one 256-thread block per image: deflate blocks in stream order.  Thread 0 reads the block header,
//                    all threads fill the lookup tables, thread 0 decodes symbols into a token batch in LDS, all threads
//                    resolve the batch (pointer doubling for sources inside it), store it and add it to the Adler-32; the
//                    expected size is sum h_p * (1 + rb_p);
//   k_pngd_unfilter  one wave per (image, pass): a band of 64 rows of the pass's h_p x rb_p at a time, row r one filter
//                    unit behind row r - 1, so that every filter sees its left, upper and upper-left neighbours
//                    reconstructed; a unit of up to 8 bytes (16-bit RGBA) in a 64-bit register when it is above 4;
//   k_pngd_expand    one thread per output pixel: its pass from (x & 7, y & 7), its place inside the pass; sub-byte samples,
//                    16-bit samples big-endian, palette and tRNS, alpha drop, grey replication; uint8 (a 16-bit sample's
//                    high byte) or float32 (byte / 255, sample / 65535).
// Everything but that division is integer arithmetic.  A corrupt stream ends in the image's status word: every read of the
// compressed bytes is bounded by the stream's length, every store by the expected inflated size.
// Animated PNG (vf_apng_inspect, vf_apng_decode_workspace_bytes, vf_apng_decode): the host walk of
// vf_apng_parse.h makes every frame an image of the full rule, the three launches decode them all, then
//   k_apng_compose   one thread per canvas pixel of a file: the frames in order, blend SOURCE, the three disposals.
#include <algorithm>
#include <string>
#include <vector>

#include "vf_apng_parse.h"
#include "vf_block.h"
#include "vf_common.h"

namespace {

constexpr int kPngdMaxSide = 16384;
constexpr int64_t kPngdMaxIdat = (int64_t)1 << 28;   // bit positions of one stream fit 32 bits
constexpr int kInfThreads = 256;
constexpr int kCap = 8192;                           // inflated bytes per token batch (uint16 indices, two blocks per CU)
constexpr int kTok = 4096;                           // tokens per batch
constexpr int kWin = 8192;                           // compressed bytes held in LDS; reloaded at the reader's place per batch
constexpr int kWinSlack = 16;                        // the symbol loop stops this far before the window's end
constexpr int kLitBits = 10, kDistBits = 9;          // primary lookup tables
constexpr int kRounds = 13;                          // ceil(log2 kCap): pointer-doubling rounds at most
static_assert((1 << kRounds) >= kCap, "a chain inside a batch has fewer than kCap links");
constexpr uint32_t kAdlerMod = 65521;

#define VF_HD __device__ __forceinline__

enum { S_HEADER = 0, S_HUFF = 1, S_STORED = 2, S_TRAILER = 3, S_END = 4 };

// one image of a batch, under either rule: the file, then its passes.  A plain file has one pass, the first; an absent pass
// has ph 0.  pinf / praw: the pass's first byte behind inf_off / raw_off (or out_off when direct)
struct PngdImage {
  int64_t src;                 // first byte of the deflate stream in the stream section of the upload (256-byte aligned)
  int64_t inf_off;             // first byte of the inflated (filtered) rows in the workspace
  int64_t raw_off;             // first byte of the unfiltered rows in the workspace (unused when direct)
  int64_t out_off;             // first ELEMENT of the H x W x C output (bytes or floats)
  int32_t slen;                // bytes of the stream (deflate blocks + Adler-32; zero-padded to 256 behind)
  int32_t expect;              // sum h_p * (1 + rb_p): the inflated size the header promises
  int32_t W, H, depth, ctype;
  int32_t rb, bpp;             // bytes per row (without the filter byte), bytes per filter unit
  int32_t rc, oc;              // samples per pixel in the rows, channels of the output
  int32_t nplte, ntrns;
  int32_t direct;              // the unfiltered rows ARE the output (one pass, uint8, 8-bit, rc == oc, no palette)
  int32_t pad;
  uint8_t plte[768];
  uint8_t trns[256];
  int32_t lace, out_kind;      // Adam7; 0: uint8, 1: float32
  int32_t ph[7], prb[7], pinf[7], praw[7];   // rows and bytes per row of each pass, its first byte in either buffer
};
static_assert(sizeof(PngdImage) == 1232, "DESIGN.md 5.6 states the descriptor's size");

// canonical code in puff's decode form: codes of length l are first[l] .. first[l] + count[l] - 1, their symbols
// sym[index[l] ...]
struct PngdHuff {
  uint16_t count[16], first[16], index[16];
  uint16_t sym[288];
};

struct PngdCtl {
  uint32_t bp;                 // bit position of the reader in the stream
  uint32_t nbits;              // 8 * slen
  uint32_t wbase;              // byte position of the window's first byte (a multiple of 4)
  int32_t state, final, build;
  int32_t remaining;           // bytes of the stored block still to copy
  int32_t out_pos;             // inflated bytes written before this batch
  int32_t nout, ntok;          // this batch: bytes, tokens (-1: a stored copy from stored_src)
  uint32_t stored_src;
  int32_t status;
  int32_t nlit, ndist;
  uint32_t s1, s2;             // Adler-32 so far
};

// all the LDS of k_pngd_inflate
struct InflateLds {
  uint32_t win[kWin / 4 + 4];
  uint16_t idx[2][kCap];       // per byte of the batch: itself (value known) or the earlier byte of the batch it copies
  uint8_t val[kCap];
  uint16_t tok_off[kTok + 1];  // first byte of each token in the batch
  uint16_t tok_v[kTok];        // 0x8000 | literal, or distance - 1
  uint16_t lit_tab[1 << kLitBits];   // (length << 9) | symbol for codes of <= kLitBits bits, 0: longer or none
  uint16_t dist_tab[1 << kDistBits];
  uint16_t code[320];          // bit-reversed canonical code of every symbol (litlen, then dist)
  uint8_t lens[320];
  PngdHuff lit, dist;
  unsigned long long s_w[kInfThreads / 64];
  PngdCtl c;
};
static_assert(2 * sizeof(InflateLds) <= 160 * 1024, "k_pngd_inflate: two blocks per CU (160 KiB of LDS)");

struct PngdBatch {
  const PngdImage* img;
  const uint8_t* streams;
  uint8_t* inf;
  uint8_t* raw;
  uint8_t* out;
  int32_t* status;
};

__constant__ uint16_t c_lbase[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                                      31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ uint8_t c_lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint16_t c_dbase[30] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
                                                      193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ uint8_t c_dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ uint8_t c_clorder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};


// 32 bits of the stream starting at bit bp, least significant first (the window holds bytes [wbase, wbase + kWin + 16),
// zeros past the stream's end)
VF_HD uint32_t pngd_peek(const InflateLds& L, uint32_t bp) {
  const uint32_t o = (bp >> 3) - L.c.wbase;
  const uint32_t d = o >> 2, sh = (o & 3) * 8 + (bp & 7);
  return (uint32_t)((((uint64_t)L.win[d + 1] << 32) | L.win[d]) >> sh);
}

// reload the window at the reader's place; every thread.  src32: the stream as dwords, ndw of them (zero-padded)
VF_HD void pngd_refill(InflateLds& L, const uint32_t* src32, uint32_t ndw, int t, int nt) {
  const uint32_t g0 = ((L.c.bp >> 3) & ~3u) >> 2;
  for (int i = t; i < kWin / 4 + 4; i += nt) L.win[i] = g0 + (uint32_t)i < ndw ? src32[g0 + i] : 0u;
}

// zlib's inflate_table validity and the canonical codes of n lengths.  kind 0: the code-length code, 1: literal/length,
// 2: distance.  code[s]: the symbol's code, bit-reversed (the order its bits come off the stream).  0: valid
VF_HD int pngd_build_code(const uint8_t* lens, int n, int kind, PngdHuff& h, uint16_t* code) {
  for (int l = 0; l < 16; ++l) h.count[l] = 0;
  for (int s = 0; s < n; ++s) ++h.count[lens[s]];
  int max = 15;
  while (max > 0 && h.count[max] == 0) --max;
  int left = 1;
  for (int l = 1; l <= 15; ++l) {
    left = (left << 1) - (int)h.count[l];
    if (left < 0) return 1;                                  // over-subscribed
  }
  if (left > 0 && max > 0 && (kind == 0 || max != 1)) return 1;   // incomplete
  int c = 0, k = 0;
  for (int l = 1; l <= 15; ++l) {
    h.first[l] = (uint16_t)c;
    h.index[l] = (uint16_t)k;
    c = (c + h.count[l]) << 1;
    k += h.count[l];
  }
  h.first[0] = h.index[0] = 0;
  uint16_t next[16];
  for (int l = 0; l < 16; ++l) next[l] = 0;
  for (int s = 0; s < n; ++s) {
    const int l = lens[s];
    if (!l) continue;
    const uint32_t cd = (uint32_t)h.first[l] + next[l];
    h.sym[h.index[l] + next[l]] = (uint16_t)s;
    ++next[l];
    uint32_t r = 0;
    for (int b = 0; b < l; ++b) r |= ((cd >> b) & 1u) << (l - 1 - b);
    code[s] = (uint16_t)r;
  }
  return 0;
}

// entries of one primary table for the symbols t, t + nt, ...; every thread, after the table was cleared
VF_HD void pngd_fill_tab(uint16_t* tab, int bits, const uint8_t* lens, const uint16_t* code, int n, int t, int nt) {
  for (int s = t; s < n; s += nt) {
    const int l = lens[s];
    if (l && l <= bits)
      for (uint32_t e = code[s]; e < (1u << bits); e += 1u << l) tab[e] = (uint16_t)((l << 9) | s);
  }
}

// one symbol from the low bits of w: its length (0: no such code) and the symbol
VF_HD int pngd_symbol(const uint16_t* tab, int bits, const PngdHuff& h, uint32_t w, int& sym) {
  const uint32_t e = tab[w & ((1u << bits) - 1)];
  if (e) {
    sym = (int)(e & 511);
    return (int)(e >> 9);
  }
  int code = 0;
  for (int l = 1; l <= 15; ++l) {
    code |= (int)(w & 1);
    w >>= 1;
    const int cnt = h.count[l], fst = h.first[l];
    if (code - cnt < fst) {
      sym = h.sym[h.index[l] + (code - fst)];
      return l;
    }
    code <<= 1;
  }
  return 0;
}

// thread 0, at the head of a batch with a fresh window: the header of a deflate block, or the trailer
VF_HD void pngd_head(InflateLds& L) {
  PngdCtl& c = L.c;
  c.build = 0;
  c.nout = 0;
  c.ntok = 0;
  if (c.state == S_TRAILER) {
    const uint32_t bp = (c.bp + 7) & ~7u;
    if (bp + 32 > c.nbits) {
      c.status = VF_PNG_SHORT_DATA;
      return;
    }
    const uint32_t v = pngd_peek(L, bp);
    const uint32_t want = ((v & 0xff) << 24) | ((v & 0xff00) << 8) | ((v >> 8) & 0xff00) | (v >> 24);
    if (want != ((c.s2 << 16) | c.s1)) c.status = VF_PNG_BAD_ADLER;
    c.state = S_END;
    return;
  }
  if (c.state != S_HEADER) return;
  uint32_t bp = c.bp;
  uint32_t w = pngd_peek(L, bp);
  c.final = (int)(w & 1);
  const int type = (int)((w >> 1) & 3);
  bp += 3;
  if (type == 3) {
    c.status = VF_PNG_BAD_CODE;
    return;
  }
  if (type == 0) {
    bp = (bp + 7) & ~7u;
    w = pngd_peek(L, bp);
    bp += 32;
    if (bp > c.nbits) {
      c.status = VF_PNG_SHORT_DATA;
      return;
    }
    const uint32_t len = w & 0xffff, nlen = w >> 16;
    if (len != (~nlen & 0xffff)) {
      c.status = VF_PNG_BAD_CODE;
      return;
    }
    c.bp = bp;
    c.remaining = (int)len;
    c.state = len ? S_STORED : (c.final ? S_TRAILER : S_HEADER);
    return;
  }
  int nlit, ndist;
  if (type == 1) {
    nlit = 288;
    ndist = 32;
    for (int s = 0; s < 288; ++s) L.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    for (int s = 0; s < 32; ++s) L.lens[288 + s] = 5;
  } else {
    nlit = (int)((w >> 3) & 31) + 257;
    ndist = (int)((w >> 8) & 31) + 1;
    const int ncl = (int)((w >> 13) & 15) + 4;
    bp += 14;
    if (nlit > 286 || ndist > 30) {
      c.status = VF_PNG_BAD_CODE;
      return;
    }
    uint8_t cl[19];
    for (int i = 0; i < 19; ++i) cl[i] = 0;
    for (int i = 0; i < ncl; ++i) {
      cl[c_clorder[i]] = (uint8_t)(pngd_peek(L, bp) & 7);
      bp += 3;
    }
    // the code-length code decodes through the distance table's place (both are rebuilt below)
    if (pngd_build_code(cl, 19, 0, L.dist, L.code)) {
      c.status = VF_PNG_BAD_CODE;
      return;
    }
    for (int e = 0; e < (1 << kDistBits); ++e) L.dist_tab[e] = 0;
    pngd_fill_tab(L.dist_tab, kDistBits, cl, L.code, 19, 0, 1);
    // HLIT + HDIST lengths are ONE sequence: a repeat may run across the boundary
    int i = 0;
    const int total = nlit + ndist;
    while (i < total) {
      if (bp > c.nbits) {
        c.status = VF_PNG_SHORT_DATA;
        return;
      }
      w = pngd_peek(L, bp);
      int sym;
      const int l = pngd_symbol(L.dist_tab, kDistBits, L.dist, w, sym);
      if (!l) {
        c.status = VF_PNG_BAD_CODE;
        return;
      }
      bp += l;
      w >>= l;
      if (sym < 16) {
        L.lens[i++] = (uint8_t)sym;
        continue;
      }
      int rep, v = 0;
      if (sym == 16) {
        if (i == 0) {
          c.status = VF_PNG_BAD_CODE;
          return;
        }
        v = L.lens[i - 1];
        rep = 3 + (int)(w & 3);
        bp += 2;
      } else if (sym == 17) {
        rep = 3 + (int)(w & 7);
        bp += 3;
      } else {
        rep = 11 + (int)(w & 127);
        bp += 7;
      }
      if (i + rep > total) {
        c.status = VF_PNG_BAD_CODE;
        return;
      }
      while (rep--) L.lens[i++] = (uint8_t)v;
    }
    if (L.lens[256] == 0) {                                   // no end-of-block code
      c.status = VF_PNG_BAD_CODE;
      return;
    }
  }
  if (bp > c.nbits) {
    c.status = VF_PNG_SHORT_DATA;
    return;
  }
  if (pngd_build_code(L.lens, nlit, 1, L.lit, L.code) || pngd_build_code(L.lens + nlit, ndist, 2, L.dist, L.code + nlit)) {
    c.status = VF_PNG_BAD_CODE;
    return;
  }
  c.nlit = nlit;
  c.ndist = ndist;
  c.bp = bp;
  c.build = 1;
  c.state = S_HUFF;
}

// every thread, when the header asked for it (two calls, a barrier between): clear, then fill the primary tables
VF_HD void pngd_tables_clear(InflateLds& L, int t, int nt) {
  for (int e = t; e < (1 << kLitBits); e += nt) L.lit_tab[e] = 0;
  for (int e = t; e < (1 << kDistBits); e += nt) L.dist_tab[e] = 0;
}
VF_HD void pngd_tables_fill(InflateLds& L, int t, int nt) {
  pngd_fill_tab(L.lit_tab, kLitBits, L.lens, L.code, L.c.nlit, t, nt);
  pngd_fill_tab(L.dist_tab, kDistBits, L.lens + L.c.nlit, L.code + L.c.nlit, L.c.ndist, t, nt);
}

// thread 0: symbols into tokens until the token buffer, the batch's output or the window is used up, or the block ends;
// or the next piece of a stored block.  Every iteration of the symbol loop consumes at least one bit, and the window's
// end stops it after at most 8 * kWin of them.  expect: the inflated size the header promises
VF_HD void pngd_tokens(InflateLds& L, int expect) {
  PngdCtl& c = L.c;
  if (c.status) return;
  if (c.state == S_STORED) {
    const int n = c.remaining < kCap ? c.remaining : kCap;
    c.stored_src = c.bp >> 3;
    c.bp += 8u * (uint32_t)n;
    if (c.bp > c.nbits) {
      c.status = VF_PNG_SHORT_DATA;
      return;
    }
    if (c.out_pos + n > expect) {
      c.status = VF_PNG_BAD_LENGTH;
      return;
    }
    c.remaining -= n;
    c.nout = n;
    c.ntok = -1;
    if (c.remaining == 0) c.state = c.final ? S_TRAILER : S_HEADER;
    return;
  }
  if (c.state != S_HUFF) return;
  uint32_t bp = c.bp;
  int ntok = 0, nout = 0;
  const uint32_t stop = 8u * (c.wbase + kWin - kWinSlack);
  int status = 0;
  while (ntok < kTok && nout + 258 <= kCap && bp <= stop) {
    uint32_t w = pngd_peek(L, bp);
    int sym;
    int l = pngd_symbol(L.lit_tab, kLitBits, L.lit, w, sym);
    if (!l) {
      status = VF_PNG_BAD_CODE;
      break;
    }
    bp += l;
    if (sym < 256) {
      if (bp > c.nbits) {
        status = VF_PNG_SHORT_DATA;
        break;
      }
      L.tok_off[ntok] = (uint16_t)nout;
      L.tok_v[ntok] = (uint16_t)(0x8000 | sym);
      ++ntok;
      ++nout;
      continue;
    }
    if (sym == 256) {
      if (bp > c.nbits) status = VF_PNG_SHORT_DATA;
      c.state = c.final ? S_TRAILER : S_HEADER;
      break;
    }
    if (sym > 285) {
      status = VF_PNG_BAD_CODE;
      break;
    }
    w >>= l;
    const int eb = c_lext[sym - 257];
    const int len = c_lbase[sym - 257] + (int)(w & ((1u << eb) - 1));
    bp += eb;
    w = pngd_peek(L, bp);
    int ds;
    l = pngd_symbol(L.dist_tab, kDistBits, L.dist, w, ds);
    if (!l || ds > 29) {
      status = VF_PNG_BAD_CODE;
      break;
    }
    w >>= l;
    const int db = c_dext[ds];
    const int dist = c_dbase[ds] + (int)(w & ((1u << db) - 1));
    bp += l + db;
    if (bp > c.nbits) {
      status = VF_PNG_SHORT_DATA;
      break;
    }
    if (dist > c.out_pos + nout) {
      status = VF_PNG_BAD_DISTANCE;
      break;
    }
    L.tok_off[ntok] = (uint16_t)nout;
    L.tok_v[ntok] = (uint16_t)(dist - 1);
    ++ntok;
    nout += len;
  }
  if (!status && c.out_pos + nout > expect) status = VF_PNG_BAD_LENGTH;
  L.tok_off[ntok] = (uint16_t)nout;
  c.bp = bp;
  c.ntok = ntok;
  c.nout = nout;
  c.status = status;
}

// every thread: the batch's bytes that are known at once (literals, copies from before the batch, stored bytes) and,
// for the others, the earlier byte of the batch they repeat.  prev: the image's inflated bytes written so far
VF_HD void pngd_resolve_init(InflateLds& L, const uint8_t* stream, const uint8_t* prev, int t, int nt) {
  const PngdCtl& c = L.c;
  if (c.ntok < 0) {
    for (int p = t; p < c.nout; p += nt) L.val[p] = stream[c.stored_src + (uint32_t)p];
    return;
  }
  for (int p = t; p < c.nout; p += nt) {
    int lo = 0, hi = c.ntok - 1;                              // the last token that starts at or before p
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (L.tok_off[mid] <= p) lo = mid;
      else hi = mid - 1;
    }
    const uint32_t v = L.tok_v[lo];
    int from = p;
    if (v & 0x8000) {
      L.val[p] = (uint8_t)v;
    } else {
      const int q = p - (int)(v + 1);
      if (q < 0) L.val[p] = prev[c.out_pos + q];             // pngd_tokens checked dist <= out_pos + offset
      else from = q;
    }
    L.idx[0][p] = (uint16_t)from;
  }
}

// every thread: one pointer-doubling round from idx[k] into idx[1 - k]; whether anything moved
VF_HD int pngd_double(InflateLds& L, int k, int t, int nt) {
  int moved = 0;
  for (int p = t; p < L.c.nout; p += nt) {
    const uint16_t a = L.idx[k][p], b = L.idx[k][a];
    L.idx[1 - k][p] = b;
    moved |= a != b;
  }
  return moved;
}

// every thread: the repeated bytes from their roots (a root's index is itself: its value is never written here)
VF_HD void pngd_resolve_final(InflateLds& L, int k, int t, int nt) {
  if (L.c.ntok < 0) return;
  for (int p = t; p < L.c.nout; p += nt) {
    const int r = L.idx[k][p];
    if (r != p) L.val[p] = L.val[r];
  }
}

// every thread: store the batch behind the image's inflated bytes; the thread's part of the two Adler sums
VF_HD void pngd_flush(const InflateLds& L, uint8_t* dst, int t, int nt, unsigned long long& a, unsigned long long& b) {
  const int n = L.c.nout;
  a = b = 0;
  for (int p = t; p < n; p += nt) {
    const uint32_t v = L.val[p];
    dst[L.c.out_pos + p] = (uint8_t)v;
    a += v;
    b += (unsigned long long)(n - p) * v;
  }
}

// thread 0: the batch's sums (over all threads) into the Adler-32, and the batch is behind us
VF_HD void pngd_advance(InflateLds& L, unsigned long long a, unsigned long long b) {
  PngdCtl& c = L.c;
  const unsigned long long n = (unsigned long long)c.nout;
  c.s2 = (uint32_t)((c.s2 + n * c.s1 + b) % kAdlerMod);
  c.s1 = (uint32_t)((c.s1 + a) % kAdlerMod);
  c.out_pos += c.nout;
}

VF_HD void pngd_ctl_init(PngdCtl& c, int slen) {
  c.bp = 0;
  c.nbits = 8u * (uint32_t)slen;
  c.wbase = 0;
  c.state = S_HEADER;
  c.final = c.build = 0;
  c.remaining = 0;
  c.out_pos = c.nout = c.ntok = 0;
  c.stored_src = 0;
  c.status = 0;
  c.nlit = c.ndist = 0;
  c.s1 = 1;
  c.s2 = 0;
}

// one block per image
__global__ __launch_bounds__(kInfThreads) void k_pngd_inflate(const PngdBatch B) {
  // L is Ls: the compiler folds + z - z away and no instruction is left of it, but only after its interprocedural constant
  // propagation, which would otherwise write the one LDS object's address into every helper below before they are simplified
  // on their own.  The code that gives is the same size and up to 3.4 % slower on streams of literals (the token loop of
  // pngd_tokens); this form keeps the helpers general until they are inlined (profiles/png_one_path_kernel_resources.txt)
  __shared__ InflateLds Ls;
  const int z = blockIdx.x;
  InflateLds& L = *(InflateLds*)((char*)&Ls + z - z);
  const int t = threadIdx.x;
  const PngdImage& im = B.img[blockIdx.x];
  const uint8_t* stream = B.streams + im.src;
  const uint32_t* src32 = (const uint32_t*)stream;
  const uint32_t ndw = ((uint32_t)im.slen + 3) >> 2;
  uint8_t* dst = B.inf + im.inf_off;
  const int expect = im.expect;
  if (t == 0) pngd_ctl_init(L.c, im.slen);
  __syncthreads();
  // every batch consumes at least one bit of the stream or ends it
  const uint32_t max_batches = 8u * (uint32_t)im.slen + 4u;
  for (uint32_t it = 0; it < max_batches; ++it) {
    if (t == 0) L.c.wbase = (L.c.bp >> 3) & ~3u;
    pngd_refill(L, src32, ndw, t, kInfThreads);
    __syncthreads();
    if (t == 0) pngd_head(L);
    __syncthreads();
    const bool stop = L.c.status || L.c.state == S_END, build = L.c.build;
    if (build) pngd_tables_clear(L, t, kInfThreads);
    __syncthreads();                                          // every thread has read what the header left before thread 0 goes on
    if (stop) break;
    if (build) {
      pngd_tables_fill(L, t, kInfThreads);
      __syncthreads();
    }
    if (t == 0) pngd_tokens(L, expect);
    __syncthreads();
    if (L.c.status) break;
    pngd_resolve_init(L, stream, dst, t, kInfThreads);
    __syncthreads();
    int k = 0;
    if (L.c.ntok > 0) {
      for (int r = 0; r < kRounds; ++r) {
        const int moved = pngd_double(L, k, t, kInfThreads);
        k = 1 - k;
        if (!__syncthreads_or(moved)) break;
      }
      pngd_resolve_final(L, k, t, kInfThreads);
      __syncthreads();
    }
    unsigned long long a, b, ta, tb;
    pngd_flush(L, dst, t, kInfThreads, a, b);
    vf_block_excl_scan<unsigned long long, kInfThreads>(a, L.s_w, ta);
    vf_block_excl_scan<unsigned long long, kInfThreads>(b, L.s_w, tb);
    __syncthreads();                                          // the batch is in memory before a later one copies from it
    if (t == 0) pngd_advance(L, ta, tb);
    __syncthreads();
  }
  if (t == 0) {
    int st = L.c.status;
    if (!st && L.c.state != S_END) st = VF_PNG_SHORT_DATA;   // the batch bound ran out: cannot happen, and is no fault
    if (!st && L.c.out_pos != expect) st = VF_PNG_BAD_LENGTH;
    B.status[blockIdx.x] = st;
  }
}

VF_HD int pngd_paeth(int a, int b, int c) {
  const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// Adam7: the pass of pixel (x & 7, y & 7), each pass's first pixel and steps
__constant__ uint8_t c_a7_pass[64] = {0, 5, 3, 5, 1, 5, 3, 5, 6, 6, 6, 6, 6, 6, 6, 6, 4, 5, 4, 5, 4, 5, 4, 5, 6, 6, 6, 6, 6, 6, 6, 6,
                                      2, 5, 3, 5, 2, 5, 3, 5, 6, 6, 6, 6, 6, 6, 6, 6, 4, 5, 4, 5, 4, 5, 4, 5, 6, 6, 6, 6, 6, 6, 6, 6};
__constant__ uint8_t c_a7_x0[7] = {0, 4, 0, 2, 0, 1, 0}, c_a7_y0[7] = {0, 0, 4, 0, 2, 0, 1};
__constant__ uint8_t c_a7_dxs[7] = {3, 3, 2, 2, 1, 1, 0}, c_a7_dys[7] = {3, 3, 3, 2, 2, 1, 1};   // log2 of dx, dy

// One wave over one pass of H rows of rb bytes; U holds one filter unit (bpp bytes).  Lane r of a band of 64 rows is at filter
// unit x = step - r, so lane r - 1 finished unit x one step earlier: its value comes by shuffle, and the one before that is
// the upper-left neighbour.  Lane 0 reads the row above the band from memory (zeros above the first row).  A filter byte
// above 4 is the image's BAD_FILTER, through atomicMax: the passes' waves share the status word
template <class U>
VF_HD void pngd_unfilter_pass(const uint8_t* in, uint8_t* dst, int H, int rb, int bpp, int32_t* status, int lane) {
  const int nx = rb / bpp;
  const int64_t stride = (int64_t)rb + 1;
  for (int band = 0; band < H; band += 64) {
    const int r = band + lane;
    const bool active = r < H;
    const int ft = active ? in[r * stride] : 0;
    if (__any(ft > 4)) {
      if (lane == 0) atomicMax(status, (int)VF_PNG_BAD_FILTER);
      return;
    }
    const uint8_t* src = in + r * stride + 1;
    uint8_t* row = dst + (int64_t)r * rb;
    const uint8_t* above = dst + (int64_t)(band - 1) * rb;    // read by lane 0 when band > 0
    const int rows = min(64, H - band);
    U cur = 0, a = 0, c = 0;
    for (int step = 0; step < nx + rows - 1; ++step) {
      U up = __shfl_up(cur, 1);                               // two shuffles for a 64-bit unit
      const int x = step - lane;
      const bool on = active && x >= 0 && x < nx;
      if (lane == 0) {
        up = 0;
        if (band > 0 && on)
          for (int k = 0; k < bpp; ++k) up |= (U)above[(int64_t)x * bpp + k] << (8 * k);
      }
      if (on) {
        U o = 0;
        for (int k = 0; k < bpp; ++k) {
          const int f = src[(int64_t)x * bpp + k];
          const int av = (int)(a >> (8 * k)) & 255, bv = (int)(up >> (8 * k)) & 255, cv = (int)(c >> (8 * k)) & 255;
          const int pred = ft == 0 ? 0 : ft == 1 ? av : ft == 2 ? bv : ft == 3 ? (av + bv) >> 1 : pngd_paeth(av, bv, cv);
          const int v = (f + pred) & 255;
          row[(int64_t)x * bpp + k] = (uint8_t)v;
          o |= (U)v << (8 * k);
        }
        cur = o;
        a = o;
        c = up;
      }
    }
    __syncthreads();   // the band's last row is in memory before lane 0 of the next band reads it
  }
}

// one wave per (image, pass): block 7 * i + p.  An absent pass returns at once
__global__ __launch_bounds__(64) void k_pngd_unfilter(const PngdBatch B) {
  const int i = blockIdx.x / 7, p = blockIdx.x % 7;
  const PngdImage& d = B.img[i];
  const int h = d.ph[p];
  if (h == 0 || B.status[i] != 0) return;
  const uint8_t* in = B.inf + d.inf_off + d.pinf[p];
  uint8_t* dst = (d.direct ? B.out + d.out_off : B.raw + d.raw_off) + d.praw[p];
  if (d.bpp <= 4) pngd_unfilter_pass<uint32_t>(in, dst, h, d.prb[p], d.bpp, B.status + i, threadIdx.x);
  else pngd_unfilter_pass<unsigned long long>(in, dst, h, d.prb[p], d.bpp, B.status + i, threadIdx.x);
}

// one thread per output pixel
__global__ void k_pngd_expand(const PngdBatch B) {
  const PngdImage& im = B.img[blockIdx.y];
  if (im.direct || B.status[blockIdx.y] != 0) return;
  const uint8_t* raw = B.raw + im.raw_off;
  const int64_t npix = (int64_t)im.W * im.H;
  const int depth = im.depth, oc = im.oc;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / im.W), x = (int)(i % im.W);
    int px = x;                                               // the pixel's place in its pass, the pass's rows
    const uint8_t* row;
    if (im.lace) {
      const int p = c_a7_pass[(y & 7) * 8 + (x & 7)];
      px = (x - c_a7_x0[p]) >> c_a7_dxs[p];
      row = raw + im.praw[p] + (int64_t)((y - c_a7_y0[p]) >> c_a7_dys[p]) * im.prb[p];
    } else {
      row = raw + (int64_t)y * im.rb;
    }
    int s[4] = {0, 0, 0, 255};
    if (depth < 8) {                                          // colour types 0 and 3 only: one sample per pixel, MSB first
      const int bit = px * depth;
      const int v = (row[bit >> 3] >> (8 - depth - (bit & 7))) & ((1 << depth) - 1);
      s[0] = im.ctype == 3 ? v : v * (255 / ((1 << depth) - 1));
    } else if (depth == 8) {
      for (int k = 0; k < im.rc; ++k) s[k] = row[(int64_t)px * im.rc + k];
    } else {                                                  // 16 bits, big-endian
      for (int k = 0; k < im.rc; ++k) {
        const uint8_t* q = row + ((int64_t)px * im.rc + k) * 2;
        s[k] = (q[0] << 8) | q[1];
      }
    }
    int v[4];                                                 // the output's channels
    if (im.ctype == 3) {
      const int ix = s[0];
      if (ix >= im.nplte) {
        atomicMax(B.status + blockIdx.y, (int)VF_PNG_BAD_INDEX);
        continue;
      }
      v[0] = im.plte[3 * ix];
      v[1] = im.plte[3 * ix + 1];
      v[2] = im.plte[3 * ix + 2];
      v[3] = ix < im.ntrns ? im.trns[ix] : 255;
    } else if (im.ctype == 0 || im.ctype == 4) {
      v[0] = s[0];
      if (oc == 2) {
        v[1] = s[1];
      } else {
        v[1] = v[2] = s[0];
        v[3] = s[1];
      }
    } else {
      v[0] = s[0];
      v[1] = s[1];
      v[2] = s[2];
      v[3] = s[3];
    }
    if (im.out_kind == 0) {
      uint8_t* o = B.out + im.out_off + i * oc;
      const int sh = depth == 16 ? 8 : 0;                     // a 16-bit sample's high byte
      for (int k = 0; k < oc; ++k) o[k] = (uint8_t)(v[k] >> sh);
    } else {
      float* o = (float*)B.out + im.out_off + i * oc;
      const float top = depth == 16 ? 65535.f : 255.f;
      for (int k = 0; k < oc; ++k) o[k] = __fdiv_rn((float)v[k], top);
    }
  }
}

// image.load(path, nc, 'float') on top of the bytes: b / 255 in float32, correctly rounded
__global__ void k_pngd_to_float(const uint8_t* src, float* dst, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = __fdiv_rn((float)src[i], 255.f);
}

// ================================================================================================ host side: parsing
struct Crc32 {
  uint32_t t[8][256];
  Crc32() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
      t[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
      for (int s = 1; s < 8; ++s) t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 255];
  }
  uint32_t run(const uint8_t* p, size_t n) const {   // slicing by 8
    uint32_t c = 0xFFFFFFFFu;
    while (n >= 8) {
      uint32_t lo, hi;
      memcpy(&lo, p, 4);
      memcpy(&hi, p + 4, 4);
      lo ^= c;
      c = t[7][lo & 255] ^ t[6][(lo >> 8) & 255] ^ t[5][(lo >> 16) & 255] ^ t[4][lo >> 24] ^ t[3][hi & 255] ^ t[2][(hi >> 8) & 255] ^
          t[1][(hi >> 16) & 255] ^ t[0][hi >> 24];
      p += 8;
      n -= 8;
    }
    while (n--) c = t[0][(c ^ *p++) & 255] ^ (c >> 8);
    return ~c;
  }
};

struct PngParsed {
  int64_t W = 0, H = 0;
  int depth = 0, ctype = 0, lace = 0;
  int rc = 0;                  // samples per pixel in the rows
  int fc = 0;                  // channels after expansion: what image.load(path) gives
  int nplte = 0, ntrns = 0;
  bool has_plte = false, has_trns = false;
  uint8_t plte[768] = {}, trns[256] = {};
  int64_t idat_bytes = 0, idat_chunks = 0;
  std::vector<std::pair<int64_t, int64_t>> idat;   // (first byte, length) of every non-empty IDAT payload
  int64_t rb = 0, inflated = 0;
  bool supported = false;
  std::string why;
};

inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// 0: parsed (P.supported says whether the decoder takes the file, P.why why not); else malformed (msg)
int png_parse(const uint8_t* d, int64_t n, PngParsed& P, std::string& msg, bool crc) {
  static const Crc32 C;
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  auto unsupported = [&](const std::string& w) {
    if (P.why.empty()) P.why = w;
  };
  if (n < 8 || memcmp(d, sig, 8) != 0) {
    msg = "not a PNG file (bad signature)";
    return 2;
  }
  int64_t pos = 8;
  bool first = true, seen_idat = false, idat_done = false, iend = false;
  while (pos < n) {
    if (pos + 12 > n) {
      msg = "truncated chunk header at byte " + std::to_string(pos);
      return 2;
    }
    const int64_t L = be32(d + pos);
    const uint8_t* ty = d + pos + 4;
    const std::string name((const char*)ty, 4);
    if (pos + 12 + L > n) {
      msg = "chunk " + name + " at byte " + std::to_string(pos) + " runs past the end of the file";
      return 2;
    }
    const uint8_t* body = d + pos + 8;
    const bool is_ihdr = name == "IHDR", is_plte = name == "PLTE", is_idat = name == "IDAT", is_iend = name == "IEND",
               is_trns = name == "tRNS";
    if (first != is_ihdr) {
      msg = first ? "IHDR is not the first chunk" : "more than one IHDR";
      return 2;
    }
    if (crc && (is_ihdr || is_plte || is_idat || is_iend || is_trns) && C.run(ty, (size_t)L + 4) != be32(body + L)) {
      msg = "wrong CRC on chunk " + name + " at byte " + std::to_string(pos);
      return 2;
    }
    if (seen_idat && !is_idat) idat_done = true;
    if (is_ihdr) {
      if (L != 13) {
        msg = "IHDR of " + std::to_string(L) + " bytes";
        return 2;
      }
      P.W = be32(body);
      P.H = be32(body + 4);
      P.depth = body[8];
      P.ctype = body[9];
      P.lace = body[12];
      const int dp = P.depth, ct = P.ctype;
      const bool depth_ok = dp == 1 || dp == 2 || dp == 4 || dp == 8 || dp == 16;
      const bool combo = depth_ok && (ct == 0 || (ct == 3 && dp <= 8) || ((ct == 2 || ct == 4 || ct == 6) && dp >= 8));
      if (P.W < 1 || P.H < 1 || P.W > 0x7fffffff || P.H > 0x7fffffff || !combo || body[10] != 0 || body[11] != 0 || P.lace > 1) {
        msg = "illegal IHDR: " + std::to_string(P.W) + "x" + std::to_string(P.H) + ", bit depth " + std::to_string(dp) +
              ", colour type " + std::to_string(ct) + ", compression " + std::to_string(body[10]) + ", filter " +
              std::to_string(body[11]) + ", interlace " + std::to_string(P.lace);
        return 2;
      }
      P.rc = ct == 0 || ct == 3 ? 1 : ct == 2 ? 3 : ct == 4 ? 2 : 4;
      first = false;
    } else if (is_plte) {
      if (seen_idat) {
        msg = "PLTE after IDAT";
        return 2;
      }
      if (P.has_plte || L == 0 || L % 3 != 0 || L > 768 || P.ctype == 0 || P.ctype == 4 || (P.ctype == 3 && L / 3 > (1 << P.depth))) {
        msg = "illegal PLTE (" + std::to_string(L) + " bytes, colour type " + std::to_string(P.ctype) + ")";
        return 2;
      }
      P.has_plte = true;
      P.nplte = (int)(L / 3);
      memcpy(P.plte, body, (size_t)L);
    } else if (is_trns) {
      const bool ok = !seen_idat && !P.has_trns &&
                      ((P.ctype == 3 && P.has_plte && L >= 1 && L <= P.nplte) || (P.ctype == 0 && L == 2) || (P.ctype == 2 && L == 6));
      if (!ok) {
        msg = "illegal tRNS (" + std::to_string(L) + " bytes, colour type " + std::to_string(P.ctype) + ")";
        return 2;
      }
      P.has_trns = true;
      P.ntrns = P.ctype == 3 ? (int)L : 1;
      if (P.ctype == 3) memcpy(P.trns, body, (size_t)L);
    } else if (is_idat) {
      if (idat_done) {
        msg = "IDAT chunks are not consecutive";
        return 2;
      }
      if (P.ctype == 3 && !P.has_plte) {
        msg = "no PLTE before IDAT for colour type 3";
        return 2;
      }
      seen_idat = true;
      ++P.idat_chunks;
      P.idat_bytes += L;
      if (L) P.idat.push_back({pos + 8, L});
    } else if (is_iend) {
      if (L != 0) {
        msg = "IEND of " + std::to_string(L) + " bytes";
        return 2;
      }
      iend = true;
      break;
    } else if (!(ty[0] & 0x20)) {
      msg = "unknown critical chunk " + name;
      return 2;
    }
    pos += 12 + L;
  }
  if (first) {
    msg = "no IHDR";
    return 2;
  }
  if (!iend) {
    msg = "no IEND chunk";
    return 2;
  }
  if (!seen_idat) {
    msg = "no IDAT chunk";
    return 2;
  }
  // the zlib header: deflate, a window of at most 32 KiB, no preset dictionary, FCHECK
  {
    int z[2], k = 0;
    for (const auto& c : P.idat)
      for (int64_t i = 0; i < c.second && k < 2; ++i) z[k++] = d[c.first + i];
    if (k < 2) {
      msg = "zlib header: the IDAT data is " + std::to_string(P.idat_bytes) + " bytes";
      return 2;
    }
    if ((z[0] & 15) != 8 || (z[0] >> 4) > 7 || (z[1] & 0x20) || (z[0] * 256 + z[1]) % 31 != 0) {
      char b[96];
      snprintf(b, sizeof b, "bad zlib header %02x %02x (deflate, window <= 32 KiB, no dictionary, FCHECK)", z[0], z[1]);
      msg = b;
      return 2;
    }
  }
  P.fc = P.ctype == 3 ? (P.has_trns ? 4 : 3) : P.rc + ((P.ctype == 0 || P.ctype == 2) && P.has_trns ? 1 : 0);
  P.rb = (P.W * P.rc * P.depth + 7) / 8;
  P.inflated = P.H * (1 + P.rb);
  if (P.depth == 16) unsupported("16-bit samples");
  if (P.lace) unsupported("Adam7 interlace");
  if (P.W > kPngdMaxSide || P.H > kPngdMaxSide) unsupported("larger than 16384 per side");
  if (P.idat_bytes > kPngdMaxIdat) unsupported("IDAT data above 256 MiB");
  P.supported = P.why.empty();
  return 0;
}

// channels of the output for a request (0: the file's); 0 with `why` when the byte rule has none
int png_out_channels(const PngParsed& P, int channels, std::string& why) {
  const bool colour = P.ctype == 2 || P.ctype == 3 || P.ctype == 6;
  if (channels == 0) {
    if (P.has_trns && P.ctype != 3) {
      why = "tRNS on colour type " + std::to_string(P.ctype) + " with the file's channels (alpha from a colour key)";
      return 0;
    }
    return P.fc;
  }
  if (channels == 1 && colour) {
    why = "colour file with channels=1 (rgb2y is not a byte rule)";
    return 0;
  }
  return channels;
}

// ---------------------------------------------------------------------------------- host side: the rules and the one path
// One pipeline, two rules for which files it takes; an entry is the path below under its rule value.
struct PngRule {
  const char* who;             // what the messages about the batch's files start with
  bool full;                   // Adam7-interlaced and 16-bit files are taken
  const char* unfilter;        // profiling labels of the unfilter and the expand launch
  const char* expand;
};
constexpr PngRule kDefaultRule = {"vf_png_decode", false, "pngd_unfilter", "pngd_expand"};
constexpr PngRule kFullRule = {"vf_png_decode_full", true, "pngd_unfilter_full", "pngd_expand_full"};

struct PngPasses {
  int64_t w[7] = {}, h[7] = {}, rb[7] = {};   // zeros for an absent pass; a plain file is one pass, the first
  int64_t inflated = 0, raw = 0;              // sum h_p * (1 + rb_p), sum h_p * rb_p
  bool supported = false;
  std::string why;
};

// a parsed file under a rule: the passes, the inflated size they promise, supported or why not.  The default rule refuses an
// interlaced file, so what it sizes is always one pass, and its refusals are png_parse's, in that order
void png_rule(const PngParsed& P, const PngRule& rule, PngPasses& F) {
  static const int x0[7] = {0, 4, 0, 2, 0, 1, 0}, y0[7] = {0, 0, 4, 0, 2, 0, 1}, dx[7] = {8, 8, 4, 4, 2, 2, 1}, dy[7] = {8, 8, 8, 4, 4, 2, 2};
  const bool lace = rule.full && P.lace;
  for (int p = 0; p < (lace ? 7 : 1); ++p) {
    const int64_t w = lace ? std::max<int64_t>(0, (P.W - x0[p] + dx[p] - 1) / dx[p]) : P.W;
    const int64_t h = lace ? std::max<int64_t>(0, (P.H - y0[p] + dy[p] - 1) / dy[p]) : P.H;
    if (w == 0 || h == 0) continue;
    F.w[p] = w;
    F.h[p] = h;
    F.rb[p] = (w * P.rc * P.depth + 7) / 8;
    F.inflated += h * (1 + F.rb[p]);
    F.raw += h * F.rb[p];
  }
  if (!rule.full) F.why = P.why;
  else if (P.W > kPngdMaxSide || P.H > kPngdMaxSide) F.why = "larger than 16384 per side";
  else if (P.idat_bytes > kPngdMaxIdat) F.why = "IDAT data above 256 MiB";
  else if (F.inflated >= ((int64_t)1 << 31)) F.why = "inflated size of 2^31 bytes or more (the decoder's sizes are int32)";
  F.supported = F.why.empty();
}

inline bool pngd_direct(const PngParsed& P, int oc, int out_kind) {
  return !P.lace && out_kind == 0 && P.depth == 8 && P.ctype != 3 && oc == P.rc;
}

// the bytes of a batch's streams, inflated rows and unfiltered rows, image by image
struct PngdSizes {
  int64_t stream_bytes = 0, inf_bytes = 0, raw_bytes = 0;
  void add(const PngParsed& P, const PngPasses& F, bool direct) {
    stream_bytes += (int64_t)vf_up256((size_t)(P.idat_bytes - 2) + 8);
    inf_bytes += (int64_t)vf_up256((size_t)F.inflated);
    if (!direct) raw_bytes += (int64_t)vf_up256((size_t)F.raw);
  }
};

struct PngdPlan : PngdSizes {
  std::vector<PngParsed> P;
  std::vector<PngPasses> F;
  std::vector<int> oc;
  int64_t max_pix = 0;
  size_t o_img = 0, o_streams = 0, stage = 0, o_inf = 0, o_raw = 0, ws = 0;
};

int pngd_plan(const PngRule& rule, const uint8_t* data, const int64_t* offs, int n, int channels, int out_kind, PngdPlan& L, bool crc) {
  const char* who = rule.who;
  VF_REQUIRE(n > 0 && data && offs, "%s: empty batch", who);
  VF_REQUIRE(n <= 65535, "%s: %d files in one batch (65535 at most)", who, n);
  VF_REQUIRE(channels == 0 || channels == 1 || channels == 3, "%s: channels %d is not 0 (the file's), 1 or 3", who, channels);
  VF_REQUIRE(out_kind == 0 || out_kind == 1, "%s: out_kind %d is not 0 (uint8) or 1 (float32)", who, out_kind);
  L.P.resize(n);
  L.F.resize(n);
  L.oc.resize(n);
  for (int i = 0; i < n; ++i) {
    std::string msg;
    VF_REQUIRE(offs[i + 1] >= offs[i], "%s: offsets decrease at image %d", who, i);
    PngParsed& P = L.P[i];
    PngPasses& F = L.F[i];
    if (png_parse(data + offs[i], offs[i + 1] - offs[i], P, msg, crc)) {
      vf_set_error("%s: image %d: %s", who, i, msg.c_str());
      return 2;
    }
    png_rule(P, rule, F);
    std::string why = F.why;
    if (F.supported) L.oc[i] = png_out_channels(P, channels, why);
    if (!F.supported || !L.oc[i]) {
      vf_set_error("%s: image %d: unsupported: %s", who, i, why.c_str());
      return 3;
    }
    L.add(P, F, pngd_direct(P, L.oc[i], out_kind));
    L.max_pix = std::max(L.max_pix, P.W * P.H);
  }
  VfCarve ws;
  L.o_img = ws.take(sizeof(PngdImage) * n);
  L.o_streams = ws.take((size_t)L.stream_bytes);
  L.stage = ws.at;
  L.o_inf = ws.take((size_t)L.inf_bytes);
  L.o_raw = ws.take((size_t)L.raw_bytes);
  L.ws = ws.at;
  return 0;
}

// where the next image's stream, inflated rows and unfiltered rows begin in their sections
struct PngdAt {
  int64_t sc = 0, inf = 0, raw = 0;
};

// one image's descriptor, and its stream into the upload: every IDAT payload behind the one before, minus the stream's first
// two bytes (the zlib header), zero-padded.  `at` moves on to the next image
void pngd_fill(PngdImage& im, const PngParsed& P, const PngPasses& F, const uint8_t* d, int oc, int out_kind, int64_t out_off,
               uint8_t* streams, PngdAt& at) {
  memset(&im, 0, sizeof(im));
  im.W = (int32_t)P.W;
  im.H = (int32_t)P.H;
  im.depth = P.depth;
  im.ctype = P.ctype;
  im.rb = (int32_t)P.rb;
  im.bpp = std::max(1, P.rc * P.depth / 8);
  im.rc = P.rc;
  im.oc = oc;
  im.nplte = P.nplte;
  im.ntrns = P.ctype == 3 ? P.ntrns : 0;
  im.direct = pngd_direct(P, oc, out_kind) ? 1 : 0;
  memcpy(im.plte, P.plte, 768);
  memcpy(im.trns, P.trns, 256);
  im.expect = (int32_t)F.inflated;
  im.src = at.sc;
  im.slen = (int32_t)(P.idat_bytes - 2);
  im.inf_off = at.inf;
  im.raw_off = at.raw;
  im.out_off = out_off;
  im.lace = P.lace;
  im.out_kind = out_kind;
  int64_t pi = 0, pr = 0;
  for (int p = 0; p < 7; ++p) {
    im.ph[p] = (int32_t)F.h[p];
    im.prb[p] = (int32_t)F.rb[p];
    im.pinf[p] = (int32_t)pi;
    im.praw[p] = (int32_t)pr;
    pi += F.h[p] * (1 + F.rb[p]);
    pr += F.h[p] * F.rb[p];
  }
  int64_t skip = 2, n = 0;
  for (const auto& c : P.idat) {
    const int64_t s = std::min(skip, c.second);
    skip -= s;
    memcpy(streams + at.sc + n, d + c.first + s, (size_t)(c.second - s));
    n += c.second - s;
  }
  const int64_t room = (int64_t)vf_up256((size_t)im.slen + 8);
  memset(streams + at.sc + n, 0, (size_t)(room - n));
  at.sc += room;
  at.inf += (int64_t)vf_up256((size_t)F.inflated);
  if (!im.direct) at.raw += (int64_t)vf_up256((size_t)F.raw);
}

void pngd_pack(const uint8_t* data, const int64_t* offs, int n, int out_kind, const int64_t* out_offs, const PngdPlan& L, uint8_t* st) {
  PngdImage* imgs = (PngdImage*)(st + L.o_img);
  PngdAt at;
  for (int i = 0; i < n; ++i) pngd_fill(imgs[i], L.P[i], L.F[i], data + offs[i], L.oc[i], out_kind, out_offs[i], st + L.o_streams, at);
}

// The device half, whatever the entry: the staged descriptors and streams go up to the workspace's head in one copy, the
// status words are cleared, and the three launches decode the batch's n images.  S: the batch's section sizes, for the
// profile's byte counts; max_pix: the largest image, which sizes the expansion's grid; upload: the label of the upload range
int pngd_run(const PngRule& rule, const char* upload, vf_ctx* ctx, const PngdBatch& B, void* ws, const void* stage, size_t stage_bytes,
             unsigned n, const PngdSizes& S, int64_t max_pix) {
  hipStream_t st = ctx->stream;
  {
    VfRange r(upload);
    VF_CHECK_HIP(hipMemcpyAsync(ws, stage, stage_bytes, hipMemcpyHostToDevice, st));
    VF_CHECK_HIP(hipMemsetAsync(B.status, 0, sizeof(int32_t) * n, st));
  }
  const double inf = (double)S.inf_bytes;
  VF_LAUNCH_TIMED(ctx, "pngd_inflate", 0.0, (double)S.stream_bytes + inf, k_pngd_inflate, dim3(n), dim3(kInfThreads), B);
  VF_LAUNCH_CHECK();
  VF_LAUNCH_TIMED(ctx, rule.unfilter, 0.0, 2.0 * inf, k_pngd_unfilter, dim3(7u * n), dim3(64), B);
  VF_LAUNCH_CHECK();
  const unsigned gp = (unsigned)std::min<int64_t>(std::max<int64_t>(1, vf_cdiv(max_pix, 256)), 4096);
  VF_LAUNCH_TIMED(ctx, rule.expand, 0.0, 2.0 * (double)S.raw_bytes, k_pngd_expand, dim3(gp, n), dim3(256), B);
  VF_LAUNCH_CHECK();
  return 0;
}

// the body of both inspect entries.  passes: seven (w, h, rb), only under the full rule and only when asked for
int png_inspect(const char* who, const PngRule& rule, const unsigned char* data, size_t len, int64_t* info, int64_t* passes, char* reason,
                int reason_cap) {
  VF_REQUIRE(data && info, "%s: NULL argument", who);
  PngParsed P;
  std::string msg;
  const int rc = png_parse(data, (int64_t)len, P, msg, true);
  if (rc) {
    vf_set_error("%s: %s", who, msg.c_str());
    return rc;
  }
  PngPasses F;
  png_rule(P, rule, F);
  const int64_t v[12] = {P.W, P.H, P.depth, P.ctype, P.lace, P.fc, P.idat_bytes, P.idat_chunks, P.nplte, P.ntrns, F.supported ? 1 : 0,
                         F.inflated};
  memcpy(info, v, sizeof v);
  for (int p = 0; passes && p < 7; ++p) {
    passes[3 * p] = F.w[p];
    passes[3 * p + 1] = F.h[p];
    passes[3 * p + 2] = F.rb[p];
  }
  if (reason && reason_cap > 0) snprintf(reason, (size_t)reason_cap, "%s", F.why.c_str());
  return 0;
}

// the body of both size queries: the chunk walk alone, the decode entry checks the CRCs
int pngd_query(const PngRule& rule, const unsigned char* data, const int64_t* offs, int n, int channels, int out_kind, size_t* ws_bytes,
               size_t* stage_bytes) {
  PngdPlan L;
  if (int e = pngd_plan(rule, data, offs, n, channels, out_kind, L, false)) return e;
  if (ws_bytes) *ws_bytes = L.ws;
  if (stage_bytes) *stage_bytes = L.stage;
  return 0;
}

// the body of both decode entries
int pngd_decode(const PngRule& rule, vf_ctx* ctx, const unsigned char* data, const int64_t* offs, int n, int channels, int out_kind,
                const int64_t* out_offs, void* out, void* stage, size_t stage_bytes, void* ws, size_t ws_bytes, int32_t* status) {
  VF_REQUIRE(out && out_offs && stage && ws && status, "%s: NULL argument", rule.who);
  PngdPlan L;
  if (int e = pngd_plan(rule, data, offs, n, channels, out_kind, L, true)) return e;
  VF_REQUIRE(stage_bytes >= L.stage && ws_bytes >= L.ws, "%s: staging %zu / workspace %zu bytes, need %zu / %zu", rule.who, stage_bytes,
             ws_bytes, L.stage, L.ws);
  pngd_pack(data, offs, n, out_kind, out_offs, L, (uint8_t*)stage);
  uint8_t* w = (uint8_t*)ws;
  PngdBatch B;
  B.img = (const PngdImage*)(w + L.o_img);
  B.streams = w + L.o_streams;
  B.inf = w + L.o_inf;
  B.raw = w + L.o_raw;
  B.out = (uint8_t*)out;
  B.status = status;
  return pngd_run(rule, "pngd_upload", ctx, B, ws, stage, L.stage, (unsigned)n, L, L.max_pix);
}


// ------------------------------------------------------------------------------------------- animated PNG
// Every frame of every file is an image of the full rule above — its fcTL's width x height under the file's IHDR, PLTE and
// tRNS, its stream the frame's IDAT or fdAT payloads — decoded by the same three launches into the file's own channels in the
// workspace; k_apng_compose then paints the canvases.
struct ApngdFile {
  int64_t out_off;             // first byte of the file's frames x H x W x oc output
  int32_t W, H;
  int32_t first, frames;       // its frames in the frame arrays
  int32_t fc, oc;              // channels of the decoded frames (1, 2, 3, 4), of the output (3, 4)
};
struct ApngdFrame {
  int64_t px;                  // first byte of the decoded h x w x fc frame in the pixel section of the workspace
  int32_t x, y, w, h;
  int32_t dispose, pad;
};

struct ApngdBatch {
  const ApngdFile* files;
  const ApngdFrame* frames;
  const uint8_t* px;
  const int32_t* frame_status; // VF_PNG_* per frame, as the three launches left them
  uint8_t* out;
  int32_t* status;             // per file: the first of its frames' that is not 0
};

// One thread per canvas pixel of a file (blockIdx.y): the frames in order, the pixel's RGBA value and the copy PREVIOUS restores in
// registers.  Blend SOURCE (OVER is refused where it differs): inside the frame's rectangle the frame's pixel replaces the canvas,
// alpha too; the value goes to output frame k; then the disposal: BACKGROUND clears the rectangle to transparent black, PREVIOUS
// restores what was there before the frame (on frame 0 that is the empty canvas).  All integer.  A file with a corrupt frame gets
// that frame's status and is left alone.
__global__ __launch_bounds__(256) void k_apng_compose(const ApngdBatch B) {
  const ApngdFile& f = B.files[blockIdx.y];
  int st = 0;
  for (int k = 0; k < f.frames && st == 0; ++k) st = B.frame_status[f.first + k];
  if (blockIdx.x == 0 && threadIdx.x == 0) B.status[blockIdx.y] = st;
  if (st != 0) return;
  const int64_t npix = (int64_t)f.W * f.H;
  const int fc = f.fc, oc = f.oc;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / f.W), x = (int)(i % f.W);
    uint32_t cur = 0;                                          // R | G << 8 | B << 16 | A << 24
    uint8_t* o = B.out + f.out_off + i * oc;
    for (int k = 0; k < f.frames; ++k) {
      const ApngdFrame& fr = B.frames[f.first + k];
      const uint32_t prev = cur;
      const bool inside = x >= fr.x && x < fr.x + fr.w && y >= fr.y && y < fr.y + fr.h;
      if (inside) {
        const uint8_t* p = B.px + fr.px + ((int64_t)(y - fr.y) * fr.w + (x - fr.x)) * fc;
        if (fc == 1) cur = p[0] * 0x010101u | 0xFF000000u;
        else if (fc == 2) cur = p[0] * 0x010101u | ((uint32_t)p[1] << 24);
        else if (fc == 3) cur = p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | 0xFF000000u;
        else cur = p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
      }
      o[0] = (uint8_t)cur;
      o[1] = (uint8_t)(cur >> 8);
      o[2] = (uint8_t)(cur >> 16);
      if (oc == 4) o[3] = (uint8_t)(cur >> 24);
      o += npix * oc;
      if (inside && fr.dispose == 1) cur = 0;
      else if (inside && fr.dispose == 2) cur = prev;
    }
  }
}

struct ApngdPlan : PngdSizes {
  std::vector<apngd::Parsed> A;
  std::vector<PngParsed> P;    // one per frame: the frame as an image of the full rule
  std::vector<PngPasses> F;
  std::vector<int> file_of;
  int64_t nframes = 0, px_bytes = 0, max_fpix = 0, max_cpix = 0;
  size_t o_img = 0, o_files = 0, o_frames = 0, o_streams = 0, stage = 0, o_inf = 0, o_raw = 0, o_px = 0, o_fstatus = 0, ws = 0;
};

// frame k of a parsed file as the image the full rule decodes
void apngd_frame_image(const apngd::Parsed& A, const apngd::Frame& f, PngParsed& P) {
  P.W = f.w;
  P.H = f.h;
  P.depth = A.depth;
  P.ctype = A.ctype;
  P.lace = A.lace;
  P.rc = A.rc;
  P.fc = A.fc;
  P.nplte = A.nplte;
  P.ntrns = A.ntrns;
  P.has_plte = A.has_plte;
  P.has_trns = A.has_trns;
  memcpy(P.plte, A.plte, 768);
  memcpy(P.trns, A.trns, 256);
  P.idat_bytes = f.data_bytes;
  P.idat_chunks = (int64_t)f.seg.size();
  P.idat = f.seg;
  P.rb = (P.W * P.rc * P.depth + 7) / 8;
  P.inflated = P.H * (1 + P.rb);
  P.supported = true;
}

// 0; 2 with the error set for a malformed file; 3 for one the device decoder does not take
int apngd_plan(const char* who, const uint8_t* data, const int64_t* offs, int n, int alpha, ApngdPlan& L) {
  VF_REQUIRE(n > 0 && data && offs, "%s: empty batch", who);
  VF_REQUIRE(n <= 65535, "%s: %d files in one batch (65535 at most)", who, n);
  VF_REQUIRE(alpha == 0 || alpha == 1, "%s: alpha %d is not 0 (RGB) or 1 (RGBA)", who, alpha);
  L.A.resize(n);
  for (int i = 0; i < n; ++i) {
    std::string msg;
    VF_REQUIRE(offs[i + 1] >= offs[i], "%s: offsets decrease at image %d", who, i);
    apngd::Parsed& A = L.A[i];
    if (apngd::parse(data + offs[i], offs[i + 1] - offs[i], A, msg)) {
      vf_set_error("%s: image %d: %s", who, i, msg.c_str());
      return 2;
    }
    if (!A.supported) {
      vf_set_error("%s: image %d: unsupported: %s", who, i, A.why.c_str());
      return 3;
    }
    for (size_t k = 0; k < A.frames.size(); ++k) {
      L.P.emplace_back();
      L.F.emplace_back();
      L.file_of.push_back(i);
      PngParsed& P = L.P.back();
      PngPasses& F = L.F.back();
      apngd_frame_image(A, A.frames[k], P);
      png_rule(P, kFullRule, F);
      if (!F.supported) {
        vf_set_error("%s: image %d: unsupported: frame %zu: %s", who, i, k, F.why.c_str());
        return 3;
      }
      L.add(P, F, pngd_direct(P, A.fc, 0));
      L.px_bytes += (int64_t)vf_up256((size_t)(P.W * P.H * A.fc));
      L.max_fpix = std::max(L.max_fpix, P.W * P.H);
    }
    L.max_cpix = std::max(L.max_cpix, A.W * A.H);
  }
  L.nframes = (int64_t)L.P.size();
  VF_REQUIRE(L.nframes <= 65535, "%s: %lld frames in one batch (65535 at most; split the batch)", who, (long long)L.nframes);
  VfCarve ws;
  L.o_img = ws.take(sizeof(PngdImage) * (size_t)L.nframes);
  L.o_files = ws.take(sizeof(ApngdFile) * (size_t)n);
  L.o_frames = ws.take(sizeof(ApngdFrame) * (size_t)L.nframes);
  L.o_streams = ws.take((size_t)L.stream_bytes);
  L.stage = ws.at;
  L.o_inf = ws.take((size_t)L.inf_bytes);
  L.o_raw = ws.take((size_t)L.raw_bytes);
  L.o_px = ws.take((size_t)L.px_bytes);
  L.o_fstatus = ws.take(sizeof(int32_t) * (size_t)L.nframes);
  L.ws = ws.at;
  return 0;
}

void apngd_pack(const uint8_t* data, const int64_t* offs, int n, int alpha, const int64_t* out_offs, const ApngdPlan& L, uint8_t* st) {
  PngdImage* imgs = (PngdImage*)(st + L.o_img);
  ApngdFile* files = (ApngdFile*)(st + L.o_files);
  ApngdFrame* frames = (ApngdFrame*)(st + L.o_frames);
  PngdAt at;
  int64_t px = 0, j = 0;
  for (int i = 0; i < n; ++i) {
    const apngd::Parsed& A = L.A[i];
    ApngdFile& fl = files[i];
    memset(&fl, 0, sizeof(fl));
    fl.out_off = out_offs[i];
    fl.W = (int32_t)A.W;
    fl.H = (int32_t)A.H;
    fl.first = (int32_t)j;
    fl.frames = (int32_t)A.frames.size();
    fl.fc = A.fc;
    fl.oc = alpha ? 4 : 3;
    for (size_t k = 0; k < A.frames.size(); ++k, ++j) {
      const PngParsed& P = L.P[j];
      pngd_fill(imgs[j], P, L.F[j], data + offs[i], A.fc, 0, px, st + L.o_streams, at);
      ApngdFrame& fr = frames[j];
      memset(&fr, 0, sizeof(fr));
      fr.px = px;
      fr.x = (int32_t)A.frames[k].x;
      fr.y = (int32_t)A.frames[k].y;
      fr.w = (int32_t)A.frames[k].w;
      fr.h = (int32_t)A.frames[k].h;
      fr.dispose = A.frames[k].dispose;
      px += (int64_t)vf_up256((size_t)(P.W * P.H * A.fc));
    }
  }
}

}  // namespace

VF_API int vf_apng_inspect(const unsigned char* data, size_t len, int64_t* info, int64_t* frames, int frame_cap, char* reason,
                           int reason_cap) {
  VF_REQUIRE(data && info && frame_cap >= 0 && (frames || frame_cap == 0), "vf_apng_inspect: NULL argument");
  apngd::Parsed A;
  std::string msg;
  const int rc = apngd::parse(data, (int64_t)len, A, msg);
  if (rc) {
    vf_set_error("vf_apng_inspect: %s", msg.c_str());
    return rc;
  }
  std::string why = A.why;
  for (size_t k = 0; k < A.frames.size() && why.empty(); ++k) {   // what the full rule refuses of a single frame
    PngParsed P;
    PngPasses F;
    apngd_frame_image(A, A.frames[k], P);
    png_rule(P, kFullRule, F);
    if (!F.supported) why = "frame " + std::to_string(k) + ": " + F.why;
  }
  const int64_t v[12] = {A.W, A.H, A.depth, A.ctype, A.lace, A.fc, (int64_t)A.frames.size(), A.num_plays, why.empty() ? 1 : 0,
                         A.animated ? 1 : 0, A.default_is_frame ? 1 : 0, A.nplte};
  memcpy(info, v, sizeof v);
  for (size_t k = 0; k < A.frames.size() && (int64_t)k < frame_cap; ++k) {
    const apngd::Frame& f = A.frames[k];
    const int64_t r[9] = {f.x, f.y, f.w, f.h, f.delay_num, f.delay_den, f.dispose, f.blend, f.data_bytes};
    memcpy(frames + 9 * k, r, sizeof r);
  }
  if (reason && reason_cap > 0) snprintf(reason, (size_t)reason_cap, "%s", why.c_str());
  return 0;
}

VF_API int vf_apng_decode_workspace_bytes(const unsigned char* data, const int64_t* offs, int n, int alpha, size_t* ws_bytes,
                                          size_t* stage_bytes) {
  ApngdPlan L;
  if (int e = apngd_plan("vf_apng_decode_workspace_bytes", data, offs, n, alpha, L)) return e;
  if (ws_bytes) *ws_bytes = L.ws;
  if (stage_bytes) *stage_bytes = L.stage;
  return 0;
}

VF_API int vf_apng_decode(vf_ctx* ctx, const unsigned char* data, const int64_t* offs, int n, int alpha, const int64_t* out_offs,
                          unsigned char* out, void* stage, size_t stage_bytes, void* ws, size_t ws_bytes, int32_t* status) {
  VF_REQUIRE(out && out_offs && stage && ws && status, "vf_apng_decode: NULL argument");
  ApngdPlan L;
  if (int e = apngd_plan("vf_apng_decode", data, offs, n, alpha, L)) return e;
  VF_REQUIRE(stage_bytes >= L.stage && ws_bytes >= L.ws, "vf_apng_decode: staging %zu / workspace %zu bytes, need %zu / %zu", stage_bytes,
             ws_bytes, L.stage, L.ws);
  apngd_pack(data, offs, n, alpha, out_offs, L, (uint8_t*)stage);
  uint8_t* w = (uint8_t*)ws;
  PngdBatch B;
  B.img = (const PngdImage*)(w + L.o_img);
  B.streams = w + L.o_streams;
  B.inf = w + L.o_inf;
  B.raw = w + L.o_raw;
  B.out = w + L.o_px;
  B.status = (int32_t*)(w + L.o_fstatus);
  ApngdBatch Cb;
  Cb.files = (const ApngdFile*)(w + L.o_files);
  Cb.frames = (const ApngdFrame*)(w + L.o_frames);
  Cb.px = w + L.o_px;
  Cb.frame_status = B.status;
  Cb.out = out;
  Cb.status = status;
  if (int e = pngd_run(kFullRule, "apngd_upload", ctx, B, ws, stage, L.stage, (unsigned)L.nframes, L, L.max_fpix)) return e;
  const unsigned gc = (unsigned)std::min<int64_t>(std::max<int64_t>(1, vf_cdiv(L.max_cpix, 256)), 4096);
  double out_bytes = 0;
  for (int i = 0; i < n; ++i) out_bytes += (double)L.A[i].frames.size() * (double)(L.A[i].W * L.A[i].H) * (alpha ? 4 : 3);
  VF_LAUNCH_TIMED(ctx, "apng_compose", 0.0, (double)L.px_bytes + out_bytes, k_apng_compose, dim3(gc, (unsigned)n), dim3(256), Cb);
  VF_LAUNCH_CHECK();
  return 0;
}

VF_API int vf_png_inspect(const unsigned char* data, size_t len, int64_t* info, char* reason, int reason_cap) {
  return png_inspect("vf_png_inspect", kDefaultRule, data, len, info, nullptr, reason, reason_cap);
}

VF_API int vf_png_decode_workspace_bytes(const unsigned char* data, const int64_t* offs, int n, int channels, size_t* ws_bytes,
                                         size_t* stage_bytes) {
  return pngd_query(kDefaultRule, data, offs, n, channels, 0, ws_bytes, stage_bytes);
}

VF_API int vf_png_decode(vf_ctx* ctx, const unsigned char* data, const int64_t* offs, int n, int channels, const int64_t* out_offs,
                         unsigned char* out, void* stage, size_t stage_bytes, void* ws, size_t ws_bytes, int32_t* status) {
  return pngd_decode(kDefaultRule, ctx, data, offs, n, channels, 0, out_offs, out, stage, stage_bytes, ws, ws_bytes, status);
}

VF_API int vf_png_inspect_full(const unsigned char* data, size_t len, int64_t* info, int64_t* passes, char* reason, int reason_cap) {
  return png_inspect("vf_png_inspect_full", kFullRule, data, len, info, passes, reason, reason_cap);
}

VF_API int vf_png_decode_full_workspace_bytes(const unsigned char* data, const int64_t* offs, int n, int channels, int out_kind,
                                              size_t* ws_bytes, size_t* stage_bytes) {
  return pngd_query(kFullRule, data, offs, n, channels, out_kind, ws_bytes, stage_bytes);
}

VF_API int vf_png_decode_full(vf_ctx* ctx, const unsigned char* data, const int64_t* offs, int n, int channels, int out_kind,
                              const int64_t* out_offs, void* out, void* stage, size_t stage_bytes, void* ws, size_t ws_bytes,
                              int32_t* status) {
  return pngd_decode(kFullRule, ctx, data, offs, n, channels, out_kind, out_offs, out, stage, stage_bytes, ws, ws_bytes, status);
}

VF_API int vf_png_bytes_to_float(vf_ctx* ctx, const unsigned char* src, float* dst, int64_t n) {
  VF_REQUIRE(src && dst && n >= 0, "vf_png_bytes_to_float: NULL argument or negative count");
  if (n == 0) return 0;
  const unsigned g = (unsigned)std::min<int64_t>(vf_cdiv(n, 256), 4096);
  VF_LAUNCH_TIMED(ctx, "pngd_to_float", 0.0, 5.0 * (double)n, k_pngd_to_float, dim3(g), dim3(256), src, dst, n);
  VF_LAUNCH_CHECK();
  return 0;
}
