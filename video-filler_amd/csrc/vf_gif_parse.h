// vf_gif_parse.h — the host side of the GIF decoder (vf_gif_decode.hip): the walk of one GIF87a / GIF89a file,
// the plan of a batch and the packing of its one upload.  Plain C++ on untrusted bytes, with no HIP in it, so that it also
// builds into a stand-alone program under the host sanitizers (scripts/gif_parse_sanitize.cpp).  Every read of the file is
// checked against its length first; every write into the staging buffer lies inside the plan's sizes.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace gifd {

constexpr int kMaxSide = 16384;
constexpr int kMaxFrames = 65535;
constexpr int64_t kMaxStream = (int64_t)1 << 28;   // bit positions of one frame's code stream fit 32 bits
constexpr int64_t kMaxRectPix = (int64_t)1 << 28;  // sum of the frame rectangles of one file (the index planes): 256 MiB
constexpr int64_t kMaxCanvas = (int64_t)1 << 31;   // frames x H x W x 4 of one file stay below 2 GiB
constexpr int kTableBytes = 1024;                  // a colour table in the upload: 256 x (r, g, b, 0)

// one frame of the upload; the kernels read it through uniform loads
struct Frame {
  int64_t src;       // first byte of the code stream in the stream section (256-byte aligned, zero-padded behind)
  int64_t idx_off;   // first byte of the frame's w x h indices in the workspace, in the stream's row order
  int32_t slen;      // bytes of the code stream (the sub-blocks without their length bytes)
  int32_t npix;      // w * h
  int32_t x, y, w, h;
  int32_t interlace, disposal;
  int32_t trans;     // transparent index, -1: none
  int32_t table;     // number of the frame's colour table in the table section
  int32_t tsize;     // entries of that table
  int32_t mincode;   // LZW minimum code size, 2 .. 8
  int32_t file;      // the file the frame belongs to
  int32_t pad;
};
static_assert(sizeof(Frame) == 72, "the frame descriptor is shared by the host packer and the kernels");

struct File {
  int64_t out_off;   // first byte of the N x H x W x oc output
  int32_t W, H;
  int32_t first;     // the file's first frame in the frame section
  int32_t nframes;
  int32_t oc;        // 3 or 4
  int32_t pad;
};
static_assert(sizeof(File) == 32, "the file descriptor is shared by the host packer and the kernels");

struct ParsedFrame {
  int x = 0, y = 0, w = 0, h = 0;
  int interlace = 0, disposal = 0, trans = -1, delay = 0;
  int tsize = 0, local = 0, mincode = 0;
  int64_t table_at = 0;                              // first byte of the active table in the file
  int64_t data_bytes = 0;
  std::vector<std::pair<int64_t, int>> blocks;       // (first byte, length) of every non-empty data sub-block
};

struct Parsed {
  int W = 0, H = 0;
  int gsize = 0;                                     // entries of the global table, 0: none
  int loop = -1;
  int version = 0;                                   // 87 or 89
  std::vector<ParsedFrame> frames;
  int64_t rect_pix = 0;
  bool supported = false;
  std::string why;
};

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// 0: parsed (P.supported says whether the decoder takes the file, P.why why not); else malformed (msg)
inline int parse(const uint8_t* d, int64_t n, Parsed& P, std::string& msg) {
  auto bad = [&](const std::string& m) {
    msg = m;
    return 2;
  };
  if (n < 6 || (memcmp(d, "GIF87a", 6) != 0 && memcmp(d, "GIF89a", 6) != 0)) return bad("not a GIF file (bad signature)");
  P.version = d[4] == '7' ? 87 : 89;
  if (n < 13) return bad("truncated logical screen descriptor");
  P.W = d[6] | (d[7] << 8);
  P.H = d[8] | (d[9] << 8);
  if (P.W < 1 || P.H < 1) return bad("logical screen of " + std::to_string(P.W) + " x " + std::to_string(P.H));
  int64_t pos = 13, gtable = 0;
  if (d[10] & 0x80) {
    P.gsize = 2 << (d[10] & 7);
    gtable = pos;
    pos += 3 * P.gsize;
    if (pos > n) return bad("truncated global colour table");
  }
  // skips the sub-blocks at pos; false: they run past the end of the file
  auto skip_blocks = [&](ParsedFrame* f) {
    for (;;) {
      if (pos >= n) return false;
      const int L = d[pos++];
      if (L == 0) return true;
      if (pos + L > n) return false;
      if (f) {
        f->blocks.push_back({pos, L});
        f->data_bytes += L;
      }
      pos += L;
    }
  };
  int disposal = 0, trans = -1, delay = 0;            // of the graphic control extension in front of the next image
  bool trailer = false;
  while (pos < n) {
    const int b = d[pos++];
    if (b == 0x3B) {
      trailer = true;
      break;
    }
    if (b == 0x21) {
      if (pos >= n) return bad("truncated extension at byte " + std::to_string(pos - 1));
      const int label = d[pos++];
      if (label == 0xF9 && pos + 6 <= n && d[pos] == 4 && d[pos + 5] == 0) {
        disposal = (d[pos + 1] >> 2) & 7;
        trans = (d[pos + 1] & 1) ? d[pos + 4] : -1;
        delay = d[pos + 2] | (d[pos + 3] << 8);
        pos += 6;
        continue;
      }
      if (label == 0xFF && pos + 12 <= n && d[pos] == 11 && memcmp(d + pos + 1, "NETSCAPE2.0", 11) == 0 && pos + 16 <= n &&
          d[pos + 12] == 3 && d[pos + 13] == 1) {
        P.loop = d[pos + 14] | (d[pos + 15] << 8);
      }
      if (!skip_blocks(nullptr)) return bad("extension with label " + std::to_string(label) + " runs past the end of the file");
      continue;
    }
    if (b != 0x2C) return bad("unknown block introducer " + std::to_string(b) + " at byte " + std::to_string(pos - 1));
    if (pos + 9 > n) return bad("truncated image descriptor at byte " + std::to_string(pos - 1));
    ParsedFrame f;
    f.x = d[pos] | (d[pos + 1] << 8);
    f.y = d[pos + 2] | (d[pos + 3] << 8);
    f.w = d[pos + 4] | (d[pos + 5] << 8);
    f.h = d[pos + 6] | (d[pos + 7] << 8);
    const int packed = d[pos + 8];
    pos += 9;
    const std::string who = "frame " + std::to_string(P.frames.size());
    if (f.w < 1 || f.h < 1 || f.x + f.w > P.W || f.y + f.h > P.H)
      return bad(who + ": rectangle " + std::to_string(f.w) + " x " + std::to_string(f.h) + " at (" + std::to_string(f.x) + ", " +
                 std::to_string(f.y) + ") leaves the " + std::to_string(P.W) + " x " + std::to_string(P.H) + " screen");
    f.interlace = (packed >> 6) & 1;
    if (packed & 0x80) {
      f.local = 1;
      f.tsize = 2 << (packed & 7);
      f.table_at = pos;
      pos += 3 * f.tsize;
      if (pos > n) return bad(who + ": truncated local colour table");
    } else if (P.gsize) {
      f.tsize = P.gsize;
      f.table_at = gtable;
    } else {
      return bad(who + ": no local colour table and no global one");
    }
    if (pos >= n) return bad(who + ": no image data");
    f.mincode = d[pos++];
    if (f.mincode < 2 || f.mincode > 8) return bad(who + ": LZW minimum code size " + std::to_string(f.mincode) + " (2 to 8)");
    if (!skip_blocks(&f)) return bad(who + ": image data runs past the end of the file");
    f.disposal = disposal;
    f.trans = trans;
    f.delay = delay;
    disposal = 0;
    trans = -1;
    delay = 0;
    P.rect_pix += (int64_t)f.w * f.h;
    if (P.frames.size() < (size_t)kMaxFrames + 1) P.frames.push_back(std::move(f));   // one past the limit shows it is passed
    else P.frames.back() = std::move(f);
  }
  if (!trailer) return bad("no trailer");
  if (P.frames.empty()) return bad("no frame");
  auto unsupported = [&](const std::string& w) {
    if (P.why.empty()) P.why = w;
  };
  if (P.W > kMaxSide || P.H > kMaxSide) unsupported("larger than 16384 per side");
  if ((int)P.frames.size() > kMaxFrames) unsupported("more than 65535 frames");
  if ((int64_t)P.frames.size() * P.W * P.H * 4 >= kMaxCanvas) unsupported("decoded frames of 2 GiB or more");
  if (P.rect_pix > kMaxRectPix) unsupported("frame rectangles above 256 Mi pixels");
  for (const ParsedFrame& f : P.frames)
    if (f.data_bytes > kMaxStream) unsupported("a frame's image data above 256 MiB");
  P.supported = P.why.empty();
  return 0;
}

struct Plan {
  std::vector<Parsed> P;
  int64_t nframes = 0, stream_bytes = 0, idx_bytes = 0, max_pix = 0, out_bytes = 0;
  size_t o_files = 0, o_frames = 0, o_tables = 0, o_streams = 0, stage = 0, o_idx = 0, ws = 0;
};

// 0: planned; 2: malformed or bad arguments; 3: unsupported (msg names the image)
inline int plan(const uint8_t* data, const int64_t* offs, int n, int alpha, Plan& L, std::string& msg) {
  auto bad = [&](const std::string& m) {
    msg = m;
    return 2;
  };
  if (n <= 0 || !data || !offs) return bad("empty batch");
  if (n > 65535) return bad(std::to_string(n) + " files in one batch (65535 at most)");
  if (alpha != 0 && alpha != 1) return bad("alpha " + std::to_string(alpha) + " is not 0 (RGB) or 1 (RGBA)");
  L.P.resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    if (offs[i + 1] < offs[i]) return bad("offsets decrease at image " + std::to_string(i));
    Parsed& P = L.P[(size_t)i];
    std::string m;
    if (parse(data + offs[i], offs[i + 1] - offs[i], P, m)) return bad("image " + std::to_string(i) + ": " + m);
    if (!P.supported) {
      msg = "image " + std::to_string(i) + ": unsupported: " + P.why;
      return 3;
    }
    L.nframes += (int64_t)P.frames.size();
    for (const ParsedFrame& f : P.frames) {
      L.stream_bytes += (int64_t)up256((size_t)f.data_bytes + 8);
      L.idx_bytes += (int64_t)up256((size_t)f.w * f.h);
    }
    L.max_pix = std::max(L.max_pix, (int64_t)P.W * P.H);
    L.out_bytes += (int64_t)P.frames.size() * P.W * P.H * (alpha ? 4 : 3);
  }
  if (L.nframes > ((int64_t)1 << 24)) return bad(std::to_string(L.nframes) + " frames in one batch (16777216 at most)");
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += up256(bytes);
    return o;
  };
  L.o_files = take(sizeof(File) * (size_t)n);
  L.o_frames = take(sizeof(Frame) * (size_t)L.nframes);
  L.o_tables = take((size_t)kTableBytes * (size_t)L.nframes);
  L.o_streams = take((size_t)L.stream_bytes);
  L.stage = at;
  L.o_idx = take((size_t)L.idx_bytes);
  L.ws = at;
  return 0;
}

// the upload: file and frame descriptors, one table per frame, every frame's sub-blocks behind one another
inline void pack(const uint8_t* data, const int64_t* offs, int n, int alpha, const int64_t* out_offs, const Plan& L, uint8_t* st) {
  File* files = (File*)(st + L.o_files);
  Frame* frames = (Frame*)(st + L.o_frames);
  uint8_t* tables = st + L.o_tables;
  uint8_t* streams = st + L.o_streams;
  int64_t sc = 0, ix = 0;
  int32_t k = 0;
  for (int i = 0; i < n; ++i) {
    const Parsed& P = L.P[(size_t)i];
    const uint8_t* d = data + offs[i];
    File& fl = files[i];
    memset(&fl, 0, sizeof(fl));
    fl.out_off = out_offs[i];
    fl.W = P.W;
    fl.H = P.H;
    fl.first = k;
    fl.nframes = (int32_t)P.frames.size();
    fl.oc = alpha ? 4 : 3;
    for (const ParsedFrame& f : P.frames) {
      Frame& fr = frames[k];
      memset(&fr, 0, sizeof(fr));
      fr.src = sc;
      fr.idx_off = ix;
      fr.slen = (int32_t)f.data_bytes;
      fr.npix = f.w * f.h;
      fr.x = f.x;
      fr.y = f.y;
      fr.w = f.w;
      fr.h = f.h;
      fr.interlace = f.interlace;
      fr.disposal = f.disposal;
      fr.trans = f.trans;
      fr.table = k;
      fr.tsize = f.tsize;
      fr.mincode = f.mincode;
      fr.file = i;
      uint8_t* t = tables + (size_t)k * kTableBytes;
      memset(t, 0, kTableBytes);
      for (int e = 0; e < f.tsize; ++e) memcpy(t + 4 * e, d + f.table_at + 3 * e, 3);
      int64_t at = 0;
      for (const auto& b : f.blocks) {
        memcpy(streams + sc + at, d + b.first, (size_t)b.second);
        at += b.second;
      }
      const int64_t room = (int64_t)up256((size_t)f.data_bytes + 8);
      memset(streams + sc + at, 0, (size_t)(room - at));
      sc += room;
      ix += (int64_t)up256((size_t)f.w * f.h);
      ++k;
    }
  }
}

}  // namespace gifd
