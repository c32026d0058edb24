// vf_apng_parse.h — the host-side chunk walk of the animated-PNG decoder (vf_png_decode.hip): the CRCs, IHDR,
// PLTE / tRNS, acTL, the sequence numbers of fcTL and fdAT, every frame's geometry and the payload segments that make its zlib
// stream.  Host only and standard C++ only, so that scripts/apng_parse_sanitize.cpp can build a stand-alone program around it.
// Every read is bounded by the length given: a chunk is looked at only once its 12 + length bytes are known to be inside.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace apngd {

constexpr int64_t kMaxSide = 16384;
constexpr int64_t kMaxFrames = 65535;

struct Frame {
  int64_t x = 0, y = 0, w = 0, h = 0;
  int delay_num = 0, delay_den = 0, dispose = 0, blend = 0;
  int64_t data_bytes = 0;                            // of the frame's zlib stream
  std::vector<std::pair<int64_t, int64_t>> seg;      // (first byte in the file, length) of every non-empty piece of it
};

struct Parsed {
  int64_t W = 0, H = 0;
  int depth = 0, ctype = 0, lace = 0;
  int rc = 0;                  // samples per pixel in the rows
  int fc = 0;                  // channels after expansion: 1 grey, 2 grey + alpha, 3 RGB, 4 RGBA
  int nplte = 0, ntrns = 0;
  bool has_plte = false, has_trns = false;
  uint8_t plte[768] = {}, trns[256] = {};
  bool animated = false;       // an acTL chunk: otherwise the file is a clip of one frame, the image
  bool default_is_frame = true;   // the IDAT image is frame 0 (an fcTL precedes it, or the file is not animated)
  int64_t num_plays = -1;      // -1 without acTL
  std::vector<Frame> frames;
  bool supported = false;
  std::string why;
};

inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

inline uint32_t crc32(const uint8_t* p, size_t n) {
  static uint32_t t[256];
  static bool made = false;
  if (!made) {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
      t[i] = c;
    }
    made = true;
  }
  uint32_t c = 0xFFFFFFFFu;
  while (n--) c = t[(c ^ *p++) & 255] ^ (c >> 8);
  return ~c;
}

// 0: parsed (P.supported says whether the device decoder takes the file, P.why why not); else malformed (msg)
inline int parse(const uint8_t* d, int64_t n, Parsed& P, std::string& msg) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  auto bad = [&](const std::string& m) {
    msg = m;
    return 2;
  };
  auto at = [](int64_t pos) { return " at byte " + std::to_string(pos); };
  if (n < 8 || memcmp(d, sig, 8) != 0) return bad("not a PNG file (bad signature)");
  int64_t pos = 8, num_frames = 0, fctls = 0, next_seq = 0;
  int64_t idat_frame = -1;                           // the frame whose data the IDAT chunks are
  bool first = true, seen_idat = false, idat_done = false, iend = false, in_idat_frame = false, over = false;
  Frame idat_image;                                  // the IDAT payloads, whether they are a frame or not
  while (pos < n) {
    if (pos + 12 > n) return bad("truncated chunk header" + at(pos));
    const int64_t L = be32(d + pos);
    const uint8_t* ty = d + pos + 4;
    const std::string name((const char*)ty, 4);
    if (pos + 12 + L > n) return bad("chunk " + name + at(pos) + " runs past the end of the file");
    const uint8_t* body = d + pos + 8;
    const bool is_ihdr = name == "IHDR", is_plte = name == "PLTE", is_idat = name == "IDAT", is_iend = name == "IEND",
               is_trns = name == "tRNS", is_actl = name == "acTL", is_fctl = name == "fcTL", is_fdat = name == "fdAT";
    if (first != is_ihdr) return bad(first ? "IHDR is not the first chunk" : "more than one IHDR");
    if ((is_ihdr || is_plte || is_idat || is_iend || is_trns || is_actl || is_fctl || is_fdat) && crc32(ty, (size_t)L + 4) != be32(body + L))
      return bad("wrong CRC on chunk " + name + at(pos));
    if (seen_idat && !is_idat) idat_done = true;
    if (is_ihdr) {
      if (L != 13) return bad("IHDR of " + std::to_string(L) + " bytes");
      P.W = be32(body);
      P.H = be32(body + 4);
      P.depth = body[8];
      P.ctype = body[9];
      P.lace = body[12];
      const int dp = P.depth, ct = P.ctype;
      const bool depth_ok = dp == 1 || dp == 2 || dp == 4 || dp == 8 || dp == 16;
      const bool combo = depth_ok && (ct == 0 || (ct == 3 && dp <= 8) || ((ct == 2 || ct == 4 || ct == 6) && dp >= 8));
      if (P.W < 1 || P.H < 1 || P.W > 0x7fffffff || P.H > 0x7fffffff || !combo || body[10] != 0 || body[11] != 0 || P.lace > 1)
        return bad("illegal IHDR: " + std::to_string(P.W) + "x" + std::to_string(P.H) + ", bit depth " + std::to_string(dp) +
                   ", colour type " + std::to_string(ct) + ", compression " + std::to_string(body[10]) + ", filter " +
                   std::to_string(body[11]) + ", interlace " + std::to_string(P.lace));
      P.rc = ct == 0 || ct == 3 ? 1 : ct == 2 ? 3 : ct == 4 ? 2 : 4;
      first = false;
    } else if (is_plte) {
      if (seen_idat) return bad("PLTE after IDAT");
      if (P.has_plte || L == 0 || L % 3 != 0 || L > 768 || P.ctype == 0 || P.ctype == 4 || (P.ctype == 3 && L / 3 > (1 << P.depth)))
        return bad("illegal PLTE (" + std::to_string(L) + " bytes, colour type " + std::to_string(P.ctype) + ")");
      P.has_plte = true;
      P.nplte = (int)(L / 3);
      memcpy(P.plte, body, (size_t)L);
    } else if (is_trns) {
      const bool ok = !seen_idat && !P.has_trns &&
                      ((P.ctype == 3 && P.has_plte && L >= 1 && L <= P.nplte) || (P.ctype == 0 && L == 2) || (P.ctype == 2 && L == 6));
      if (!ok) return bad("illegal tRNS (" + std::to_string(L) + " bytes, colour type " + std::to_string(P.ctype) + ")");
      P.has_trns = true;
      P.ntrns = P.ctype == 3 ? (int)L : 1;
      if (P.ctype == 3) memcpy(P.trns, body, (size_t)L);
    } else if (is_actl) {
      if (P.animated) return bad("a second acTL" + at(pos));
      if (seen_idat) return bad("acTL after IDAT" + at(pos));
      if (L != 8) return bad("acTL of " + std::to_string(L) + " bytes");
      P.animated = true;
      num_frames = be32(body);
      P.num_plays = be32(body + 4);
      if (num_frames == 0) return bad("acTL: num_frames is 0");
    } else if (is_fctl && P.animated) {
      if (L != 26) return bad("fcTL of " + std::to_string(L) + " bytes");
      if (be32(body) != next_seq)
        return bad("fcTL" + at(pos) + " has sequence number " + std::to_string(be32(body)) + ", " + std::to_string(next_seq) + " is due");
      ++next_seq;
      if (idat_frame >= 0 && !seen_idat) return bad("two fcTL chunks in front of IDAT");
      Frame f;
      f.w = be32(body + 4);
      f.h = be32(body + 8);
      f.x = be32(body + 12);
      f.y = be32(body + 16);
      f.delay_num = (body[20] << 8) | body[21];
      f.delay_den = (body[22] << 8) | body[23];
      f.dispose = body[24];
      f.blend = body[25];
      const std::string who = "frame " + std::to_string(fctls);
      if (f.w == 0 || f.h == 0) return bad(who + " is " + std::to_string(f.w) + "x" + std::to_string(f.h));
      if (f.x + f.w > P.W || f.y + f.h > P.H)
        return bad(who + ": " + std::to_string(f.w) + "x" + std::to_string(f.h) + " at (" + std::to_string(f.x) + "," + std::to_string(f.y) +
                   ") leaves the " + std::to_string(P.W) + "x" + std::to_string(P.H) + " canvas");
      if (f.dispose > 2) return bad(who + ": dispose " + std::to_string(f.dispose));
      if (f.blend > 1) return bad(who + ": blend " + std::to_string(f.blend));
      if (!seen_idat) {
        if (f.x != 0 || f.y != 0 || f.w != P.W || f.h != P.H) return bad("the fcTL in front of IDAT is not the whole canvas at (0,0)");
        idat_frame = fctls;                            // 0: an earlier one was refused above
      }
      in_idat_frame = !seen_idat;
      if (f.blend == 1) over = true;
      ++fctls;
      if ((int64_t)P.frames.size() < kMaxFrames + 1) P.frames.push_back(f);   // counted beyond; refused below
    } else if (is_fdat && P.animated) {
      if (fctls == 0) return bad("fdAT" + at(pos) + " before the first fcTL");
      if (L < 4) return bad("fdAT of " + std::to_string(L) + " bytes" + at(pos));
      if (be32(body) != next_seq)
        return bad("fdAT" + at(pos) + " has sequence number " + std::to_string(be32(body)) + ", " + std::to_string(next_seq) + " is due");
      ++next_seq;
      if (in_idat_frame) return bad("fdAT" + at(pos) + " in the frame that the IDAT chunks hold");
      if (fctls == (int64_t)P.frames.size()) {
        Frame& f = P.frames.back();
        f.data_bytes += L - 4;
        if (L > 4) f.seg.push_back({pos + 12, L - 4});
      }
    } else if (is_idat) {
      if (idat_done) return bad("IDAT chunks are not consecutive");
      if (P.ctype == 3 && !P.has_plte) return bad("no PLTE before IDAT for colour type 3");
      seen_idat = true;
      idat_image.data_bytes += L;
      if (L) idat_image.seg.push_back({pos + 8, L});
    } else if (is_iend) {
      if (L != 0) return bad("IEND of " + std::to_string(L) + " bytes");
      iend = true;
      break;
    } else if (!(ty[0] & 0x20)) {
      return bad("unknown critical chunk " + name);
    }
    pos += 12 + L;
  }
  if (first) return bad("no IHDR");
  if (!iend) return bad("no IEND chunk");
  if (!seen_idat) return bad("no IDAT chunk");
  if (!P.animated) {
    Frame f = idat_image;
    f.w = P.W;
    f.h = P.H;
    P.frames.assign(1, f);
  } else {
    if (fctls != num_frames) return bad(std::to_string(fctls) + " fcTL chunks, acTL says " + std::to_string(num_frames) + " frames");
    P.default_is_frame = idat_frame == 0;
    if (idat_frame == 0) {
      P.frames[0].data_bytes = idat_image.data_bytes;
      P.frames[0].seg = idat_image.seg;
    }
  }
  // every frame is a zlib stream of its own: deflate, a window of at most 32 KiB, no preset dictionary, FCHECK
  for (size_t k = 0; k < P.frames.size(); ++k) {
    const Frame& f = P.frames[k];
    const std::string who = "frame " + std::to_string(k);
    if (f.data_bytes == 0) return bad(who + " has no data");
    int z[2], m = 0;
    for (const auto& c : f.seg)
      for (int64_t i = 0; i < c.second && m < 2; ++i) z[m++] = d[c.first + i];
    if (m < 2) return bad(who + ": zlib header: the data is " + std::to_string(f.data_bytes) + " bytes");
    if ((z[0] & 15) != 8 || (z[0] >> 4) > 7 || (z[1] & 0x20) || (z[0] * 256 + z[1]) % 31 != 0) {
      char b[112];
      snprintf(b, sizeof b, ": bad zlib header %02x %02x (deflate, window <= 32 KiB, no dictionary, FCHECK)", z[0], z[1]);
      return bad(who + b);
    }
  }
  P.fc = P.ctype == 3 ? (P.has_trns ? 4 : 3) : P.rc + ((P.ctype == 0 || P.ctype == 2) && P.has_trns ? 1 : 0);
  auto unsupported = [&](const std::string& w) {
    if (P.why.empty()) P.why = w;
  };
  if (P.has_trns && P.ctype != 3) unsupported("tRNS on colour type " + std::to_string(P.ctype) + " (alpha from a colour key)");
  if (over && (P.ctype == 4 || P.ctype == 6 || P.has_trns)) unsupported("blend OVER in a file that carries alpha");
  if (P.W > kMaxSide || P.H > kMaxSide) unsupported("larger than 16384 per side");
  else if (fctls > kMaxFrames) unsupported("more than 65535 frames");
  else if ((int64_t)P.frames.size() * P.W * P.H * 4 >= ((int64_t)1 << 31)) unsupported("2 GiB or more of RGBA frames");
  P.supported = P.why.empty();
  return 0;
}

}  // namespace apngd
