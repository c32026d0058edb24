// apng_parse_sanitize.cpp — the APNG decoder's host-side chunk walk (csrc/vf_apng_parse.h) as a stand-alone program for the
// host sanitizers.  scripts/apng_parse_sanitize.py builds it with -fsanitize=address,undefined and feeds it the fixtures of
// tests/apng_cases.py.
// For every file named on the command line: the whole file, then the file cut at every byte offset, each copy in a heap block
// of exactly its size (a read past the end is a report) — parse it; when it parses, check what the batch plan and the kernels
// rely on: every frame lies inside the canvas, every payload segment inside the file, the segments add up to data_bytes.
#include <cstdio>
#include <cstdlib>

#include "../video-filler_amd/csrc/vf_apng_parse.h"

static long g_parsed = 0, g_malformed = 0, g_unsupported = 0, g_frames = 0;

static void feed(const uint8_t* src, size_t n) {
  uint8_t* d = (uint8_t*)malloc(n ? n : 1);
  memcpy(d, src, n);
  apngd::Parsed P;
  std::string msg;
  if (apngd::parse(d, (int64_t)n, P, msg)) {
    ++g_malformed;
    if (msg.empty()) {
      fprintf(stderr, "a malformed file without a message\n");
      exit(2);
    }
  } else {
    ++g_parsed;
    if (!P.supported) {
      ++g_unsupported;
      if (P.why.empty()) {
        fprintf(stderr, "an unsupported file without a reason\n");
        exit(2);
      }
    }
    bool ok = !P.frames.empty() && P.fc >= 1 && P.fc <= 4;
    unsigned sum = 0;
    for (const apngd::Frame& f : P.frames) {
      int64_t bytes = 0;
      ok = ok && f.w >= 1 && f.h >= 1 && f.x >= 0 && f.y >= 0 && f.x + f.w <= P.W && f.y + f.h <= P.H && f.dispose <= 2 && f.blend <= 1;
      for (const auto& s : f.seg) {
        ok = ok && s.first >= 8 && s.second >= 1 && s.first + s.second <= (int64_t)n;
        if (ok)
          for (int64_t i = 0; i < s.second; ++i) sum += d[s.first + i];       // every byte the packer would copy
        bytes += s.second;
      }
      ok = ok && bytes == f.data_bytes && bytes >= 2;
      ++g_frames;
    }
    if (!ok) {
      fprintf(stderr, "a parsed file breaks a bound (checksum %u)\n", sum);
      exit(2);
    }
  }
  free(d);
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    FILE* fh = fopen(argv[i], "rb");
    if (!fh) {
      fprintf(stderr, "cannot open %s\n", argv[i]);
      return 2;
    }
    std::vector<uint8_t> buf;
    uint8_t tmp[4096];
    size_t got;
    while ((got = fread(tmp, 1, sizeof tmp, fh)) > 0) buf.insert(buf.end(), tmp, tmp + got);
    fclose(fh);
    feed(buf.data(), buf.size());
    // a file above 16 KiB (tens of thousands of chunks in one fixture) is cut at every offset of its first and last 4096 bytes only
    const size_t lim = 16384;
    for (size_t cut = 0; cut < buf.size(); ++cut)
      if (buf.size() <= lim || cut < 4096 || cut + 4096 >= buf.size()) feed(buf.data(), cut);
  }
  printf("%d files: %ld inputs parsed (%ld unsupported, %ld frames), %ld malformed\n", argc - 1, g_parsed, g_unsupported, g_frames,
         g_malformed);
  return 0;
}
