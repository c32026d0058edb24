// gif_parse_sanitize.cpp — the GIF decoder's host side (csrc/vf_gif_parse.h: the file walk, the batch plan and the packing of
// the upload) as a stand-alone program for the host sanitizers.  scripts/gif_parse_sanitize.py builds it with
// -fsanitize=address,undefined and feeds it the fixtures of tests/gif_decode_cases.py.
// For every file named on the command line: the whole file, then the file cut at every byte offset, each copy in a heap block
// of exactly its size (a read past the end is a report) — parse it; when it parses and is supported, plan it alone and in a
// batch of two, and pack the upload into a block of exactly the planned size (a write past the plan is a report).
#include <cstdio>
#include <cstdlib>

#include "../video-filler_amd/csrc/vf_gif_parse.h"

static long g_parsed = 0, g_malformed = 0, g_unsupported = 0, g_packed = 0;

static void feed(const uint8_t* src, size_t n) {
  uint8_t* d = (uint8_t*)malloc(n ? n : 1);
  memcpy(d, src, n);
  gifd::Parsed P;
  std::string msg;
  if (gifd::parse(d, (int64_t)n, P, msg)) {
    ++g_malformed;
    if (msg.empty()) {
      fprintf(stderr, "a malformed file without a message\n");
      exit(2);
    }
  } else {
    ++g_parsed;
    if (!P.supported) ++g_unsupported;
  }
  // the batch entry's path: this file alone, and twice in one batch, RGB and RGBA
  uint8_t* two = (uint8_t*)malloc(2 * n ? 2 * n : 1);
  memcpy(two, d, n);
  memcpy(two + n, d, n);
  const int64_t offs[3] = {0, (int64_t)n, (int64_t)(2 * n)};
  for (int count = 1; count <= 2; ++count)
    for (int alpha = 0; alpha <= 1; ++alpha) {
      gifd::Plan L;
      if (gifd::plan(two, offs, count, alpha, L, msg)) continue;
      uint8_t* stage = (uint8_t*)malloc(L.stage);
      const int64_t out_offs[2] = {0, L.out_bytes / count};
      gifd::pack(two, offs, count, alpha, out_offs, L, stage);
      // what the kernels rely on: every stream lies inside the stream section with its padding, every plane inside the workspace
      const gifd::Frame* fr = (const gifd::Frame*)(stage + L.o_frames);
      for (int64_t k = 0; k < L.nframes; ++k) {
        const bool ok = fr[k].src >= 0 && fr[k].src + (int64_t)gifd::up256((size_t)fr[k].slen + 8) <= L.stream_bytes &&
                        fr[k].idx_off >= 0 && fr[k].idx_off + fr[k].npix <= L.idx_bytes && fr[k].npix == fr[k].w * fr[k].h &&
                        fr[k].mincode >= 2 && fr[k].mincode <= 8 && fr[k].tsize >= 2 && fr[k].tsize <= 256 && fr[k].file < count;
        if (!ok) {
          fprintf(stderr, "frame %lld of the plan breaks a bound\n", (long long)k);
          exit(2);
        }
      }
      ++g_packed;
      free(stage);
    }
  free(two);
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
    for (size_t cut = 0; cut < buf.size(); ++cut) feed(buf.data(), cut);
  }
  printf("%d files: %ld inputs parsed (%ld unsupported), %ld malformed, %ld uploads packed\n", argc - 1, g_parsed, g_unsupported,
         g_malformed, g_packed);
  return 0;
}
