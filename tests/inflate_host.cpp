// inflate_host -- the host build of the BGZF decoder (csrc/inflate_core.h, inflate_host.h) as a program of
// its own, for tests/test_inflate_host.py (built there under AddressSanitizer + UndefinedBehaviorSanitizer).
//   inflate_host IN OUT     IN: u32 count, then per case u32 size and that many bytes, a concatenation of
//                           BGZF members.  OUT, per case: u8 kind, then
//                             kind 0  u64 length and the inflated bytes
//                             kind 1  the member walk refused the input: u32 length and the message
//                             kind 2  the decoder refused a member: u32 member index, u32 status word
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "inflate_host.h"

static std::vector<uint8_t> slurp(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  std::vector<uint8_t> v;
  uint8_t buf[1 << 16];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
  fclose(f);
  return v;
}

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: inflate_host IN OUT\n");
    return 2;
  }
  const std::vector<uint8_t> in = slurp(argv[1]);
  FILE *o = fopen(argv[2], "wb");
  if (!o) return 2;
  size_t at = 0;
  auto u32 = [&]() {
    uint32_t v = 0;
    if (at + 4 > in.size()) exit(2);
    memcpy(&v, in.data() + at, 4);
    at += 4;
    return v;
  };
  const uint32_t cases = u32();
  for (uint32_t c = 0; c < cases; ++c) {
    const uint32_t size = u32();
    if (at + size > in.size()) return 2;
    // (an exact-size copy: reads past the input's end are the sanitizer's to find)
    std::vector<uint8_t> exact(in.begin() + (long)at, in.begin() + (long)(at + size));
    at += size;
    std::vector<gwa::inflate::Member> ms;
    std::vector<uint64_t> offs;
    uint64_t total = 0;
    try {
      total = gwa::inflate::walkMembers(exact.data(), exact.size(), ms, offs);
    } catch (std::exception &e) {
      const uint8_t kind = 1;
      const uint32_t n = (uint32_t)strlen(e.what());
      fwrite(&kind, 1, 1, o);
      fwrite(&n, 4, 1, o);
      fwrite(e.what(), 1, n, o);
      continue;
    }
    std::vector<uint8_t> text(total);  // (exactly the members' ISIZEs: a store past them is the sanitizer's to find)
    std::vector<uint32_t> status(ms.size() + 1);
    const uint64_t bad = gwa::inflate::inflateHost(exact.data(), exact.size(), ms.data(), ms.size(), text.data(), total, status.data());
    if (bad < ms.size()) {
      const uint8_t kind = 2;
      const uint32_t idx = (uint32_t)bad;
      fwrite(&kind, 1, 1, o);
      fwrite(&idx, 4, 1, o);
      fwrite(&status[bad], 4, 1, o);
    } else {
      const uint8_t kind = 0;
      fwrite(&kind, 1, 1, o);
      fwrite(&total, 8, 1, o);
      if (total) fwrite(text.data(), 1, total, o);
    }
  }
  fclose(o);
  return 0;
}
