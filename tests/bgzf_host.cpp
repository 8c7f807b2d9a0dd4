// bgzf_host -- the host build of the BGZF encoder (csrc/bgzf_core.h, bgzf_host.h) as a program of its
// own, for tests/test_bgzf_host.py (built there under AddressSanitizer + UndefinedBehaviorSanitizer).
//   bgzf_host IN OUT          the BGZF blocks of file IN into OUT; "blocks stored" on stdout
//   bgzf_host -p N IN OUT     for every L in 0..N: u32 size, then the blocks of IN[0, L), into OUT
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bgzf_host.h"

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
  int prefixes = -1, a = 1;
  if (argc > 2 && !strcmp(argv[1], "-p")) {
    prefixes = atoi(argv[2]);
    a = 3;
  }
  if (argc - a != 2) {
    fprintf(stderr, "usage: bgzf_host [-p N] IN OUT\n");
    return 2;
  }
  const std::vector<uint8_t> in = slurp(argv[a]);
  FILE *o = fopen(argv[a + 1], "wb");
  if (!o) return 2;
  gwa::bgzf::HostStats st;
  if (prefixes < 0) {
    std::vector<uint8_t> out;
    // (an exact-size copy: reads past the input's end are the sanitizer's to find)
    std::vector<uint8_t> exact(in.begin(), in.end());
    gwa::bgzf::compressHost(exact.data(), exact.size(), out, &st);
    if (!out.empty()) fwrite(out.data(), 1, out.size(), o);
  } else {
    for (int len = 0; len <= prefixes && (size_t)len <= in.size(); ++len) {
      std::vector<uint8_t> exact(in.begin(), in.begin() + len), out;
      gwa::bgzf::compressHost(exact.data(), exact.size(), out, &st);
      const uint32_t n = (uint32_t)out.size();
      fwrite(&n, 4, 1, o);
      if (!out.empty()) fwrite(out.data(), 1, out.size(), o);
    }
  }
  fclose(o);
  printf("%llu %llu\n", (unsigned long long)st.blocks, (unsigned long long)st.stored);
  return 0;
}
