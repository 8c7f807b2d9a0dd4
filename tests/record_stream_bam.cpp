// record_stream_bam.cpp -- stand-alone driver of the pipeline's HIP-free reader (csrc/record_stream.cpp) for
// the BAM cases of tests/test_record_stream_bam.py, which compiles it with the address and
// undefined-behaviour sanitizers together with record_stream.cpp, reads_io.cpp and snappy_stream.cpp.  No
// inflater is passed, so the BGZF members are inflated by the host build of the decoder.
//
//   record_stream_bam CHUNK_BYTES BATCH single PATH
//   record_stream_bam CHUNK_BYTES BATCH pair PATH1 PATH2
//   record_stream_bam CHUNK_BYTES BATCH inter PATH
//
// Prints "K <kind of each stream>" (3 = BGZF) and "F <format of each stream>", then one line per slice or
// pair batch: "B <records or pairs>" and per slice " <format> <recIndex> <byteOff> <len> x<hex> <starts>".
// An error prints "E <message>" and exits with status 3.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <string>

#include "../genome-weaver-align_amd/csrc/record_stream.h"

static std::string g_err;
extern "C" int gwa_fail_message(const char *msg) {  // (reads_io.cpp reports through it)
  g_err = msg;
  return -1;
}

static void show(const gwa::RecordSlice &s) {
  if (!s.buf) {
    printf(" - 0 0 0 x -");
    return;
  }
  printf(" %d %llu %llu %llu x", s.format, (unsigned long long)s.recIndex, (unsigned long long)s.byteOff,
         (unsigned long long)(s.te - s.tb));
  for (uint64_t i = s.tb; i < s.te; ++i) printf("%02x", (unsigned char)s.buf->p[i]);
  printf(" ");
  if (s.starts.empty()) printf("-");
  for (size_t i = 0; i < s.starts.size(); ++i) printf(i ? ",%llu" : "%llu", (unsigned long long)s.starts[i]);
}

int main(int argc, char **argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: record_stream_bam CHUNK_BYTES BATCH single|pair|inter PATH1 [PATH2]\n");
    return 2;
  }
  setenv("GWA_PIPE_CHUNK", argv[1], 1);
  const uint64_t batch = strtoull(argv[2], nullptr, 10);
  const std::string mode = argv[3];
  auto alloc = [](size_t cap) {
    auto *b = new gwa::TextBuf();
    b->p = (char *)malloc(cap ? cap : 1);
    b->cap = cap;
    return std::shared_ptr<gwa::TextBuf>(b, [](gwa::TextBuf *x) {
      free(x->p);
      delete x;
    });
  };
  try {
    if (mode == "single") {
      gwa::RecordStream rs(argv[4], 0, ~0ull, batch, alloc);
      printf("K %d\nF %d\n", rs.bgzf() ? 3 : 0, rs.format());
      gwa::RecordSlice s;
      while (rs.next(&s)) {
        printf("B %llu", (unsigned long long)s.n);
        show(s);
        printf("\n");
      }
    } else {
      gwa::PairedRecordStream prs(argv[4], mode == "pair" && argc > 5 ? argv[5] : nullptr, batch, alloc);
      printf("K");
      for (gwa::RecordStream *r : prs.streams()) printf(" %d", r->bgzf() ? 3 : 0);
      printf("\nF");
      for (gwa::RecordStream *r : prs.streams()) printf(" %d", r->format());
      printf("\n");
      gwa::RecordSlice m1, m2;
      uint64_t pairs = 0;
      while (prs.next(&m1, &m2, &pairs)) {
        printf("B %llu", (unsigned long long)pairs);
        show(m1);
        show(m2);
        printf("\n");
      }
    }
  } catch (std::exception &e) {
    printf("E %s\n", e.what());
    return 3;
  }
  return 0;
}
