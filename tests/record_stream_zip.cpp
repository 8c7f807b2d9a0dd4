// record_stream_zip.cpp -- stand-alone driver of the pipeline's HIP-free reader (csrc/record_stream.cpp)
// for tests/test_record_stream.py, which compiles it with the address and undefined-behaviour
// sanitizers together with record_stream.cpp, reads_io.cpp and snappy_stream.cpp.
//
//   record_stream_zip CHUNK_BYTES BATCH PATH1 [PATH2]
//
// Zips the two mate files (or splits the one interleaved file) into pair batches and prints one line
// per batch: "B <pairs> <len1> x<hex1> <starts1> <len2> x<hex2> <starts2>" -- the byte length and
// the bytes (hex) of each slice's text and its FASTQ record starts ("-" when none are kept).  An
// error prints "E <message>" and exits with status 3.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
    printf(" 0 x -");
    return;
  }
  printf(" %llu x", (unsigned long long)(s.te - s.tb));
  for (uint64_t i = s.tb; i < s.te; ++i) printf("%02x", (unsigned char)s.buf->p[i]);
  printf(" ");
  if (s.starts.empty()) printf("-");
  for (size_t i = 0; i < s.starts.size(); ++i) printf(i ? ",%llu" : "%llu", (unsigned long long)s.starts[i]);
}

int main(int argc, char **argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: record_stream_zip CHUNK_BYTES BATCH PATH1 [PATH2]\n");
    return 2;
  }
  setenv("GWA_PIPE_CHUNK", argv[1], 1);
  const uint64_t batch = strtoull(argv[2], nullptr, 10);
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
    gwa::PairedRecordStream prs(argv[3], argc > 4 ? argv[4] : nullptr, batch, alloc);
    gwa::RecordSlice m1, m2;
    uint64_t pairs = 0;
    while (prs.next(&m1, &m2, &pairs)) {
      printf("B %llu", (unsigned long long)pairs);
      show(m1);
      show(m2);
      printf("\n");
    }
  } catch (std::exception &e) {
    printf("E %s\n", e.what());
    return 3;
  }
  return 0;
}
