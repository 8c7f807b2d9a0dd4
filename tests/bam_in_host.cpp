// bam_in_host.cpp -- stand-alone driver of the host build of the BAM input decoder (csrc/bam_in_core.h) for
// tests/test_bam_in_host.py, which compiles it with the address and undefined-behaviour sanitizers.  Each
// case's records sit in a heap block of exactly their size, so a load past the data is a sanitizer report.
//
//   bam_in_host CASES_FILE
//
// CASES_FILE: u32 count, then per case u64 length and the headerless records.  Prints per case "C <index>",
// then "R <name hex> <seq> <qual hex | *>" per read (an empty field prints "-"), or "E <message>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "../genome-weaver-align_amd/csrc/bam_in_core.h"

using namespace gwa;

static void hex(const uint8_t *p, uint64_t n) {
  if (!n) printf("-");
  for (uint64_t i = 0; i < n; ++i) printf("%02x", p[i]);
}

static void runCase(const uint8_t *bytes, uint64_t len) {
  std::vector<uint64_t> st, idx;
  uint64_t nAll = 0;
  (void)bamin::walkChain(bytes, len, true, 0, 0, &st, &idx, &nAll);
  std::string lines;
  for (size_t r = 0; r < st.size(); ++r) {
    const uint8_t *rec = bytes + st[r];
    const uint64_t l = bamin::fieldsOf(rec).lSeq, slot = bamin::pad16(l);
    std::vector<uint8_t> seq(slot), qual(slot);
    uint32_t nl = 0;
    bool qn = false;
    if (bamin::decodeRecord(rec, bytes + len, &nl, &qn, seq.data(), qual.data()) != bamin::kOk)
      throw std::runtime_error(bamin::recordLabel(idx[r], st[r]) + bamin::recordProblem(rec));
    for (uint64_t i = l; i < slot; ++i)
      if (seq[i] || qual[i]) throw std::runtime_error("a slot is not zero behind the read");
    printf("R ");
    hex(rec + bamin::kFixed, nl);
    printf(" %s ", l ? std::string((const char *)seq.data(), l).c_str() : "-");
    if (qn) printf("*");
    else hex(qual.data(), l);
    printf("\n");
  }
}

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: bam_in_host CASES_FILE\n");
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t n = 0;
  if (fread(&n, 4, 1, f) != 1) return 2;
  for (uint32_t c = 0; c < n; ++c) {
    uint64_t len = 0;
    if (fread(&len, 8, 1, f) != 1) return 2;
    uint8_t *bytes = (uint8_t *)malloc(len ? len : 1);
    if (len && fread(bytes, 1, len, f) != len) return 2;
    printf("C %u\n", c);
    try {
      runCase(bytes, len);
    } catch (std::exception &e) {
      printf("E %s\n", e.what());
    }
    free(bytes);
  }
  fclose(f);
  return 0;
}
