// bam_sort_host.cpp -- TEST-ONLY stand-alone program (tests/test_bam_sort_host.py): the host build of the
// coordinate sort (csrc/bam_sort_core.h), the run sorter (csrc/bam_sorter.cpp, built with
// GWA_BAM_SORT_HOST_ONLY) and the .bai writer over record files the test wrote.  Never linked into libgwa.so.
//
//   bam_sort_host <contigs> <mem_bytes> <tmp_dir | -> <part_slices> <out.bam> <out.bai | -> [<run id>:<file>]...
//
// contigs: one "<name> <length>" per line.  Every run file holds unsorted records; the runs are added in the
// order given.  For every run file F the host batch sort writes F.sorted (the records in key order) and F.keys
// (their keys, u64 LE).  out.bam = BGZF(sorted header) + what finish() writes + the EOF marker.
// stdout: "STATS <records> <bytes> <runs> <spilled runs> <blocks> <bai bytes>".  A refused call prints
// "ERROR <message>" and ends the program with status 3.
#include <fcntl.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "bam_sorter.h"
#include "bgzf_host.h"
#include "host_index.h"
#include "sam.h"

using namespace gwa;

static void die(const std::string &m) {
  fprintf(stderr, "bam_sort_host: %s\n", m.c_str());
  exit(2);
}

static std::vector<uint8_t> slurp(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) die("cannot read " + path);
  std::stringstream ss;
  ss << f.rdbuf();
  const std::string s = ss.str();
  return std::vector<uint8_t>(s.begin(), s.end());
}

static void spit(const std::string &path, const void *p, size_t n) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f || (n && fwrite(p, 1, n, f) != n) || fclose(f) != 0) die("cannot write " + path);
}

int main(int argc, char **argv) {
  if (argc < 7) die("usage: bam_sort_host <contigs> <mem_bytes> <tmp_dir|-> <part_slices> <out.bam> <out.bai|-> [id:file]...");
  std::vector<std::string> names;
  std::vector<int64_t> lengths;
  {
    std::ifstream cf(argv[1]);
    std::string n;
    long long l;
    while (cf >> n >> l) {
      names.push_back(n);
      lengths.push_back(l);
    }
  }
  const uint64_t mem = strtoull(argv[2], nullptr, 10);
  const std::string tmp = argv[3], bai = argv[6];
  try {
    BamSorter s(names, lengths, -1, tmp == "-" ? nullptr : tmp.c_str(), mem);
    s.setPartSlices((uint32_t)atoi(argv[4]));
    for (int i = 7; i < argc; ++i) {
      const std::string a = argv[i];
      const size_t c = a.find(':');
      if (c == std::string::npos) die("bad run " + a);
      const uint64_t id = strtoull(a.substr(0, c).c_str(), nullptr, 10);
      const std::string path = a.substr(c + 1);
      const std::vector<uint8_t> bytes = slurp(path);
      // (an exact-size copy: the sanitizer sees a read behind the records)
      std::vector<uint8_t> exact(bytes.begin(), bytes.end());
      s.addRecords(id, exact.data(), exact.size());
      const std::vector<uint64_t> off = bamsort::validateChain(exact.data(), exact.size());
      std::vector<uint8_t> sorted;
      std::vector<bamsort::BamRecInfo> info;
      bamsort::sortHost(exact.data(), off.data(), off.size() - 1, sorted, info);
      std::vector<uint8_t> keys;
      for (const auto &x : info)
        for (int k = 0; k < 8; ++k) keys.push_back((uint8_t)(x.key >> (8 * k)));
      spit(path + ".sorted", sorted.data(), sorted.size());
      spit(path + ".keys", keys.data(), keys.size());
    }
    const int fd = open(argv[5], O_CREAT | O_TRUNC | O_WRONLY, 0600);
    if (fd < 0) die("cannot create the BAM file");
    HostIndex hi;  // (bamHeader reads the contig table only)
    hi.names = names;
    hi.lengths = lengths;
    const std::string hdr = bamsort::sortedHeader(bamHeader(hi));
    std::vector<uint8_t> z;
    bgzf::compressHost((const uint8_t *)hdr.data(), hdr.size(), z);
    if (write(fd, z.data(), z.size()) != (ssize_t)z.size()) die("cannot write the header");
    int fdBai = -1;
    if (bai != "-") {
      fdBai = open(bai.c_str(), O_CREAT | O_TRUNC | O_WRONLY, 0600);
      if (fdBai < 0) die("cannot create the index file");
    }
    BamSorterStats st;
    s.finish(fd, fdBai, &st);
    uint8_t eof[28];
    bgzf::eofMarker(eof);
    if (write(fd, eof, 28) != 28) die("cannot write the EOF marker");
    close(fd);
    if (fdBai >= 0) close(fdBai);
    printf("STATS %llu %llu %llu %llu %llu %llu\n", (unsigned long long)st.records, (unsigned long long)st.bytes,
           (unsigned long long)st.runs, (unsigned long long)st.spilled_runs, (unsigned long long)st.blocks,
           (unsigned long long)st.bai_bytes);
  } catch (std::exception &e) {
    printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
