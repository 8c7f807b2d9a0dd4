// markdup_host.cpp -- TEST-ONLY stand-alone program (tests/test_markdup_host.py): the host build of duplicate
// marking (csrc/bam_dup_core.h) and the run sorter with the option (csrc/bam_sorter.cpp, built with
// GWA_BAM_SORT_HOST_ONLY) over record files the test wrote.  Never linked into libgwa.so.
//
//   markdup_host <contigs> <mem_bytes> <tmp_dir | -> <part_slices> <out.bam> <out.bai | -> <0 | 1 | late>
//                [<run id>:<file>]...
//
// contigs: one "<name> <length>" per line.  Every run file holds unsorted records; the runs are added in the
// order given.  1: marking on; 0: off; late: switched on after the first run was added (refused).  For every
// run file F: F.own holds per record, in input order, 13 bytes computed from a heap copy of exactly the
// record's size (endKey u64, own score u32, 1 where the record pairs with the next one, each record again an
// exact copy); F.dup holds the per-run pass's 24-byte entries in input order.  out.bam = BGZF(sorted header) +
// what finish() writes + the EOF marker.
// stdout: "STATS <records> <runs> <spilled runs> <blocks>" and "DUP <templates> <pair> <fragment> <duplicate
// pair> <duplicate fragment> <duplicate records>".  A refused call prints "ERROR <message>", status 3.
#include <fcntl.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "bam_dup_core.h"
#include "bam_sorter.h"
#include "bgzf_host.h"
#include "host_index.h"
#include "sam.h"

using namespace gwa;

static void die(const std::string &m) {
  fprintf(stderr, "markdup_host: %s\n", m.c_str());
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

static std::unique_ptr<uint8_t[]> exactCopy(const uint8_t *p, size_t n) {
  std::unique_ptr<uint8_t[]> c(new uint8_t[n]);
  memcpy(c.get(), p, n);
  return c;
}

int main(int argc, char **argv) {
  if (argc < 8) die("usage: markdup_host <contigs> <mem_bytes> <tmp_dir|-> <part_slices> <out.bam> <out.bai|-> <0|1|late> [id:file]...");
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
  const std::string tmp = argv[3], bai = argv[6], mode = argv[7];
  try {
    BamSorter s(names, lengths, -1, tmp == "-" ? nullptr : tmp.c_str(), mem);
    s.setPartSlices((uint32_t)atoi(argv[4]));
    if (mode == "1") s.setMarkdup(true);
    for (int i = 8; i < argc; ++i) {
      const std::string a = argv[i];
      const size_t c = a.find(':');
      if (c == std::string::npos) die("bad run " + a);
      const uint64_t id = strtoull(a.substr(0, c).c_str(), nullptr, 10);
      const std::string path = a.substr(c + 1);
      const std::vector<uint8_t> bytes = slurp(path);
      // (an exact-size copy: the sanitizer sees a read behind the records)
      std::vector<uint8_t> exact(bytes.begin(), bytes.end());
      s.addRecords(id, exact.data(), exact.size());
      if (mode == "late") s.setMarkdup(true);
      const std::vector<uint64_t> off = bamsort::validateChain(exact.data(), exact.size());
      const uint64_t n = off.size() - 1;
      std::vector<uint8_t> own;
      for (uint64_t r = 0; r < n; ++r) {
        const uint32_t size = (uint32_t)(off[r + 1] - off[r]);
        const auto rec = exactCopy(exact.data() + off[r], size);
        const uint64_t k = bamdup::endKeyOf(rec.get(), size);
        const uint32_t sc = bamdup::scoreOf(rec.get(), size);
        uint8_t pairs = 0;
        if (r + 1 < n) {
          const uint32_t sizeB = (uint32_t)(off[r + 2] - off[r + 1]);
          const auto next = exactCopy(exact.data() + off[r + 1], sizeB);
          pairs = bamdup::pairsWith(rec.get(), size, next.get(), sizeB) ? 1 : 0;
        }
        for (int b = 0; b < 8; ++b) own.push_back((uint8_t)(k >> (8 * b)));
        for (int b = 0; b < 4; ++b) own.push_back((uint8_t)(sc >> (8 * b)));
        own.push_back(pairs);
      }
      spit(path + ".own", own.data(), own.size());
      std::vector<bamdup::BamDupInfo> dup;
      bamdup::runHost(exact.data(), off.data(), n, dup);
      spit(path + ".dup", dup.data(), dup.size() * sizeof(bamdup::BamDupInfo));
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
    const bamdup::DupStats d = s.markdupStats();
    printf("STATS %llu %llu %llu %llu\n", (unsigned long long)st.records, (unsigned long long)st.runs,
           (unsigned long long)st.spilled_runs, (unsigned long long)st.blocks);
    printf("DUP %llu %llu %llu %llu %llu %llu\n", (unsigned long long)d.templates, (unsigned long long)d.pair_templates,
           (unsigned long long)d.frag_templates, (unsigned long long)d.dup_pair_templates,
           (unsigned long long)d.dup_frag_templates, (unsigned long long)d.dup_records);
  } catch (std::exception &e) {
    printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
