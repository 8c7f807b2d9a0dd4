// bam_host.cpp -- TEST-ONLY stand-alone program (tests/test_bam_host.py): the BAM record writer of
// bam_core.h on the CPU over hand-written hits, next to the SAM writer of sam_core.h over the same hits.
// It builds a HostIndex from a FASTA file, reads units from a case file, and for every unit runs
// samRead / samPair with a BamOut in counting and then in writing mode (the two must agree, and nothing
// may be written behind the counted size), and the same with a SamOut.  Never linked into libgwa.so.
//
//   bam_host <fasta> <cases> <sam_tags> <out.sam> <out.bam> <out.hdr>
//
// out.sam / out.bam: the units' lines / records back to back; out.hdr: the BAM header (bamHeader).
// stdout, one line per case record that reports:
//   UNIT <sam bytes> <bam bytes>          a unit written
//   LONGNAME <bytes>                      a unit refused: a read name longer than 254 bytes (nothing written)
//   BIN <bin>                             the answer to a BIN record
//
// Case file, one record per line (md_host.cpp's, and):
//   READ <name | @empty> <bases | -> <qual | *>
//   HIT <contig index | -2 (empty name) | -3 ("*")> <pos> <matchLength> <qStart> <qEnd> <diff> <strand> <numHits> <next> <cigar | ->
//   END
//   RESCUE <1 | 2> <contig index> <pos> <strand> <diff> <numHits> <cigar>
//   PAIR <minInsert> <maxInsert>
//   BIN <flag> <beg> <reflen>             bamBin called directly
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "bam_core.h"
#include "host_index.h"
#include "sam.h"

using namespace gwa;

struct Read {
  std::string name, seq, qual;
  bool hasQual = false;
  std::vector<OutHit> hits;
  std::vector<uint16_t> cig;
};

static void die(const std::string &m) {
  fprintf(stderr, "bam_host: %s\n", m.c_str());
  exit(2);
}

static std::vector<uint16_t> parseCigar(const std::string &s) {
  std::vector<uint16_t> out;
  if (s == "-") return out;
  const char *ops = "MIDNSHPX";
  size_t i = 0;
  while (i < s.size()) {
    long n = 0;
    if (!isdigit((unsigned char)s[i])) die("bad CIGAR " + s);
    while (i < s.size() && isdigit((unsigned char)s[i])) n = n * 10 + (s[i++] - '0');
    const char *p = i < s.size() ? strchr(ops, s[i]) : nullptr;
    if (!p || n > 8191) die("bad CIGAR " + s);
    out.push_back((uint16_t)(n << 3 | (p - ops)));
    ++i;
  }
  return out;
}

// the reads' text as the formatter reads it: 16-B aligned, zero-padded code rows (ReadsView); names and
// qualities without any padding (the host build reads no byte behind a field)
struct Text {
  std::vector<char> names, quals;
  std::vector<uint64_t> nameB, nameE, qualB, qualE;
  std::vector<uint8_t> qualNull, codes;
  std::vector<uint32_t> codeOff, codeLen;
  bool anyQual = false;
  Text() {  // (data() of an empty blob must not be null: a null quality blob means "no qualities")
    names.reserve(16);
    quals.reserve(16);
  }
  void add(const Read &r) {
    nameB.push_back(names.size());
    names.insert(names.end(), r.name.begin(), r.name.end());
    nameE.push_back(names.size());
    qualB.push_back(quals.size());
    if (r.hasQual) quals.insert(quals.end(), r.qual.begin(), r.qual.end());
    qualE.push_back(quals.size());
    qualNull.push_back(r.hasQual ? 0 : 1);
    anyQual = anyQual || r.hasQual;
    codeOff.push_back((uint32_t)codes.size());
    uint32_t m = 0;
    for (char c : r.seq)
      if (c != ' ') { codes.push_back(to3bit((unsigned char)c)); ++m; }
    codeLen.push_back(m);
    codes.resize((codes.size() + 15) & ~(size_t)15, 0);
  }
};

int main(int argc, char **argv) {
  if (argc != 7) die("usage: bam_host <fasta> <cases> <sam_tags> <out.sam> <out.bam> <out.hdr>");
  std::ifstream ff(argv[1]);
  std::stringstream fs;
  fs << ff.rdbuf();
  const std::string fasta = fs.str();
  HostIndex h;
  packFasta(fasta.data(), fasta.size(), h);
  if (h.N == 0) die("empty FASTA");
  std::vector<uint8_t> R(h.T.rbegin(), h.T.rend());
  if (!cyclicSAHost(h.T.data(), h.N, h.sa[0]) || !cyclicSAHost(R.data(), h.N, h.sa[1])) die("periodic text");
  finishIndex(h);
  const SamNames sn = samNames(h);
  const uint32_t tags = (uint32_t)atoi(argv[3]);

  std::ifstream cf(argv[2]);
  std::string line, samOut, bamOut;
  std::vector<Read> reads;
  RescueOut resc{};
  bool haveResc = false;
  auto samText = [&](const Text &t) {
    SamText s{t.names.data(), t.nameB.data(), t.nameE.data(), t.anyQual ? t.quals.data() : nullptr, t.qualB.data(),
              t.qualE.data(), t.qualNull.data(), t.codes.data(), t.codeOff.data(), t.codeLen.data(), sn.blob.data(),
              sn.off.data(), h.chrRank.data(), sn.starKey, sn.emptyKey};
    if (tags) {
      s.text2 = h.text2.data();
      s.textN = h.textN.data();
      s.ctgStart = h.offsets.data();
      s.ctgLen = h.lengths.data();
      s.tags = tags;
    }
    return s;
  };
  auto chains = [](const std::vector<OutHit> &hits) {
    int n = 0;
    for (size_t head = 0; head < hits.size(); ++n) {
      size_t x = head;
      while (hits[x].next >= 0) x = (size_t)hits[x].next;
      head = x + 1;
    }
    return n;
  };
  // one unit through both writers; each counts, then writes: the two passes must agree
  auto emit = [&](auto &&run) {
    BamOut bc{nullptr, 0};
    if (run(bc) != 0) die("the BAM writer reports an error");
    if (bc.longName) {
      printf("LONGNAME %u\n", bc.longName);
      return;
    }
    std::vector<uint8_t> bb(bc.n + 1, 0xA5);  // (one guard byte behind the records)
    BamOut bo{bb.data(), 0};
    run(bo);
    if (bo.n != bc.n) die("BAM count " + std::to_string(bc.n) + " != written " + std::to_string(bo.n));
    if (bb[bc.n] != 0xA5) die("the BAM writer wrote past the counted size");
    SamOut sc{nullptr, 0};
    if (run(sc) != 0) die("the SAM writer reports an error");
    std::vector<char> sb(sc.n + 1, '#');
    SamOut so{sb.data(), 0};
    run(so);
    if (so.n != sc.n || sb[sc.n] != '#') die("the SAM passes disagree");
    samOut.append(sb.data(), sc.n);
    bamOut.append((const char *)bb.data(), bc.n);
    printf("UNIT %llu %llu\n", (unsigned long long)sc.n, (unsigned long long)bc.n);
  };
  while (std::getline(cf, line)) {
    std::istringstream is(line);
    std::string k;
    if (!(is >> k) || k[0] == '#') continue;
    if (k == "READ") {
      Read r;
      is >> r.name >> r.seq >> r.qual;
      if (r.name == "@empty") r.name.clear();
      if (r.seq == "-") r.seq.clear();
      r.hasQual = r.qual != "*";
      if (r.qual == "@empty") r.qual.clear();
      reads.push_back(r);
    } else if (k == "HIT") {
      if (reads.empty()) die("HIT without READ");
      Read &r = reads.back();
      OutHit x{};
      std::string cg;
      is >> x.chr >> x.pos >> x.matchLength >> x.qStart >> x.qEnd >> x.diff >> x.strand >> x.numHits >> x.next >> cg;
      if (!is) die("bad HIT: " + line);
      const auto c = parseCigar(cg);
      x.cigarOff = (uint32_t)r.cig.size();
      x.cigarLen = (uint32_t)c.size();
      r.cig.insert(r.cig.end(), c.begin(), c.end());
      r.hits.push_back(x);
    } else if (k == "END") {
      if (reads.size() != 1) die("END needs one READ");
      const Read &r = reads[0];
      Text t;
      t.add(r);
      const SamText st = samText(t);
      OutHeader oh{};
      oh.status = r.hits.empty() ? ST_UNMAPPED : ST_MAPPED;
      oh.nChains = chains(r.hits);
      oh.nHits = (int32_t)r.hits.size();
      oh.nCigar = (int32_t)r.cig.size();
      std::vector<uint16_t> cig = r.cig;
      cig.push_back(0);
      emit([&](auto &o) { return samRead(o, st, 0, oh, r.hits.data(), cig.data()); });
      reads.clear();
    } else if (k == "RESCUE") {
      std::string cg;
      OutHit &x = resc.hit;
      x = OutHit{};
      is >> resc.status >> x.chr >> x.pos >> x.strand >> x.diff >> x.numHits >> cg;
      if (!is) die("bad RESCUE: " + line);
      const auto c = parseCigar(cg);
      if (c.size() > (size_t)kRescueCig) die("RESCUE CIGAR too long");
      for (size_t i = 0; i < c.size(); ++i) resc.cig[i] = c[i];
      x.cigarOff = 0;
      x.cigarLen = (uint32_t)c.size();
      x.next = -1;
      x.matchLength = 0;
      haveResc = true;
    } else if (k == "PAIR") {
      if (reads.size() != 2) die("PAIR needs two READs");
      int32_t minIns = 0, maxIns = 0;
      is >> minIns >> maxIns;
      Text t;
      t.add(reads[0]);
      t.add(reads[1]);
      const SamText st = samText(t);
      std::vector<OutHit> hits = reads[0].hits;
      hits.insert(hits.end(), reads[1].hits.begin(), reads[1].hits.end());
      std::vector<uint16_t> cig = reads[0].cig;
      cig.insert(cig.end(), reads[1].cig.begin(), reads[1].cig.end());
      cig.push_back(0);
      hits.push_back(OutHit{});
      OutHeader oh[2] = {};
      for (int i = 0; i < 2; ++i) {
        oh[i].status = reads[i].hits.empty() ? ST_UNMAPPED : ST_MAPPED;
        oh[i].nChains = chains(reads[i].hits);
        oh[i].nHits = (int32_t)reads[i].hits.size();
        oh[i].nCigar = (int32_t)reads[i].cig.size();
      }
      oh[1].hitOff = (uint32_t)reads[0].hits.size();
      oh[1].cigOff = (uint32_t)reads[0].cig.size();
      const RescueOut *rp = nullptr;
      if (haveResc) {  // the choice as the pair kernels leave it (pool indices)
        const PairChoice P = pairChoose(st, 0, 1, oh, hits.data(), cig.data(), minIns, maxIns);
        auto ix = [&](const OutHit *p) { return p ? (int32_t)(p - hits.data()) : -1; };
        resc.a = ix(P.a); resc.b = ix(P.b); resc.fa = ix(P.fa); resc.fb = ix(P.fb);
        rp = &resc;
      }
      emit([&](auto &o) { return samPair(o, st, 0, 1, oh, hits.data(), cig.data(), minIns, maxIns, rp); });
      reads.clear();
      haveResc = false;
    } else if (k == "BIN") {
      int flag = 0;
      long long beg = 0, reflen = 0;
      is >> flag >> beg >> reflen;
      if (!is) die("bad BIN: " + line);
      printf("BIN %u\n", bamBin(flag, beg, reflen));
    } else {
      die("unknown record " + k);
    }
  }
  const std::string hdr = bamHeader(h);
  const std::string *outs[3] = {&samOut, &bamOut, &hdr};
  for (int i = 0; i < 3; ++i) {
    FILE *f = fopen(argv[4 + i], "wb");
    if (!f || fwrite(outs[i]->data(), 1, outs[i]->size(), f) != outs[i]->size() || fclose(f) != 0) die("cannot write an output file");
  }
  return 0;
}
