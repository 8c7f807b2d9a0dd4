// bam_dup_core.h -- duplicate marking of BAM records (include/gwa.h "Duplicate marking"), for the device
// (bam_dup.hip), the run sorter (bam_sorter.cpp) and the host test (tests/markdup_host.cpp).  Everything here
// is a function of the input-order record stream alone: the end key, the score and the pairing of a record
// with its neighbour (the per-run pass), and the decision over the entries of all runs (the global resolve).
// The host builds of both passes are the restatement the device is tested against.
#pragma once
#include <cstdint>
#include <cstring>

#include "bam_sort_core.h"

#include <algorithm>
#include <tuple>
#include <vector>

namespace gwa {
namespace bamdup {

using bamsort::ld16;
using bamsort::ld32;

constexpr uint64_t kNoKey = ~(uint64_t)0;  // (an end key has refID < 2^31: never all ones)
constexpr uint32_t kDupFlag = 0x400;
constexpr uint32_t kFlagByte = 19;  // FLAG's high byte inside a record (block_size counted)

// What the sorter keeps of a record for the decision, beside its BamRecInfo and in the same order.
struct BamDupInfo {
  uint64_t endKey;   // kNoKey: the record does not participate
  uint64_t mateKey;  // the other record's endKey in a pair template with both participating, else kNoKey
  uint32_t score;    // the template's score
  uint32_t leader;   // run-input ordinal of the template's first record
};
static_assert(sizeof(BamDupInfo) == 24, "BamDupInfo is 24 bytes per record");

// how the per-run pass leaves a record before its neighbour is looked at: endKey and the record's own score
// as above, leader = its own ordinal, mateKey = one of these
constexpr uint64_t kLinkNone = 0, kLinkNext = 1, kLinkPrev = 2;

GWA_HD bool participates(uint32_t flag, int32_t refId) { return (flag & (0x4u | 0x100u | 0x800u)) == 0 && refId >= 0; }
GWA_HD bool firstOfPair(uint32_t flag) { return (flag & (0x1u | 0x40u | 0x80u | 0x100u | 0x800u)) == (0x1u | 0x40u); }
GWA_HD bool secondOfPair(uint32_t flag) { return (flag & (0x1u | 0x40u | 0x80u | 0x100u | 0x800u)) == (0x1u | 0x80u); }

GWA_HD uint64_t endKeyFrom(int32_t refId, int64_t u5, uint32_t reverse) {
  return (uint64_t)(uint32_t)refId << 33 | (uint64_t)(uint32_t)((uint32_t)(uint64_t)u5 + 0x80000000u) << 1 | (reverse ? 1u : 0u);
}

// the name, the CIGAR, and SEQ + QUAL lie inside the record's `size` bytes (validateChain's guarantee; where
// a record breaks it the CIGAR counts as empty and the score as 0, and nothing outside the record is read)
GWA_HD bool cigarInside(const uint8_t *rec, uint32_t size) { return (uint64_t)36 + rec[12] + 4ull * ld16(rec + 16) <= size; }
GWA_HD uint64_t qualOffset(const uint8_t *rec) {
  const uint64_t lseq = ld32(rec + 20);
  return (uint64_t)36 + rec[12] + 4ull * ld16(rec + 16) + (lseq + 1) / 2;
}
GWA_HD bool qualInside(const uint8_t *rec, uint32_t size) { return qualOffset(rec) + ld32(rec + 20) <= size; }

// u5 from the record's fields and three sums over its CIGAR
GWA_HD int64_t u5From(int32_t pos, uint32_t reverse, int64_t reflen, int64_t lead, int64_t trail, uint32_t ncig) {
  if (ncig == 0) return pos;
  return reverse ? (int64_t)pos + reflen + trail - 1 : (int64_t)pos - lead;
}

// The end key of the record at rec (size bytes), kNoKey where it does not participate.
GWA_HD uint64_t endKeyOf(const uint8_t *rec, uint32_t size) {
  const int32_t refId = (int32_t)ld32(rec + 4), pos = (int32_t)ld32(rec + 8);
  const uint32_t flag = ld16(rec + 18);
  if (!participates(flag, refId)) return kNoKey;
  const uint32_t ncig = cigarInside(rec, size) ? ld16(rec + 16) : 0u;
  const uint8_t *c = rec + 36 + rec[12];
  int64_t reflen = 0, lead = 0, trail = 0;
  for (uint32_t i = 0; i < ncig; ++i) {
    const uint32_t v = ld32(c + 4 * i), op = v & 15u;
    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) reflen += v >> 4;
  }
  for (uint32_t i = 0; i < ncig; ++i) {
    const uint32_t v = ld32(c + 4 * i), op = v & 15u;
    if (op != 4 && op != 5) break;
    lead += v >> 4;
  }
  for (uint32_t i = ncig; i-- > 0;) {
    const uint32_t v = ld32(c + 4 * i), op = v & 15u;
    if (op != 4 && op != 5) break;
    trail += v >> 4;
  }
  return endKeyFrom(refId, u5From(pos, flag & 0x10u, reflen, lead, trail, ncig), flag & 0x10u);
}

GWA_HD uint32_t qualValue(uint32_t q) { return q - 15u <= 78u ? q : 0u; }  // 15 <= q <= 93

// The record's own score: 0 where it does not participate.
GWA_HD uint32_t scoreOf(const uint8_t *rec, uint32_t size) {
  if (!participates(ld16(rec + 18), (int32_t)ld32(rec + 4)) || !qualInside(rec, size)) return 0;
  const uint8_t *q = rec + qualOffset(rec);
  const uint32_t lseq = ld32(rec + 20);
  uint32_t s = 0;
  for (uint32_t i = 0; i < lseq; ++i) s += qualValue(q[i]);
  return s;
}

// Records a then b, neighbours in one run's input order, are a pair.
GWA_HD bool pairsWith(const uint8_t *a, uint32_t sizeA, const uint8_t *b, uint32_t sizeB) {
  if (!firstOfPair(ld16(a + 18)) || !secondOfPair(ld16(b + 18))) return false;
  const uint32_t ln = a[12];
  if (ln != b[12] || (uint64_t)36 + ln > sizeA || (uint64_t)36 + ln > sizeB) return false;
  for (uint32_t i = 0; i < ln; ++i)
    if (a[36 + i] != b[36 + i]) return false;
  return true;
}

// The entry of record j from the per-run pass's entries st[0, n) (input order): the template's score and
// leader, and the other record's key.
GWA_HD BamDupInfo linked(const BamDupInfo *st, uint64_t j) {
  BamDupInfo x = st[j];
  const uint64_t link = x.mateKey;
  x.mateKey = kNoKey;
  if (link == kLinkNone) return x;
  const BamDupInfo m = st[link == kLinkNext ? j + 1 : j - 1];
  x.score += m.score;
  if (link == kLinkPrev) x.leader = m.leader;
  if (x.endKey != kNoKey && m.endKey != kNoKey) x.mateKey = m.endKey;
  return x;
}

// how an entry enters the resolve
GWA_HD bool isFragment(const BamDupInfo &x) { return x.endKey != kNoKey && x.mateKey == kNoKey; }
GWA_HD bool isPairEnd(const BamDupInfo &x) { return x.endKey != kNoKey && x.mateKey != kNoKey; }
// a pair template enters once, by its record with the lower key; with equal keys its two entries are the same
// and enter twice (the resolve counts an ordinal once)
GWA_HD bool isPairEntry(const BamDupInfo &x) { return isPairEnd(x) && x.endKey <= x.mateKey; }

struct DupStats {
  uint64_t templates = 0, pair_templates = 0, frag_templates = 0, dup_pair_templates = 0, dup_frag_templates = 0, dup_records = 0;
  double keys_s = 0, resolve_s = 0;
};

// ---- host only ----

// The host build of the per-run pass: the entries of the records at off[0 .. n] of bytes, in input order.
inline void runHost(const uint8_t *bytes, const uint64_t *off, uint64_t n, std::vector<BamDupInfo> &out) {
  std::vector<BamDupInfo> st(n);
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t *r = bytes + off[i];
    const uint32_t size = (uint32_t)(off[i + 1] - off[i]);
    st[i].endKey = endKeyOf(r, size);
    st[i].score = scoreOf(r, size);
    st[i].leader = (uint32_t)i;
    st[i].mateKey = kLinkNone;
  }
  for (uint64_t i = 0; i + 1 < n; ++i)
    if (pairsWith(bytes + off[i], (uint32_t)(off[i + 1] - off[i]), bytes + off[i + 1], (uint32_t)(off[i + 2] - off[i + 1]))) {
      st[i].mateKey = kLinkNext;
      st[i + 1].mateKey = kLinkPrev;
    }
  out.resize(n);
  for (uint64_t i = 0; i < n; ++i) out[i] = linked(st.data(), i);
}

// The host build of the global resolve.  e[0, n): the entries of all runs, in any order, `leader` already the
// template's global ordinal (< nOrdinals).  Sets bit o of bits for every duplicate template o and counts
// the classes (pair_templates, frag_templates, dup_pair_templates, dup_frag_templates).
inline void resolveHost(const BamDupInfo *e, uint64_t n, uint64_t nOrdinals, std::vector<uint32_t> &bits, DupStats *st) {
  bits.assign((size_t)((nOrdinals + 31) / 32), 0u);
  typedef std::tuple<uint64_t, uint64_t, uint32_t, uint32_t> T;  // lo, hi, ~score, ordinal
  std::vector<T> pairs, frags;
  std::vector<uint64_t> ends;
  for (uint64_t i = 0; i < n; ++i) {
    const BamDupInfo &x = e[i];
    if (isPairEnd(x)) ends.push_back(x.endKey);
    if (isPairEntry(x)) pairs.emplace_back(x.endKey, x.mateKey, ~x.score, x.leader);
    if (isFragment(x)) frags.emplace_back(x.endKey, 0, ~x.score, x.leader);
  }
  std::sort(pairs.begin(), pairs.end());
  std::sort(frags.begin(), frags.end());
  std::sort(ends.begin(), ends.end());
  auto mark = [&](uint32_t o) { bits[o >> 5] |= 1u << (o & 31); };
  for (size_t i = 0; i < pairs.size(); ++i) {
    const bool hasPrev = i > 0;
    if (hasPrev && std::get<3>(pairs[i - 1]) == std::get<3>(pairs[i])) continue;  // the template's second entry
    ++st->pair_templates;
    if (hasPrev && std::get<0>(pairs[i - 1]) == std::get<0>(pairs[i]) && std::get<1>(pairs[i - 1]) == std::get<1>(pairs[i])) {
      ++st->dup_pair_templates;
      mark(std::get<3>(pairs[i]));
    }
  }
  for (size_t i = 0; i < frags.size(); ++i) {
    ++st->frag_templates;
    const uint64_t k = std::get<0>(frags[i]);
    if ((i > 0 && std::get<0>(frags[i - 1]) == k) || std::binary_search(ends.begin(), ends.end(), k)) {
      ++st->dup_frag_templates;
      mark(std::get<3>(frags[i]));
    }
  }
}

}  // namespace bamdup
}  // namespace gwa
