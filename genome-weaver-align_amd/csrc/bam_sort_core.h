// bam_sort_core.h -- coordinate order and the .bai index of BAM records (include/gwa.h "Sorted BAM"), for
// the device (bam_sort.hip) and for the host (bam_sorter.cpp, tests/bam_sort_host.cpp).  Everything here is
// a function of the record bytes alone: the sort key, the per-record index fields (BamRecInfo), the walk
// over a block_size chain, the host build of the batch sort (std::stable_sort) and the index writer.
#pragma once
#include <cstdint>
#include <cstring>

#include "gwa_layout.h"

#include <algorithm>
#include <map>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

namespace gwa {
namespace bamsort {

constexpr uint32_t kSlice = 65280;               // the BGZF slice (bgzf_core.h kSlice)
constexpr uint64_t kKeyNoRef = 0xFFFFFFFF00000000ull;
constexpr int64_t kMaxEnd = 1ll << 29;           // what the .bai bins cover
constexpr uint32_t kPseudoBin = 37450;
constexpr uint32_t kMinRecord = 36;              // block_size (4) + the 32 fixed bytes
constexpr uint32_t kUnmappedBit = 0x80000000u;   // of BamRecInfo.bin

// What the sorter keeps of a record besides its bytes: 24 bytes per record.
struct BamRecInfo {
  uint64_t key;
  uint32_t size;  // block_size + 4
  int32_t beg;    // max(pos, 0)
  int32_t end;    // min(max(pos + max(reflen, 1), beg + 1), 2^29)
  uint32_t bin;   // reg2bin(beg, end) of the index (not the record's bin field) | kUnmappedBit for FLAG 0x4
};
static_assert(sizeof(BamRecInfo) == 24, "BamRecInfo is 24 bytes per record");

GWA_HD uint32_t ld16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
GWA_HD uint32_t ld32(const uint8_t *p) { return ld16(p) | ld16(p + 2) << 16; }

GWA_HD uint64_t keyOf(int32_t refId, int32_t pos) {
  if (refId == -1) return kKeyNoRef;
  return (uint64_t)(uint32_t)refId << 32 | ((uint32_t)pos ^ 0x80000000u);
}

// the specification's reg2bin (section 5.3) for [beg, end)
GWA_HD uint32_t reg2bin(int64_t beg, int64_t end) {
  --end;
  if (beg >> 14 == end >> 14) return (uint32_t)(4681 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (uint32_t)(585 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (uint32_t)(73 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (uint32_t)(9 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (uint32_t)(1 + (beg >> 26));
  return 0;
}

// The record at rec, `size` bytes long (size >= kMinRecord).  The CIGAR is read only where it lies inside
// the record (a validated chain: always); otherwise reflen counts as 0.
GWA_HD BamRecInfo infoOf(const uint8_t *rec, uint32_t size) {
  const int32_t refId = (int32_t)ld32(rec + 4), pos = (int32_t)ld32(rec + 8);
  const uint32_t lname = rec[12], ncig = ld16(rec + 16), flag = ld16(rec + 18);
  int64_t reflen = 0;
  if ((uint64_t)36 + lname + 4ull * ncig <= size) {
    const uint8_t *c = rec + 36 + lname;
    for (uint32_t i = 0; i < ncig; ++i) {
      const uint32_t v = ld32(c + 4 * i), op = v & 15u;
      if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) reflen += v >> 4;
    }
  }
  const int64_t beg = pos > 0 ? pos : 0;
  int64_t end = (int64_t)pos + (reflen > 1 ? reflen : 1);
  if (end < beg + 1) end = beg + 1;
  if (end > kMaxEnd) end = kMaxEnd;
  BamRecInfo r;
  r.key = keyOf(refId, pos);
  r.size = size;
  r.beg = (int32_t)beg;
  r.end = (int32_t)end;
  r.bin = reg2bin(beg, end) | ((flag & 0x4u) ? kUnmappedBit : 0u);
  return r;
}

// The size of the record at p inside [p, end), or 0 where no whole record of at least kMinRecord bytes
// starts there (the walks stop; a chain the writer or the validation produced never does before `end`).
GWA_HD uint32_t recordAt(const uint8_t *p, uint64_t room) {
  if (room < kMinRecord) return 0;
  const uint32_t bs = ld32(p);
  if (bs < kMinRecord - 4 || (uint64_t)bs + 4 > room) return 0;
  return bs + 4;
}

// ---- host only ----

// Offsets of the records of bytes[0, len) (n + 1 of them), validated: every block_size >= 32, name, CIGAR,
// SEQ and QUAL inside the record, the chain ending exactly at len.  Throws with the record's index and offset.
inline std::vector<uint64_t> validateChain(const uint8_t *bytes, uint64_t len) {
  std::vector<uint64_t> off;
  uint64_t at = 0;
  auto bad = [&](const std::string &what) {
    throw std::runtime_error("BAM record " + std::to_string(off.size()) + " at byte " + std::to_string(at) + ": " + what);
  };
  while (at < len) {
    if (len - at < 4) bad("the chain of block_size fields ends " + std::to_string(len - at) + " bytes before the data's end");
    const uint32_t bs = ld32(bytes + at);
    if (bs < 32) bad("block_size " + std::to_string(bs) + " is below the 32 fixed bytes");
    if ((uint64_t)bs + 4 > len - at)
      bad("block_size " + std::to_string(bs) + " runs past the data's end (" + std::to_string(len) + " bytes)");
    const uint8_t *r = bytes + at;
    const uint64_t lname = r[12], ncig = ld16(r + 16), lseq = ld32(r + 20);
    if (lname > bs - 32) bad("the read name (" + std::to_string(lname) + " bytes) runs past the record");
    if (lname + 4 * ncig > bs - 32) bad("the CIGAR (" + std::to_string(ncig) + " elements) runs past the record");
    if (lname + 4 * ncig + (lseq + 1) / 2 + lseq > bs - 32) bad("SEQ and QUAL (l_seq " + std::to_string(lseq) + ") run past the record");
    off.push_back(at);
    at += (uint64_t)bs + 4;
  }
  off.push_back(len);
  return off;
}

// The host build of the batch sort: the records of bytes (record offsets off[0 .. n]) stably sorted by key.
// permOut (may be null): the input ordinal of every sorted record.
inline void sortHost(const uint8_t *bytes, const uint64_t *off, uint64_t n, std::vector<uint8_t> &sorted,
                     std::vector<BamRecInfo> &info, std::vector<uint64_t> *permOut = nullptr) {
  std::vector<BamRecInfo> in(n);
  for (uint64_t i = 0; i < n; ++i) in[i] = infoOf(bytes + off[i], (uint32_t)(off[i + 1] - off[i]));
  std::vector<uint64_t> perm(n);
  std::iota(perm.begin(), perm.end(), (uint64_t)0);
  std::stable_sort(perm.begin(), perm.end(), [&](uint64_t a, uint64_t b) { return in[a].key < in[b].key; });
  sorted.resize(n ? off[n] - off[0] : 0);
  info.resize(n);
  uint64_t at = 0;
  for (uint64_t i = 0; i < n; ++i) {
    info[i] = in[perm[i]];
    memcpy(sorted.data() + at, bytes + off[perm[i]], info[i].size);
    at += info[i].size;
  }
  if (permOut) permOut->swap(perm);
}

// The uncompressed header of a sorted file from the plain one (bamHeader's bytes: "BAM\1", l_text, the text,
// the contig table): the same with "@HD\tVN:1.6\tSO:coordinate\n" put before the text.
inline std::string sortedHeader(const std::string &plain) {
  static const char hd[] = "@HD\tVN:1.6\tSO:coordinate\n";
  if (plain.size() < 8 || plain.compare(0, 4, "BAM\1", 4) != 0) throw std::runtime_error("sortedHeader: not a BAM header");
  const uint64_t lt = (uint64_t)ld32((const uint8_t *)plain.data() + 4) + (sizeof hd - 1);
  std::string h(plain, 0, 4);
  for (int i = 0; i < 4; ++i) h += (char)(lt >> (8 * i));
  h += hd;
  h.append(plain, 8, std::string::npos);
  return h;
}

// The stable order of concatenated keys (the sorter's finish on the host)
inline void orderHost(const uint64_t *keys, uint64_t n, uint32_t *perm) {
  std::iota(perm, perm + n, (uint32_t)0);
  std::stable_sort(perm, perm + n, [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
}

// The .bai of a sorted stream (include/gwa.h): add() takes the stream's records in order, write() appends the
// index to out.  blockStart[k] = file offset of block k (the stream's slice k), blockStart[nBlocks] = the end
// of the last block.
struct BaiWriter {
  struct Ref {
    std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins;
    std::vector<uint64_t> lin;
    std::vector<uint8_t> linSet;
    uint64_t first = 0, last = 0, mapped = 0, unmapped = 0;
    uint32_t lastBin = 0xFFFFFFFFu;
    std::pair<uint64_t, uint64_t> *cur = nullptr;
    int64_t maxEnd = 0;
    bool any = false;
  };
  std::vector<Ref> refs;
  const std::vector<uint64_t> &blockStart;
  uint64_t u = 0, noCoor = 0;

  BaiWriter(size_t nRef, const std::vector<uint64_t> &bs) : refs(nRef), blockStart(bs) {}
  uint64_t voff(uint64_t at) const {
    const uint64_t k = at / kSlice;
    if (k >= blockStart.size()) throw std::runtime_error("bai: a record lies behind the last block");
    return blockStart[k] << 16 | at % kSlice;
  }
  void add(const BamRecInfo &r) {
    const uint64_t a = u;
    u += r.size;
    const int32_t ref = (int32_t)(r.key >> 32);
    if (ref == -1) {
      ++noCoor;
      return;
    }
    if (ref < 0 || (size_t)ref >= refs.size())
      throw std::runtime_error("bai: a record's refID " + std::to_string(ref) + " names none of the " + std::to_string(refs.size()) +
                               " contigs");
    Ref &c = refs[(size_t)ref];
    const uint64_t vb = voff(a), ve = voff(u);
    const uint32_t bin = r.bin & ~kUnmappedBit;
    if (!c.any) c.first = vb;
    c.any = true;
    c.last = ve;
    if (r.bin & kUnmappedBit) ++c.unmapped;
    else ++c.mapped;
    if (bin == c.lastBin && c.cur) {
      c.cur->second = ve;
    } else {
      auto &v = c.bins[bin];
      v.push_back({vb, ve});
      // (a vector's growth moves its elements: the pointer is taken after the push, and no other push
      // into this bin's vector happens while it is current)
      c.cur = &v.back();
      c.lastBin = bin;
    }
    if (r.end > c.maxEnd) {
      c.maxEnd = r.end;
      const size_t n = (size_t)((c.maxEnd - 1) >> 14) + 1;
      c.lin.resize(n, 0);
      c.linSet.resize(n, 0);
    }
    for (int64_t w = r.beg >> 14; w <= ((int64_t)r.end - 1) >> 14; ++w)
      if (!c.linSet[(size_t)w]) {
        c.linSet[(size_t)w] = 1;
        c.lin[(size_t)w] = vb;
      }
  }
  void write(std::vector<uint8_t> &out) {
    auto p32 = [&](uint32_t v) { for (int i = 0; i < 4; ++i) out.push_back((uint8_t)(v >> (8 * i))); };
    auto p64 = [&](uint64_t v) { for (int i = 0; i < 8; ++i) out.push_back((uint8_t)(v >> (8 * i))); };
    out.insert(out.end(), {'B', 'A', 'I', 1});
    p32((uint32_t)refs.size());
    for (Ref &c : refs) {
      if (!c.any) {
        p32(0);
        p32(0);
        continue;
      }
      p32((uint32_t)c.bins.size() + 1);
      for (auto &b : c.bins) {
        p32(b.first);
        p32((uint32_t)b.second.size());
        for (auto &ch : b.second) {
          p64(ch.first);
          p64(ch.second);
        }
      }
      p32(kPseudoBin);
      p32(2);
      p64(c.first);
      p64(c.last);
      p64(c.mapped);
      p64(c.unmapped);
      p32((uint32_t)c.lin.size());
      for (size_t w = c.lin.size(); w-- > 0;)  // a window without a record takes the next later one's
        if (!c.linSet[w] && w + 1 < c.lin.size()) c.lin[w] = c.lin[w + 1];
      for (uint64_t v : c.lin) p64(v);
    }
    p64(noCoor);
  }
};

}  // namespace bamsort
}  // namespace gwa
