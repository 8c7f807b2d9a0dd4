// bam_in_core.h -- BAM alignment records read as reads (include/gwa.h "BAM input"): the per-record field
// math, the nibble-to-letter and complement tables and the quality rule, for a GPU lane (bam_in.hip) and
// for the host build; and the host-only walks over a BAM header and a block_size chain.
//
// A record is laid out as bam_core.h writes it: block_size, refID, pos, l_read_name (byte 12), mapq, bin,
// n_cigar_op (16), flag (18), l_seq (20), next_refID, next_pos, tlen, read_name from byte 36, cigar, seq
// (4 bits per base, high nibble first), qual, tags.  The chain walk establishes, for every record, that
// its 36 fixed bytes, name, CIGAR, SEQ and QUAL lie inside the record and the record inside the data; the
// functions below read nothing else of a record, and the chunk loads reach at most 16 bytes past a field
// (the device buffers carry 32 bytes of room; the host loads stop at `end`).
//
// The read is produced in 16-byte chunks of output: chunk c of SEQ holds the letters 16c .. 16c + 15 of
// the read (zero beyond l_seq), chunk c of QUAL the same of the quality string.  With FLAG 0x10 the read
// is the reverse complement of the stored SEQ and the quality is reversed, so chunk c draws on the stored
// positions l_seq - 1 - 16c downwards.
#pragma once
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "gwa_layout.h"

namespace gwa {
namespace bamin {

constexpr uint32_t kFlagPaired = 0x1, kFlagReverse = 0x10, kFlagMate1 = 0x40, kFlagMate2 = 0x80;
constexpr uint32_t kFlagNotARead = 0x100 | 0x800;  // secondary, supplementary: skipped by the framing walk
constexpr uint32_t kQualMax = 93;                  // + 33 = '~', the last character SAM QUAL prints
constexpr uint32_t kFixed = 36;                    // block_size and the 32 fixed bytes
// content errors of one record (the lowest of a record is reported)
enum : uint32_t { kOk = 0, kErrNameEmpty = 1, kErrNameNoNul = 2, kErrQual = 3 };

GWA_HD uint32_t ld16(const uint8_t *p) { return p[0] | (uint32_t)p[1] << 8; }
GWA_HD uint32_t ld32(const uint8_t *p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// "=ACMGRSVTWYHKDBN"[nib]
GWA_HD uint64_t letterOf(uint32_t nib) {
  const uint64_t lo = 0x565352474D43413DULL, hi = 0x4E42444B48595754ULL;
  return ((nib & 8 ? hi : lo) >> ((nib & 7) * 8)) & 0xFF;
}
// The codes are sets of bases (A 1, C 2, G 4, T 8), so the complement reverses the four bits: A<->T,
// C<->G, M<->K, R<->Y, V<->B, H<->D; S, W, N and '=' stay.
GWA_HD uint32_t compNib(uint32_t n) { return (n & 1) << 3 | (n & 2) << 1 | (n & 4) >> 1 | (n & 8) >> 3; }

GWA_HD uint64_t pad16(uint64_t n) { return (n + 15) & ~(uint64_t)15; }

// Bytes [p, p + 8) little-endian.  Device: two aligned 8-B loads funnel-shifted (the buffer starts 8-B
// aligned and has room behind it); host: the bytes before `end`, zero beyond.
GWA_HD uint64_t ld64u(const uint8_t *p, const uint8_t *end) {
#if defined(__HIP_DEVICE_COMPILE__)
  (void)end;
  const uintptr_t a = (uintptr_t)p;
  const uint32_t sh = (uint32_t)(a & 7) * 8;
  const uint64_t *q = (const uint64_t *)(a & ~(uintptr_t)7);
  const uint64_t lo = q[0];
  if (!sh) return lo;
  return lo >> sh | q[1] << (64 - sh);
#else
  uint64_t v = 0;
  if (p < end) memcpy(&v, p, (size_t)(end - p < 8 ? end - p : 8));
  return v;
#endif
}

struct Fields {
  uint32_t lName, nCigar, flag, lSeq;
  uint64_t seq, qual;  // byte offsets in the record (the name is at kFixed)
};
GWA_HD Fields fieldsOf(const uint8_t *rec) {
  Fields f;
  f.lName = rec[12];
  f.nCigar = ld16(rec + 16);
  f.flag = ld16(rec + 18);
  f.lSeq = ld32(rec + 20);
  f.seq = kFixed + (uint64_t)f.lName + 4ull * f.nCigar;
  f.qual = f.seq + ((uint64_t)f.lSeq + 1) / 2;
  return f;
}
// what the fields of a record need of its block_size
GWA_HD uint64_t fieldBytes(const Fields &f) { return f.qual + f.lSeq - 4; }

// the name: the bytes before the first NUL inside l_read_name bytes; *err = kErrNameEmpty / kErrNameNoNul
GWA_HD uint32_t nameLenOf(const uint8_t *rec, const Fields &f, uint32_t *err) {
  if (f.lName == 0) {
    *err = kErrNameEmpty;
    return 0;
  }
  for (uint32_t i = 0; i < f.lName; ++i)
    if (rec[kFixed + i] == 0) return i;
  *err = kErrNameNoNul;
  return f.lName;
}
// l_seq > 0 and qual[0] = 0xFF: the read has no quality
GWA_HD bool qualNullOf(const uint8_t *rec, const Fields &f) { return f.lSeq > 0 && rec[f.qual] == 0xFF; }
// the bytes of the read in the unpacked text: a SEQ slot and a QUAL slot of pad16(l_seq) each
GWA_HD uint64_t slotBytes(const Fields &f) { return 2 * pad16(f.lSeq); }

// SEQ chunk c (16 c < l_seq): 16 letters of the read as two little-endian words
GWA_HD void seqChunk(const uint8_t *rec, const uint8_t *end, const Fields &f, uint64_t c, uint64_t *lo, uint64_t *hi) {
  const uint64_t l = f.lSeq, j0 = 16 * c;
  const uint8_t *sq = rec + f.seq;
  uint64_t out[2] = {0, 0};
  if (!(f.flag & kFlagReverse)) {
    const uint64_t w = ld64u(sq + 8 * c, end);
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i)
      if (j0 + i < l) out[i >> 3] |= letterOf((uint32_t)(w >> (8 * (i >> 1) + (i & 1 ? 0 : 4))) & 15) << (8 * (i & 7));
  } else {
    // stored positions pHi down to max(pHi - 15, 0): at most nine packed bytes from `base`
    const uint64_t pHi = l - 1 - j0, pLo = pHi >= 15 ? pHi - 15 : 0, base = pLo >> 1;
    const uint64_t w = ld64u(sq + base, end);
    const uint32_t x = (pHi >> 1) - base == 8 ? sq[base + 8] : 0;
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i)
      if (j0 + i < l) {
        const uint64_t p = pHi - i, k = (p >> 1) - base;
        const uint32_t byte = k < 8 ? (uint32_t)(w >> (8 * k)) & 0xFF : x;
        out[i >> 3] |= letterOf(compNib(p & 1 ? byte & 15 : byte >> 4)) << (8 * (i & 7));
      }
  }
  *lo = out[0];
  *hi = out[1];
}

// QUAL chunk c (16 c < l_seq) of a record with a quality: byte + 33 each; false when one of its bytes is
// above kQualMax
GWA_HD bool qualChunk(const uint8_t *rec, const uint8_t *end, const Fields &f, uint64_t c, uint64_t *lo, uint64_t *hi) {
  const uint64_t l = f.lSeq, j0 = 16 * c;
  const uint8_t *q = rec + f.qual;
  uint64_t a, b;
  if (!(f.flag & kFlagReverse)) {
    a = ld64u(q + j0, end);
    b = ld64u(q + j0 + 8, end);
  } else {  // the 16 stored bytes ending at l - 1 - j0, reversed (it may start before QUAL: inside the record)
    const uint8_t *src = q + l - j0 - 16;
    a = __builtin_bswap64(ld64u(src + 8, end));
    b = __builtin_bswap64(ld64u(src, end));
  }
  const uint64_t valid = l - j0 < 16 ? l - j0 : 16;  // bytes of the chunk that belong to the read
  const uint64_t ma = valid >= 8 ? ~0ULL : (1ULL << (8 * valid)) - 1;
  const uint64_t mb = valid >= 16 ? ~0ULL : valid <= 8 ? 0 : (1ULL << (8 * (valid - 8))) - 1;
  a &= ma;
  b &= mb;
  // a byte is above 93 when its low seven bits + 34 carry into bit 7, or bit 7 is set
  const uint64_t k7 = 0x7F7F7F7F7F7F7F7FULL, k22 = 0x2222222222222222ULL, k80 = 0x8080808080808080ULL;
  const bool ok = (((((a & k7) + k22) | a) | (((b & k7) + k22) | b)) & k80) == 0;
  const uint64_t k21 = 0x2121212121212121ULL;
  *lo = (a + k21) & ma;  // (no carry between bytes when ok)
  *hi = (b + k21) & mb;
  return ok;
}

// ---- host only ----

inline std::string recordLabel(uint64_t index, uint64_t offset) {
  return "BAM record " + std::to_string(index) + " at byte " + std::to_string(offset) + ": ";
}

// The size of the header at the front of an inflated BAM: magic, l_text, text, n_ref, and per contig
// l_name, name, l_ref.  -1: the bytes end inside the header; -2: not a BAM (*why says so).
inline int64_t headerSize(const uint8_t *p, uint64_t len, std::string *why) {
  const uint64_t m = len < 4 ? len : 4;
  if (memcmp(p, "BAM\1", (size_t)m) != 0) {
    *why = "no BAM magic (the inflated bytes do not start with \"BAM\\1\")";
    return -2;
  }
  if (len < 8) return -1;
  uint64_t at = 8 + (uint64_t)ld32(p + 4);
  if (len < at + 4 || at + 4 < at) return -1;
  const uint32_t nRef = ld32(p + at);
  at += 4;
  for (uint32_t i = 0; i < nRef; ++i) {
    if (len < at + 4) return -1;
    at += 4 + (uint64_t)ld32(p + at) + 4;
    if (len < at) return -1;
  }
  return (int64_t)at;
}

// The block_size chain of bytes[0, len): the start of every record that is a read (relative to bytes)
// and, in idx, its number among all records from index0 on.  final: the chain must end exactly at len;
// otherwise the walk stops before a record that is not whole yet.  Returns the bytes walked, *nAll = the
// records in them.  A record whose fields do not fit fails as gwa_bam_sorter_add_records words it, with
// index0 and byte0 added to the record's index and offset.
inline uint64_t walkChain(const uint8_t *bytes, uint64_t len, bool final, uint64_t index0, uint64_t byte0,
                          std::vector<uint64_t> *starts, std::vector<uint64_t> *idx, uint64_t *nAll) {
  uint64_t at = 0, n = 0;
  auto bad = [&](const std::string &what) { throw std::runtime_error(recordLabel(index0 + n, byte0 + at) + what); };
  while (at < len) {
    if (len - at < 4) {
      if (!final) break;
      bad("the chain of block_size fields ends " + std::to_string(len - at) + " bytes before the data's end");
    }
    const uint32_t bs = ld32(bytes + at);
    if (bs < 32) bad("block_size " + std::to_string(bs) + " is below the 32 fixed bytes");
    if ((uint64_t)bs + 4 > len - at) {
      if (!final) break;
      bad("block_size " + std::to_string(bs) + " runs past the data's end (" + std::to_string(byte0 + len) + " bytes)");
    }
    const uint8_t *r = bytes + at;
    const Fields f = fieldsOf(r);
    if (f.lName > bs - 32) bad("the read name (" + std::to_string(f.lName) + " bytes) runs past the record");
    if ((uint64_t)f.lName + 4ull * f.nCigar > bs - 32) bad("the CIGAR (" + std::to_string(f.nCigar) + " elements) runs past the record");
    if (fieldBytes(f) > bs) bad("SEQ and QUAL (l_seq " + std::to_string(f.lSeq) + ") run past the record");
    if (!(f.flag & kFlagNotARead)) {
      starts->push_back(at);
      if (idx) idx->push_back(index0 + n);
    }
    ++n;
    at += (uint64_t)bs + 4;
  }
  if (nAll) *nAll = n;
  return at;
}

// what is wrong with the content of one (framed) record, "" when nothing
inline std::string recordProblem(const uint8_t *rec) {
  const Fields f = fieldsOf(rec);
  uint32_t err = kOk;
  (void)nameLenOf(rec, f, &err);
  if (err == kErrNameEmpty) return "l_read_name is 0 (a read name holds at least its NUL)";
  if (err == kErrNameNoNul) return "the read name has no NUL inside its l_read_name " + std::to_string(f.lName) + " bytes";
  if (!qualNullOf(rec, f))
    for (uint32_t i = 0; i < f.lSeq; ++i)
      if (rec[f.qual + i] > kQualMax)
        return "quality byte " + std::to_string(i) + " is " + std::to_string(rec[f.qual + i]) + " (at most 93 prints as SAM QUAL)";
  return "";
}

// One read of the host build: its name length, and its SEQ and QUAL slots written chunk by chunk as the
// kernel writes them (seqOut and qualOut: pad16(l_seq) bytes each).  Returns the record's content error.
inline uint32_t decodeRecord(const uint8_t *rec, const uint8_t *end, uint32_t *nameLen, bool *qualNull, uint8_t *seqOut,
                             uint8_t *qualOut) {
  const Fields f = fieldsOf(rec);
  uint32_t err = kOk;
  *nameLen = nameLenOf(rec, f, &err);
  *qualNull = qualNullOf(rec, f);
  const uint64_t chunks = pad16(f.lSeq) / 16;
  for (uint64_t c = 0; c < chunks; ++c) {
    uint64_t w[2];
    seqChunk(rec, end, f, c, &w[0], &w[1]);
    memcpy(seqOut + 16 * c, w, 16);
    if (*qualNull) {
      w[0] = w[1] = 0;
    } else if (!qualChunk(rec, end, f, c, &w[0], &w[1]) && err == kOk) {
      err = kErrQual;
    }
    memcpy(qualOut + 16 * c, w, 16);
  }
  return err;
}

// An interleaved BAM's pairs: kept records 2i and 2i + 1 must carry 0x1 | 0x40 and 0x1 | 0x80.  Throws for
// the lowest pair of the slice that does not, as pair pair0 + i.
inline void checkMateFlags(const uint8_t *bytes, const uint64_t *starts, uint64_t np, uint64_t pair0) {
  for (uint64_t i = 0; i < np; ++i) {
    const uint32_t f1 = ld16(bytes + starts[2 * i] + 18), f2 = ld16(bytes + starts[2 * i + 1] + 18);
    const uint32_t w1 = kFlagPaired | kFlagMate1, w2 = kFlagPaired | kFlagMate2;
    if ((f1 & w1) != w1 || (f2 & w2) != w2)
      throw std::runtime_error("the records of pair " + std::to_string(pair0 + i) + " carry FLAG " + std::to_string(f1) + " and " +
                               std::to_string(f2) + ": an interleaved BAM holds mate 1 (0x1 and 0x40) and then mate 2 (0x1 and "
                               "0x80) of each pair; a coordinate-sorted file does not");
  }
}

}  // namespace bamin
}  // namespace gwa
