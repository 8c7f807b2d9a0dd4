// sam_core.h -- the SAM records of one read, written by one GPU lane (or by the host test harness):
//   AlignmentRecord.convert   (R/AlignmentRecord.java:181-276)
//   AlignmentRecord.toSAMLine (R/AlignmentRecord.java:109-170)
//   SAMOutput.emit            (A/SAMOutput.java:73-82)
// The same function measures a record (SamOut with p == nullptr counts bytes) and writes it, so the
// device formats a batch in two passes: lengths, an exclusive scan, then every read's text at its
// offset (batch_io.hip).  SAM flag values follow the SAM spec (utgb SAMReadFlag is unvendored;
// SURVEY.md §8c).
//
// The bulk fields of a line (read name, SEQ, QUAL) go through SamOut::text / seq / qual.  On the host
// and in counting mode they are copied (or counted) at once.  In the device write pass a lane only
// advances its cursor over a bulk field of more than kSamDeferMin bytes and leaves a SamField
// descriptor in LDS; the workgroup then copies all deferred fields together with coalesced 16-B
// loads (batch_io.hip samServeFields).  Everything else is written by the lane itself.
#pragma once
#include "gwa_layout.h"

namespace gwa {

// Read text and contig names as the formatter reads them (device or host memory).  Read r's name
// is name[nameB[r], nameE[r]) and its quality qual[qualB[r], qualE[r]): SoA blobs (nameE = nameB + 1)
// or the fields of FASTQ records inside the file text itself.
struct SamText {
  const char *name;
  const uint64_t *nameB, *nameE;
  const char *qual;          // nullptr: no qualities (SAM "*", as for FASTA input)
  const uint64_t *qualB, *qualE;
  const uint8_t *qualNull;   // nullptr, or per read: nonzero = this read's quality is null ("*")
  const uint8_t *codes;      // ReadsView: the read as codes 0..4 (spaces skipped)
  const uint32_t *codeOff, *codeLen;
  const char *ctg;           // contig names
  const uint64_t *ctgOff;    // nContig + 1
  const int32_t *chrKey;     // per contig: equal names <=> equal keys (String.equals)
  int32_t starKey, emptyKey; // the keys of the names "*" and "" (a contig may be called that)
  // optional tags (tags & kSamTagMd: MD:Z, samfmt::mdTag): the index's forward text (IndexView::text2 /
  // textN) and each contig's start offset in it and length.  The defaults mean "no MD".
  const uint64_t *text2 = nullptr, *textN = nullptr;
  const int64_t *ctgStart = nullptr, *ctgLen = nullptr;
  uint32_t tags = 0;
};
constexpr uint32_t kSamTagMd = 1u;  // GWA_SAM_TAG_MD (include/gwa.h)

// A bulk field left to the workgroup (device write pass): out[i] = f(src[i]), or, for the reversed
// kinds, out[i] = f(src[len - 1 - i]), at byte `at` of the workgroup's staging buffer.
enum : uint32_t {
  SAM_COPY = 0,    // bytes as they are
  SAM_SEQ = 1,     // codes 0..4 -> ACGTN
  SAM_SEQ_RC = 2,  // reversed, codes -> the complement's letter
  SAM_REV = 3      // reversed bytes
};
constexpr uint32_t kSamDeferMin = 16;       // longer fields are deferred, shorter ones copied by the lane
constexpr uint32_t kSamDeferMax = 1 << 14;  // (14 bits of length in a descriptor)
struct SamField {
  uint32_t srcLo, srcHi;  // source address
  uint32_t w;             // at | len << 16 | kind << 30
};
struct SamDefer {
  SamField *f = nullptr;      // descriptor list (LDS); nullptr: nothing is deferred
  uint32_t *count = nullptr;  // fields pushed so far (may exceed cap: those were copied at once)
  uint32_t cap = 0;
  char *stage = nullptr;      // the staging buffer `at` is relative to
};
#if defined(__HIP_DEVICE_COMPILE__)
// up to 16 bytes of read text copied by one lane (batch_io.hip)
__device__ void samSmallCopy(char *dst, const char *src, uint32_t len);
#endif

// byte sink: counts when p == nullptr
struct SamOut {
  char *p;
  uint64_t n;
  SamDefer d{};  // device write pass: where bulk fields are deferred to
  GWA_HD void ch(char c) {
    if (p) p[n] = c;
    ++n;
  }
  // true: the field [p + n, p + n + len) was left to the workgroup and the cursor moved past it
  GWA_HD bool defer(const void *src, uint64_t len, uint32_t kind) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (d.f && len > kSamDeferMin && len < kSamDeferMax) {
      const uint32_t slot = atomicAdd(d.count, 1u);
      if (slot < d.cap) {
        const uint64_t a = (uint64_t)src;
        d.f[slot] = SamField{(uint32_t)a, (uint32_t)(a >> 32),
                             (uint32_t)(p + n - d.stage) | (uint32_t)len << 16 | kind << 30};
        n += len;
        return true;
      }
    }
#endif
    return false;
  }
  // Text copies run 16 bytes per pass with the 16 loads issued before any store (short fields, contig
  // names and literals on the device; every field on the host)
  GWA_HD void bytes(const char *s, uint64_t len) {
    if (p) {
      for (uint64_t i = 0; i < len; i += 16) {
        char b[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) b[k] = i + k < len ? s[i + k] : 0;
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if (i + k < len) p[n + i + k] = b[k];
      }
    }
    n += len;
  }
  // read text (a name, a forward quality): s lies in a text allocation padded for 16-B chunk loads
  GWA_HD void text(const char *s, uint64_t len) {
    if (defer(s, len, SAM_COPY)) return;
#if defined(__HIP_DEVICE_COMPILE__)
    if (p && len <= 16) {
      samSmallCopy(p + n, s, (uint32_t)len);
      n += len;
      return;
    }
#endif
    bytes(s, len);
  }
  // SEQ: positions [a, b) of the read c[0, m) as letters; rc: of its reverse complement
  GWA_HD void seq(const uint8_t *c, int m, int a, int b, bool rc);
  // QUAL: positions [a, b) of the quality q[0, qn); rev: of the reversed quality
  GWA_HD void qual(const char *q, uint64_t qn, int a, int b, bool rev);
  template <unsigned long L>
  GWA_HD void lit(const char (&s)[L]) {  // a string literal (without its terminating 0)
    bytes(s, L - 1);
  }
  GWA_HD void num(int64_t v) {  // Integer.toString
    // the digits, least significant first, packed 8 per register (no runtime-indexed array, which
    // would live in scratch memory on the device)
    const bool neg = v < 0;
    uint64_t u = neg ? (uint64_t)(-(v + 1)) + 1 : (uint64_t)v;
    uint64_t d0 = 0, d1 = 0, d2 = 0;
    int k = 0;
    do {
      const uint64_t q = u / 10, dig = u - q * 10;
      if (k < 8) d0 |= dig << (8 * k);
      else if (k < 16) d1 |= dig << (8 * (k - 8));
      else d2 |= dig << (8 * (k - 16));
      ++k;
      u = q;
    } while (u);
    if (neg) ch('-');
    for (int i = k - 1; i >= 0; --i) {
      const uint64_t w = i < 8 ? d0 : i < 16 ? d1 : d2;
      ch((char)('0' + (int)((w >> (8 * (i & 7))) & 0xFF)));
    }
  }
};

// Read.getQual(0) == null for read r: the batch has no qualities or this read has none
GWA_HD bool qualAbsent(const SamText &t, uint32_t r) { return t.qual == nullptr || (t.qualNull && t.qualNull[r]); }

namespace samfmt {

constexpr char kSym[5] = {'A', 'C', 'G', 'T', 'N'};
// kSym[x] as a shift of one packed constant (a table lookup is a memory load per base on the device)
GWA_HD char sym(unsigned x) { return (char)((0x4E54474341ULL >> (8 * x)) & 0xFF); }
constexpr char kOp[8] = {'M', 'I', 'D', 'N', 'S', 'H', 'P', 'X'};
}  // namespace samfmt

// (16 positions per pass, loads first: SamOut::bytes)
GWA_HD void SamOut::seq(const uint8_t *c, int m, int a, int b, bool rc) {
  if (b <= a) return;
  if (!p) {
    n += (uint64_t)(b - a);
    return;
  }
  if (defer(rc ? c + (m - b) : c + a, (uint64_t)(b - a), rc ? SAM_SEQ_RC : SAM_SEQ)) return;
  for (int j0 = a; j0 < b; j0 += 16) {
    uint8_t x[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int j = j0 + k;
      x[k] = j < b ? (rc ? c[m - 1 - j] : c[j]) : 0;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (j0 + k < b) ch(samfmt::sym(rc ? (x[k] < 4 ? 3 - x[k] : 4) : (x[k] > 4 ? 4 : x[k])));
  }
}

GWA_HD void SamOut::qual(const char *q, uint64_t qn, int a, int b, bool rev) {
  if (b <= a) return;
  if (!p) {
    n += (uint64_t)(b - a);
    return;
  }
  if (defer(rev ? q + (qn - (uint64_t)b) : q + a, (uint64_t)(b - a), rev ? SAM_REV : SAM_COPY)) return;
  for (int j0 = a; j0 < b; j0 += 16) {
    char x[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int j = j0 + k;
      x[k] = j < b ? (rev ? q[qn - 1 - j] : q[j]) : 0;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (j0 + k < b) ch(x[k]);
  }
}

namespace samfmt {

GWA_HD char stateCh(int numHits) { return numHits > 0 ? (numHits == 1 ? 'U' : 'R') : 'N'; }

// CIGAR of a record as items: elements copied from a hit's list keep that list as it is (a fresh
// CIGAR built from an element list), later add() calls merge with the last element
// (CIGAR.add, A/CIGAR.java:158-170)
struct CigSpec {
  const uint16_t *a;  // first element list (raw), or nullptr
  int na;
  int preS;           // -1, or add(S, preS) first (on an empty CIGAR)
  int postS;          // -1, or add(S, postS) after list a
  const uint16_t *b;  // elements added one by one after list a (merged), or nullptr
  int nb;
};

struct CigEmit {
  SamOut &o;
  int pt = -1;
  int64_t pl = 0;
  GWA_HD explicit CigEmit(SamOut &o_) : o(o_) {}
  GWA_HD void flush() {
    if (pt >= 0) {
      o.num(pl);
      o.ch(kOp[pt & 7]);
    }
  }
  GWA_HD void raw(int t, int64_t l) {
    flush();
    pt = t;
    pl = l;
  }
  GWA_HD void add(int t, int64_t l) {
    if (pt == t) pl += l;
    else raw(t, l);
  }
};

// The items of c handed to e (raw / add / flush as CigEmit has them): the printed CIGAR's elements, for
// the BAM writer (bam_core.h).  emitCigar below, lineOne and samMateLine keep their own statements next to
// cigarItems, lineFlag, rnextSame and mateFlag: routing the SAM emitters through the helpers changes the
// code the compiler generates for samLenKernel / samWriteKernel, and those kernels are to stay as they are
// (their disassembly is unchanged).  tests/test_bam_host.py holds the two sides together: every BAM field is
// compared with the line the SAM emitter prints for the same hits.
template <class E>
GWA_HD void cigarItems(E &e, const CigSpec &c) {
  if (c.preS >= 0) e.add(4, c.preS);
  for (int i = 0; i < c.na; ++i) e.raw(c.a[i] & 7, c.a[i] >> 3);
  if (c.postS >= 0) e.add(4, c.postS);
  for (int i = 0; i < c.nb; ++i) e.add(c.b[i] & 7, c.b[i] >> 3);
  e.flush();
}

GWA_HD void emitCigar(SamOut &o, const CigSpec &c) {
  CigEmit e(o);
  if (c.preS >= 0) e.add(4, c.preS);
  for (int i = 0; i < c.na; ++i) e.raw(c.a[i] & 7, c.a[i] >> 3);
  if (c.postS >= 0) e.add(4, c.postS);
  for (int i = 0; i < c.nb; ++i) e.add(c.b[i] & 7, c.b[i] >> 3);
  e.flush();
}

// ---- MD:Z (SamText::tags & kSamTagMd) ----
// The tag is defined from the printed line alone: walk the printed CIGAR from POS on
// the printed contig and compare the printed SEQ with the contig; a base outside [1, contig length],
// an N on either side and a SEQ position past the end of SEQ never match.  The reference has no MD.
// Matches are counted 32 bases per step: the contig window as text2 / textN words, the read's codes
// from 16-B chunks of its row packed to 2-bit fields, compared by XOR; only mismatches and deleted
// bases are looked at one by one.

// reverse the order of the 32 two-bit fields / of the 32 bits
GWA_HD uint64_t mdRev2(uint64_t x) {
  x = ((x >> 2) & 0x3333333333333333ULL) | ((x & 0x3333333333333333ULL) << 2);
  x = ((x >> 4) & 0x0F0F0F0F0F0F0F0FULL) | ((x & 0x0F0F0F0F0F0F0F0FULL) << 4);
  return __builtin_bswap64(x);
}
GWA_HD uint32_t mdRev1(uint32_t x) {
  x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
  x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
  x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
  return __builtin_bswap32(x);
}

// chunk k (16 codes 0..4) of a read's code row as 16 two-bit fields and 16 N flags; rows are 16-B
// aligned and zero-padded to a multiple of 16 (ReadsView), chunks outside [0, m) read as zero
GWA_HD void mdChunk(const uint8_t *row, int m, int k, uint64_t *c2, uint64_t *nn) {
  *c2 = 0;
  *nn = 0;
  if (k < 0 || 16 * k >= m) return;
  uint32_t w[4];
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 v = *reinterpret_cast<const uint4 *>(row + 16 * k);
  w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
#else
  __builtin_memcpy(w, row + 16 * k, 16);
#endif
  uint32_t c = 0, n = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t x = w[i] & 0x03030303u;  // the low two bits of each byte, gathered into one byte
    x = (x | x >> 6) & 0x000F000Fu;
    x = (x | x >> 12) & 0xFFu;
    uint32_t y = (w[i] >> 2) & 0x01010101u;  // bit 2 (code 4 = N) of each byte, into four bits
    y = (y | y >> 7) & 0x00030003u;
    y = (y | y >> 14) & 0xFu;
    c |= x << (8 * i);
    n |= y << (4 * i);
  }
  *c2 = c;
  *nn = n;
}

// the printed SEQ: positions [seqA, seqA + seqLen) of the read row[0, m), or of its reverse complement
struct MdSeq {
  const uint8_t *row;
  int m, seqA, seqLen;
  bool rc;
};

// SEQ[q, q + 32) as two-bit fields and N flags; positions past the end of SEQ are N
GWA_HD void mdSeqWin(const MdSeq &s, int q, uint64_t *codes, uint32_t *nb) {
  const int left = s.seqLen - q;
  if (left <= 0) {
    *codes = 0;
    *nb = 0xFFFFFFFFu;
    return;
  }
  // the 32 read positions [a, a + 32) behind them (-31 <= a: the reverse strand reads them backwards)
  const int j = s.seqA + q;
  const int a = s.rc ? s.m - 1 - j - 31 : j;
  const int k0 = ((a + 32) >> 4) - 2, sh = a - 16 * k0;
  uint64_t c0, c1, c2, n0, n1, n2;
  mdChunk(s.row, s.m, k0, &c0, &n0);
  mdChunk(s.row, s.m, k0 + 1, &c1, &n1);
  c2 = n2 = 0;
  if (sh) mdChunk(s.row, s.m, k0 + 2, &c2, &n2);
  const uint64_t lo = c0 | c1 << 32;
  uint64_t c = sh ? (lo >> (2 * sh)) | (c2 << (64 - 2 * sh)) : lo;
  uint32_t n = (uint32_t)((n0 | n1 << 16 | n2 << 32) >> sh);
  if (s.rc) {
    c = ~mdRev2(c);
    n = mdRev1(n);
  }
  *codes = c;
  *nb = left < 32 ? n | 0xFFFFFFFFu << left : n;
}

// text positions [p, p + cnt) (1 <= cnt <= 32, all inside the text) as two-bit fields and N flags
GWA_HD void mdTextWin(const uint64_t *t2, const uint64_t *tn, int64_t p, int cnt, uint64_t *codes, uint32_t *nb) {
  const int64_t a = p >> 5, b = p >> 6;
  const int sa = (int)(p & 31), sn = (int)(p & 63);
  const uint64_t a0 = t2[a], a1 = sa + cnt > 32 ? t2[a + 1] : 0ULL;
  const uint64_t n0 = tn[b], n1 = sn + cnt > 64 ? tn[b + 1] : 0ULL;
  *codes = sa ? (a0 >> (2 * sa)) | (a1 << (64 - 2 * sa)) : a0;
  *nb = (uint32_t)(sn ? (n0 >> sn) | (n1 << (64 - sn)) : n0);
}

struct MdWalk {
  SamOut o;
  const uint64_t *t2, *tn;
  int64_t cs, cl;  // the contig: start offset in the text, length
  MdSeq s;
  int64_t r;       // 1-based position on the contig (may lie outside it)
  int q = 0;       // position in SEQ
  int64_t run = 0;
  int pt = -1;     // the pending CIGAR element, merged as CigEmit merges
  int64_t pl = 0;

  GWA_HD char refLetter(int64_t x) const {
    if (x < 1 || x > cl) return 'N';
    const int64_t p = cs + x - 1;
    if ((tn[p >> 6] >> (p & 63)) & 1) return 'N';
    return sym((unsigned)((t2[p >> 5] >> ((p & 31) * 2)) & 3));
  }
  GWA_HD void miss(char c) {
    o.num(run);
    o.ch(c);
    run = 0;
  }
  // k bases off the contig: N, never a match
  GWA_HD void outside(int64_t k) {
    for (int64_t i = 0; i < k; ++i) miss('N');
    r += k;
    q += (int)k;
  }
  GWA_HD void match(int64_t l) {
    // the element clamped to the contig, once: [r, r + l) = before | inside | behind
    const int64_t before = r >= 1 ? 0 : (1 - r < l ? 1 - r : l);
    const int64_t room = cl - (r + before) + 1;  // of the contig, from the first base not before it
    int64_t inside = l - before;
    if (inside > room) inside = room > 0 ? room : 0;
    const int64_t behind = l - before - inside;
    outside(before);
    while (inside > 0) {
      const int cnt = inside > 32 ? 32 : (int)inside;
      uint64_t tw, sw;
      uint32_t tN, sN;
      mdTextWin(t2, tn, cs + r - 1, cnt, &tw, &tN);
      mdSeqWin(s, q, &sw, &sN);
      const uint64_t x = tw ^ sw;
      uint64_t nz = (x | (x >> 1)) & 0x5555555555555555ULL;
      uint32_t nm = tN | sN;
      int base = 0;
      for (;;) {
        const int j1 = nz ? __builtin_ctzll(nz) >> 1 : 32, j2 = nm ? __builtin_ctz(nm) : 32;
        const int j = j1 < j2 ? j1 : j2;
        if (j >= cnt) break;
        run += j - base;
        miss(((tN >> j) & 1) ? 'N' : sym((unsigned)((tw >> (2 * j)) & 3)));
        base = j + 1;
        nz &= ~(3ULL << (2 * j));
        nm &= ~(1u << j);
      }
      run += cnt - base;
      r += cnt;
      q += cnt;
      inside -= cnt;
    }
    outside(behind);
  }
  GWA_HD void element(int t, int64_t l) {
    if (t == 0 || t == 7) {  // M X (the writer never prints '=')
      match(l);
    } else if (t == 2) {  // D
      o.num(run);
      o.ch('^');
      for (int64_t i = 0; i < l; ++i) o.ch(refLetter(r + i));
      run = 0;
      r += l;
    } else if (t == 3) {  // N
      r += l;
    } else if (t == 1 || t == 4) {  // I S
      q += (int)l;
    }
  }
  GWA_HD void flush() {
    if (pt >= 0) element(pt, pl);
  }
  GWA_HD void raw(int t, int64_t l) {
    flush();
    pt = t;
    pl = l;
  }
  GWA_HD void add(int t, int64_t l) {
    if (pt == t) pl += l;
    else raw(t, l);
  }
};

// "\tMD:Z:<value>" of one line at p + n (p == nullptr: counted); returns the new n.  Not inlined: the
// writer's callers are inlined into each of samChain's record forms.
GWA_HDNI inline uint64_t mdEmit(char *p, uint64_t n, const uint64_t *t2, const uint64_t *tn, int64_t cs, int64_t cl,
                                int64_t pos, const uint16_t *ca, int na, int preS, int postS, const uint16_t *cb, int nb,
                                const uint8_t *row, int m, int seqA, int seqLen, bool rc) {
  MdWalk w{SamOut{p, n}, t2, tn, cs, cl, MdSeq{row, m, seqA, seqLen, rc}, pos};
  w.o.lit("\tMD:Z:");
  // the printed CIGAR's elements (emitCigar)
  if (preS >= 0) w.add(4, preS);
  for (int i = 0; i < na; ++i) w.raw(ca[i] & 7, ca[i] >> 3);
  if (postS >= 0) w.add(4, postS);
  for (int i = 0; i < nb; ++i) w.add(cb[i] & 7, cb[i] >> 3);
  w.flush();
  w.o.num(w.run);
  return w.o.n;
}

// the MD tag of a mapped line on contig chr >= 0 at POS pos with the printed CIGAR c, whose SEQ is
// [seqA, seqB) of read r's strand-oriented query
GWA_HD void mdTag(SamOut &o, const SamText &t, uint32_t r, int chr, int64_t pos, const CigSpec &c, int seqA, int seqB,
                  bool rc) {
  o.n = mdEmit(o.p, o.n, t.text2, t.textN, t.ctgStart[chr], t.ctgLen[chr], pos, c.a, c.na, c.preS, c.postS, c.b, c.nb,
               t.codes + t.codeOff[r], (int)t.codeLen[r], seqA, seqB > seqA ? seqB - seqA : 0, rc);
}

// one AlignmentRecord to print
struct Rec {
  int chr, strand, start, end, nm, numBestHits;
  CigSpec cig;
  int seqA, seqB;       // SEQ = the strand-oriented query [seqA, seqB)
  int qualA, qualB;     // QUAL = the strand-oriented quality [qualA, qualB)
  int stateHead, stateSelf;  // XP = ReadHit.getAlignmentState over the chain from stateHead
  bool hasSplit;
};

struct Ctx {
  const SamText &t;
  uint32_t r;
  const OutHit *hits;   // the read's hits (chain indices are relative to this)
  int m;
  int strand;           // of the chain head: orientation of SEQ / QUAL
  bool qualNull;
  uint64_t q0, qn;      // quality text [q0, q0 + qn)
  bool npe = false;     // the reference would throw
};

GWA_HD int32_t nameKey(const Ctx &cx, int chr) {
  if (chr >= 0) return cx.t.chrKey[chr];
  if (chr == CHR_STAR) return cx.t.starKey;
  if (chr == CHR_EMPTY) return cx.t.emptyKey;
  return -2147483647 - 1;
}

GWA_HD void chrName(SamOut &o, Ctx &cx, int chr) {
  if (chr >= 0) o.bytes(cx.t.ctg + cx.t.ctgOff[chr], cx.t.ctgOff[chr + 1] - cx.t.ctgOff[chr]);
  else if (chr == CHR_STAR) o.ch('*');
  else if (chr == CHR_EMPTY) {
  } else cx.npe = true;  // null chr
}

GWA_HD void emitSeq(SamOut &o, const Ctx &cx, int a, int b) {
  o.seq(cx.t.codes + cx.t.codeOff[cx.r], cx.m, a, b, cx.strand != 0);
}

GWA_HD void emitQual(SamOut &o, const Ctx &cx, int a, int b) {
  if (cx.qualNull) {
    o.ch('*');
    return;
  }
  o.qual(cx.t.qual + cx.q0, cx.qn, a, b, cx.strand != 0);
}

template <class O>
GWA_HD void emitState(O &o, const Ctx &cx, int head, int self) {
  for (int t = head; t >= 0; t = cx.hits[t].next) {
    const char c = stateCh(cx.hits[t].numHits);
    o.ch(t == self ? c : (char)(c - 'A' + 'a'));
  }
}

// AlignmentRecord.toSAMLine (R/AlignmentRecord.java:109-170) of one record; returns the
// eachFragmentIsMapped value handed on to the split record's line
// FLAG of one record's line as lineOne computes it; eachMapped is updated to the value handed on to the
// split record's line
GWA_HD int lineFlag(const Rec &r, const Rec *split, bool hasSegments, bool isFirst, bool &eachMapped) {
  int flag = 0;
  if (hasSegments) flag |= 0x1;
  if (r.strand == 1) flag |= 0x10;
  if (isFirst) {
    flag |= 0x40;
    if (r.numBestHits <= 0 || (split && split->numBestHits <= 0)) eachMapped = false;
  } else if (!split) {
    flag |= 0x80;
  }
  if (eachMapped) flag |= 0x2;
  if (r.numBestHits <= 0) flag |= 0x4;
  if (split && split->numBestHits <= 0) flag |= 0x8;
  return flag;
}

// lineOne's RNEXT prints "=": both contigs are named alike and not "*"
GWA_HD bool rnextSame(const Ctx &cx, const Rec &r, const Rec &split) {
  const int32_t ck = nameKey(cx, r.chr), sk = nameKey(cx, split.chr);
  return r.chr != CHR_NULL && split.chr != CHR_NULL && ck != cx.t.starKey && ck == sk;
}

GWA_HD bool lineOne(SamOut &o, Ctx &cx, const Rec &r, const Rec *split, bool hasSegments, bool isFirst, bool eachMapped) {
  int flag = 0;
  if (hasSegments) flag |= 0x1;
  if (r.strand == 1) flag |= 0x10;
  if (isFirst) {
    flag |= 0x40;
    if (r.numBestHits <= 0 || (split && split->numBestHits <= 0)) eachMapped = false;
  } else if (!split) {
    flag |= 0x80;
  }
  if (eachMapped) flag |= 0x2;
  if (r.numBestHits <= 0) flag |= 0x4;
  if (split && split->numBestHits <= 0) flag |= 0x8;
  o.text(cx.t.name + cx.t.nameB[cx.r], cx.t.nameE[cx.r] - cx.t.nameB[cx.r]);
  o.ch('\t');
  o.num(flag);
  o.ch('\t');
  chrName(o, cx, r.chr);
  o.ch('\t');
  o.num(r.start);
  o.lit("\t1\t");  // MAPQ column = AlignmentRecord.score, always 1 (:199)
  emitCigar(o, r.cig);
  if (!split) {
    o.lit("\t*\t0\t0");
  } else {
    const int32_t ck = nameKey(cx, r.chr), sk = nameKey(cx, split->chr);
    if (r.chr != CHR_NULL && split->chr != CHR_NULL && ck != cx.t.starKey && ck == sk) {
      o.lit("\t=");
    } else {
      o.ch('\t');
      chrName(o, cx, split->chr);
    }
    o.ch('\t');
    o.num(split->start);
    o.ch('\t');
    o.num((int64_t)split->end - r.start);
  }
  o.ch('\t');
  emitSeq(o, cx, r.seqA, r.seqB);
  o.ch('\t');
  emitQual(o, cx, r.qualA, r.qualB);
  if (r.numBestHits > 0) {
    if (r.nm >= 0) {
      o.lit("\tNM:i:");
      o.num(r.nm);
    }
    o.lit("\tXP:Z:");
    emitState(o, cx, r.stateHead, r.stateSelf);
    o.lit("\tX0:i:");
    o.num(r.numBestHits);
    if ((cx.t.tags & kSamTagMd) && r.chr >= 0) mdTag(o, cx.t, cx.r, r.chr, r.start, r.cig, r.seqA, r.seqB, cx.strand != 0);
  }
  return eachMapped;
}

// a record and, when it has one, its split record on the next line
GWA_HD void emitRec(SamOut &o, Ctx &cx, const Rec &r, const Rec *split, bool hasSegments) {
  const bool em = lineOne(o, cx, r, split, hasSegments, true, true);
  if (split) {
    o.ch('\n');
    lineOne(o, cx, *split, nullptr, hasSegments, false, em);
  }
}

// the end of a chain's records
GWA_HD void chainEnd(SamOut &o, const Ctx &) { o.ch('\n'); }

}  // namespace samfmt

// samChain, samRead and samPair choose the records (the split forms, the pair choice, the rescued mate)
// for any sink O that has emitRec / chainEnd / samUnmapped / samMateLine overloads: SamOut here, the BAM
// records' BamOut in bam_core.h.

// One reported ReadHit chain (head = index into hits) -> SAM text, '\n' terminated.  Returns 0, or
// -1 where the reference would throw (the run aborts, S/BidirectionalSuffixFilter.java:264-267).
template <class O>
GWA_HD int samChain(O &o, const SamText &t, uint32_t r, const OutHit *hits, const uint16_t *cig, int head) {
  using namespace samfmt;
  const OutHit &h = hits[head];
  Ctx cx{t, r, hits, (int)t.codeLen[r], h.strand != 0 ? 1 : 0, qualAbsent(t, r), 0, 0};
  if (!cx.qualNull) {
    cx.q0 = t.qualB[r];
    cx.qn = t.qualE[r] - t.qualB[r];
  }
  const int m = cx.m;
  const int fullQual = cx.qualNull ? 0 : (int)cx.qn;
  Rec rec{};
  rec.cig = CigSpec{cig + h.cigarOff, (int)h.cigarLen, -1, -1, nullptr, 0};
  rec.seqA = 0; rec.seqB = m;
  rec.qualA = 0; rec.qualB = fullQual;
  rec.stateHead = head;
  rec.stateSelf = head;
  if (h.next < 0) {
    rec.chr = h.chr; rec.strand = h.strand; rec.start = h.pos; rec.end = h.pos + h.matchLength; rec.nm = h.diff;
    rec.numBestHits = h.numHits;
    emitRec(o, cx, rec, nullptr, false);
  } else {
    // the head and its first split are converted; later fragments of a longer chain are dropped
    // (R/AlignmentRecord.java:201-206 reads hit.nextSplit only), but still named in XP
    const OutHit &s = hits[h.next];
    const int numHits = h.numHits;
    const int qualLen = !cx.qualNull ? (int)cx.qn : h.matchLength;
    const bool hU = h.numHits == 1, sU = s.numHits == 1;
    // substrings taken by convert (:187-196): a bad range is a Java exception
    auto bad = [](int a, int b, int size) { return a < 0 || b > size || a > b; };
    const int b1 = qualLen < h.matchLength ? qualLen : h.matchLength;
    const int b2 = qualLen < m ? qualLen : m;
    if (bad(h.qStart, h.qEnd, m) || bad(s.qStart, s.qEnd, m)) return -1;
    if (!cx.qualNull && (bad(0, b1, (int)cx.qn) || bad(b1, b2, (int)cx.qn))) return -1;
    if (hU) {
      if (sU) {
        if (h.chr == CHR_NULL) return -1;
        bool same = (h.chr >= 0 && s.chr >= 0) ? t.chrKey[h.chr] == t.chrKey[s.chr] : h.chr == s.chr;
        if (s.chr == CHR_NULL) same = false;
        if (same) {
          Rec srec{};
          rec.chr = h.chr; rec.strand = h.strand; rec.start = h.pos; rec.end = h.pos + h.matchLength; rec.nm = h.diff;
          rec.seqA = h.qStart; rec.seqB = h.qEnd; rec.qualA = 0; rec.qualB = b1; rec.numBestHits = 1;
          srec.chr = s.chr; srec.strand = s.strand; srec.start = s.pos; srec.end = s.pos + s.matchLength; srec.nm = s.diff;
          srec.cig = CigSpec{cig + s.cigarOff, (int)s.cigarLen, -1, -1, nullptr, 0};
          srec.seqA = s.qStart; srec.seqB = s.qEnd; srec.qualA = b1; srec.qualB = b2; srec.numBestHits = 1;
          srec.stateHead = head;
          srec.stateSelf = h.next;
          if (cx.qualNull) { rec.qualB = srec.qualB = 0; }
          emitRec(o, cx, rec, &srec, true);
        } else if (h.matchLength >= s.matchLength) {
          rec.cig.postS = s.matchLength;
          rec.chr = h.chr; rec.strand = h.strand; rec.start = h.pos; rec.end = h.pos + m; rec.nm = h.diff;
          rec.numBestHits = numHits;
          emitRec(o, cx, rec, nullptr, false);
        } else {
          if (s.chr == CHR_NULL) return -1;
          rec.cig.b = cig + s.cigarOff;
          rec.cig.nb = (int)s.cigarLen;
          rec.chr = s.chr; rec.strand = s.strand; rec.start = s.pos - h.matchLength; rec.end = s.pos - h.matchLength + m;
          rec.nm = s.diff; rec.numBestHits = numHits; rec.stateSelf = h.next;
          emitRec(o, cx, rec, nullptr, false);
        }
      } else {
        if (h.chr == CHR_NULL) return -1;
        rec.cig.postS = s.qEnd - s.qStart;
        rec.chr = h.chr; rec.strand = h.strand; rec.start = h.pos; rec.end = h.pos; rec.nm = h.diff;
        rec.numBestHits = numHits;
        emitRec(o, cx, rec, nullptr, false);
      }
    } else {
      if (!sU) return 0;  // convert returns null: SAMOutput.emit prints nothing (:78-81)
      if (s.chr == CHR_NULL) return -1;
      rec.cig = CigSpec{nullptr, 0, h.matchLength, -1, cig + s.cigarOff, (int)s.cigarLen};
      rec.chr = s.chr; rec.strand = s.strand; rec.start = s.pos - h.matchLength; rec.end = s.pos - h.matchLength + m;
      rec.nm = s.diff; rec.numBestHits = numHits; rec.stateSelf = h.next;
      emitRec(o, cx, rec, nullptr, false);
    }
  }
  chainEnd(o, cx);
  return cx.npe ? -1 : 0;
}

// The unmapped record: ReadHit("*", 0, 0, 0, 0, -1, FORWARD, CIGAR(), 0)
// (S/BidirectionalSuffixFilter.java:258-261)
GWA_HD void samUnmapped(SamOut &o, const SamText &t, uint32_t r) {
  o.text(t.name + t.nameB[r], t.nameE[r] - t.nameB[r]);
  o.lit("\t68\t*\t0\t1\t\t*\t0\t0\t");
  o.seq(t.codes + t.codeOff[r], (int)t.codeLen[r], 0, (int)t.codeLen[r], false);
  o.ch('\t');
  if (!qualAbsent(t, r)) o.text(t.qual + t.qualB[r], t.qualE[r] - t.qualB[r]);
  else o.ch('*');
  o.ch('\n');
}

// Every record of read r: its reported chains (OutHeader: hits at hitOff, CIGAR ops at cigOff,
// chains back to back) or the unmapped record.  0, or -1 where the reference would throw.
template <class O>
GWA_HD int samRead(O &o, const SamText &t, uint32_t r, const OutHeader &h, const OutHit *hits, const uint16_t *cig) {
  if (h.status == ST_UNMAPPED) {
    samUnmapped(o, t, r);
    return 0;
  }
  if (h.status != ST_MAPPED) return -1;
  const OutHit *hb = hits + h.hitOff;
  const uint16_t *cb = cig + h.cigOff;
  int head = 0;
  for (int c = 0; c < h.nChains; ++c) {
    if (samChain(o, t, r, hb, cb, head) != 0) return -1;
    int x = head;
    while (hb[x].next >= 0) x = hb[x].next;
    head = x + 1;
  }
  return 0;
}

// ---- paired-end (config C5): the build's own design, the reference has none
// (R/ReadReaderFactory.java:60-84); the rules are stated with their CPU restatement, oracle/
// gwa_oracle.cpp orc_align_pairs.  Mate 1 of pair i is read i, mate 2 is read np + i; each mate was
// aligned as a single-end read with every best hit reported (ALLHITS). ----

// unclipped size of a hit's CIGAR (CIGAR.getUnclippedSize: M X D P N, A/CIGAR.java:115-131)
GWA_HD int samRefLen(const uint16_t *cig, const OutHit &h) {
  int l = 0;
  for (uint32_t i = 0; i < h.cigarLen; ++i) {
    const int t = cig[h.cigarOff + i] & 7;
    if (t == 0 || t == 7 || t == 2 || t == 6 || t == 3) l += cig[h.cigarOff + i] >> 3;
  }
  return l;
}

// one mate's SAM line; h / mate = its chosen hit and its mate's (nullptr: unmapped)
// FLAG of a mate's line as samMateLine computes it
GWA_HD int mateFlag(const OutHit *h, const OutHit *mate, bool first, bool proper) {
  int flag = 0x1 | (first ? 0x40 : 0x80);
  if (proper) flag |= 0x2;
  if (!h) flag |= 0x4;
  if (!mate) flag |= 0x8;
  if (h && h->strand == 1) flag |= 0x10;
  if (mate && mate->strand == 1) flag |= 0x20;
  return flag;
}
GWA_HD void samMateLine(SamOut &o, const SamText &t, uint32_t r, const OutHit *h, const uint16_t *hc, const OutHit *mate,
                        bool first, bool proper, bool leftmost, int64_t tlenAbs, bool sameChr) {
  int flag = 0x1 | (first ? 0x40 : 0x80);
  if (proper) flag |= 0x2;
  if (!h) flag |= 0x4;
  if (!mate) flag |= 0x8;
  if (h && h->strand == 1) flag |= 0x10;
  if (mate && mate->strand == 1) flag |= 0x20;
  o.text(t.name + t.nameB[r], t.nameE[r] - t.nameB[r]);
  o.ch('\t');
  o.num(flag);
  o.ch('\t');
  if (h) {
    o.bytes(t.ctg + t.ctgOff[h->chr], t.ctgOff[h->chr + 1] - t.ctgOff[h->chr]);
    o.ch('\t');
    o.num(h->pos);
    o.lit("\t1\t");
    for (uint32_t i = 0; i < h->cigarLen; ++i) {
      o.num(hc[h->cigarOff + i] >> 3);
      o.ch(samfmt::kOp[hc[h->cigarOff + i] & 7]);
    }
    o.ch('\t');
  } else {
    o.lit("*\t0\t1\t*\t");
  }
  if (mate) {
    if (h && sameChr) o.ch('=');
    else o.bytes(t.ctg + t.ctgOff[mate->chr], t.ctgOff[mate->chr + 1] - t.ctgOff[mate->chr]);
    o.ch('\t');
    o.num(mate->pos);
    o.ch('\t');
  } else {
    o.lit("*\t0\t");
  }
  o.num(h && mate && sameChr ? (leftmost ? tlenAbs : -tlenAbs) : 0);
  o.ch('\t');
  const bool rev = h && h->strand == 1;
  const int m = (int)t.codeLen[r];
  o.seq(t.codes + t.codeOff[r], m, 0, m, rev);
  o.ch('\t');
  if (qualAbsent(t, r)) {
    o.ch('*');
  } else {
    const uint64_t qn = t.qualE[r] - t.qualB[r];
    o.qual(t.qual + t.qualB[r], qn, 0, (int)qn, rev);
  }
  if (h) {
    o.lit("\tNM:i:");
    o.num(h->diff);
    o.lit("\tXP:Z:");
    o.ch(h->numHits == 1 ? 'U' : 'R');
    o.lit("\tX0:i:");
    o.num(h->numHits);
    if (t.tags & kSamTagMd)
      samfmt::mdTag(o, t, r, h->chr, h->pos, samfmt::CigSpec{hc + h->cigarOff, (int)h->cigarLen, -1, -1, nullptr, 0}, 0, m, rev);
  }
  o.ch('\n');
}

// The mates' candidates and the best proper pair of pair i (orc_align_pairs rules 1-2): fa / fb = each
// mate's first candidate (a chain head without a split and with a contig, in report order), a / b =
// the proper pair with the fewest differences (ties: the first in mate-1, then mate-2 order), or null.
// ok = false where a mate's search failed.
struct PairChoice {
  const OutHit *a = nullptr, *b = nullptr, *fa = nullptr, *fb = nullptr;
  const uint16_t *ca = nullptr, *cb = nullptr;  // the CIGAR bases of mate 1's / mate 2's hits
  bool ok = true;
};

// rule 2's test: one contig, opposite strands, forward start <= reverse end, template length in range
GWA_HD bool pairProper(const SamText &t, const OutHit &u, const uint16_t *cu, const OutHit &v, const uint16_t *cv,
                       int32_t minIns, int32_t maxIns) {
  if (t.chrKey[u.chr] != t.chrKey[v.chr] || u.strand == v.strand) return false;
  const OutHit &fw = u.strand == 0 ? u : v, &rv = u.strand == 0 ? v : u;
  const uint16_t *rc = u.strand == 0 ? cv : cu;
  const int64_t fs = fw.pos, re = (int64_t)rv.pos + samRefLen(rc, rv) - 1;
  const int64_t tl = re - fs + 1;
  return !(fs > re || tl < minIns || tl > maxIns);
}

GWA_HD bool pairStatusOk(const OutHeader &A, const OutHeader &B) {
  return (A.status == ST_MAPPED || A.status == ST_UNMAPPED) && (B.status == ST_MAPPED || B.status == ST_UNMAPPED);
}
// a mate's pairing candidates (chain heads without a split and with a contig): their count, and the
// pool index of the first one in report order (-1 = none)
GWA_HD int pairCandidates(const OutHeader &H, const OutHit *hits, int32_t *first) {
  *first = -1;
  const int nc = H.status == ST_MAPPED ? (int)H.nChains : 0;
  const OutHit *h = hits + H.hitOff;
  int count = 0;
  for (int x = 0, hx = 0; x < nc; ++x) {
    const OutHit &u = h[hx];
    int e = hx;
    while (h[e].next >= 0) e = h[e].next;
    if (u.next < 0 && u.chr >= 0) {
      if (*first < 0) *first = (int32_t)(H.hitOff + hx);
      ++count;
    }
    hx = e + 1;
  }
  return count;
}

GWA_HD PairChoice pairChoose(const SamText &t, uint32_t i, uint32_t np, const OutHeader *oh, const OutHit *hits,
                             const uint16_t *cig, int32_t minIns, int32_t maxIns) {
  PairChoice P;
  const OutHeader &A = oh[i], &B = oh[np + i];
  if ((A.status != ST_MAPPED && A.status != ST_UNMAPPED) || (B.status != ST_MAPPED && B.status != ST_UNMAPPED)) {
    P.ok = false;
    return P;
  }
  const OutHit *ha = hits + A.hitOff, *hb = hits + B.hitOff;
  P.ca = cig + A.cigOff;
  P.cb = cig + B.cigOff;
  const int na = A.status == ST_MAPPED ? A.nChains : 0, nb = B.status == ST_MAPPED ? B.nChains : 0;
  int best = 0x7FFFFFFF;
  for (int x = 0, hx = 0; x < na; ++x) {
    const OutHit &u = ha[hx];
    int e = hx;
    while (ha[e].next >= 0) e = ha[e].next;
    const int next = e + 1;
    if (u.next < 0 && u.chr >= 0) {
      if (!P.fa) P.fa = &u;
      for (int y = 0, hy = 0; y < nb; ++y) {
        const OutHit &v = hb[hy];
        int f = hy;
        while (hb[f].next >= 0) f = hb[f].next;
        const int nextB = f + 1;
        if (v.next < 0 && v.chr >= 0 && u.diff + v.diff < best && pairProper(t, u, P.ca, v, P.cb, minIns, maxIns)) {
          best = u.diff + v.diff;
          P.a = &u;
          P.b = &v;
        }
        hy = nextB;
      }
    }
    hx = next;
  }
  for (int y = 0, hy = 0; y < nb && !P.fb; ++y) {
    const OutHit &v = hb[hy];
    if (v.next < 0 && v.chr >= 0) P.fb = &v;
    int f = hy;
    while (hb[f].next >= 0) f = hb[f].next;
    hy = f + 1;
  }
  return P;
}

// Pair i: choose the mates' hits (orc_align_pairs rules 1-3; rule 3's rescued hit from `resc`, the
// pair_rescue kernel's output) and write both lines.  -1 where a mate's search failed.
template <class O>
GWA_HD int samPair(O &o, const SamText &t, uint32_t i, uint32_t np, const OutHeader *oh, const OutHit *hits,
                   const uint16_t *cig, int32_t minIns, int32_t maxIns, const RescueOut *resc) {
  PairChoice P;
  if (resc) {  // the choice made by pair_rescue_kernel / pair_choose_kernel
    if (!pairStatusOk(oh[i], oh[np + i])) return -1;
    const RescueOut &R = resc[i];
    P.a = R.a >= 0 ? hits + R.a : nullptr;
    P.b = R.b >= 0 ? hits + R.b : nullptr;
    P.fa = R.fa >= 0 ? hits + R.fa : nullptr;
    P.fb = R.fb >= 0 ? hits + R.fb : nullptr;
    P.ca = cig + oh[i].cigOff;
    P.cb = cig + oh[np + i].cigOff;
  } else {
    P = pairChoose(t, i, np, oh, hits, cig, minIns, maxIns);
    if (!P.ok) return -1;
  }
  const OutHit *a = P.a, *b = P.b;
  const uint16_t *ca = P.ca, *cb = P.cb;
  bool proper = a != nullptr;
  if (!proper) {
    a = P.fa;
    b = P.fb;
    if (resc && resc[i].status != 0) {  // rule 3: the rescued mate is that mate's only candidate
      const RescueOut &R = resc[i];
      if (R.status == 1) { a = &R.hit; ca = R.cig; }
      else { b = &R.hit; cb = R.cig; }
      proper = a && b && pairProper(t, *a, ca, *b, cb, minIns, maxIns);
    }
  }
  const bool sameChr = a && b && t.chrKey[a->chr] == t.chrKey[b->chr];
  int64_t tlen = 0;
  bool aLeft = true;
  if (sameChr) {
    const int64_t ea = (int64_t)a->pos + samRefLen(ca, *a) - 1, eb = (int64_t)b->pos + samRefLen(cb, *b) - 1;
    tlen = (ea > eb ? ea : eb) - (a->pos < b->pos ? a->pos : b->pos) + 1;
    aLeft = a->pos <= b->pos;
  }
  samMateLine(o, t, i, a, ca, b, true, proper, aLeft, tlen, sameChr);
  samMateLine(o, t, np + i, b, cb, a, false, proper, !aLeft, tlen, sameChr);
  return 0;
}

}  // namespace gwa
