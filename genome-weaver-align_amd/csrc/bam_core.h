// bam_core.h -- the BAM alignment records of one read (SAM specification §4.2), written by one GPU lane
// or by the host test harness.  The reference has no BAM; a record is a total function of the SAM line
// sam_core.h prints for the same hits (include/gwa.h), and it is chosen by the same code:
// samChain / samRead / samPair (sam_core.h) run with a BamOut sink, whose emitRec / samUnmapped /
// samMateLine overloads below write records instead of lines.
//
// Like SamOut, BamOut counts when p == nullptr, so a batch is sized and written by the same code in two
// passes (bam.hip).  A record's block_size is its first field and known only at its end: the lane that
// writes the record stores it last, into its own bytes.  Bulk fields (name, SEQ nibbles, QUAL) of more
// than kSamDeferMin output bytes are left to the workgroup as BamField descriptors in the device write
// pass; bamChunk produces any 16 output bytes of any field kind, for the lane and for the workgroup.
#pragma once
#include "sam_core.h"

namespace gwa {

// A bulk field: `len` items from src.  Output byte i of the field is
enum : uint32_t {
  BAM_COPY = 0,      // src[i]
  BAM_SEQ = 1,       // codes 0..4 as nibbles 1 2 4 8 15: nib(src[2i]) << 4 | nib(src[2i + 1]); len = bases
  BAM_SEQ_RC = 2,    // the same of the reverse complement: base j = complement of src[len - 1 - j]
  BAM_QUAL = 3,      // src[i] - 33
  BAM_QUAL_REV = 4,  // src[len - 1 - i] - 33
  BAM_FILL = 5       // 0xFF
};
struct BamField {
  uint32_t srcLo, srcHi;  // source address
  uint32_t at;            // byte of the workgroup's staging buffer
  uint32_t w;             // len | kind << 24
};
struct BamDefer {
  BamField *f = nullptr;      // descriptor list (LDS); nullptr: nothing is deferred
  uint32_t *count = nullptr;  // fields pushed so far (may exceed cap: those were written at once)
  uint32_t cap = 0;
  uint8_t *stage = nullptr;
};
constexpr uint32_t kBamNameMax = 254;  // l_read_name is one byte and counts the NUL
constexpr uint32_t kBamBinUnmapped = 4680;  // reg2bin(-1, 0)

GWA_HD uint32_t bamFieldBytes(uint32_t kind, uint32_t len) {
  return kind == BAM_SEQ || kind == BAM_SEQ_RC ? (len + 1) / 2 : len;
}

// 16 bytes as one little-endian 128-bit value
struct Bam16 {
  uint64_t lo, hi;
};
GWA_HD Bam16 bamShr(Bam16 v, uint32_t bits) {  // bits <= 128
  if (bits >= 64) {
    v.lo = bits >= 128 ? 0 : v.hi >> (bits - 64);
    v.hi = 0;
  } else if (bits) {
    v.lo = v.lo >> bits | v.hi << (64 - bits);
    v.hi >>= bits;
  }
  return v;
}
GWA_HD Bam16 bamKeep(Bam16 v, uint32_t bits) {  // the low `bits` bits, bits <= 128
  if (bits < 64) {
    v.hi = 0;
    v.lo &= (1ULL << bits) - 1;
  } else if (bits < 128) {
    v.hi &= (1ULL << (bits - 64)) - 1;
  }
  return v;
}
GWA_HD uint64_t bamNibSwap(uint64_t x) {
  return (x & 0x0F0F0F0F0F0F0F0FULL) << 4 | ((x >> 4) & 0x0F0F0F0F0F0F0F0FULL);
}

// 16 bytes at p.  Device: one unaligned 16-B global load (read text and code rows lie in padded
// allocations, the 15 bytes behind a field are inside them).  Host: the `avail` bytes that exist.
GWA_HD Bam16 bamLoad(const uint8_t *p, uint32_t avail) {
  Bam16 v{0, 0};
#if defined(__HIP_DEVICE_COMPILE__)
  (void)avail;
  typedef unsigned int bamU32x4 __attribute__((ext_vector_type(4)));
  typedef const __attribute__((address_space(1))) char *GlobalBytes;
  bamU32x4 q;
  __builtin_memcpy(&q, (GlobalBytes)(uintptr_t)p, 16);
  v.lo = (uint64_t)q.y << 32 | q.x;
  v.hi = (uint64_t)q.w << 32 | q.z;
#else
  for (uint32_t i = 0; i < 16 && i < avail; ++i) {
    if (i < 8) v.lo |= (uint64_t)p[i] << (8 * i);
    else v.hi |= (uint64_t)p[i] << (8 * (i - 8));
  }
#endif
  return v;
}

// 16 codes (one per byte) as 16 nibbles, code k at bits [4k, 4k + 4): A 1, C 2, G 4, T 8, N 15, or the
// complement's (T G C A N)
GWA_HD uint64_t bamNib16(Bam16 c, bool comp) {
  uint64_t out = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t w = (uint32_t)(i < 2 ? c.lo >> (32 * i) : c.hi >> (32 * (i - 2)));
    uint32_t x;
#if defined(__HIP_DEVICE_COMPILE__)
    // codes 0..4 select a byte of the table (byte 4 is the first operand's byte 0)
    x = comp ? __builtin_amdgcn_perm(0x0Fu, 0x01020408u, w) : __builtin_amdgcn_perm(0x0Fu, 0x08040201u, w);
#else
    x = 0;
    for (int k = 0; k < 4; ++k) {
      const uint32_t code = (w >> (8 * k)) & 0xFFu;
      const uint32_t nib = code < 4 ? (comp ? 8u >> code : 1u << code) : 15u;
      x |= nib << (8 * k);
    }
#endif
    const uint32_t t = x | x >> 4;  // nibbles of bytes 0|1 in byte 0, of bytes 2|3 in byte 2
    out |= (uint64_t)((t & 0xFFu) | ((t >> 8) & 0xFF00u)) << (16 * i);
  }
  return out;
}

// Output bytes [i0, i0 + 16) of a field (i0 inside it); bytes behind the field's end are not meaningful,
// but the unused low nibble of an odd SEQ is 0.
GWA_HD Bam16 bamChunk(uint32_t kind, const uint8_t *src, uint32_t len, uint32_t i0) {
  Bam16 v{~0ULL, ~0ULL};
  if (kind == BAM_FILL) return v;
  if (kind == BAM_SEQ || kind == BAM_SEQ_RC) {
    const bool rc = kind == BAM_SEQ_RC;
    const uint32_t left = len - 2 * i0;           // bases still to come
    const uint32_t cnt = left < 32 ? left : 32;   // of them in this chunk
    const uint32_t s = rc ? left - cnt : 2 * i0;  // their codes are src[s, s + cnt)
    const Bam16 a = bamLoad(src + s, len - s);
    Bam16 b{0, 0};
    if (cnt > 16) b = bamLoad(src + s + 16, len - s - 16);
    v.lo = bamNib16(a, rc);  // nibble k = base of code s + k
    v.hi = bamNib16(b, rc);
    if (rc) {  // nibble k = code s + 31 - k, then the codes behind s + cnt shifted out
      const uint64_t l = __builtin_bswap64(bamNibSwap(v.hi)), h = __builtin_bswap64(bamNibSwap(v.lo));
      v.lo = l;
      v.hi = h;
      v = bamShr(v, 4 * (32 - cnt));
    } else {
      v = bamKeep(v, 4 * cnt);
    }
    v.lo = bamNibSwap(v.lo);  // the first base of a byte in its high nibble
    v.hi = bamNibSwap(v.hi);
    return v;
  }
  const uint32_t left = len - i0, cnt = left < 16 ? left : 16;
  if (kind == BAM_QUAL_REV) {
    const uint32_t s = left - cnt;
    v = bamLoad(src + s, len - s);
    const uint64_t l = __builtin_bswap64(v.hi), h = __builtin_bswap64(v.lo);
    v.lo = l;
    v.hi = h;
    v = bamShr(v, 8 * (16 - cnt));
  } else {
    v = bamLoad(src + i0, left);
  }
  if (kind != BAM_COPY) {  // every byte - 33 (mod 256): no borrow leaves a byte whose top bit is set
    constexpr uint64_t H = 0x8080808080808080ULL, Y = 0x2121212121212121ULL;
    v.lo = ((v.lo | H) - Y) ^ (~v.lo & H);
    v.hi = ((v.hi | H) - Y) ^ (~v.hi & H);
  }
  return v;
}

// the first k bytes of v to q (k <= 16)
GWA_HD void bamPut(uint8_t *q, Bam16 v, uint32_t k) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const uint32_t w = (uint32_t)(g < 2 ? v.lo >> (32 * g) : v.hi >> (32 * (g - 2)));
#if defined(__HIP_DEVICE_COMPILE__)
    if (k >= 4u * g + 4 && (((uint32_t)(uintptr_t)q) & 3) == 0) {
      *reinterpret_cast<uint32_t *>(q + 4 * g) = w;
      continue;
    }
#endif
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (4u * g + i < k) q[4 * g + i] = (uint8_t)(w >> (8 * i));
  }
}

// byte sink: counts when p == nullptr
struct BamOut {
  uint8_t *p;
  uint64_t n;
  BamDefer d{};
  uint32_t longName = 0;  // nonzero: a read name of this many bytes (> kBamNameMax) was met
  GWA_HD void ch(uint8_t c) {
    if (p) p[n] = c;
    ++n;
  }
  GWA_HD void u16(uint32_t v) {
    ch((uint8_t)v);
    ch((uint8_t)(v >> 8));
  }
  GWA_HD void u32(uint32_t v) {
    if (p) {
      p[n] = (uint8_t)v;
      p[n + 1] = (uint8_t)(v >> 8);
      p[n + 2] = (uint8_t)(v >> 16);
      p[n + 3] = (uint8_t)(v >> 24);
    }
    n += 4;
  }
  GWA_HD void tagInt(char a, char b, int32_t v) {  // type i, so that a record's size does not depend on the value
    ch((uint8_t)a);
    ch((uint8_t)b);
    ch('i');
    u32((uint32_t)v);
  }
  // a bulk field of `len` items
  GWA_HD void field(uint32_t kind, const void *src, uint32_t len) {
    const uint32_t nb = bamFieldBytes(kind, len);
    if (!p) {
      n += nb;
      return;
    }
#if defined(__HIP_DEVICE_COMPILE__)
    if (d.f && nb > kSamDeferMin && len < (1u << 24)) {
      const uint32_t slot = atomicAdd(d.count, 1u);
      if (slot < d.cap) {
        const uint64_t a = (uint64_t)src;
        d.f[slot] = BamField{(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)(p + n - d.stage), len | kind << 24};
        n += nb;
        return;
      }
    }
#endif
    for (uint32_t i0 = 0; i0 < nb; i0 += 16)
      bamPut(p + n + i0, bamChunk(kind, (const uint8_t *)src, len, i0), nb - i0 < 16 ? nb - i0 : 16);
    n += nb;
  }
};

// reg2bin of the SAM specification §5.3 (14-bit minimum shift, 5 levels) for [beg, end), end > beg >= 0
GWA_HD uint32_t bamReg2bin(int64_t beg, int64_t end) {
  --end;
  if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
  return 0;
}
// the bin field of a line with this FLAG and 0-based pos whose CIGAR spans reflen reference bases
GWA_HD uint32_t bamBin(int flag, int64_t beg, int64_t reflen) {
  if ((flag & 0x4) || beg < 0) return kBamBinUnmapped;
  return bamReg2bin(beg, beg + (reflen > 1 ? reflen : 1)) & 0xFFFFu;
}

namespace samfmt {

// the printed CIGAR's elements (cigarItems) counted, with the reference bases they span (M D N X)
struct CigCount {
  int n = 0;
  int64_t ref = 0;
  int pt = -1;
  int64_t pl = 0;
  GWA_HD void flush() {
    if (pt >= 0) {
      ++n;
      if (pt == 0 || pt == 2 || pt == 3 || pt == 7) ref += pl;
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
// and written, len << 4 | op with the BAM op codes MIDNSHP=X: the writer's code 7 (X) is 8
struct CigBam {
  BamOut &o;
  int pt = -1;
  int64_t pl = 0;
  GWA_HD explicit CigBam(BamOut &o_) : o(o_) {}
  GWA_HD void flush() {
    if (pt >= 0) o.u32((uint32_t)pl << 4 | (uint32_t)(pt == 7 ? 8 : pt));
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

// refID of a printed contig name: its index, -1 for "*" and the empty name (also where a contig is
// called that) and for the names that are not contigs
GWA_HD int32_t bamRefId(const SamText &t, int chr) {
  return chr >= 0 && t.chrKey[chr] != t.starKey && t.chrKey[chr] != t.emptyKey ? chr : -1;
}
// RNEXT's name is printed as "*"
GWA_HD bool bamNameIsStar(const SamText &t, int chr) { return chr == CHR_STAR || (chr >= 0 && t.chrKey[chr] == t.starKey); }

// One record from block_size to qual; returns where the record starts (bamClose).  pos, pnext: the
// printed POS and PNEXT; SEQ = [seqA, seqB) of read r's query on strand rc; QUAL: the printed one is "*"
// (qualNull) or [qualA, qualB) of the quality q[0, qn) on the same strand.
GWA_HD uint64_t bamHead(BamOut &o, const SamText &t, uint32_t r, int flag, int32_t refId, int64_t pos, const CigSpec &cig,
                        int32_t nextRef, int64_t pnext, int64_t tlen, int seqA, int seqB, bool rc, bool qualNull,
                        const char *q, uint64_t qn, int qualA, int qualB) {
  const uint64_t start = o.n;
  const uint64_t nl = t.nameE[r] - t.nameB[r];
  if (nl > kBamNameMax) o.longName = (uint32_t)(nl > 0xFFFFFFFFull ? 0xFFFFFFFFull : nl);
  CigCount cc;
  cigarItems(cc, cig);
  const uint32_t lseq = seqB > seqA ? (uint32_t)(seqB - seqA) : 0;
  const int64_t beg = pos - 1;
  o.u32(0);  // block_size (bamClose)
  o.u32((uint32_t)refId);
  o.u32((uint32_t)beg);
  o.ch((uint8_t)(nl + 1));
  o.ch(1);  // MAPQ: the column the reference always prints
  o.u16(bamBin(flag, beg, cc.ref));
  o.u16((uint32_t)cc.n);
  o.u16((uint32_t)flag);
  o.u32(lseq);
  o.u32((uint32_t)nextRef);
  o.u32((uint32_t)(pnext - 1));
  o.u32((uint32_t)tlen);
  o.field(BAM_COPY, t.name + t.nameB[r], (uint32_t)nl);
  o.ch(0);
  CigBam cb(o);
  cigarItems(cb, cig);
  const uint8_t *c = t.codes + t.codeOff[r];
  const int m = (int)t.codeLen[r];
  if (lseq) o.field(rc ? BAM_SEQ_RC : BAM_SEQ, rc ? c + (m - seqB) : c + seqA, lseq);
  const uint64_t ql = qualNull ? 1 : (qualB > qualA ? (uint64_t)(qualB - qualA) : 0);
  if (ql != lseq) {
    o.field(BAM_FILL, nullptr, lseq);
  } else if (qualNull) {
    o.ch((uint8_t)('*' - 33));  // (a one-base SEQ: the printed "*" has its length)
  } else if (lseq) {
    o.field(rc ? BAM_QUAL_REV : BAM_QUAL, rc ? q + (qn - (uint64_t)qualB) : q + qualA, lseq);
  }
  return start;
}
GWA_HD void bamClose(BamOut &o, uint64_t start) {
  const uint64_t end = o.n;
  o.n = start;
  o.u32((uint32_t)(end - start - 4));
  o.n = end;
}
// X0:i and, where the line has one, MD:Z.  mdEmit writes the text form's six bytes "\tMD:Z:" before the
// value; they are put where X0 and "MDZ" then overwrite them, so the value lands in its place.
GWA_HD void bamTail(BamOut &o, const SamText &t, uint32_t r, int x0, bool md, int chr, int64_t pos, const CigSpec &c,
                    int seqA, int seqB, bool rc) {
  if (!md) {
    o.tagInt('X', '0', x0);
    return;
  }
  const uint64_t e = mdEmit((char *)o.p, o.n + 4, t.text2, t.textN, t.ctgStart[chr], t.ctgLen[chr], pos, c.a, c.na, c.preS,
                            c.postS, c.b, c.nb, t.codes + t.codeOff[r], (int)t.codeLen[r], seqA, seqB > seqA ? seqB - seqA : 0, rc);
  o.tagInt('X', '0', x0);
  o.ch('M');
  o.ch('D');
  o.ch('Z');
  o.n = e;
  o.ch(0);
}

// the record of lineOne's line
GWA_HD bool bamLineOne(BamOut &o, Ctx &cx, const Rec &r, const Rec *split, bool hasSegments, bool isFirst, bool eachMapped) {
  const int flag = lineFlag(r, split, hasSegments, isFirst, eachMapped);
  const SamText &t = cx.t;
  if (r.chr == CHR_NULL) cx.npe = true;
  int32_t nextRef = -1;
  int64_t pnext = 0, tlen = 0;  // RNEXT "*", PNEXT 0, TLEN 0
  if (split) {
    tlen = (int64_t)split->end - r.start;
    if (rnextSame(cx, r, *split)) {  // "=": this line's contig
      nextRef = bamRefId(t, r.chr);
      pnext = split->start;
    } else {
      if (split->chr == CHR_NULL) cx.npe = true;
      nextRef = bamRefId(t, split->chr);
      pnext = bamNameIsStar(t, split->chr) ? 0 : split->start;
    }
  }
  const uint64_t start = bamHead(o, t, cx.r, flag, bamRefId(t, r.chr), r.start, r.cig, nextRef, pnext, tlen, r.seqA, r.seqB,
                                 cx.strand != 0, cx.qualNull, cx.qualNull ? nullptr : t.qual + cx.q0, cx.qn, r.qualA, r.qualB);
  if (r.numBestHits > 0) {
    if (r.nm >= 0) o.tagInt('N', 'M', r.nm);
    o.ch('X');
    o.ch('P');
    o.ch('Z');
    emitState(o, cx, r.stateHead, r.stateSelf);
    o.ch(0);
    bamTail(o, t, cx.r, r.numBestHits, (t.tags & kSamTagMd) && r.chr >= 0, r.chr, r.start, r.cig, r.seqA, r.seqB, cx.strand != 0);
  }
  bamClose(o, start);
  return eachMapped;
}

GWA_HD void emitRec(BamOut &o, Ctx &cx, const Rec &r, const Rec *split, bool hasSegments) {
  const bool em = bamLineOne(o, cx, r, split, hasSegments, true, true);
  if (split) bamLineOne(o, cx, *split, nullptr, hasSegments, false, em);
}
GWA_HD void chainEnd(BamOut &, const Ctx &) {}

}  // namespace samfmt

// samUnmapped's record: FLAG 68, RNAME "*", POS 0, an empty CIGAR, the whole read forward
GWA_HD void samUnmapped(BamOut &o, const SamText &t, uint32_t r) {
  const bool qn = qualAbsent(t, r);
  const uint64_t ql = qn ? 0 : t.qualE[r] - t.qualB[r];
  const uint64_t start = samfmt::bamHead(o, t, r, 68, -1, 0, samfmt::CigSpec{nullptr, 0, -1, -1, nullptr, 0}, -1, 0, 0, 0,
                                         (int)t.codeLen[r], false, qn, qn ? nullptr : t.qual + t.qualB[r], ql, 0, (int)ql);
  samfmt::bamClose(o, start);
}

// samMateLine's record
GWA_HD void samMateLine(BamOut &o, const SamText &t, uint32_t r, const OutHit *h, const uint16_t *hc, const OutHit *mate,
                        bool first, bool proper, bool leftmost, int64_t tlenAbs, bool sameChr) {
  using namespace samfmt;
  const int flag = mateFlag(h, mate, first, proper);
  const CigSpec cig = h ? CigSpec{hc + h->cigarOff, (int)h->cigarLen, -1, -1, nullptr, 0} : CigSpec{nullptr, 0, -1, -1, nullptr, 0};
  const int32_t refId = h ? bamRefId(t, h->chr) : -1;
  int32_t nextRef = -1;
  int64_t pnext = 0;
  if (mate) {
    nextRef = h && sameChr ? refId : bamRefId(t, mate->chr);
    pnext = !(h && sameChr) && bamNameIsStar(t, mate->chr) ? 0 : mate->pos;
  }
  const bool rev = h && h->strand == 1;
  const int m = (int)t.codeLen[r];
  const bool qn = qualAbsent(t, r);
  const uint64_t ql = qn ? 0 : t.qualE[r] - t.qualB[r];
  const uint64_t start = bamHead(o, t, r, flag, refId, h ? h->pos : 0, cig, nextRef, pnext,
                                 h && mate && sameChr ? (leftmost ? tlenAbs : -tlenAbs) : 0, 0, m, rev, qn,
                                 qn ? nullptr : t.qual + t.qualB[r], ql, 0, (int)ql);
  if (h) {
    o.tagInt('N', 'M', h->diff);
    o.ch('X');
    o.ch('P');
    o.ch('Z');
    o.ch(h->numHits == 1 ? 'U' : 'R');
    o.ch(0);
    bamTail(o, t, r, h->numHits, (t.tags & kSamTagMd) != 0, h->chr, h->pos, cig, 0, m, rev);
  }
  bamClose(o, start);
}

}  // namespace gwa
