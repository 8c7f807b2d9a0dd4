// batch_io.hip -- a batch's reads in and SAM text out, on the GPU.
//
// Reads in: the caller's read text (names, bases, qualities) is copied to HBM as it is and encoded
// there -- ACGTSequence(String) (A/ACGTSequence.java:86-97: spaces skipped, ACGT.to3bitCode,
// A/ACGT.java:36-43) into 16-B aligned, zero-padded code rows (ReadsView).
//
// SAM out: the text of a batch is written on the GPU (the reporting tail of the align path:
// AlignmentRecord.convert / toSAMLine and SAMOutput.emit, R/AlignmentRecord.java:109-276,
// A/SAMOutput.java:73-82; the per-read logic is sam_core.h).
//
// The reference formats one record at a time on the host thread that aligned it.  Here one lane
// formats one read: a length pass (the writer in counting mode), an exclusive scan of the lengths
// (rocPRIM), and a write pass that puts every read's records at its offset.  In the write pass a
// lane writes the short fields of its records itself (flag, position, CIGAR, tags) and the workgroup
// then copies the bulk fields (name, SEQ, QUAL) of all its records together, consecutive lanes on
// consecutive 16-B chunks (samServeFields).  The host receives
// the finished text of the batch in one copy, in input order.  A read on which the reference
// would throw (or whose search failed) is reported through `err` (lowest failing position).
//
// Also here: the batch statistics as a device reduction over the per-read output headers.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <cstdlib>
#include <stdexcept>
#include <string>

#include "kernels.h"
#include "sam_core.h"
#include "text_core.h"

namespace gwa {

#define FCHK(x)                                                                                         \
  do {                                                                                                  \
    hipError_t e_ = (x);                                                                                \
    if (e_ != hipSuccess) throw std::runtime_error(std::string("sam_format: ") + #x + ": " + hipGetErrorString(e_)); \
  } while (0)

// ---- reads in ----

__device__ __forceinline__ uint8_t to3bitDev(unsigned char c) {
  switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': case 'U': case 'u': return 3;
    default: return 4;
  }
}

// Read text loads: 16-B aligned chunks (the text allocations are padded by 32 bytes, so the chunk
// holding a field's last byte is always inside the allocation) funnel-shifted to the field start.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4 loadChunk(const char *__restrict__ base, uint64_t a16) {
  return *reinterpret_cast<const u32x4 *>(base + a16);
}
// bytes [p, p + 16) of the text as 4 dwords (p any alignment)
__device__ __forceinline__ void load16(const char *__restrict__ t, uint64_t p, uint32_t (&w)[4]) {
  const uint64_t a = p & ~(uint64_t)15;
  const int sh = (int)(p & 15);
  const u32x4 c0 = loadChunk(t, a);
  uint32_t x[8] = {c0.x, c0.y, c0.z, c0.w, 0, 0, 0, 0};
  if (sh) {
    const u32x4 c1 = loadChunk(t, a + 16);
    x[4] = c1.x; x[5] = c1.y; x[6] = c1.z; x[7] = c1.w;
  }
  const int q = sh >> 2, r = (sh & 3) * 8;
#pragma unroll
  for (int i = 0; i < 4; ++i) {  // dwords q + i and q + i + 1 (q = 0..3) through selects
    uint32_t lo = x[i], hi = x[i + 1];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      lo = q == k ? x[k + i] : lo;
      hi = q == k ? x[k + i + 1] : hi;
    }
    w[i] = r ? (lo >> r) | (hi << (32 - r)) : lo;
  }
}
// per read: bases after skipping spaces, its padded row size, and a mark in the length table
__global__ void __launch_bounds__(256) encodeLenKernel(const char *__restrict__ seq, const uint64_t *__restrict__ seqB,
                                                       const uint64_t *__restrict__ seqE, uint32_t n, uint32_t *__restrict__ codeLen,
                                                       uint32_t *__restrict__ rowLen, uint32_t *__restrict__ lenSeen) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r > n) return;
  if (r == n) {  // the scan's tail: 16 zero bytes after the last row
    rowLen[n] = 16;
    return;
  }
  const uint64_t b = seqB[r], e = seqE[r];
  uint32_t spaces = 0;
  // aligned 16-B chunks over [b, e); bytes outside the field are masked off
  for (uint64_t a = b & ~(uint64_t)15; a < e; a += 16) {
    const u32x4 c = loadChunk(seq, a);
    const uint32_t w[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint64_t p = a + 4 * i;
      uint32_t m = bytesEq(w[i], ' ');
      // keep bytes p + j with b <= p + j < e
      const int64_t lo = (int64_t)b - (int64_t)p, hi = (int64_t)e - (int64_t)p;
      const uint32_t keepLo = lo <= 0 ? 0xFFFFFFFFu : lo >= 4 ? 0u : (0xFFFFFFFFu << (8 * lo));
      const uint32_t keepHi = hi >= 4 ? 0xFFFFFFFFu : hi <= 0 ? 0u : (0xFFFFFFFFu >> (8 * (4 - hi)));
      spaces += __builtin_popcount(m & keepLo & keepHi);
    }
  }
  const uint32_t m = (uint32_t)(e - b) - spaces;
  codeLen[r] = m;
  rowLen[r] = (m + 15) & ~15u;
  lenSeen[m < kLenSeen - 1 ? m : kLenSeen - 1] = 1;
}

// Code rows: kEncLanes consecutive lanes share a read, each converting one 16-B chunk of its text
// into 16 codes of its row (rows are 16-B aligned and zero-padded), so a wavefront reads the text of
// 8 neighbouring reads and writes their rows as consecutive 16-B chunks.  A read with spaces in its
// text (skipped, A/ACGTSequence.java:86-97) takes the byte loop on its first lane.
constexpr uint32_t kEncLanes = 8;
__global__ void __launch_bounds__(256) encodeWriteKernel(const char *__restrict__ seq, const uint64_t *__restrict__ seqB,
                                                         const uint64_t *__restrict__ seqE, uint32_t n,
                                                         const uint32_t *__restrict__ codeOff,
                                                         const uint32_t *__restrict__ codeLen,
                                                         uint8_t *__restrict__ codes) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t r = (uint32_t)(tid / kEncLanes), sub = (uint32_t)(tid % kEncLanes);
  if (r >= n) return;
  const uint32_t o0 = codeOff[r];
  uint8_t *o = codes + o0;
  const uint64_t b = seqB[r], e = seqE[r];
  const uint32_t m = codeLen[r], row = codeOff[r + 1] - o0;
  if (m == e - b) {
    for (uint32_t k = 16 * sub; k < row; k += 16 * kEncLanes) {
      uint32_t w[4];
      load16(seq, b + k, w);
      u32x4 v;
      uint32_t c[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int valid = (int)m - (int)(k + 4 * i);  // bytes of this dword inside the read
        const uint32_t keep = valid >= 4 ? 0xFFFFFFFFu : valid <= 0 ? 0u : (0xFFFFFFFFu >> (8 * (4 - valid)));
        c[i] = to3bit4(w[i]) & keep;
      }
      v.x = c[0]; v.y = c[1]; v.z = c[2]; v.w = c[3];
      *reinterpret_cast<u32x4 *>(o + k) = v;
    }
    return;
  }
  if (sub != 0) return;
  uint32_t k = 0;
  for (uint64_t i = b; i < e; ++i)
    if (seq[i] != ' ') o[k++] = to3bitDev((unsigned char)seq[i]);
  for (; k < row; ++k) o[k] = 0;
}

void launchEncode(const char *seq, const uint64_t *seqB, const uint64_t *seqE, uint32_t n, uint32_t *codeLen, uint32_t *rowLen,
                  uint32_t *codeOff, uint32_t *lenSeen, uint8_t *codes, void *scanTmp, size_t scanTmpBytes, int pass,
                  hipStream_t s) {
  const dim3 grid((n + 1 + 255) / 256);
  if (pass == 0) {
    hipLaunchKernelGGL(encodeLenKernel, grid, dim3(256), 0, s, seq, seqB, seqE, n, codeLen, rowLen, lenSeen);
    FCHK(hipGetLastError());
    size_t b = scanTmpBytes;
    FCHK(rocprim::exclusive_scan(scanTmp, b, rowLen, codeOff, (uint32_t)0, (size_t)n + 1, rocprim::plus<uint32_t>(), s));
  } else {
    if (n == 0) return;
    const dim3 g8((unsigned)(((uint64_t)n * kEncLanes + 255) / 256));
    hipLaunchKernelGGL(encodeWriteKernel, g8, dim3(256), 0, s, seq, seqB, seqE, n, codeOff, codeLen, codes);
    FCHK(hipGetLastError());
  }
}

size_t encodeScanTempBytes(uint32_t n) {
  size_t b = 0;
  FCHK(rocprim::exclusive_scan(nullptr, b, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t)0, (size_t)n + 1,
                               rocprim::plus<uint32_t>(), (hipStream_t)0));
  return b;
}

// FASTQ records straight from the file text (the pipeline's zero-copy path): record r starts at
// start[r] (its header line; the host framed the text into complete records, reads_io.cpp
// frameRecords).  The fields are located under the record rules of reads_io.cpp parseFastq: lines
// end at "\n", "\r\n" or "\r"; a line missing at the end of the text reads as ""; the name is the
// first whitespace-delimited token after '@'; the third line must start with '+' and the quality
// must be as long as the sequence.  A malformed record sets err (lowest record index); the host
// then re-parses the text to report it as the host parser words it.
__device__ __forceinline__ bool isWsDev(unsigned char c) { return c == ' ' || (c >= '\t' && c <= '\r') || (c >= 0x1c && c <= 0x1f); }

__device__ __forceinline__ uint64_t lineAt(const char *__restrict__ t, uint64_t len, uint64_t pos, uint64_t *e) {
  if (pos >= len) {
    *e = len;
    return len;
  }
  uint64_t i = pos;
  while (i < len && t[i] != '\n' && t[i] != '\r') ++i;
  *e = i;
  if (i == len) return len;
  if (t[i] == '\r' && i + 1 < len && t[i + 1] == '\n') return i + 2;
  return i + 1;
}

// Two segments (a paired batch: mate 1's slice, then mate 2's at base2): records [0, n1) lie in
// [0, end1), records [n1, n) in [base2, len) with their starts relative to base2.  Every line is
// bounded by the end of its record's own segment -- a first segment whose last line has no newline
// must not run on into the bytes behind it.  One segment: n1 = n, end1 = len, base2 = 0.
__global__ void __launch_bounds__(256) fastqFieldsKernel(const char *__restrict__ t, uint64_t total, const uint64_t *__restrict__ start,
                                                         uint32_t n, uint64_t *__restrict__ f, uint32_t *__restrict__ err,
                                                         uint32_t n1, uint64_t end1, uint64_t base2) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  uint64_t he, se, pe, qe;
  const bool second = r >= n1;
  const uint64_t len = second ? total : end1;
  const uint64_t hb = start[r] + (second ? base2 : 0);
  const uint64_t sb = lineAt(t, len, hb, &he);
  const uint64_t pb = lineAt(t, len, sb, &se);
  const uint64_t qb = lineAt(t, len, pb, &pe);
  (void)lineAt(t, len, qb, &qe);
  if (he == hb || t[hb] != '@' || pe == pb || t[pb] != '+' || qe - qb != se - sb) atomicMin(err, r);
  uint64_t nb = hb + 1;
  while (nb < he && isWsDev((unsigned char)t[nb])) ++nb;
  uint64_t ne = nb;
  while (ne < he && !isWsDev((unsigned char)t[ne])) ++ne;
  // six field arrays of n: name [b, e), sequence [b, e), quality [b, e)
  f[r] = nb;
  f[(size_t)n + r] = ne;
  f[2 * (size_t)n + r] = sb;
  f[3 * (size_t)n + r] = se;
  f[4 * (size_t)n + r] = qb;
  f[5 * (size_t)n + r] = qe;
}

void launchFastqFields(const char *text, uint64_t len, const uint64_t *start, uint32_t n, uint64_t *fields,
                       uint32_t *err, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(fastqFieldsKernel, dim3((n + 255) / 256), dim3(256), 0, s, text, len, start, n, fields, err, n,
                     len, (uint64_t)0);
  FCHK(hipGetLastError());
}

void launchFastqFieldsPair(const char *text, uint64_t len1, uint64_t base2, uint64_t len2, const uint64_t *start,
                           uint32_t np, uint64_t *fields, uint32_t *err, hipStream_t s) {
  if (np == 0) return;
  const uint32_t n = 2 * np;
  hipLaunchKernelGGL(fastqFieldsKernel, dim3((n + 255) / 256), dim3(256), 0, s, text, base2 + len2, start, n, fields, err,
                     np, len1, base2);
  FCHK(hipGetLastError());
}

// Mate names of a paired batch (mate 1 of pair i = read i, mate 2 = read np + i; text or blob
// batches alike): one pair per lane, each name without one trailing "/1" or "/2"; the lowest pair
// whose names differ goes to err.
__device__ __forceinline__ uint64_t mateNameEnd(const char *__restrict__ t, uint64_t b, uint64_t e) {
  if (e - b >= 2 && t[e - 2] == '/' && (t[e - 1] == '1' || t[e - 1] == '2')) return e - 2;
  return e;
}

__global__ void __launch_bounds__(256) mateNameKernel(const char *__restrict__ t, const uint64_t *__restrict__ nameB,
                                                      const uint64_t *__restrict__ nameE, uint32_t np,
                                                      uint32_t *__restrict__ err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
  const uint64_t b1 = nameB[i], b2 = nameB[(size_t)np + i];
  const uint64_t e1 = mateNameEnd(t, b1, nameE[i]), e2 = mateNameEnd(t, b2, nameE[(size_t)np + i]);
  bool same = e1 - b1 == e2 - b2;
  for (uint64_t k = 0; same && k < e1 - b1; ++k) same = t[b1 + k] == t[b2 + k];
  if (!same) atomicMin(err, i);
}

void launchMateNames(const char *nameText, const uint64_t *nameB, const uint64_t *nameE, uint32_t np, uint32_t *err,
                     hipStream_t s) {
  if (np == 0) return;
  hipLaunchKernelGGL(mateNameKernel, dim3((np + 255) / 256), dim3(256), 0, s, nameText, nameB, nameE, np, err);
  FCHK(hipGetLastError());
}

// ---- SAM out ----

// one read's records, or (pairs mode, ps.np > 0) pair r's two mate lines
__device__ __forceinline__ int samUnit(SamOut &o, const SamText &t, uint32_t r, const OutHeader *oh, const OutHit *hits,
                                       const uint16_t *cig, const PairSpec &ps) {
  if (ps.np) return samPair(o, t, r, ps.np, oh, hits, cig, ps.minIns, ps.maxIns, ps.resc);
  return samRead(o, t, r, oh[r], hits, cig);
}

// Both passes exist in two instances: TAGS = false is the default output's code, with the optional tags
// (SamText::tags: MD:Z) compiled out; TAGS = true formats them (the lane walks its records' reference
// windows, sam_core.h mdEmit).
template <bool TAGS>
__global__ void __launch_bounds__(256) samLenKernel(SamText t, const OutHeader *__restrict__ oh, const OutHit *__restrict__ hits,
                                                    const uint16_t *__restrict__ cig, const uint32_t *__restrict__ idx,
                                                    uint32_t first, uint32_t n, uint64_t *__restrict__ len,
                                                    uint32_t *__restrict__ err, PairSpec ps) {
  if (!TAGS) t.tags = 0;
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j > n) return;
  if (j == n) {  // the scan's total
    len[n] = 0;
    return;
  }
  const uint32_t r = idx ? idx[j] : first + j;
  SamOut o{nullptr, 0};
  if (samUnit(o, t, r, oh, hits, cig, ps) != 0) {
    atomicMin(err, j);
    o.n = 0;
  }
  len[j] = o.n;
}

// ---- write pass ----

// bytes [u, u + k) of the 16 bytes W to q[0, k): dword stores where q is 4-B aligned and 4 bytes
// remain, byte stores otherwise (no store touches a byte outside the range: the neighbouring bytes
// belong to other lanes)
__device__ __forceinline__ void putBytes(char *q, const uint32_t (&W)[4], uint32_t u, uint32_t k) {
  while (k > 0) {
    const uint32_t d = u >> 2;
    const uint32_t lo = d == 0 ? W[0] : d == 1 ? W[1] : d == 2 ? W[2] : W[3];
    const uint32_t hi = d == 0 ? W[1] : d == 1 ? W[2] : d == 2 ? W[3] : 0u;
    const uint32_t v = __builtin_amdgcn_alignbit(hi, lo, (u & 3) * 8);
    if ((((uint32_t)(uintptr_t)q) & 3) == 0 && k >= 4) {
      *reinterpret_cast<uint32_t *>(q) = v;
      q += 4; u += 4; k -= 4;
    } else {
      *q = (char)v;
      q += 1; u += 1; k -= 1;
    }
  }
}

// 16 bytes of read text or code rows from any address: one unaligned 16-B global load (the text and
// code allocations are padded, so the 15 bytes after a field's last byte are inside them)
typedef const __attribute__((address_space(1))) char *GlobalText;
__device__ __forceinline__ void loadText16(const char *p, uint32_t (&w)[4]) {
  u32x4 v;
  __builtin_memcpy(&v, (GlobalText)(uintptr_t)p, 16);
  w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
}

// SamOut::text of up to 16 bytes: one lane, one 16-B load instead of a load per byte
__device__ void samSmallCopy(char *dst, const char *src, uint32_t len) {
  if (len == 0) return;
  uint32_t w[4];
  loadText16(src, w);
  putBytes(dst, w, 0, len);
}

// A deferred field in the stage: a partial 16-B chunk at its head (up to the first 16-B boundary of
// the stage), ni whole chunks, a partial chunk at its tail.
struct SamSpan {
  const char *src;
  uint32_t at, len, kind, head, ni;
};
__device__ __forceinline__ SamSpan samSpan(const SamField &f) {
  SamSpan s;
  s.src = reinterpret_cast<const char *>((uint64_t)f.srcHi << 32 | f.srcLo);
  s.at = f.w & 0xFFFFu;
  s.len = (f.w >> 16) & 0x3FFFu;
  s.kind = f.w >> 30;
  s.head = (16u - (s.at & 15u)) & 15u;  // (len > 16 > head)
  s.ni = (s.len - s.head) >> 4;
  return s;
}
// the source of the k output bytes from i0 on (reversed kinds: out[i0 + t] = src[len - 1 - i0 - t])
__device__ __forceinline__ const char *spanSrc(const SamSpan &s, uint32_t i0, uint32_t k) {
  return s.kind >= SAM_SEQ_RC ? s.src + (s.len - i0 - k) : s.src + i0;
}
// 16 loaded bytes to output bytes: letters for the SEQ kinds; the reversed kinds byte-reversed, so
// that the k bytes of a partial chunk are then bytes [16 - k, 16)
__device__ __forceinline__ void spanConvert(uint32_t kind, const uint32_t (&w)[4], uint32_t (&W)[4]) {
  if (kind >= SAM_SEQ_RC) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // the complement's letter of codes 0..4 (T G C A N) by byte select
      const uint32_t x = kind == SAM_SEQ_RC ? __builtin_amdgcn_perm(0x4Eu, 0x41434754u, w[3 - i]) : w[3 - i];
      W[i] = __builtin_bswap32(x);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)  // SAM_SEQ: the letter of codes 0..4 (A C G T N) by byte select
      W[i] = kind == SAM_SEQ ? __builtin_amdgcn_perm(0x4Eu, 0x54474341u, w[i]) : w[i];
  }
}

// The workgroup's deferred fields, four loads in flight per lane (issued before the first store).
// Whole chunks: 1 << lshift consecutive lanes share a field, lane `sub` of them takes chunks sub,
// sub + (1 << lshift), ... (16-B loads of consecutive addresses, aligned 16-B LDS stores).  Then the
// partial chunks, two per field, one per lane (putBytes).
__device__ __forceinline__ void samServeFields(const SamField *fields, uint32_t D, char *stage, uint32_t lshift) {
  const uint32_t L = 1u << lshift, G = blockDim.x >> lshift;
  const uint32_t sub = threadIdx.x & (L - 1), g = threadIdx.x >> lshift;
  constexpr int U = 4;
  for (uint32_t d0 = 0; d0 < D; d0 += G * U) {
    SamSpan sp[U];
    uint32_t w[U][4];
    bool on[U];
#pragma unroll
    for (int x = 0; x < U; ++x) {
      const uint32_t d = d0 + x * G + g;
      on[x] = false;
      sp[x].ni = 0;
      if (d < D) {
        sp[x] = samSpan(fields[d]);
        on[x] = sub < sp[x].ni;
        if (on[x]) loadText16(spanSrc(sp[x], sp[x].head + 16 * sub, 16), w[x]);
      }
    }
#pragma unroll
    for (int x = 0; x < U; ++x)
      if (on[x]) {
        uint32_t W[4];
        spanConvert(sp[x].kind, w[x], W);
        u32x4 v;
        v.x = W[0]; v.y = W[1]; v.z = W[2]; v.w = W[3];
        *reinterpret_cast<u32x4 *>(stage + sp[x].at + sp[x].head + 16 * sub) = v;
      }
#pragma unroll
    for (int x = 0; x < U; ++x)  // fields of more than L whole chunks
      for (uint32_t c = sub + L; c < sp[x].ni; c += L) {
        uint32_t w2[4], W[4];
        loadText16(spanSrc(sp[x], sp[x].head + 16 * c, 16), w2);
        spanConvert(sp[x].kind, w2, W);
        u32x4 v;
        v.x = W[0]; v.y = W[1]; v.z = W[2]; v.w = W[3];
        *reinterpret_cast<u32x4 *>(stage + sp[x].at + sp[x].head + 16 * c) = v;
      }
  }
  for (uint32_t e0 = 0; e0 < 2 * D; e0 += blockDim.x * U) {
    SamSpan sp[U];
    uint32_t w[U][4], i0[U], k[U];
#pragma unroll
    for (int x = 0; x < U; ++x) {
      const uint32_t e = e0 + blockDim.x * x + threadIdx.x;
      k[x] = 0;
      if (e < 2 * D) {
        sp[x] = samSpan(fields[e >> 1]);
        i0[x] = e & 1 ? sp[x].head + 16 * sp[x].ni : 0;
        k[x] = e & 1 ? sp[x].len - i0[x] : sp[x].head;
        if (k[x]) loadText16(spanSrc(sp[x], i0[x], k[x]), w[x]);
      }
    }
#pragma unroll
    for (int x = 0; x < U; ++x)
      if (k[x]) {
        uint32_t W[4];
        spanConvert(sp[x].kind, w[x], W);
        putBytes(stage + sp[x].at + i0[x], W, sp[x].kind >= SAM_SEQ_RC ? 16 - k[x] : 0, k[x]);
      }
  }
}

// units (= lanes) per workgroup of the write pass (128 measured the same: 3.93 against 3.92 ms of
// gwa_batch_format for 10M 100 bp reads)
constexpr uint32_t kSamWg = 64;

// Write pass.  The text of a workgroup's units is one contiguous range of the output
// [off[j0], off[j0 + wg]); it is put together in LDS at the position it has relative to the 16-B
// aligned start of that range, then copied out with coalesced 16-B stores (the two partial chunks at
// the range's ends are written bytewise, the neighbouring workgroups own their other bytes).  The
// stage is filled in two phases: each lane formats its unit, writing the short fields and leaving a
// descriptor for every bulk field (sam_core.h SamOut::defer; up to `cap` per workgroup, further ones
// are copied by the lane); after a barrier the workgroup copies the deferred fields
// (samServeFields).  A range larger than the staging buffer (many reported lines) is written
// directly to HBM by its lanes.  `out` is only ever written (it may be pinned host memory).
// Dynamic LDS: cap descriptors of 12 B, the counter, the stage of stageBytes.
template <bool TAGS>
__global__ void __launch_bounds__(kSamWg) samWriteKernel(SamText t, const OutHeader *__restrict__ oh, const OutHit *__restrict__ hits,
                                                     const uint16_t *__restrict__ cig, const uint32_t *__restrict__ idx,
                                                     uint32_t first, uint32_t n, const uint64_t *__restrict__ off,
                                                     char *__restrict__ out, PairSpec ps, uint32_t stageBytes, uint32_t cap,
                                                     uint32_t lshift) {
  if (!TAGS) t.tags = 0;
  extern __shared__ u32x4 samLds[];
  SamField *fields = reinterpret_cast<SamField *>(samLds);
  const uint32_t descBytes = (cap * (uint32_t)sizeof(SamField) + 4 + 15) & ~15u;
  uint32_t *count = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(samLds) + descBytes - 4);
  char *stage = reinterpret_cast<char *>(samLds) + descBytes;
  const uint32_t j0 = blockIdx.x * blockDim.x, j = j0 + threadIdx.x;
  const uint32_t jEnd = j0 + blockDim.x < n ? j0 + blockDim.x : n;
  const uint64_t gBeg = off[j0], gEnd = off[jEnd];
  const uint64_t base = gBeg & ~(uint64_t)15;
  if (gEnd - base > (uint64_t)stageBytes) {
    if (j < n) {
      SamOut o{out + off[j], 0};
      (void)samUnit(o, t, idx ? idx[j] : first + j, oh, hits, cig, ps);
    }
    return;
  }
  if (threadIdx.x == 0) *count = 0;
  __syncthreads();
  if (j < n) {
    SamOut o{stage + (off[j] - base), 0, SamDefer{fields, count, cap, stage}};
    (void)samUnit(o, t, idx ? idx[j] : first + j, oh, hits, cig, ps);
  }
  __syncthreads();
  const uint32_t D = *count < cap ? *count : cap;
  samServeFields(fields, D, stage, lshift);
  __syncthreads();
  const uint32_t chunks = (uint32_t)((gEnd - base + 15) >> 4);
  const u32x4 *st = reinterpret_cast<const u32x4 *>(stage);
  for (uint32_t c = threadIdx.x; c < chunks; c += blockDim.x) {
    const uint64_t a = base + 16ull * c;
    if (a >= gBeg && a + 16 <= gEnd) {
      *reinterpret_cast<u32x4 *>(out + a) = st[c];
    } else {
      const char *sb = stage + 16ull * c;
      for (int i = 0; i < 16; ++i)
        if (a + i >= gBeg && a + i < gEnd) out[a + i] = sb[i];
    }
  }
}

void launchSamFormat(const SamText &t, const OutHeader *oh, const OutHit *hits, const uint16_t *cig, const uint32_t *idx,
                     uint32_t first, uint32_t n, uint64_t *len, uint64_t *off, void *scanTmp, size_t *scanTmpBytes,
                     uint32_t *err, char *out, int pass, hipStream_t s, const PairSpec &ps, uint64_t totalBytes) {
  const dim3 grid((n + 1 + 255) / 256);
  if (pass == 0) {
    if (t.tags)
      hipLaunchKernelGGL(samLenKernel<true>, grid, dim3(256), 0, s, t, oh, hits, cig, idx, first, n, len, err, ps);
    else
      hipLaunchKernelGGL(samLenKernel<false>, grid, dim3(256), 0, s, t, oh, hits, cig, idx, first, n, len, err, ps);
    FCHK(hipGetLastError());
  } else if (pass == 1) {  // exclusive scan of n + 1 lengths: off[n] = total bytes
    FCHK(rocprim::exclusive_scan(scanTmp, *scanTmpBytes, len, off, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), s));
  } else {
    if (n == 0) return;
    const uint32_t wg = kSamWg;
    const dim3 grid2((n + wg - 1) / wg);
    // Staging for wg units: what wg units of the batch's average length need with 3 % to spare, in
    // steps of 256 B (a workgroup whose units do not fit writes them directly, correct but
    // uncoalesced), so that as many workgroups as possible share a CU's 160 KiB of LDS.
    // Without a total (totalBytes = 0) 384 B per unit; descriptors and stage together at most 64 KiB.
    // descriptors: name, SEQ and QUAL of one line per unit (two lines per pair)
    // (GWA_SAM_DEFER=0, tests and measurements: no descriptors, every lane copies its own fields)
    const char *dfr = getenv("GWA_SAM_DEFER");
    const uint32_t lines = ps.np ? 2 : 1, cap = dfr && atoi(dfr) == 0 ? 0 : wg * 3 * lines;
    const uint32_t descBytes = (cap * (uint32_t)sizeof(SamField) + 4 + 15) & ~15u;
    const uint64_t stageMax = (65536 - descBytes) & ~255u;  // (and 16 bits of stage offset in a descriptor)
    uint64_t need = totalBytes ? totalBytes * wg * 103 / 100 / n + 16 : 384 * wg;
    need = (need + 255) & ~(uint64_t)255;
    uint32_t stage = (uint32_t)(need < 4096 ? 4096 : need > stageMax ? stageMax : need);
    // GWA_SAM_STAGE (tests): a small staging buffer, so that workgroups whose records do not fit
    // take the direct-write path next to workgroups that stage theirs
    const char *stg = getenv("GWA_SAM_STAGE");
    if (stg && atoi(stg) > 0) stage = atoi(stg) <= 1024 ? 1024 : 4096;
    // lanes per field from the average field length (a line's SEQ and QUAL are all but ~60 of its bytes)
    const uint64_t avgLine = totalBytes / n / lines;
    const uint64_t fieldItems = (avgLine > 64 ? (avgLine - 60) / 2 : 2) / 16;  // whole chunks per field
    uint32_t lshift = 2;
    while (lshift < 6 && (1u << lshift) < fieldItems) ++lshift;
    const uint32_t lds = descBytes + stage;
    if (t.tags)
      hipLaunchKernelGGL(samWriteKernel<true>, grid2, dim3(wg), lds, s, t, oh, hits, cig, idx, first, n, off, out, ps, stage,
                         cap, lshift);
    else
      hipLaunchKernelGGL(samWriteKernel<false>, grid2, dim3(wg), lds, s, t, oh, hits, cig, idx, first, n, off, out, ps, stage,
                         cap, lshift);
    FCHK(hipGetLastError());
  }
}

size_t samScanTempBytes(uint32_t n) {
  size_t b = 0;
  FCHK(rocprim::exclusive_scan(nullptr, b, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0, (size_t)n + 1,
                               rocprim::plus<uint64_t>(), (hipStream_t)0));
  return b;
}

// Batch statistics: sums of the per-read instrumentation (gwa_batch_stats_t), one atomic per
// workgroup and field.
__global__ void __launch_bounds__(256) statsKernel(const OutHeader *__restrict__ oh, uint32_t n,
                                                   unsigned long long *__restrict__ acc) {
  __shared__ unsigned long long sh[kStatFields];
  if (threadIdx.x < kStatFields) sh[threadIdx.x] = 0;
  __syncthreads();
  unsigned long long v[kStatFields];
  for (int f = 0; f < kStatFields; ++f) v[f] = 0;
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
    const OutHeader &h = oh[r];
    v[0] += (unsigned)h.fmSearches;
    v[1] += (unsigned)h.quickSteps;
    v[2] += (unsigned)h.blocks;
    v[3] += (unsigned)h.searchBlocks;
    v[4] += (unsigned)h.kmerLookups;
    v[5] += (unsigned)h.saReads;
    v[6] += (unsigned)h.quickSa;
    v[7] += (unsigned)h.quickShort;
    v[8] += (unsigned)h.searchShort;
    v[9] += (unsigned)h.states;
    v[10] += (unsigned)h.numSW;
    v[11] += (unsigned)h.verifyBytes;
    v[12] += h.status == ST_MAPPED;
    v[13] += h.status == ST_UNMAPPED;
    v[14] += (unsigned)h.quickText;
  }
  for (int f = 0; f < kStatFields; ++f) atomicAdd(&sh[f], v[f]);
  __syncthreads();
  if (threadIdx.x < kStatFields) atomicAdd(&acc[threadIdx.x], sh[threadIdx.x]);
}

void launchStats(const OutHeader *oh, uint32_t n, unsigned long long *acc, hipStream_t s) {
  FCHK(hipMemsetAsync(acc, 0, kStatFields * sizeof(unsigned long long), s));
  if (n == 0) return;
  const uint32_t g = (n + 255) / 256;
  hipLaunchKernelGGL(statsKernel, dim3(g > 2048 ? 2048 : g), dim3(256), 0, s, oh, n, acc);
  FCHK(hipGetLastError());
}

// ---- the first tier's search list in quick-scan order (gwa_batch_run) ----
// The searched reads' order does not change any result (each lane runs its own reads to the end), but
// it decides which reads share a wavefront.  A read's best-first search starts from seeds given by its
// quick scan (each strand's numMismatches and longest-match start, S/BidirectionalSuffixFilter.java:
// 318-341), so reads whose scans match alike walk search trees of a similar shape: they reach their
// reports and finish at similar times, and the lanes of a wavefront take the same paths through a
// micro-step together.  Key (byKey), of the strand with fewer mismatches ("lo"; forward on a tie): its
// longest-match start, then both strands' mismatch counts, then its first empty step (2-base buckets).
// !byKey: the read index (a deep tier's list back in input order).  A stable radix sort keeps input
// order inside a key.  Measured per 10M C2 reads (first-tier search ms, hg19 / hg19r): unsorted
// 89.0 / 132.0, this key 65.3 / 111.1; DESIGN.md §4 lists the keys tried.
__global__ void searchKeyKernel(const uint32_t *list, uint32_t n, const ScanRes *sres, int byKey, uint32_t *keys) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = list[i];
  if (!byKey) {
    keys[i] = r;
    return;
  }
  const ScanRes q = sres[r];
  const bool f = q.nmF <= q.nmR;
  const uint32_t lo = (uint32_t)(f ? q.nmF : q.nmR) & 15, hi = (uint32_t)(f ? q.nmR : q.nmF) & 15;
  const uint32_t lm = (uint32_t)(f ? q.lmF : q.lmR) & 511, fe = (uint32_t)(f ? q.feF : q.feR) & 511;
  keys[i] = (((lm >> 1) << 4 | lo) << 4 | hi) << 8 | fe >> 1;
}

size_t sortSearchListTmpBytes(uint32_t n) {
  size_t b = 0;
  FCHK(rocprim::radix_sort_pairs(nullptr, b, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                 (uint32_t *)nullptr, (size_t)n, 0, 32, (hipStream_t)0));
  return b;
}

void launchSortSearchList(const uint32_t *listIn, uint32_t *listOut, uint32_t *keysIn, uint32_t *keysOut, uint32_t n,
                          const ScanRes *sres, bool byKey, void *tmp, size_t tmpBytes, hipStream_t s) {
  hipLaunchKernelGGL(searchKeyKernel, dim3((n + 255) / 256), dim3(256), 0, s, listIn, n, sres, byKey ? 1 : 0, keysIn);
  FCHK(hipGetLastError());
  size_t b = tmpBytes;
  FCHK(rocprim::radix_sort_pairs(tmp, b, keysIn, keysOut, listIn, listOut, (size_t)n, 0, byKey ? 24 : 32, s));
}

}  // namespace gwa
