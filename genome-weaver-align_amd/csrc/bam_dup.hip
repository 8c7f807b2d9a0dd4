// bam_dup.hip -- duplicate marking on the GPU (the rule: include/gwa.h "Duplicate marking", the per-record
// logic: bam_dup_core.h).
//
// Per run, after the sort's walk has written every record's source offset and BamRecInfo in input order:
//   1. bamDupKernel: 16 lanes own a record.  They read the fixed fields, compare the name with the next or
//      the previous record's where the flags allow a pair (16 bytes per lane), sum the reference length over
//      the CIGAR (one element per lane-step) and walk its two ends for u5, and sum the qualities from aligned
//      16-byte loads (head and tail masked, a piece that does not lie inside the record read bytewise), with
//      a reduction over the 16 lanes.  Lane 0 writes the record's own entry and how it links to a neighbour.
//   2. bamDupPermuteKernel: one lane per sorted record takes its entry through the sort's permutation and
//      completes it from the neighbour's (the template's score and leader, the other record's key).
// At finish, over the entries of all runs (bamDupResolveDevice): three key arrays, ordered by stable rocPRIM
// radix sorts of (key, index), the least significant key first -- pairs by (lo, hi, score descending, ordinal),
// fragments by (key, score descending, ordinal), the pairs' ends by key alone -- then one lane per sorted
// entry compares with its predecessor (a fragment also searches the sorted ends) and sets its template's bit
// with an atomic OR: every bit's value is a function of the sorted arrays, whatever the order of the ORs.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <stdexcept>
#include <string>

#include "bam_dup.h"

namespace gwa {

using namespace bamdup;
using bamsort::BamRecInfo;

#define DCHK(x)                                                                                        \
  do {                                                                                                 \
    hipError_t e_ = (x);                                                                               \
    if (e_ != hipSuccess) throw std::runtime_error(std::string("bam_dup: ") + #x + ": " + hipGetErrorString(e_)); \
  } while (0)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) char *GlobalBytes;

constexpr uint32_t kGroup = 16;  // lanes per record

__device__ __forceinline__ u32x4 load16(const uint8_t *p) {  // (any alignment)
  u32x4 q;
  __builtin_memcpy(&q, (GlobalBytes)(uintptr_t)p, 16);
  return q;
}

template <class T>
__device__ __forceinline__ T groupSum(T v) {
  for (int m = kGroup / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, kGroup);
  return v;
}

// the names at a and b, ln bytes each, are equal: lane `sub` compares bytes [16 sub, 16 sub + 16)
__device__ __forceinline__ bool namesEqual(const uint8_t *a, const uint8_t *b, uint32_t ln, uint32_t sub) {
  const uint32_t at = 16 * sub;
  int same = 1;
  if (at + 16 <= ln) {
    const u32x4 x = load16(a + at), y = load16(b + at);
    same = x.x == y.x && x.y == y.y && x.z == y.z && x.w == y.w;
  } else {
    for (uint32_t i = at; i < ln; ++i) same &= a[i] == b[i];
  }
  for (int m = kGroup / 2; m > 0; m >>= 1) same &= __shfl_xor(same, m, kGroup);
  return same != 0;
}

__global__ void __launch_bounds__(256) bamDupKernel(const uint8_t *__restrict__ text, const uint64_t *__restrict__ srcOff,
                                                    const BamRecInfo *__restrict__ info, uint64_t R,
                                                    BamDupInfo *__restrict__ stage) {
  const uint64_t r = (uint64_t)blockIdx.x * (256 / kGroup) + threadIdx.x / kGroup;
  const uint32_t sub = threadIdx.x % kGroup;
  if (r >= R) return;  // (a whole group leaves together)
  const uint8_t *p = text + srcOff[r];
  const uint32_t size = info[r].size;
  const int32_t refId = (int32_t)ld32(p + 4), pos = (int32_t)ld32(p + 8);
  const uint32_t lname = p[12], flag = ld16(p + 18), lseq = ld32(p + 20);
  const bool part = participates(flag, refId);

  uint64_t link = kLinkNone;
  if (firstOfPair(flag) && r + 1 < R) {
    const uint8_t *q = text + srcOff[r + 1];
    if (secondOfPair(ld16(q + 18)) && q[12] == lname && (uint64_t)36 + lname <= size && (uint64_t)36 + lname <= info[r + 1].size &&
        namesEqual(p + 36, q + 36, lname, sub))
      link = kLinkNext;
  } else if (secondOfPair(flag) && r > 0) {
    const uint8_t *q = text + srcOff[r - 1];
    if (firstOfPair(ld16(q + 18)) && q[12] == lname && (uint64_t)36 + lname <= size && (uint64_t)36 + lname <= info[r - 1].size &&
        namesEqual(q + 36, p + 36, lname, sub))
      link = kLinkPrev;
  }

  uint64_t endKey = kNoKey;
  uint32_t score = 0;
  if (part) {
    const uint32_t ncig = cigarInside(p, size) ? ld16(p + 16) : 0u;
    const uint8_t *c = p + 36 + lname;
    long long reflen = 0, lead = 0, trail = 0;
    for (uint32_t i = sub; i < ncig; i += kGroup) {
      const uint32_t v = ld32(c + 4 * i), op = v & 15u;
      if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) reflen += v >> 4;
    }
    reflen = groupSum(reflen);
    if (flag & 0x10u) {
      for (uint32_t i = ncig; i-- > 0;) {
        const uint32_t v = ld32(c + 4 * i), op = v & 15u;
        if (op != 4 && op != 5) break;
        trail += v >> 4;
      }
    } else {
      for (uint32_t i = 0; i < ncig; ++i) {
        const uint32_t v = ld32(c + 4 * i), op = v & 15u;
        if (op != 4 && op != 5) break;
        lead += v >> 4;
      }
    }
    endKey = endKeyFrom(refId, u5From(pos, flag & 0x10u, reflen, lead, trail, ncig), flag & 0x10u);

    if (qualInside(p, size)) {
      const uintptr_t recB = (uintptr_t)p, recE = recB + size;
      const uintptr_t qB = recB + qualOffset(p), qE = qB + lseq;
      for (uintptr_t ca = (qB & ~(uintptr_t)15) + 16 * (uintptr_t)sub; ca < qE; ca += 16 * kGroup) {
        const uint32_t from = ca < qB ? (uint32_t)(qB - ca) : 0u, to = qE - ca < 16 ? (uint32_t)(qE - ca) : 16u;
        if (ca >= recB && ca + 16 <= recE) {
          const u32x4 v = *reinterpret_cast<const u32x4 *>(ca);
          const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (uint32_t j = 0; j < 16; ++j)
            if (j >= from && j < to) score += qualValue((w[j >> 2] >> (8 * (j & 3))) & 255u);
        } else {
          for (uint32_t j = from; j < to; ++j) score += qualValue(reinterpret_cast<const uint8_t *>(ca)[j]);
        }
      }
      score = groupSum(score);
    }
  }
  if (sub == 0) {
    BamDupInfo x;
    x.endKey = endKey;
    x.mateKey = link;
    x.score = score;
    x.leader = (uint32_t)r;
    stage[r] = x;
  }
}

__global__ void __launch_bounds__(256) bamDupPermuteKernel(const BamDupInfo *__restrict__ stage, const uint32_t *__restrict__ perm,
                                                           uint64_t R, BamDupInfo *__restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < R) out[i] = linked(stage, perm[i]);
}

static inline dim3 gridFor(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

void bamDupLaunch(const uint8_t *d_text, const uint64_t *d_srcOff, const BamRecInfo *d_info, uint64_t R, BamDupInfo *d_stage,
                  void *stream) {
  if (!R) return;
  const uint64_t per = 256 / kGroup;
  hipLaunchKernelGGL(bamDupKernel, dim3((uint32_t)((R + per - 1) / per)), dim3(256), 0, (hipStream_t)stream, d_text, d_srcOff,
                     d_info, R, d_stage);
  DCHK(hipGetLastError());
}

void bamDupPermuteLaunch(const BamDupInfo *d_stage, const uint32_t *d_perm, uint64_t R, BamDupInfo *d_out, void *stream) {
  if (!R) return;
  hipLaunchKernelGGL(bamDupPermuteKernel, gridFor(R), dim3(256), 0, (hipStream_t)stream, d_stage, d_perm, R, d_out);
  DCHK(hipGetLastError());
}

void bamDupRunTimed(int device, const uint8_t *bytes, const uint64_t *off, uint64_t n, int repeat, BamDupInfo *out, double *kernelMs) {
  if (kernelMs) *kernelMs = 0;
  if (n == 0) return;
  if (n > 0xFFFFFFFEull) throw std::runtime_error("bam_dup: more than 2^32 - 2 records in one run");
  DCHK(hipSetDevice(device));
  const uint64_t len = off[n];
  std::vector<BamRecInfo> info(n);
  for (uint64_t i = 0; i < n; ++i) info[i] = bamsort::infoOf(bytes + off[i], (uint32_t)(off[i + 1] - off[i]));
  uint8_t *dText = nullptr;
  uint64_t *dOff = nullptr;
  BamRecInfo *dInfo = nullptr;
  BamDupInfo *dStage = nullptr, *dOut = nullptr;
  uint32_t *dPerm = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  auto release = [&]() {
    (void)hipDeviceSynchronize();
    for (void *p : {(void *)dText, (void *)dOff, (void *)dInfo, (void *)dStage, (void *)dOut, (void *)dPerm})
      if (p) (void)hipFree(p);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  };
  try {
    DCHK(hipMalloc((void **)&dText, len));
    DCHK(hipMalloc((void **)&dOff, n * sizeof(uint64_t)));
    DCHK(hipMalloc((void **)&dInfo, n * sizeof(BamRecInfo)));
    DCHK(hipMalloc((void **)&dStage, n * sizeof(BamDupInfo)));
    DCHK(hipEventCreate(&e0));
    DCHK(hipEventCreate(&e1));
    DCHK(hipMemcpy(dText, bytes, len, hipMemcpyHostToDevice));
    DCHK(hipMemcpy(dOff, off, n * sizeof(uint64_t), hipMemcpyHostToDevice));
    DCHK(hipMemcpy(dInfo, info.data(), n * sizeof(BamRecInfo), hipMemcpyHostToDevice));
    float ms = 0;
    for (int k = 0; k < (repeat > 0 ? repeat : 1); ++k) {
      DCHK(hipEventRecord(e0, nullptr));
      bamDupLaunch(dText, dOff, dInfo, n, dStage, nullptr);
      DCHK(hipEventRecord(e1, nullptr));
      DCHK(hipEventSynchronize(e1));
      DCHK(hipEventElapsedTime(&ms, e0, e1));
    }
    if (kernelMs) *kernelMs = ms;
    if (out) {  // the completed entries, through the identity permutation
      std::vector<uint32_t> iota(n);
      for (uint64_t i = 0; i < n; ++i) iota[i] = (uint32_t)i;
      DCHK(hipMalloc((void **)&dPerm, n * sizeof(uint32_t)));
      DCHK(hipMalloc((void **)&dOut, n * sizeof(BamDupInfo)));
      DCHK(hipMemcpy(dPerm, iota.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
      bamDupPermuteLaunch(dStage, dPerm, n, dOut, nullptr);
      DCHK(hipMemcpy(out, dOut, n * sizeof(BamDupInfo), hipMemcpyDeviceToHost));
    }
  } catch (...) {
    release();
    throw;
  }
  release();
}

// ---- the global resolve ----

enum { kArrEnds = 0, kArrPairScore, kArrPairHi, kArrPairLo, kArrFragScore, kArrFragKey };

// key of entry x in array `arr`; entries that are not in the array sort last
__device__ __forceinline__ uint64_t resolveKey(const BamDupInfo &x, int arr) {
  const uint64_t scoreOrd = (uint64_t)~x.score << 32 | x.leader;
  switch (arr) {
    case kArrEnds: return isPairEnd(x) ? x.endKey : kNoKey;
    case kArrPairScore: return isPairEntry(x) ? scoreOrd : kNoKey;
    case kArrPairHi: return isPairEntry(x) ? x.mateKey : kNoKey;
    case kArrPairLo: return isPairEntry(x) ? x.endKey : kNoKey;
    case kArrFragScore: return isFragment(x) ? scoreOrd : kNoKey;
    default: return isFragment(x) ? x.endKey : kNoKey;
  }
}

// keys[p] = the key of entry idx[p] (idx null: entry p, and idxOut[p] = p)
__global__ void __launch_bounds__(256) bamDupKeysKernel(const BamDupInfo *__restrict__ e, const uint32_t *__restrict__ idx, uint64_t n,
                                                        int arr, uint64_t *__restrict__ keys, uint32_t *__restrict__ idxOut) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const uint32_t i = idx ? idx[p] : (uint32_t)p;
  keys[p] = resolveKey(e[i], arr);
  if (idxOut) idxOut[p] = i;
}

__device__ __forceinline__ void setBit(uint32_t *bits, uint32_t o) { atomicOr(bits + (o >> 5), 1u << (o & 31)); }

// cnt: pair templates, duplicate pair templates, fragment templates, duplicate fragment templates
__global__ void __launch_bounds__(256) bamDupFlagPairsKernel(const BamDupInfo *__restrict__ e, const uint32_t *__restrict__ idx,
                                                             uint64_t n, uint32_t *__restrict__ bits,
                                                             unsigned long long *__restrict__ cnt) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const BamDupInfo x = e[idx[p]];
  if (!isPairEntry(x)) return;
  bool sameKey = false;
  if (p > 0) {
    const BamDupInfo y = e[idx[p - 1]];
    if (isPairEntry(y)) {
      if (y.leader == x.leader) return;  // the second entry of a template whose two keys are equal
      sameKey = y.endKey == x.endKey && y.mateKey == x.mateKey;
    }
  }
  atomicAdd(cnt + 0, 1ull);
  if (sameKey) {
    atomicAdd(cnt + 1, 1ull);
    setBit(bits, x.leader);
  }
}

__global__ void __launch_bounds__(256) bamDupFlagFragsKernel(const BamDupInfo *__restrict__ e, const uint32_t *__restrict__ idx,
                                                             uint64_t n, const uint64_t *__restrict__ ends,
                                                             uint32_t *__restrict__ bits, unsigned long long *__restrict__ cnt) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const BamDupInfo x = e[idx[p]];
  if (!isFragment(x)) return;
  bool dup = false;
  if (p > 0) {
    const BamDupInfo y = e[idx[p - 1]];
    dup = isFragment(y) && y.endKey == x.endKey;
  }
  if (!dup) {  // a pair's end at the same key: the first of ends[0, n) that is not below it
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (ends[mid] < x.endKey) lo = mid + 1;
      else hi = mid;
    }
    dup = lo < n && ends[lo] == x.endKey;
  }
  atomicAdd(cnt + 2, 1ull);
  if (dup) {
    atomicAdd(cnt + 3, 1ull);
    setBit(bits, x.leader);
  }
}

void bamDupResolveDevice(int device, const BamDupInfo *e, uint64_t n, uint64_t nOrdinals, uint32_t *bits, DupStats *st) {
  const size_t words = (size_t)((nOrdinals + 31) / 32);
  for (size_t i = 0; i < words; ++i) bits[i] = 0;
  if (n == 0) return;
  if (n > 0xFFFFFFFEull) throw std::runtime_error("bam_dup: more than 2^32 - 2 records in one scope");
  for (uint64_t i = 0; i < n; ++i)  // (the kernels set bit `leader`)
    if (e[i].leader >= nOrdinals) throw std::runtime_error("bam_dup: entry " + std::to_string(i) + " names a template ordinal outside the scope");
  DCHK(hipSetDevice(device));
  size_t pairTmp = 0, keyTmp = 0;
  DCHK(rocprim::radix_sort_pairs(nullptr, pairTmp, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                 (size_t)n, 0, 64, (hipStream_t) nullptr));
  DCHK(rocprim::radix_sort_keys(nullptr, keyTmp, (uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n, 0, 64, (hipStream_t) nullptr));
  auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t bE = pad(n * sizeof(BamDupInfo)), bK = pad(n * 8), bV = pad(n * 4), bBits = pad(words * 4 + 8), bCnt = 256,
               bTmp = pad((pairTmp > keyTmp ? pairTmp : keyTmp) + 16);
  const size_t need = bE + 3 * bK + 2 * bV + bBits + bCnt + bTmp;
  uint8_t *slab = nullptr;
  const hipError_t ae = hipMalloc((void **)&slab, need);
  if (ae != hipSuccess) {
    (void)hipGetLastError();
    throw std::runtime_error("bam_dup: the duplicate resolve of " + std::to_string(n) + " records needs " + std::to_string(need) +
                             " bytes of device memory: " + hipGetErrorString(ae));
  }
  try {
    uint8_t *at = slab;
    auto take = [&](size_t b) {
      uint8_t *p = at;
      at += b;
      return p;
    };
    BamDupInfo *dE = (BamDupInfo *)take(bE);
    uint64_t *kA = (uint64_t *)take(bK), *kB = (uint64_t *)take(bK), *ends = (uint64_t *)take(bK);
    uint32_t *vA = (uint32_t *)take(bV), *vB = (uint32_t *)take(bV);
    uint32_t *dBits = (uint32_t *)take(bBits);
    unsigned long long *dCnt = (unsigned long long *)take(bCnt);
    void *tmp = take(bTmp);
    hipStream_t s = nullptr;
    DCHK(hipMemcpy(dE, e, n * sizeof(BamDupInfo), hipMemcpyHostToDevice));
    DCHK(hipMemsetAsync(dBits, 0, bBits, s));
    DCHK(hipMemsetAsync(dCnt, 0, bCnt, s));
    auto keys = [&](const uint32_t *idx, int arr, uint32_t *idxOut) {
      hipLaunchKernelGGL(bamDupKeysKernel, gridFor(n), dim3(256), 0, s, dE, idx, n, arr, kA, idxOut);
      DCHK(hipGetLastError());
    };
    auto sortPairs = [&](uint32_t *vin, uint32_t *vout) {
      DCHK(rocprim::radix_sort_pairs(tmp, pairTmp, kA, kB, vin, vout, (size_t)n, 0, 64, s));
    };
    // the pairs' ends
    keys(nullptr, kArrEnds, nullptr);
    DCHK(rocprim::radix_sort_keys(tmp, keyTmp, kA, ends, (size_t)n, 0, 64, s));
    // the pairs: (lo, hi, score descending, ordinal), the least significant key first
    keys(nullptr, kArrPairScore, vA);
    sortPairs(vA, vB);
    keys(vB, kArrPairHi, nullptr);
    sortPairs(vB, vA);
    keys(vA, kArrPairLo, nullptr);
    sortPairs(vA, vB);
    hipLaunchKernelGGL(bamDupFlagPairsKernel, gridFor(n), dim3(256), 0, s, dE, vB, n, dBits, dCnt);
    DCHK(hipGetLastError());
    // the fragments: (key, score descending, ordinal)
    keys(nullptr, kArrFragScore, vA);
    sortPairs(vA, vB);
    keys(vB, kArrFragKey, nullptr);
    sortPairs(vB, vA);
    hipLaunchKernelGGL(bamDupFlagFragsKernel, gridFor(n), dim3(256), 0, s, dE, vA, n, ends, dBits, dCnt);
    DCHK(hipGetLastError());
    unsigned long long cnt[4];
    DCHK(hipMemcpy(cnt, dCnt, sizeof cnt, hipMemcpyDeviceToHost));
    if (words) DCHK(hipMemcpy(bits, dBits, words * 4, hipMemcpyDeviceToHost));
    st->pair_templates += cnt[0];
    st->dup_pair_templates += cnt[1];
    st->frag_templates += cnt[2];
    st->dup_frag_templates += cnt[3];
  } catch (...) {
    (void)hipDeviceSynchronize();
    (void)hipFree(slab);
    throw;
  }
  (void)hipFree(slab);
}

}  // namespace gwa
