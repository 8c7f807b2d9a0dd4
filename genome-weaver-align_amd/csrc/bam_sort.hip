// bam_sort.hip -- a batch's BAM records put into coordinate order on the GPU (the rule: include/gwa.h
// "Sorted BAM", the per-record logic: bam_sort_core.h).
//
// Passes, all on the batch's stream:
//   1. one lane per unit walks the unit's block_size chain and counts its records (bamCountKernel);
//   2. an exclusive scan of the counts (rocPRIM) gives every unit its first record ordinal;
//   3. the same walk writes per record its source offset, its BamRecInfo (key, size, beg, end, index bin),
//      the key and the ordinal (bamFieldsKernel);
//   4. rocprim::radix_sort_pairs of (key, ordinal): stable, so equal keys keep input order;
//   5. the permuted BamRecInfo and sizes (bamPermuteKernel) and an exclusive scan of the sizes: every
//      record's place in the sorted stream;
//   6. the gather (bamGatherKernel), destination-tiled: a workgroup owns kTile contiguous output bytes, finds
//      the records that overlap them by two binary searches in the destination offsets, puts their
//      (destination, source) offsets in LDS, and every lane builds aligned 16-byte output pieces from
//      unaligned 16-byte loads of the one or two records a piece spans.  Every output byte is written by
//      exactly one lane from exactly one source byte: nothing depends on a race.
//   7. only with duplicate marking (wantDup): the records' entries in input order and their permuted,
//      completed form (bam_dup.hip).  Without it nothing here is launched or allocated.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <stdexcept>
#include <string>
#include <vector>

#include "bam_dup.h"
#include "bam_sort.h"

namespace gwa {

using namespace bamsort;

#define SCHK(x)                                                                                        \
  do {                                                                                                 \
    hipError_t e_ = (x);                                                                               \
    if (e_ != hipSuccess) throw std::runtime_error(std::string("bam_sort: ") + #x + ": " + hipGetErrorString(e_)); \
  } while (0)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned __int128 u128;

__global__ void __launch_bounds__(256) bamCountKernel(const uint8_t *__restrict__ text, const uint64_t *__restrict__ off, uint64_t n,
                                                      uint64_t *__restrict__ cnt) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j > n) return;
  uint64_t c = 0;
  if (j < n) {
    uint64_t p = off[j];
    const uint64_t e = off[j + 1];
    while (p < e) {
      const uint32_t sz = recordAt(text + p, e - p);
      if (!sz) break;
      ++c;
      p += sz;
    }
  }
  cnt[j] = c;  // (cnt[n] = 0: the scan's total)
}

__global__ void __launch_bounds__(256) bamFieldsKernel(const uint8_t *__restrict__ text, const uint64_t *__restrict__ off, uint64_t n,
                                                       const uint64_t *__restrict__ first, uint64_t *__restrict__ srcOff,
                                                       BamRecInfo *__restrict__ info, uint64_t *__restrict__ keys,
                                                       uint32_t *__restrict__ ord) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  uint64_t p = off[j], r = first[j];
  const uint64_t e = off[j + 1], rEnd = first[j + 1];
  while (p < e && r < rEnd) {
    const uint32_t sz = recordAt(text + p, e - p);
    if (!sz) break;
    const BamRecInfo x = infoOf(text + p, sz);
    srcOff[r] = p;
    info[r] = x;
    keys[r] = x.key;
    ord[r] = (uint32_t)r;
    ++r;
    p += sz;
  }
}

__global__ void __launch_bounds__(256) bamIotaKernel(uint32_t *__restrict__ ord, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ord[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(256) bamPermuteKernel(const BamRecInfo *__restrict__ info, const uint32_t *__restrict__ perm, uint64_t R,
                                                        BamRecInfo *__restrict__ infoSorted, uint64_t *__restrict__ psize) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > R) return;
  if (i == R) {
    psize[R] = 0;
    return;
  }
  const BamRecInfo x = info[perm[i]];
  infoSorted[i] = x;
  psize[i] = x.size;
}

constexpr uint32_t kTile = 16384;                         // output bytes per workgroup
constexpr uint32_t kGatherWg = 256;
constexpr uint32_t kTileRecs = kTile / kMinRecord + 2;    // records that can overlap a tile

// the largest k in [0, R) with a[k] <= x, for a[0] = 0 <= x < a[R]
__device__ __forceinline__ uint64_t lastNotAfter(const uint64_t *__restrict__ a, uint64_t R, uint64_t x) {
  uint64_t lo = 0, hi = R;  // a[lo] <= x < a[hi]
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (a[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// 16 bytes at src + at as a little-endian value; bytes behind srcCap read as 0
__device__ __forceinline__ u128 gatherLoad(const uint8_t *__restrict__ src, uint64_t at, uint64_t srcCap) {
  if (at + 16 <= srcCap) {
    typedef const __attribute__((address_space(1))) char *GlobalBytes;
    u32x4 q;
    __builtin_memcpy(&q, (GlobalBytes)(uintptr_t)(src + at), 16);
    return (u128)((uint64_t)q.y << 32 | q.x) | (u128)((uint64_t)q.w << 32 | q.z) << 64;
  }
  u128 v = 0;
  for (uint32_t i = 0; i < 16 && at + i < srcCap; ++i) v |= (u128)src[at + i] << (8 * i);
  return v;
}

__global__ void __launch_bounds__(kGatherWg) bamGatherKernel(const uint8_t *__restrict__ src, uint64_t srcCap,
                                                             const uint64_t *__restrict__ srcOff, const uint32_t *__restrict__ perm,
                                                             const uint64_t *__restrict__ dstOff, uint64_t R, uint64_t total,
                                                             uint8_t *__restrict__ dst) {
  __shared__ uint64_t sDst[kTileRecs + 1];
  __shared__ uint64_t sSrc[kTileRecs];
  __shared__ uint64_t sK[2];
  const uint64_t base = (uint64_t)blockIdx.x * kTile;
  if (base >= total) return;
  const uint64_t end = base + kTile < total ? base + kTile : total;
  if (threadIdx.x == 0) sK[0] = lastNotAfter(dstOff, R, base);
  if (threadIdx.x == 64) sK[1] = lastNotAfter(dstOff, R, end - 1);
  __syncthreads();
  const uint64_t k0 = sK[0];
  uint32_t cnt = (uint32_t)(sK[1] - k0 + 1);
  if (cnt > kTileRecs) cnt = kTileRecs;  // (cannot happen: every record has at least kMinRecord bytes)
  for (uint32_t i = threadIdx.x; i <= cnt; i += kGatherWg) {
    sDst[i] = dstOff[k0 + i];
    if (i < cnt) sSrc[i] = srcOff[perm[k0 + i]];
  }
  __syncthreads();
  const uint32_t pieces = (uint32_t)((end - base + 15) >> 4);
  for (uint32_t c = threadIdx.x; c < pieces; c += kGatherWg) {
    const uint64_t a = base + 16ull * c;
    const uint32_t nb = end - a < 16 ? (uint32_t)(end - a) : 16u;
    uint32_t lo = 0, hi = cnt;  // sDst[lo] <= a < sDst[hi]
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (sDst[mid] <= a) lo = mid;
      else hi = mid;
    }
    u128 v = 0;
    uint32_t filled = 0, i = lo;
    while (filled < nb && i < cnt) {  // one or two records (a record is longer than a piece)
      const uint64_t pos = a + filled, left = sDst[i + 1] - pos;
      const uint32_t take = left < nb - filled ? (uint32_t)left : nb - filled;
      u128 x = gatherLoad(src, sSrc[i] + (pos - sDst[i]), srcCap);
      if (take < 16) x &= ((u128)1 << (8 * take)) - 1;
      v |= x << (8 * filled);
      filled += take;
      ++i;
    }
    u32x4 q;
    q.x = (uint32_t)v;
    q.y = (uint32_t)(v >> 32);
    q.z = (uint32_t)(v >> 64);
    q.w = (uint32_t)(v >> 96);
    *reinterpret_cast<u32x4 *>(dst + a) = q;  // (dst is 16-byte aligned and holds total rounded up to 16 bytes)
  }
}

namespace {
template <class T>
void grow(T **p, size_t *cap, size_t need) {
  if (*p && *cap >= need) return;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  const size_t want = need + need / 8 + 64;
  SCHK(hipMalloc((void **)p, want * sizeof(T)));
  *cap = want;
}
struct Ev {
  hipEvent_t e[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  Ev() {
    for (auto &x : e) SCHK(hipEventCreate(&x));
  }
  ~Ev() {
    for (auto &x : e)
      if (x) (void)hipEventDestroy(x);
  }
};
}  // namespace

struct BamSortBuf {
  uint64_t *cnt = nullptr, *first = nullptr, *srcOff = nullptr, *keys = nullptr, *keysOut = nullptr, *psize = nullptr, *dstOff = nullptr;
  uint32_t *ord = nullptr, *perm = nullptr;
  BamRecInfo *info = nullptr, *infoSorted = nullptr;
  bamdup::BamDupInfo *dupStage = nullptr, *dupSorted = nullptr;  // only with duplicate marking
  size_t dupStageCap = 0, dupSortedCap = 0;
  uint8_t *tmp = nullptr, *sorted = nullptr;
  size_t cntCap = 0, firstCap = 0, srcOffCap = 0, keysCap = 0, keysOutCap = 0, psizeCap = 0, dstOffCap = 0, ordCap = 0, permCap = 0,
         infoCap = 0, infoSortedCap = 0, tmpCap = 0, sortedCap = 0;
};

BamSortBuf *bamSortCreate() { return new BamSortBuf(); }
void bamSortFree(BamSortBuf *b) {
  if (!b) return;
  void *ps[] = {b->cnt, b->first, b->srcOff, b->keys, b->keysOut, b->psize, b->dstOff, b->ord, b->perm, b->info, b->infoSorted, b->tmp,
                b->sorted, b->dupStage, b->dupSorted};
  for (void *p : ps)
    if (p) (void)hipFree(p);
  delete b;
}

static inline dim3 gridFor(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

void bamSortRun(BamSortBuf *b, const uint8_t *d_text, uint64_t bytes, uint64_t textCap, const uint64_t *d_off, uint64_t n,
                void *stream, BamSortResult *out, bool wantDup) {
  hipStream_t s = (hipStream_t)stream;
  *out = BamSortResult{};
  if (n == 0 || bytes == 0) return;
  if (n >= 0xFFFFFFFFull) throw std::runtime_error("bam_sort: more than 2^32 - 2 units in one batch");
  Ev ev;
  SCHK(hipEventRecord(ev.e[0], s));
  grow(&b->cnt, &b->cntCap, n + 1);
  grow(&b->first, &b->firstCap, n + 1);
  size_t scanBytes = 0;
  SCHK(rocprim::exclusive_scan(nullptr, scanBytes, b->cnt, b->first, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), s));
  grow(&b->tmp, &b->tmpCap, scanBytes);
  hipLaunchKernelGGL(bamCountKernel, gridFor(n + 1), dim3(256), 0, s, d_text, d_off, n, b->cnt);
  SCHK(hipGetLastError());
  SCHK(rocprim::exclusive_scan(b->tmp, scanBytes, b->cnt, b->first, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), s));
  uint64_t R = 0;
  SCHK(hipMemcpyAsync(&R, b->first + n, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  SCHK(hipStreamSynchronize(s));
  if (R == 0) throw std::runtime_error("bam_sort: " + std::to_string(bytes) + " bytes hold no record");
  if (R > 0xFFFFFFFEull) throw std::runtime_error("bam_sort: more than 2^32 - 2 records in one batch");
  grow(&b->srcOff, &b->srcOffCap, R);
  grow(&b->info, &b->infoCap, R);
  grow(&b->infoSorted, &b->infoSortedCap, R);
  grow(&b->keys, &b->keysCap, R);
  grow(&b->keysOut, &b->keysOutCap, R);
  grow(&b->ord, &b->ordCap, R);
  grow(&b->perm, &b->permCap, R);
  grow(&b->psize, &b->psizeCap, R + 1);
  grow(&b->dstOff, &b->dstOffCap, R + 1);
  grow(&b->sorted, &b->sortedCap, (size_t)((bytes + 15) & ~(uint64_t)15) + 16);
  size_t sortBytes = 0, scan2 = 0;
  SCHK(rocprim::radix_sort_pairs(nullptr, sortBytes, b->keys, b->keysOut, b->ord, b->perm, (size_t)R, 0, 64, s));
  SCHK(rocprim::exclusive_scan(nullptr, scan2, b->psize, b->dstOff, (uint64_t)0, (size_t)R + 1, rocprim::plus<uint64_t>(), s));
  const size_t tmpNeed = sortBytes > scan2 ? sortBytes : scan2;
  grow(&b->tmp, &b->tmpCap, tmpNeed);
  hipLaunchKernelGGL(bamFieldsKernel, gridFor(n), dim3(256), 0, s, d_text, d_off, n, b->first, b->srcOff, b->info, b->keys, b->ord);
  SCHK(hipGetLastError());
  SCHK(hipEventRecord(ev.e[1], s));
  SCHK(rocprim::radix_sort_pairs(b->tmp, sortBytes, b->keys, b->keysOut, b->ord, b->perm, (size_t)R, 0, 64, s));
  SCHK(hipEventRecord(ev.e[2], s));
  hipLaunchKernelGGL(bamPermuteKernel, gridFor(R + 1), dim3(256), 0, s, b->info, b->perm, R, b->infoSorted, b->psize);
  SCHK(hipGetLastError());
  SCHK(rocprim::exclusive_scan(b->tmp, scan2, b->psize, b->dstOff, (uint64_t)0, (size_t)R + 1, rocprim::plus<uint64_t>(), s));
  uint64_t total = 0;
  SCHK(hipMemcpyAsync(&total, b->dstOff + R, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  SCHK(hipStreamSynchronize(s));
  // (checked before the gather: its stores are sized from the scan, the buffer from `bytes`)
  if (total != bytes)
    throw std::runtime_error("bam_sort: the records' block_size chain covers " + std::to_string(total) + " of " +
                             std::to_string(bytes) + " bytes");
  SCHK(hipEventRecord(ev.e[4], s));
  hipLaunchKernelGGL(bamGatherKernel, dim3((uint32_t)((total + kTile - 1) / kTile)), dim3(kGatherWg), 0, s, d_text, textCap, b->srcOff,
                     b->perm, b->dstOff, R, total, b->sorted);
  SCHK(hipGetLastError());
  SCHK(hipEventRecord(ev.e[3], s));
  if (wantDup) {  // the records' duplicate-marking entries, in sorted order (bam_dup.hip)
    grow(&b->dupStage, &b->dupStageCap, R);
    grow(&b->dupSorted, &b->dupSortedCap, R);
    bamDupLaunch(d_text, b->srcOff, b->info, R, b->dupStage, s);
    bamDupPermuteLaunch(b->dupStage, b->perm, R, b->dupSorted, s);
    SCHK(hipEventRecord(ev.e[5], s));
    SCHK(hipEventSynchronize(ev.e[5]));
    SCHK(hipEventElapsedTime(&out->dup_ms, ev.e[3], ev.e[5]));
    out->d_dup = b->dupSorted;
  }
  SCHK(hipEventSynchronize(ev.e[3]));
  SCHK(hipEventElapsedTime(&out->walk_ms, ev.e[0], ev.e[1]));
  SCHK(hipEventElapsedTime(&out->sort_ms, ev.e[1], ev.e[2]));
  SCHK(hipEventElapsedTime(&out->permute_ms, ev.e[2], ev.e[4]));
  SCHK(hipEventElapsedTime(&out->gather_ms, ev.e[4], ev.e[3]));
  out->d_sorted = b->sorted;
  out->d_info = b->infoSorted;
  out->d_keys = b->keysOut;
  out->records = R;
  out->bytes = total;
}

void bamSortBytesDevice(int device, const uint8_t *bytes, const uint64_t *off, uint64_t n, uint8_t *sorted, BamRecInfo *info,
                        bamdup::BamDupInfo *dup, double *dupSeconds) {
  if (n == 0) return;
  SCHK(hipSetDevice(device));
  const uint64_t len = off[n];
  uint8_t *dText = nullptr;
  uint64_t *dOff = nullptr;
  BamSortBuf *b = nullptr;
  hipStream_t s = nullptr;
  auto release = [&]() {
    if (s) (void)hipStreamSynchronize(s);
    bamSortFree(b);
    if (dText) (void)hipFree(dText);
    if (dOff) (void)hipFree(dOff);
    if (s) (void)hipStreamDestroy(s);
  };
  try {
    SCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    SCHK(hipMalloc((void **)&dText, len + 16));
    SCHK(hipMalloc((void **)&dOff, (n + 1) * sizeof(uint64_t)));
    SCHK(hipMemcpyAsync(dText, bytes, len, hipMemcpyHostToDevice, s));
    SCHK(hipMemcpyAsync(dOff, off, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    b = bamSortCreate();
    BamSortResult r;
    bamSortRun(b, dText, len, len, dOff, n, s, &r, dup != nullptr);
    if (r.records != n) throw std::runtime_error("bam_sort: the device counted " + std::to_string(r.records) + " of " + std::to_string(n) + " records");
    SCHK(hipMemcpyAsync(sorted, r.d_sorted, len, hipMemcpyDeviceToHost, s));
    SCHK(hipMemcpyAsync(info, r.d_info, n * sizeof(BamRecInfo), hipMemcpyDeviceToHost, s));
    if (dup) {
      SCHK(hipMemcpyAsync(dup, r.d_dup, n * sizeof(bamdup::BamDupInfo), hipMemcpyDeviceToHost, s));
      if (dupSeconds) *dupSeconds += r.dup_ms * 1e-3;
    }
    SCHK(hipStreamSynchronize(s));
  } catch (...) {
    release();
    throw;
  }
  release();
}

void bamSortOrderDevice(int device, const uint64_t *keys, uint64_t n, uint32_t *perm) {
  if (n == 0) return;
  if (n > 0xFFFFFFFEull) throw std::runtime_error("bam_sort: more than 2^32 - 2 records in one sort scope");
  SCHK(hipSetDevice(device));
  uint64_t *dK = nullptr, *dKo = nullptr;
  uint32_t *dV = nullptr, *dVo = nullptr;
  void *tmp = nullptr;
  auto release = [&]() {
    for (void *p : {(void *)dK, (void *)dKo, (void *)dV, (void *)dVo, tmp})
      if (p) (void)hipFree(p);
  };
  try {
    SCHK(hipMalloc((void **)&dK, n * 8));
    SCHK(hipMalloc((void **)&dKo, n * 8));
    SCHK(hipMalloc((void **)&dV, n * 4));
    SCHK(hipMalloc((void **)&dVo, n * 4));
    size_t tb = 0;
    SCHK(rocprim::radix_sort_pairs(nullptr, tb, dK, dKo, dV, dVo, (size_t)n, 0, 64, (hipStream_t) nullptr));
    SCHK(hipMalloc(&tmp, tb ? tb : 16));
    SCHK(hipMemcpy(dK, keys, n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(bamIotaKernel, gridFor(n), dim3(256), 0, (hipStream_t) nullptr, dV, n);
    SCHK(hipGetLastError());
    SCHK(rocprim::radix_sort_pairs(tmp, tb, dK, dKo, dV, dVo, (size_t)n, 0, 64, (hipStream_t) nullptr));
    SCHK(hipMemcpy(perm, dVo, n * 4, hipMemcpyDeviceToHost));
  } catch (...) {
    release();
    throw;
  }
  release();
}

}  // namespace gwa
