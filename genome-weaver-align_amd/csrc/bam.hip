// bam.hip -- a batch's BAM alignment records written on the GPU (the record rule: include/gwa.h, the
// per-read logic: bam_core.h over sam_core.h's record selection).
//
// The shape is the SAM writer's (batch_io.hip): one lane per unit (a read, or a pair), a length pass
// (the writer in counting mode), an exclusive scan of the lengths (rocPRIM), and a write pass in which a
// workgroup puts its units' contiguous output range together in LDS and stores it with coalesced 16-B
// stores.  A lane writes the fixed fields, the CIGAR and the tags of its records itself and leaves a
// BamField descriptor for each bulk field (name, SEQ nibbles, QUAL - 33, 0xFF fill); after a barrier
// the workgroup produces those, 16 output bytes per lane and step (bamChunk).  The records go to the
// BGZF encoder (bgzf.hip) as they are.  The SAM kernels are separate instances and are not touched.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <cstdlib>
#include <stdexcept>
#include <string>

#include "bam_core.h"
#include "kernels.h"

namespace gwa {

#define BCHK(x)                                                                                         \
  do {                                                                                                  \
    hipError_t e_ = (x);                                                                                \
    if (e_ != hipSuccess) throw std::runtime_error(std::string("bam_format: ") + #x + ": " + hipGetErrorString(e_)); \
  } while (0)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// one unit's records: a read's, or a pair's two
__device__ __forceinline__ int bamUnit(BamOut &o, const SamText &t, uint32_t r, const OutHeader *oh, const OutHit *hits,
                                       const uint16_t *cig, const PairSpec &ps) {
  if (ps.np) return samPair(o, t, r, ps.np, oh, hits, cig, ps.minIns, ps.maxIns, ps.resc);
  return samRead(o, t, r, oh[r], hits, cig);
}

// err[0]: the lowest unit the SAM writer fails on too; err[1]: the lowest unit with a read name longer
// than kBamNameMax bytes
__global__ void __launch_bounds__(256) bamLenKernel(SamText t, const OutHeader *__restrict__ oh, const OutHit *__restrict__ hits,
                                                    const uint16_t *__restrict__ cig, const uint32_t *__restrict__ idx,
                                                    uint32_t first, uint32_t n, uint64_t *__restrict__ len,
                                                    uint32_t *__restrict__ err, PairSpec ps) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j > n) return;
  if (j == n) {  // the scan's total
    len[n] = 0;
    return;
  }
  const uint32_t r = idx ? idx[j] : first + j;
  BamOut o{nullptr, 0};
  if (bamUnit(o, t, r, oh, hits, cig, ps) != 0) {
    atomicMin(err, j);
    o.n = 0;
  } else if (o.longName) {
    atomicMin(err + 1, j);
    o.n = 0;
  }
  len[j] = o.n;
}

// The workgroup's deferred fields: 1 << lshift consecutive lanes share a field, each takes every
// (1 << lshift)-th 16-byte piece of its output.
__device__ __forceinline__ void bamServeFields(const BamField *fields, uint32_t D, uint8_t *stage, uint32_t lshift) {
  const uint32_t L = 1u << lshift, G = blockDim.x >> lshift;
  const uint32_t sub = threadIdx.x & (L - 1), g = threadIdx.x >> lshift;
  for (uint32_t d = g; d < D; d += G) {
    const BamField f = fields[d];
    const uint8_t *src = reinterpret_cast<const uint8_t *>((uint64_t)f.srcHi << 32 | f.srcLo);
    const uint32_t len = f.w & 0xFFFFFFu, kind = f.w >> 24;
    const uint32_t nb = bamFieldBytes(kind, len);
    for (uint32_t i0 = 16 * sub; i0 < nb; i0 += 16 * L)
      bamPut(stage + f.at + i0, bamChunk(kind, src, len, i0), nb - i0 < 16 ? nb - i0 : 16);
  }
}

constexpr uint32_t kBamWg = 64;  // units (= lanes) per workgroup of the write pass

// Write pass (samWriteKernel's scheme).  Dynamic LDS: cap descriptors of 16 B, the counter, the stage.
// A range larger than the stage is written directly to HBM by its lanes.
__global__ void __launch_bounds__(kBamWg) bamWriteKernel(SamText t, const OutHeader *__restrict__ oh, const OutHit *__restrict__ hits,
                                                     const uint16_t *__restrict__ cig, const uint32_t *__restrict__ idx,
                                                     uint32_t first, uint32_t n, const uint64_t *__restrict__ off,
                                                     uint8_t *__restrict__ out, PairSpec ps, uint32_t stageBytes, uint32_t cap,
                                                     uint32_t lshift) {
  extern __shared__ u32x4 bamLds[];
  BamField *fields = reinterpret_cast<BamField *>(bamLds);
  const uint32_t descBytes = cap * (uint32_t)sizeof(BamField) + 16;
  uint32_t *count = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(bamLds) + descBytes - 16);
  uint8_t *stage = reinterpret_cast<uint8_t *>(bamLds) + descBytes;
  const uint32_t j0 = blockIdx.x * blockDim.x, j = j0 + threadIdx.x;
  const uint32_t jEnd = j0 + blockDim.x < n ? j0 + blockDim.x : n;
  const uint64_t gBeg = off[j0], gEnd = off[jEnd];
  const uint64_t base = gBeg & ~(uint64_t)15;
  if (gEnd - base > (uint64_t)stageBytes) {
    if (j < n) {
      BamOut o{out + off[j], 0};
      (void)bamUnit(o, t, idx ? idx[j] : first + j, oh, hits, cig, ps);
    }
    return;
  }
  if (threadIdx.x == 0) *count = 0;
  __syncthreads();
  if (j < n) {
    BamOut o{stage + (off[j] - base), 0, BamDefer{fields, count, cap, stage}};
    (void)bamUnit(o, t, idx ? idx[j] : first + j, oh, hits, cig, ps);
  }
  __syncthreads();
  const uint32_t D = *count < cap ? *count : cap;
  bamServeFields(fields, D, stage, lshift);
  __syncthreads();
  const uint32_t chunks = (uint32_t)((gEnd - base + 15) >> 4);
  const u32x4 *st = reinterpret_cast<const u32x4 *>(stage);
  for (uint32_t c = threadIdx.x; c < chunks; c += blockDim.x) {
    const uint64_t a = base + 16ull * c;
    if (a >= gBeg && a + 16 <= gEnd) {
      *reinterpret_cast<u32x4 *>(out + a) = st[c];
    } else {
      const uint8_t *sb = stage + 16ull * c;
      for (int i = 0; i < 16; ++i)
        if (a + i >= gBeg && a + i < gEnd) out[a + i] = sb[i];
    }
  }
}

// launchSamFormat's three passes for BAM records; err points at two words (bamLenKernel)
void launchBamFormat(const SamText &t, const OutHeader *oh, const OutHit *hits, const uint16_t *cig, const uint32_t *idx,
                     uint32_t first, uint32_t n, uint64_t *len, uint64_t *off, void *scanTmp, size_t *scanTmpBytes,
                     uint32_t *err, uint8_t *out, int pass, hipStream_t s, const PairSpec &ps, uint64_t totalBytes) {
  if (pass == 0) {
    hipLaunchKernelGGL(bamLenKernel, dim3((n + 1 + 255) / 256), dim3(256), 0, s, t, oh, hits, cig, idx, first, n, len, err, ps);
    BCHK(hipGetLastError());
  } else if (pass == 1) {  // exclusive scan of n + 1 lengths: off[n] = total bytes
    BCHK(rocprim::exclusive_scan(scanTmp, *scanTmpBytes, len, off, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), s));
  } else {
    if (n == 0) return;
    const uint32_t wg = kBamWg;
    // descriptors: name, SEQ and QUAL of one record per unit (two per pair); the stage sized from the
    // batch's average as the SAM writer's is; GWA_SAM_DEFER and GWA_SAM_STAGE mean here what they mean there
    const char *dfr = getenv("GWA_SAM_DEFER");
    const uint32_t lines = ps.np ? 2 : 1, cap = dfr && atoi(dfr) == 0 ? 0 : wg * 3 * lines;
    const uint32_t descBytes = cap * (uint32_t)sizeof(BamField) + 16;
    const uint64_t stageMax = (65536 - descBytes) & ~255u;
    uint64_t need = totalBytes ? totalBytes * wg * 103 / 100 / n + 16 : 384 * wg;
    need = (need + 255) & ~(uint64_t)255;
    uint32_t stage = (uint32_t)(need < 4096 ? 4096 : need > stageMax ? stageMax : need);
    const char *stg = getenv("GWA_SAM_STAGE");
    if (stg && atoi(stg) > 0) stage = atoi(stg) <= 1024 ? 1024 : 4096;
    // lanes per field from the average QUAL length (two thirds of what a record holds beyond ~50 bytes)
    const uint64_t avgRec = totalBytes / n / lines;
    const uint64_t fieldItems = (avgRec > 64 ? (avgRec - 50) * 2 / 3 : 2) / 16;
    uint32_t lshift = 1;
    while (lshift < 6 && (1u << lshift) < fieldItems) ++lshift;
    hipLaunchKernelGGL(bamWriteKernel, dim3((n + wg - 1) / wg), dim3(wg), descBytes + stage, s, t, oh, hits, cig, idx, first, n,
                       off, out, ps, stage, cap, lshift);
    BCHK(hipGetLastError());
  }
}

}  // namespace gwa
