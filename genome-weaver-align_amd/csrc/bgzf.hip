// bgzf.hip -- BGZF compression of a text in HBM (bgzf_core.h compiled for the device).
//
//   bgzf_block_kernel    one workgroup of 1024 lanes per 65 280-byte slice, everything in LDS (157.8 KiB:
//                        one workgroup = 16 waves per CU); the block goes into its own zeroed slot of
//                        kSlotBytes, its size into sizes[block]
//   bgzf_offsets_kernel  exclusive scan of the sizes (one workgroup)
//   bgzf_compact_kernel  the slots copied side by side: 8-byte stores at the destination's alignment,
//                        source words funnel-shifted
#include <hip/hip_runtime.h>

#include "bgzf_core.h"
#include "kernels.h"

namespace gwa {

using namespace bgzf;

__global__ __launch_bounds__(kLanes) void bgzf_block_kernel(const uint8_t *in, uint64_t n, uint64_t *slots, uint32_t *sizes,
                                                           uint32_t *stored) {
  __shared__ Shared sh;
  const uint64_t off = (uint64_t)blockIdx.x * kSlice;
  const uint32_t len = (uint32_t)(n - off < kSlice ? n - off : kSlice);
  compressSlice(sh, in + off, len, slots + (uint64_t)blockIdx.x * (kSlotBytes / 8), sizes + blockIdx.x, stored);
}

// offs[i] = sizes[0] + .. + sizes[i - 1], offs[nb] = the total
__global__ __launch_bounds__(1024) void bgzf_offsets_kernel(const uint32_t *sizes, uint32_t nb, uint64_t *offs) {
  __shared__ uint64_t part[1024];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (nb + 1023) / 1024;
  const uint32_t b = t * per, e = b + per < nb ? b + per : nb;
  uint64_t s = 0;
  for (uint32_t i = b; i < e; ++i) s += sizes[i];
  part[t] = s;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {
    const uint64_t v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint64_t at = part[t] - s;
  for (uint32_t i = b; i < e; ++i) {
    offs[i] = at;
    at += sizes[i];
  }
  if (t == 1023) offs[nb] = part[1023];
}

__global__ __launch_bounds__(256) void bgzf_compact_kernel(const uint64_t *slots, const uint32_t *sizes, const uint64_t *offs,
                                                          uint8_t *out) {
  const uint64_t *src = slots + (uint64_t)blockIdx.x * (kSlotBytes / 8);
  const uint8_t *srcB = reinterpret_cast<const uint8_t *>(src);
  const uint32_t size = sizes[blockIdx.x];
  uint8_t *dst = out + offs[blockIdx.x];
  const uint32_t head = (uint32_t)((8 - (reinterpret_cast<uintptr_t>(dst) & 7)) & 7);  // bytes up to the first aligned word
  const uint32_t h = head < size ? head : size;
  if (threadIdx.x < h) dst[threadIdx.x] = srcB[threadIdx.x];
  const uint32_t words = (size - h) / 8;
  uint64_t *dw = reinterpret_cast<uint64_t *>(dst + h);
  const uint32_t sh = 8 * (h & 7);
  for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) {
    // source bytes [h + 8 w, h + 8 w + 8): two aligned words of the slot (the second within the slot:
    // h + 8 w + 15 < size + 8 <= kSlotBytes)
    const uint32_t sw = (h + 8 * w) >> 3;
    const uint64_t lo = src[sw];
    dw[w] = sh ? (lo >> sh) | (src[sw + 1] << (64 - sh)) : lo;
  }
  const uint32_t done = h + 8 * words;
  if (threadIdx.x < size - done) dst[done + threadIdx.x] = srcB[done + threadIdx.x];
}

size_t bgzfSlotBytes(uint64_t nBlocks) { return (size_t)nBlocks * kSlotBytes + 16; }

void launchBgzfBlocks(const uint8_t *in, uint64_t n, uint64_t nBlocks, void *slots, uint32_t *sizes, uint64_t *offs,
                      uint32_t *stored, hipStream_t s) {
  if (!nBlocks) return;
  (void)hipMemsetAsync(slots, 0, bgzfSlotBytes(nBlocks), s);
  (void)hipMemsetAsync(stored, 0, sizeof(uint32_t), s);
  hipLaunchKernelGGL(bgzf_block_kernel, dim3((uint32_t)nBlocks), dim3(kLanes), 0, s, in, n, (uint64_t *)slots, sizes, stored);
  hipLaunchKernelGGL(bgzf_offsets_kernel, dim3(1), dim3(1024), 0, s, sizes, (uint32_t)nBlocks, offs);
}

void launchBgzfCompact(const void *slots, const uint32_t *sizes, const uint64_t *offs, uint64_t nBlocks, uint8_t *out,
                       hipStream_t s) {
  if (!nBlocks) return;
  hipLaunchKernelGGL(bgzf_compact_kernel, dim3((uint32_t)nBlocks), dim3(256), 0, s, (const uint64_t *)slots, sizes, offs, out);
}

}  // namespace gwa
