// inflate.hip -- BGZF members inflated in HBM (inflate_core.h compiled for the device).
//
//   inflate_block_kernel  one workgroup of 256 lanes per member; the slice, the payload window and the
//                         lookup tables live in LDS (74.4 KiB: two workgroups per CU); wave 0 walks the
//                         member's bit stream, all lanes build tables, check the CRC32 and store the slice
//   DeviceInflater        pooled device buffers and a stream of their own around one launch: compressed
//                         bytes and the member table H2D, the kernel, text and statuses D2H
#include <hip/hip_runtime.h>

#include <mutex>
#include <stdexcept>
#include <string>

#include "inflate_host.h"
#include "kernels.h"

namespace gwa {

using namespace inflate;

__global__ __launch_bounds__(kLanes) void inflate_block_kernel(const uint8_t *in, uint64_t n, const Member *ms, uint8_t *out,
                                                              uint64_t outCap, uint32_t *status) {
  __shared__ Shared sh;
  const Member m = ms[blockIdx.x];
  // (the table comes from the host's walk of the headers; a member outside the buffers is refused all the same)
  if (m.payOff > n || m.payLen > n - m.payOff) {
    if (threadIdx.x == 0) status[blockIdx.x] = makeStatus(kErrTruncated, 0);
    return;
  }
  if (m.outOff > outCap || m.isize > outCap - m.outOff) {
    if (threadIdx.x == 0) status[blockIdx.x] = makeStatus(kErrLength, 0);
    return;
  }
  const uint64_t base = m.payOff & ~15ull;  // in is 16-byte aligned: so is in + base
  const uint64_t rem = n - base;
  inflateMember(sh, in + base, (uint32_t)(rem < (1u << 20) ? rem : (1u << 20)), (uint32_t)(m.payOff - base), m.payLen, m.isize,
                m.crc, out + m.outOff, status + blockIdx.x);
}

void launchInflate(const uint8_t *in, uint64_t n, const inflate::Member *ms, uint64_t nMembers, uint8_t *out, uint64_t outCap,
                   uint32_t *status, hipStream_t s) {
  if (!nMembers) return;
  hipLaunchKernelGGL(inflate_block_kernel, dim3((uint32_t)nMembers), dim3(kLanes), 0, s, in, n, ms, out, outCap, status);
}

namespace {
void chk(hipError_t e, const char *what) {
  if (e != hipSuccess) throw std::runtime_error(std::string("HIP error in the BGZF inflater (") + what + "): " + hipGetErrorString(e));
}
}  // namespace

struct DeviceInflater {
  int device = 0;
  std::mutex mu;  // (the two streams of a paired run share one inflater)
  hipStream_t stream = nullptr;
  uint8_t *dIn = nullptr, *dOut = nullptr;
  Member *dMs = nullptr;
  uint32_t *dSt = nullptr, *hSt = nullptr;
  size_t inCap = 0, outCap = 0, msCap = 0;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  float lastKernelMs = 0;

  template <class T>
  void grow(T **p, size_t *cap, size_t need) {
    if (*cap >= need) return;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    const size_t want = need + need / 8 + 4096;
    chk(hipMalloc((void **)p, want), "hipMalloc");
    *cap = want;
  }
  ~DeviceInflater() {
    (void)hipSetDevice(device);
    for (void *p : {(void *)dIn, (void *)dOut, (void *)dMs, (void *)dSt})
      if (p) (void)hipFree(p);
    if (hSt) (void)hipHostFree(hSt);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

DeviceInflater *inflaterCreate(int device) {
  auto *d = new DeviceInflater();
  d->device = device;
  try {
    chk(hipSetDevice(device), "hipSetDevice");
    chk(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking), "stream");
    chk(hipEventCreate(&d->e0), "event");
    chk(hipEventCreate(&d->e1), "event");
  } catch (...) {
    delete d;
    throw;
  }
  return d;
}

void inflaterFree(DeviceInflater *d) { delete d; }

float inflaterKernelMs(const DeviceInflater *d) { return d->lastKernelMs; }

// members ms[0, nm) of comp[0, n) inflated into dst[0, dstLen) (host memory); throws inflate::InflateError
// for the first member the kernel refused.  repeat > 1 (measurements): the kernel is launched that many
// times, lastKernelMs is the last launch's time.
void inflaterRun(DeviceInflater *d, const uint8_t *comp, uint64_t n, const Member *ms, uint64_t nm, uint8_t *dst, uint64_t dstLen,
                 int repeat) {
  if (!nm) return;
  std::lock_guard<std::mutex> g(d->mu);
  chk(hipSetDevice(d->device), "hipSetDevice");
  size_t stCap = d->msCap;
  d->grow(&d->dIn, &d->inCap, n + 16);
  d->grow(&d->dOut, &d->outCap, dstLen + 16);
  d->grow(&d->dMs, &d->msCap, nm * sizeof(Member));
  if (stCap != d->msCap || !d->dSt) {  // the statuses grow with the member table
    if (d->dSt) (void)hipFree(d->dSt);
    if (d->hSt) (void)hipHostFree(d->hSt);
    d->dSt = d->hSt = nullptr;
    const size_t words = d->msCap / sizeof(Member) + 1;
    chk(hipMalloc((void **)&d->dSt, words * sizeof(uint32_t)), "hipMalloc");
    chk(hipHostMalloc((void **)&d->hSt, words * sizeof(uint32_t), hipHostMallocDefault), "hipHostMalloc");
  }
  hipStream_t s = d->stream;
  chk(hipMemcpyAsync(d->dIn, comp, n, hipMemcpyHostToDevice, s), "H2D of the compressed bytes");
  chk(hipMemcpyAsync(d->dMs, ms, nm * sizeof(Member), hipMemcpyHostToDevice, s), "H2D of the member table");
  for (int r = 0; r < (repeat > 1 ? repeat : 1); ++r) {
    chk(hipEventRecord(d->e0, s), "event");
    launchInflate(d->dIn, n, d->dMs, nm, d->dOut, dstLen, d->dSt, s);
    chk(hipGetLastError(), "launch");
    chk(hipEventRecord(d->e1, s), "event");
  }
  if (dstLen) chk(hipMemcpyAsync(dst, d->dOut, dstLen, hipMemcpyDeviceToHost, s), "D2H of the text");
  chk(hipMemcpyAsync(d->hSt, d->dSt, nm * sizeof(uint32_t), hipMemcpyDeviceToHost, s), "D2H of the statuses");
  chk(hipStreamSynchronize(s), "synchronize");
  chk(hipEventElapsedTime(&d->lastKernelMs, d->e0, d->e1), "event");
  for (uint64_t k = 0; k < nm; ++k)
    if (d->hSt[k]) throw InflateError(k, d->hSt[k]);
}

}  // namespace gwa
