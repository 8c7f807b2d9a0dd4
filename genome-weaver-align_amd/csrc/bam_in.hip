// bam_in.hip -- BAM alignment records decoded into reads on the GPU (include/gwa.h "BAM input"; the
// per-record logic is bam_in_core.h).
//
// The host frames the records (the block_size chain, record_stream.cpp) and hands over their bytes and
// the starts of the records that are reads.  Three passes turn them into the text a batch keeps:
//   length  one lane per record: the header fields, the name's length (the name stays where it is, in
//           the record bytes), whether the record has a quality, and the size of its slot in the
//           unpacked text: pad16(l_seq) bytes of SEQ, then pad16(l_seq) bytes of QUAL;
//   scan    rocPRIM exclusive scan of the slot sizes (every slot starts 16-B aligned);
//   unpack  work dealt by output bytes: 16 lanes own a record, each lane produces one 16-byte chunk of
//           output per step -- 16 letters from 8 packed bytes, or 16 quality characters from 16 bytes --
//           with 8-B aligned loads and one 16-B store, consecutive lanes on consecutive chunks; a 100-bp
//           read keeps 14 of its 16 lanes busy for one step.  Reverse-strand records (FLAG 0x10) are
//           reverse-complemented in the same pass: the chunk draws on the packed bytes from the far end.
// Content errors (no NUL in the name, a quality byte above 93) go to err[0] as the lowest offending
// record (atomicMin), err[1] counts the records without a quality; the host words the message.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <stdexcept>
#include <string>

#include "bam_in_core.h"
#include "kernels.h"

namespace gwa {

#define BCHK(x)                                                                                          \
  do {                                                                                                   \
    hipError_t e_ = (x);                                                                                 \
    if (e_ != hipSuccess) throw std::runtime_error(std::string("bam_in: ") + #x + ": " + hipGetErrorString(e_)); \
  } while (0)

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

// fields: nameB, nameE, seqB, seqE, qualB, qualE, n entries each (the last four are set by the unpack pass)
__global__ void __launch_bounds__(256) bamInLenKernel(const uint8_t *__restrict__ rec, const uint64_t *__restrict__ start,
                                                      uint32_t n, uint64_t *__restrict__ len, uint64_t *__restrict__ fields,
                                                      uint8_t *__restrict__ qualNull, uint32_t *__restrict__ err) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r == n) len[n] = 0;
  if (r >= n) return;
  const uint8_t *p = rec + start[r];
  const bamin::Fields f = bamin::fieldsOf(p);
  uint32_t e = bamin::kOk;
  const uint32_t nl = bamin::nameLenOf(p, f, &e);
  fields[r] = start[r] + bamin::kFixed;
  fields[(size_t)n + r] = start[r] + bamin::kFixed + nl;
  const bool qn = bamin::qualNullOf(p, f);
  qualNull[r] = qn ? 1 : 0;
  len[r] = bamin::slotBytes(f);
  if (qn) atomicAdd(err + 1, 1u);
  if (e != bamin::kOk) atomicMin(err, r);
}

constexpr uint32_t kGroup = 16;  // lanes per record

__global__ void __launch_bounds__(256) bamInUnpackKernel(const uint8_t *__restrict__ rec, const uint64_t *__restrict__ start,
                                                         uint32_t n, const uint64_t *__restrict__ off, uint64_t *__restrict__ fields,
                                                         const uint8_t *__restrict__ qualNull, uint8_t *__restrict__ out,
                                                         uint64_t outBytes, uint32_t *__restrict__ err) {
  const uint32_t r = blockIdx.x * (256 / kGroup) + threadIdx.x / kGroup, sub = threadIdx.x % kGroup;
  if (r >= n) return;
  const uint8_t *p = rec + start[r];
  const bamin::Fields f = bamin::fieldsOf(p);
  const uint64_t o = off[r], slot = bamin::pad16(f.lSeq), chunks = slot / 16;
  if (o + 2 * slot > outBytes) {  // (the host sized the text from the same fields: never taken)
    atomicMin(err, r);
    return;
  }
  if (sub == 0) {
    const size_t N = n;
    fields[2 * N + r] = o;
    fields[3 * N + r] = o + f.lSeq;
    fields[4 * N + r] = o + slot;
    fields[5 * N + r] = o + slot + f.lSeq;
  }
  const bool qn = qualNull[r] != 0;
  bool ok = true;
  for (uint64_t c = sub; c < 2 * chunks; c += kGroup) {
    uint64_t lo = 0, hi = 0;
    if (c < chunks) bamin::seqChunk(p, nullptr, f, c, &lo, &hi);
    else if (!qn) ok = bamin::qualChunk(p, nullptr, f, c - chunks, &lo, &hi) && ok;
    u64x2 v;
    v.x = lo;
    v.y = hi;
    *reinterpret_cast<u64x2 *>(out + o + 16 * c) = v;
  }
  if (!ok) atomicMin(err, r);
}

size_t bamInScanTempBytes(uint32_t n) {
  size_t b = 0;
  BCHK(rocprim::exclusive_scan(nullptr, b, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0, (size_t)n + 1,
                               rocprim::plus<uint64_t>(), (hipStream_t)0));
  return b ? b : 8;
}

void launchBamInLengths(const uint8_t *rec, const uint64_t *start, uint32_t n, uint64_t *len, uint64_t *off, uint64_t *fields,
                        uint8_t *qualNull, uint32_t *err, void *scanTmp, size_t scanTmpBytes, hipStream_t s) {
  hipLaunchKernelGGL(bamInLenKernel, dim3(n / 256 + 1), dim3(256), 0, s, rec, start, n, len, fields, qualNull, err);
  BCHK(hipGetLastError());
  BCHK(rocprim::exclusive_scan(scanTmp, scanTmpBytes, len, off, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), s));
}

void launchBamInUnpack(const uint8_t *rec, const uint64_t *start, uint32_t n, const uint64_t *off, uint64_t *fields,
                       const uint8_t *qualNull, uint8_t *out, uint64_t outBytes, uint32_t *err, hipStream_t s) {
  if (!n) return;
  const uint32_t per = 256 / kGroup;
  hipLaunchKernelGGL(bamInUnpackKernel, dim3((n + per - 1) / per), dim3(256), 0, s, rec, start, n, off, fields, qualNull, out,
                     outBytes, err);
  BCHK(hipGetLastError());
}

}  // namespace gwa
