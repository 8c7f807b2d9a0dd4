// bam_sort.h -- the device side of the coordinate sort (bam_sort.hip) as the host code calls it
// (gwa_api.cpp, bam_sorter.cpp).  No HIP types: `stream` is a hipStream_t.
#pragma once
#include <cstdint>

#include "bam_dup_core.h"
#include "bam_sort_core.h"

namespace gwa {

struct BamSortBuf;  // the device buffers of one batch's sorts, grown on demand and kept between calls
BamSortBuf *bamSortCreate();
void bamSortFree(BamSortBuf *b);

struct BamSortResult {
  const uint8_t *d_sorted = nullptr;          // the records in key order (device memory of the BamSortBuf)
  const bamsort::BamRecInfo *d_info = nullptr;  // per record, in that order
  const uint64_t *d_keys = nullptr;
  const bamdup::BamDupInfo *d_dup = nullptr;    // per record, in that order: only with wantDup
  float dup_ms = 0;                             // the duplicate-marking kernels (wantDup)
  uint64_t records = 0, bytes = 0;
  // walk + keys (a batch's first sort: its buffer allocations too), radix sort, permuted sizes + scan, gather kernel
  float walk_ms = 0, sort_ms = 0, permute_ms = 0, gather_ms = 0;
};
// Sorts the records of d_text[0, bytes): unit j's records lie in [d_off[j], d_off[j + 1]), j < n (a unit is
// any run of whole records).  textCap: the bytes that may be read behind d_text (>= bytes).
void bamSortRun(BamSortBuf *b, const uint8_t *d_text, uint64_t bytes, uint64_t textCap, const uint64_t *d_off, uint64_t n,
                void *stream, BamSortResult *out, bool wantDup = false);

// Host bytes with host record offsets off[0 .. n] sorted on `device` into sorted[0, off[n]) and info[0, n).
// dup (may be null): the records' duplicate-marking entries in sorted order, their kernels' time added to *dupSeconds.
void bamSortBytesDevice(int device, const uint8_t *bytes, const uint64_t *off, uint64_t n, uint8_t *sorted,
                        bamsort::BamRecInfo *info, bamdup::BamDupInfo *dup = nullptr, double *dupSeconds = nullptr);
// perm[0, n): the stable order of keys[0, n) (n < 2^32), sorted on `device`.
void bamSortOrderDevice(int device, const uint64_t *keys, uint64_t n, uint32_t *perm);

}  // namespace gwa
