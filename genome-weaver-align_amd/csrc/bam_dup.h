// bam_dup.h -- the device side of duplicate marking (bam_dup.hip) as the host code calls it (bam_sort.hip,
// bam_sorter.cpp, gwa_api.cpp).  No HIP types: `stream` is a hipStream_t.
#pragma once
#include <cstdint>

#include "bam_dup_core.h"

namespace gwa {

// The per-run pass over R records in input order (d_srcOff[r]: record r's offset in d_text, d_info[r].size its
// size): d_stage[r] = the record's own entry and its link (bam_dup_core.h kLink*).
void bamDupLaunch(const uint8_t *d_text, const uint64_t *d_srcOff, const bamsort::BamRecInfo *d_info, uint64_t R,
                  bamdup::BamDupInfo *d_stage, void *stream);
// d_out[i] = the completed entry of record d_perm[i]
void bamDupPermuteLaunch(const bamdup::BamDupInfo *d_stage, const uint32_t *d_perm, uint64_t R, bamdup::BamDupInfo *d_out, void *stream);
// The per-run kernel alone over host records (offsets off[0 .. n]) resident in HBM, launched `repeat` times:
// *kernelMs = the last launch between HIP events; out (may be null): the n completed entries, in input order.
void bamDupRunTimed(int device, const uint8_t *bytes, const uint64_t *off, uint64_t n, int repeat, bamdup::BamDupInfo *out,
                    double *kernelMs);
// The global resolve on `device`, as bamdup::resolveHost: bits must hold (nOrdinals + 31) / 32 words.  Fails
// with the bytes it needs where the device cannot give them.
void bamDupResolveDevice(int device, const bamdup::BamDupInfo *e, uint64_t n, uint64_t nOrdinals, uint32_t *bits, bamdup::DupStats *st);

}  // namespace gwa
