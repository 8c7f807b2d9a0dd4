// bgzf_host.h -- the host build of the BGZF encoder (bgzf_core.h): the lanes of a workgroup replayed
// phase by phase, one slice after the other.  Byte-identical to the device kernels (bgzf.hip); used for
// the SAM header of `align --bgzf`, by gwa_bgzf_compress(device < 0) and by tests/bgzf_host.cpp.
#pragma once
#include <cstring>
#include <memory>
#include <vector>

#include "bgzf_core.h"

namespace gwa {
namespace bgzf {

struct HostStats {
  uint64_t blocks = 0, stored = 0;
};

// the BGZF blocks of in[0, n) appended to out (no EOF marker; n = 0 appends nothing)
inline void compressHost(const uint8_t *in, uint64_t n, std::vector<uint8_t> &out, HostStats *st = nullptr) {
  std::unique_ptr<Shared> sh(new Shared());
  std::vector<uint64_t> slot(kSlotBytes / 8);
  for (uint64_t off = 0; off < n; off += kSlice) {
    const uint32_t len = (uint32_t)(n - off < kSlice ? n - off : kSlice);
    std::fill(slot.begin(), slot.end(), 0);
    uint32_t size = 0, stored = 0;
    compressSlice(*sh, in + off, len, slot.data(), &size, &stored);
    const size_t at = out.size();
    out.resize(at + size);
    memcpy(out.data() + at, slot.data(), size);
    if (st) {
      ++st->blocks;
      st->stored += stored;
    }
  }
}

}  // namespace bgzf
}  // namespace gwa
