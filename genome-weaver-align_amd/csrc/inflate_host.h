// inflate_host.h -- the host side of the BGZF decoder: the walk over the members' headers (host only,
// for the device path too) and the host build of inflate_core.h, the lanes of a workgroup replayed phase
// by phase, one member after the other.  Bytes and statuses identical to the device kernel
// (inflate.hip); used by gwa_bgzf_decompress(device < 0), by a RecordStream without a device inflater
// and by tests/inflate_host.cpp.
#pragma once
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "inflate_core.h"

namespace gwa {
namespace inflate {

// a member the decoder refused: its index in the run handed to the inflater, and its status word
struct InflateError : std::runtime_error {
  uint64_t member;
  uint32_t status;
  InflateError(uint64_t m, uint32_t st)
      : std::runtime_error(std::string(statusText(st & 0xff)) + " at payload bit " + std::to_string(st >> 8) + " (status " +
                           std::to_string(st & 0xff) + ")"),
        member(m), status(st) {}
};

// The header of the member at p[0, avail): 1 = a whole member, *size its bytes and *m its payload
// (offsets relative to p), 0 = more bytes are needed to tell (fewer than the member's size are there),
// -1 = not a BGZF member, *why says what was wrong.
inline int parseMember(const uint8_t *p, uint64_t avail, Member *m, uint32_t *size, std::string *why) {
  if (avail < 12) return 0;
  if (p[0] != 0x1f || p[1] != 0x8b) {
    *why = "no gzip magic";
    return -1;
  }
  if (p[2] != 8) {
    *why = "compression method " + std::to_string(p[2]) + " (deflate is 8)";
    return -1;
  }
  if (!(p[3] & 4)) {
    *why = "no extra field (FLG.FEXTRA): a gzip member without BGZF's BC subfield";
    return -1;
  }
  const uint32_t xlen = p[10] | (uint32_t)p[11] << 8;
  if (avail < 12 + (uint64_t)xlen) return 0;
  uint32_t at = 12, bsize = 0;
  bool found = false;
  while (at + 4 <= 12 + xlen) {
    const uint32_t slen = p[at + 2] | (uint32_t)p[at + 3] << 8;
    if (at + 4 + slen > 12 + xlen) break;
    if (p[at] == 'B' && p[at + 1] == 'C' && slen == 2 && !found) {
      bsize = p[at + 4] | (uint32_t)p[at + 5] << 8;
      found = true;
    }
    at += 4 + slen;
  }
  if (!found) {
    *why = "no BC subfield of length 2 in the extra field";
    return -1;
  }
  // (other FLG bits -- name, comment, header CRC -- would put fields before the payload that BSIZE alone
  // cannot delimit; BGZF writers set FEXTRA only)
  if (p[3] & ~4u) {
    *why = "FLG " + std::to_string(p[3]) + " (BGZF sets FEXTRA only)";
    return -1;
  }
  const uint32_t total = bsize + 1, hdr = 12 + xlen;
  if (total < hdr + 8) {
    *why = "BSIZE + 1 = " + std::to_string(total) + " is less than header and trailer (" + std::to_string(hdr + 8) + ")";
    return -1;
  }
  if (avail < total) return 0;
  const uint8_t *t = p + total - 8;
  m->payOff = hdr;
  m->payLen = total - hdr - 8;
  m->crc = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
  m->isize = t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
  m->outOff = 0;
  m->pad = 0;
  *size = total;
  if (m->isize > kMaxOut) {
    *why = "ISIZE " + std::to_string(m->isize) + " (a BGZF member holds at most 65536 bytes)";
    return -1;
  }
  return 1;
}

inline std::string memberLabel(uint64_t index, uint64_t offset) {
  return "BGZF member " + std::to_string(index) + " at byte " + std::to_string(offset) + ": ";
}

// every member of in[0, n), which must be a concatenation of whole members: their payloads, and their
// texts side by side from output offset 0; offs[k] = member k's first byte.  Returns the text's length.
inline uint64_t walkMembers(const uint8_t *in, uint64_t n, std::vector<Member> &ms, std::vector<uint64_t> &offs) {
  uint64_t at = 0, outAt = 0;
  while (at < n) {
    Member m;
    uint32_t size = 0;
    std::string why;
    const int r = parseMember(in + at, n - at, &m, &size, &why);
    if (r < 0) throw std::runtime_error(memberLabel(ms.size(), at) + why);
    if (r == 0) throw std::runtime_error(memberLabel(ms.size(), at) + "the member runs past the input's end (" + std::to_string(n - at) + " bytes left)");
    m.payOff += at;
    m.outOff = outAt;
    offs.push_back(at);
    ms.push_back(m);
    outAt += m.isize;
    at += size;
  }
  return outAt;
}

// The host build: members ms[0, nm) of comp[0, n) inflated to dst + outOff, one after the other;
// status[k] = member k's status word.  Returns the first member with a nonzero status, nm when none.
inline uint64_t inflateHost(const uint8_t *comp, uint64_t n, const Member *ms, uint64_t nm, uint8_t *dst, uint64_t dstLen,
                            uint32_t *status) {
  std::unique_ptr<Shared> sh(new Shared());
  uint64_t firstBad = nm;
  for (uint64_t k = 0; k < nm; ++k) {
    const Member &m = ms[k];
    uint32_t st = 0;
    if (m.payOff > n || m.payLen > n - m.payOff) st = makeStatus(kErrTruncated, 0);
    else if (m.outOff > dstLen || m.isize > dstLen - m.outOff) st = makeStatus(kErrLength, 0);
    else inflateMember(*sh, comp + m.payOff, m.payLen, 0, m.payLen, m.isize, m.crc, dst + m.outOff, &st);
    status[k] = st;
    if (st && firstBad == nm) firstBad = k;
  }
  return firstBad;
}

}  // namespace inflate
}  // namespace gwa
