// inflate_core.h -- raw-deflate (RFC 1951) decoder for one BGZF member, the counterpart of bgzf_core.h.
//
// One header for the device and the host.  On the device a workgroup of kLanes threads inflates one
// member into LDS (inflate.hip); the host build replays the same lanes phase by phase -- a loop over the
// lanes wherever the device has a barrier -- so both give the same bytes and the same status
// (tests/inflate_host.cpp runs the replay under sanitizers, gwa_bgzf_decompress(device < 0) and a
// RecordStream without a device inflater use it).
//
// Symbol decoding is serial within a deflate stream, so wave 0 walks the bit stream: its 64 lanes hold
// the same reader state and decode the same symbol (one lookup in a 10-bit table in LDS; longer codes
// take the canonical walk over the per-length counts), lane 0 stores a literal, and the 64 lanes share
// an LZ77 copy, out[p + i] = out[p - d + i mod d].  Lanes of one wave run in step, so no barrier stands
// between two tokens; the host replays a copy byte by byte.  All kLanes lanes build the lookup tables
// from the code lengths (every lane the canonical code of its own symbols: no lane waits for another),
// compute the CRC32 of 256-byte segments (combined as the encoder does) and store the slice with 16-byte
// stores.  A phase touches shared words other lanes touch only through commutative atomics (add, xor).
//
// The payload is untrusted, so no access depends on its being well formed:
//   the bit reader feeds zeros past the payload's end and every token ends with an overrun check;
//   every table index is masked, every symbol range-checked before it is used;
//   every output store is bounded by ISIZE, every copy's distance by the bytes produced so far;
//   every loop consumes at least one payload bit per turn or ends, so clen bounds them all.
// A malformed member ends with a status (code | payload bit offset << 8) and stores nothing.
#pragma once
#include "bgzf_core.h"

namespace gwa {
namespace inflate {

constexpr uint32_t kLanes = 256;        // lanes of a workgroup
constexpr uint32_t kWave = 64;          // the lanes that walk the bit stream
constexpr uint32_t kMaxOut = 65536;     // ISIZE of a BGZF member is at most this
constexpr uint32_t kWinWords = 1024;    // the payload window in LDS: 4 KiB, refilled 16 bytes per lane x 4
constexpr uint32_t kTabBits = 10;       // first-level lookup: codes of up to 10 bits
constexpr uint32_t kTab = 1u << kTabBits;
constexpr uint32_t kSegCrc = kMaxOut / kLanes;  // bytes per lane in the CRC phase

// status codes (the low 8 bits of a member's status word; 0 = the member inflated and verified)
enum : uint32_t {
  kOk = 0,
  kErrBlockType = 1,   // BTYPE 3
  kErrStoredLen = 2,   // stored block: LEN != ~NLEN
  kErrTruncated = 3,   // the payload ends inside a block
  kErrCounts = 4,      // HLIT > 286 or HDIST > 30
  kErrClCode = 5,      // the code-length code is over-subscribed or incomplete
  kErrRepeat = 6,      // a repeat with no previous length, or running past HLIT + HDIST
  kErrNoEob = 7,       // no code for symbol 256
  kErrCodeSet = 8,     // literal/length or distance code lengths over-subscribed or incomplete
  kErrBadCode = 9,     // a bit pattern that is no code, literal/length symbol 286/287, distance symbol 30/31
  kErrDistance = 10,   // a distance reaching before the member's own output
  kErrLength = 11,     // the output is not exactly ISIZE bytes (or ISIZE > 65 536)
  kErrCrc = 12,        // CRC32 of the output differs from the trailer's
  kNumErr = 13
};
inline const char *statusText(uint32_t code) {
  switch (code) {
    case kOk: return "ok";
    case kErrBlockType: return "reserved deflate block type 3";
    case kErrStoredLen: return "stored block whose LEN and NLEN disagree";
    case kErrTruncated: return "deflate payload ends inside a block";
    case kErrCounts: return "more than 286 literal/length or 30 distance code lengths";
    case kErrClCode: return "invalid code-length code";
    case kErrRepeat: return "code-length repeat without a previous length or past the last length";
    case kErrNoEob: return "no code for the end-of-block symbol";
    case kErrCodeSet: return "over-subscribed or incomplete literal/length or distance code";
    case kErrBadCode: return "invalid literal/length or distance code";
    case kErrDistance: return "distance reaches before the member's output";
    case kErrLength: return "inflated length differs from ISIZE";
    case kErrCrc: return "CRC32 mismatch";
  }
  return "unknown status";
}

// one member of a run: where its deflate payload lies in the compressed bytes, where its text goes
struct Member {
  uint64_t payOff, outOff;
  uint32_t payLen, isize, crc, pad;
};
static_assert(sizeof(Member) == 32, "two 16-byte loads");

#if defined(__HIP_DEVICE_COMPILE__)
#define INF_LANES(...)                 \
  {                                    \
    const uint32_t lane = threadIdx.x; \
    (void)lane;                        \
    __VA_ARGS__                        \
  }                                    \
  __syncthreads();
// wave 0 alone (the other waves wait at the barrier)
#define INF_WAVE0(...)                    \
  if (threadIdx.x < kWave) {              \
    const uint32_t wlane = threadIdx.x;   \
    __VA_ARGS__                           \
  }                                       \
  __syncthreads();
// what the wave's lanes stored to LDS before is visible to its loads after (the lanes run in step)
#define INF_WAVE_SYNC()                                    \
  {                                                        \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
    __builtin_amdgcn_wave_barrier();                       \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
  }
constexpr uint32_t kWaveStep = kWave;
#else
#define INF_LANES(...) \
  for (uint32_t lane = 0; lane < kLanes; ++lane) { __VA_ARGS__ }
#define INF_WAVE0(...)      \
  {                         \
    const uint32_t wlane = 0; \
    __VA_ARGS__             \
  }
#define INF_WAVE_SYNC()
constexpr uint32_t kWaveStep = 1;  // the host replays the wave's shared loops element by element
#endif

struct Shared {
  uint32_t out[kMaxOut / 4 + 8];  // the slice (8 words of room for the store phase's funnel reads)
  uint32_t win[kWinWords];        // payload window: 16-byte chunks of the compressed bytes
  uint16_t litTab[kTab], distTab[kTab];  // code (bit-reversed) -> symbol << 4 | length; 0: none
  uint16_t clTab[128];
  uint16_t litSym[288], distSym[32];     // symbols in canonical order, for codes longer than kTabBits
  uint32_t litCount[16], distCount[16];  // codes per length
  uint32_t crcTab[256];
  uint8_t lens[320];  // the code lengths as a dynamic block's header sends them
  uint8_t clLen[20];
  uint32_t litKraft, distKraft, litUsed, distUsed;  // sums of 2^(15 - length), codes in use
  uint32_t status, bitPos, op, btype, bfinal, hlit, hdist, crc;
};
static_assert(sizeof(Shared) <= 80 * 1024, "two workgroups per CU");

GWA_HD uint32_t makeStatus(uint32_t code, uint32_t bitPos) { return code | bitPos << 8; }

// The payload as a bit string, read through the LDS window.  `in` is 16-byte aligned on the device and
// readable over [0, nIn); the payload is in[pay, pay + clen).  Bits past the payload read as zero;
// pos() may then exceed 8 * clen, which the caller checks after every token.
struct BitReader {
  Shared *sh;
  const uint8_t *in;
  uint32_t nIn, pay, payEnd;
  uint32_t winBase;  // first word of the window (a multiple of 4), ~0: nothing loaded
  uint32_t wi;       // next word to take
  uint64_t acc;
  uint32_t cnt;

  GWA_HD void refill(uint32_t word, uint32_t wlane) {
    winBase = word & ~3u;
    INF_WAVE_SYNC()
    for (uint32_t c = wlane; c < kWinWords / 4; c += kWaveStep) {
      uint32_t w[4];
      bgzf::loadChunk(in, winBase * 4 + c * 16, nIn, w);  // (bytes from nIn on read as zero)
      for (uint32_t k = 0; k < 4; ++k) sh->win[(c * 4 + k) & (kWinWords - 1)] = w[k];
    }
    INF_WAVE_SYNC()
  }
  GWA_HD uint32_t fetch(uint32_t word, uint32_t wlane) {
    if (word * 4 >= payEnd) return 0;
    if (winBase == ~0u || word < winBase || word - winBase >= kWinWords) refill(word, wlane);
    uint32_t w = sh->win[(word - winBase) & (kWinWords - 1)];
    if (word * 4 + 4 > payEnd) w &= (1u << (8 * (payEnd - word * 4))) - 1;  // (1..3 bytes of the payload)
    return w;
  }
  GWA_HD void seek(uint32_t bitPos, uint32_t wlane) {
    const uint32_t abs = pay * 8 + bitPos;
    wi = abs >> 5;
    const uint32_t s = abs & 31;
    acc = (uint64_t)(fetch(wi, wlane) >> s);
    cnt = 32 - s;
    ++wi;
  }
  GWA_HD void need32(uint32_t wlane) {  // at least 32 bits in acc
    if (cnt < 32) {
      acc |= (uint64_t)fetch(wi, wlane) << cnt;
      cnt += 32;
      ++wi;
    }
  }
  GWA_HD uint32_t peek(uint32_t n) const { return (uint32_t)acc & ((1u << n) - 1); }  // n <= 16
  GWA_HD void drop(uint32_t n) {  // n <= cnt
    acc >>= n;
    cnt -= n;
  }
  GWA_HD uint32_t bits(uint32_t n) {  // n <= 16, after need32
    const uint32_t v = peek(n);
    drop(n);
    return v;
  }
  GWA_HD uint32_t pos() const { return wi * 32 - cnt - pay * 8; }
  GWA_HD bool overrun() const { return pos() > (payEnd - pay) * 8; }
};

// a code longer than kTabBits (or none): the canonical walk, one length at a time.  v: the next 15 bits.
// Returns symbol << 4 | length, 0 when the bits are no code.
GWA_HD uint32_t slowDecode(const uint32_t *count, const uint16_t *sym, uint32_t nSym, uint32_t v) {
  uint32_t code = 0, first = 0, index = 0;
  for (uint32_t len = 1; len <= 15; ++len) {
    code |= (v >> (len - 1)) & 1;
    const uint32_t c = count[len];
    if (code < first + c) {
      const uint32_t at = index + (code - first);
      return at < nSym ? (uint32_t)sym[at] << 4 | len : 0u;
    }
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return 0;
}

// code length of literal/length symbol s (< 288) and of distance symbol s (< 32) in the current block
GWA_HD uint32_t litLenOf(const Shared &sh, uint32_t s) {
  if (sh.btype == 1) return s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u;
  return s < sh.hlit ? sh.lens[s] : 0u;
}
GWA_HD uint32_t distLenOf(const Shared &sh, uint32_t s) {
  if (sh.btype == 1) return 5;
  return s < sh.hdist ? sh.lens[sh.hlit + s < 320 ? sh.hlit + s : 319] : 0u;
}

// every lane, for symbol s of an alphabet of nSym symbols with lengths lenOf(j): its canonical code and
// its place in canonical order, then its entries of the lookup table
#define INF_FILL(sh, s, nSym, LENOF, tab, symArr)                                     \
  {                                                                                   \
    const uint32_t L_ = LENOF(sh, s);                                                 \
    if (L_) {                                                                         \
      uint32_t code_ = 0, rank_ = 0;                                                  \
      for (uint32_t j_ = 0; j_ < (nSym); ++j_) {                                      \
        const uint32_t l_ = LENOF(sh, j_);                                            \
        if (l_ && l_ < L_) {                                                          \
          code_ += 1u << (L_ - l_);                                                   \
          ++rank_;                                                                    \
        } else if (l_ == L_ && j_ < (s)) {                                            \
          ++code_;                                                                    \
          ++rank_;                                                                    \
        }                                                                             \
      }                                                                               \
      if (rank_ < (nSym)) (symArr)[rank_] = (uint16_t)(s);                            \
      if (L_ <= kTabBits) {                                                           \
        const uint32_t rev_ = bgzf::bitrev(code_ & ((1u << L_) - 1), L_);             \
        for (uint32_t e_ = rev_; e_ < kTab; e_ += 1u << L_) (tab)[e_ & (kTab - 1)] = (uint16_t)((s) << 4 | L_); \
      }                                                                               \
    }                                                                                 \
  }

// whether a code set is usable (zlib's rule): complete, or a single code of one bit, or no code at all
GWA_HD bool codeSetOk(uint32_t kraft, uint32_t used) {
  return kraft == (1u << 15) || (used == 1 && kraft == (1u << 14)) || used == 0;
}

// ---- wave 0: a block's header ------------------------------------------------------------------------
// Reads BFINAL and BTYPE; a stored block is copied here; a dynamic block's code lengths go into sh.lens.
GWA_HD void blockHeader(Shared &sh, BitReader &br, uint32_t isize, uint32_t wlane) {
  if (sh.status) return;
  br.seek(sh.bitPos, wlane);
  br.need32(wlane);
  const uint32_t bfinal = br.bits(1), btype = br.bits(2);
  uint32_t err = 0, op = sh.op, hlit = 0, hdist = 0;
  if (br.overrun()) err = kErrTruncated;
  else if (btype == 3) err = kErrBlockType;
  else if (btype == 0) {
    br.drop(br.cnt & 7);  // (cnt and the position are congruent mod 8: words are 32 bits)
    br.need32(wlane);
    const uint32_t len = br.bits(16), nlen = br.bits(16);
    const uint32_t clen = br.payEnd - br.pay, at = br.pos() >> 3;
    if (br.overrun()) err = kErrTruncated;
    else if (len != (nlen ^ 0xffffu)) err = kErrStoredLen;
    else if (len > clen - at) err = kErrTruncated;
    else if (len > isize - op) err = kErrLength;
    else {
      uint8_t *ob = reinterpret_cast<uint8_t *>(sh.out);
      for (uint32_t i = wlane; i < len; i += kWaveStep) ob[op + i] = br.in[br.pay + at + i];
      op += len;
      INF_WAVE_SYNC()
      br.seek(br.pos() + len * 8, wlane);
    }
  } else if (btype == 2) {
    hlit = br.bits(5) + 257;
    hdist = br.bits(5) + 1;
    const uint32_t hclen = br.bits(4) + 4;
    if (br.overrun()) err = kErrTruncated;
    else if (hlit > 286 || hdist > 30) err = kErrCounts;
    else {
      // the code-length code: lane 0 stores its lengths, then every lane its own symbol's table entries
      INF_WAVE_SYNC()
      if (wlane == 0)
        for (uint32_t i = 0; i < 20; ++i) sh.clLen[i] = 0;
      INF_WAVE_SYNC()
      for (uint32_t i = 0; i < hclen; ++i) {
        br.need32(wlane);
        const uint32_t v = br.bits(3);
        // the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
        const uint32_t sym = i < 3 ? 16 + i : i == 3 ? 0u : (i & 1) ? 8u - ((i - 3) >> 1) : 8u + ((i - 4) >> 1);
        if (wlane == 0) sh.clLen[sym < 19 ? sym : 19] = (uint8_t)v;
      }
      INF_WAVE_SYNC()
      uint32_t kraft = 0, used = 0;
      for (uint32_t j = 0; j < 19; ++j) {
        const uint32_t l = sh.clLen[j];
        if (l) {
          kraft += 1u << (7 - l);
          ++used;
        }
      }
      if (br.overrun()) err = kErrTruncated;
      else if (kraft > 128 || (used && kraft < 128)) err = kErrClCode;
      else {
        for (uint32_t e = wlane; e < 128; e += kWaveStep) sh.clTab[e] = 0;
        INF_WAVE_SYNC()
        for (uint32_t s = wlane; s < 19; s += kWaveStep) {
          const uint32_t L = sh.clLen[s];
          if (L) {
            uint32_t code = 0;
            for (uint32_t j = 0; j < 19; ++j) {
              const uint32_t l = sh.clLen[j];
              if (l && l < L) code += 1u << (L - l);
              else if (l == L && j < s) ++code;
            }
            const uint32_t rev = bgzf::bitrev(code & ((1u << L) - 1), L);
            for (uint32_t e = rev; e < 128; e += 1u << L) sh.clTab[e & 127] = (uint16_t)(s << 4 | L);
          }
        }
        INF_WAVE_SYNC()
        // the HLIT + HDIST code lengths
        const uint32_t n = hlit + hdist;
        uint32_t i = 0, prev = 0;
        while (i < n && !err) {  // (every turn takes at least one bit, or ends)
          br.need32(wlane);
          const uint32_t e = sh.clTab[br.peek(7)];
          const uint32_t sym = e >> 4;
          if (!e) {
            err = kErrBadCode;
            break;
          }
          br.drop(e & 15);
          uint32_t val = sym, rep = 1;
          if (sym == 16) {
            if (i == 0) err = kErrRepeat;
            val = prev;
            rep = 3 + br.bits(2);
          } else if (sym == 17) {
            val = 0;
            rep = 3 + br.bits(3);
          } else if (sym == 18) {
            val = 0;
            rep = 11 + br.bits(7);
          }
          if (br.overrun()) err = kErrTruncated;
          else if (!err && rep > n - i) err = kErrRepeat;
          if (err) break;
          if (wlane == 0)
            for (uint32_t r = 0; r < rep; ++r) sh.lens[(i + r) < 320 ? i + r : 319] = (uint8_t)val;
          i += rep;
          prev = val;
        }
        INF_WAVE_SYNC()
      }
    }
  }
  if (wlane == 0) {
    sh.btype = btype;
    sh.bfinal = bfinal;
    sh.hlit = hlit;
    sh.hdist = hdist;
    sh.op = op;
    sh.bitPos = br.pos();
    sh.litKraft = sh.distKraft = sh.litUsed = sh.distUsed = 0;
    for (uint32_t i = 0; i < 16; ++i) sh.litCount[i] = sh.distCount[i] = 0;
    if (err) sh.status = makeStatus(err, br.pos());
  }
}

// ---- wave 0: a Huffman block's symbols, up to its end-of-block ---------------------------------------
GWA_HD void blockSymbols(Shared &sh, BitReader &br, uint32_t isize, uint32_t wlane) {
  if (sh.status || sh.btype == 0) return;
  br.seek(sh.bitPos, wlane);
  uint8_t *ob = reinterpret_cast<uint8_t *>(sh.out);
  uint32_t op = sh.op, err = 0;
  for (;;) {  // (every turn takes at least one bit, or ends)
    br.need32(wlane);
    uint32_t e = sh.litTab[br.peek(kTabBits)];
    if (!e) e = slowDecode(sh.litCount, sh.litSym, 288, br.peek(15));
    if (!e) {
      err = kErrBadCode;
      break;
    }
    br.drop(e & 15);
    const uint32_t sym = e >> 4;
    if (sym < 256) {
      if (br.overrun()) {
        err = kErrTruncated;
        break;
      }
      if (op >= isize) {
        err = kErrLength;
        break;
      }
      if (wlane == 0) ob[op & (kMaxOut - 1)] = (uint8_t)sym;
      ++op;
      continue;
    }
    if (sym == 256) {
      if (br.overrun()) err = kErrTruncated;
      break;
    }
    if (sym > 285) {
      err = kErrBadCode;
      break;
    }
    const uint32_t s = sym - 257;
    uint32_t len;
    if (s < 8) len = 3 + s;
    else if (s == 28) len = 258;
    else {
      const uint32_t eb = (s >> 2) - 1;
      len = 3 + ((4 + (s & 3)) << eb) + br.bits(eb);
    }
    br.need32(wlane);
    uint32_t d = sh.distTab[br.peek(kTabBits)];
    if (!d) d = slowDecode(sh.distCount, sh.distSym, 32, br.peek(15));
    if (!d) {
      err = kErrBadCode;
      break;
    }
    br.drop(d & 15);
    const uint32_t ds = d >> 4;
    if (ds > 29) {
      err = kErrBadCode;
      break;
    }
    uint32_t dist = ds + 1;
    if (ds >= 4) {
      const uint32_t eb = (ds >> 1) - 1;
      dist = 1 + ((2 + (ds & 1)) << eb) + br.bits(eb);
    }
    if (br.overrun()) {
      err = kErrTruncated;
      break;
    }
    if (dist > op) {
      err = kErrDistance;
      break;
    }
    if (len > isize - op) {
      err = kErrLength;
      break;
    }
    // the copy, shared by the wave: sources lie before op, so no element waits for another
    INF_WAVE_SYNC()
    const uint32_t from = op - dist;
    if (dist >= len) {
      for (uint32_t i = wlane; i < len; i += kWaveStep) ob[(op + i) & (kMaxOut - 1)] = ob[(from + i) & (kMaxOut - 1)];
    } else {
      for (uint32_t i = wlane; i < len; i += kWaveStep) ob[(op + i) & (kMaxOut - 1)] = ob[(from + i % dist) & (kMaxOut - 1)];
    }
    INF_WAVE_SYNC()
    op += len;
  }
  if (wlane == 0) {
    sh.op = op;
    sh.bitPos = br.pos();
    if (err) sh.status = makeStatus(err, br.pos());
  }
}

// ---- one member --------------------------------------------------------------------------------------
// in: compressed bytes, readable over [0, nIn) (device: 16-byte aligned); the payload is in[pay, pay +
// clen).  On status 0 exactly isize bytes are stored at dst; otherwise nothing is.  *status is written by
// lane 0.  Uniform control flow: every lane of the workgroup calls it with the same arguments.
GWA_HD void inflateMember(Shared &sh, const uint8_t *in, uint32_t nIn, uint32_t pay, uint32_t clen, uint32_t isize,
                          uint32_t crc, uint8_t *dst, uint32_t *status) {
  const bool fits = pay <= nIn && clen <= nIn - pay;
  INF_LANES(
    if (lane == 0) {
      sh.status = !fits ? makeStatus(kErrTruncated, 0) : isize > kMaxOut ? makeStatus(kErrLength, 0) : 0u;
      sh.bitPos = 0;
      sh.op = 0;
      sh.bfinal = 0;
      sh.btype = 0;
      sh.hlit = sh.hdist = 0;
      sh.crc = 0;
    }
    uint32_t c = lane;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0xedb88320u : c >> 1;
    sh.crcTab[lane] = c;)
  BitReader br;
  br.sh = &sh;
  br.in = in;
  br.nIn = nIn;
  br.pay = fits ? pay : 0;
  br.payEnd = fits ? pay + clen : 0;
  // a block's header takes at least three bits, so the payload's bits bound the number of blocks
  const uint32_t maxBlocks = clen * 8 / 3 + 1;
  bool more = true;
  for (uint32_t b = 0; b < maxBlocks && more; ++b) {
    INF_WAVE0(br.winBase = ~0u; blockHeader(sh, br, isize, wlane);)
    // the lookup tables: zero them and sum up the code set, then every lane its own symbols
    INF_LANES(
      if (!sh.status && sh.btype) {
        for (uint32_t e = lane; e < kTab; e += kLanes) sh.litTab[e] = sh.distTab[e] = 0;
        for (uint32_t s = lane; s < 288; s += kLanes) {
          const uint32_t l = litLenOf(sh, s) & 15;
          if (l) {
            BGZF_ADD(&sh.litKraft, 1u << (15 - l));
            BGZF_ADD(&sh.litUsed, 1u);
            BGZF_ADD(&sh.litCount[l], 1u);
          }
        }
        if (lane < 32) {
          const uint32_t l = distLenOf(sh, lane) & 15;
          if (l) {
            BGZF_ADD(&sh.distKraft, 1u << (15 - l));
            BGZF_ADD(&sh.distUsed, 1u);
            BGZF_ADD(&sh.distCount[l], 1u);
          }
        }
      })
    bool ok = false;
    INF_LANES(
      ok = !sh.status && sh.btype;
      if (ok) {
        const bool eob = litLenOf(sh, 256) != 0;
        const bool sets = codeSetOk(sh.litKraft, sh.litUsed) && codeSetOk(sh.distKraft, sh.distUsed);
        ok = eob && sets;
        if (ok) {
          for (uint32_t s = lane; s < 288; s += kLanes) INF_FILL(sh, s, 288u, litLenOf, sh.litTab, sh.litSym)
          if (lane < 32) INF_FILL(sh, lane, 32u, distLenOf, sh.distTab, sh.distSym)
        }
      })
    INF_LANES(
      if (lane == 0 && !sh.status && sh.btype && !ok) {
        sh.status = makeStatus(litLenOf(sh, 256) ? kErrCodeSet : kErrNoEob, sh.bitPos);
      })
    INF_WAVE0(br.winBase = ~0u; blockSymbols(sh, br, isize, wlane);)
    INF_LANES(more = !sh.status && !sh.bfinal;)
  }
  // length and CRC32
  INF_LANES(
    if (lane == 0 && !sh.status) {
      if (!sh.bfinal) sh.status = makeStatus(kErrTruncated, sh.bitPos);
      else if (sh.op != isize) sh.status = makeStatus(kErrLength, sh.bitPos);
    })
  INF_LANES(
    const uint32_t b = lane * kSegCrc;
    if (!sh.status && (b < isize || lane == 0)) {
      const uint32_t e = b + kSegCrc < isize ? b + kSegCrc : isize;
      uint32_t c = lane == 0 ? 0xffffffffu : 0u;
      for (uint32_t p = b; p < e; ++p) c = sh.crcTab[(c ^ bgzf::byteAt(sh.out, p)) & 0xff] ^ (c >> 8);
      BGZF_XOR(&sh.crc, bgzf::crcMul(c, bgzf::crcXpow8(isize - e)));
    })
  INF_LANES(
    if (lane == 0 && !sh.status && (sh.crc ^ 0xffffffffu) != crc) sh.status = makeStatus(kErrCrc, sh.bitPos);)
  // the slice to its place: bytes up to the first 16-byte boundary of dst, aligned 16-byte stores whose
  // source words are funnel-shifted out of LDS, then the bytes left
  INF_LANES(
    if (lane == 0) *status = sh.status;
    if (!sh.status) {
      const uint8_t *ob = reinterpret_cast<const uint8_t *>(sh.out);
#if defined(__HIP_DEVICE_COMPILE__)
      const uint32_t head = (uint32_t)((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15);
      const uint32_t h = head < isize ? head : isize;
      if (lane < h) dst[lane] = ob[lane];
      const uint32_t chunks = (isize - h) / 16;
      const uint32_t s8 = 8 * (h & 3);
      for (uint32_t c = lane; c < chunks; c += kLanes) {
        const uint32_t w0 = (h + 16 * c) >> 2;  // (w0 + 4 <= 16384 + 3: inside sh.out's room)
        uint32_t v[5];
        for (uint32_t k = 0; k < 5; ++k) v[k] = sh.out[w0 + k];
        uint4 o;
        o.x = s8 ? (v[0] >> s8) | (v[1] << (32 - s8)) : v[0];
        o.y = s8 ? (v[1] >> s8) | (v[2] << (32 - s8)) : v[1];
        o.z = s8 ? (v[2] >> s8) | (v[3] << (32 - s8)) : v[2];
        o.w = s8 ? (v[3] >> s8) | (v[4] << (32 - s8)) : v[3];
        *reinterpret_cast<uint4 *>(dst + h + 16 * c) = o;
      }
      const uint32_t done = h + 16 * chunks;
      if (lane < isize - done) dst[done + lane] = ob[done + lane];
#else
      for (uint32_t p = lane; p < isize; p += kLanes) dst[p] = ob[p];
#endif
    })
}

}  // namespace inflate
}  // namespace gwa
