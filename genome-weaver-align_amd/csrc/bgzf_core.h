// bgzf_core.h -- BGZF (SAM specification §4.1) encoder, one 65 280-byte slice of text per block.
//
// One header for the device and the host.  On the device a workgroup of kLanes threads compresses one
// slice out of LDS (bgzf.hip); the host build replays the same lanes phase by phase -- a loop over the
// lanes wherever the device has a barrier -- so both give the same bytes (tests/bgzf_host.cpp runs the
// replay under sanitizers, gwa_bgzf_compress(device < 0) uses it for the SAM header).  Everything a
// lane carries from one phase to the next lives in Shared; a phase touches shared words other lanes
// touch only through commutative atomics (add, or, xor, max), so no result depends on lane order.
//
// Block contract (include/gwa.h): 18 header bytes, one final deflate block with dynamic Huffman codes
// (or a stored block when that would exceed slice + 5 bytes), CRC32 and ISIZE.
//
// Phases of compressSlice:
//   stage     the slice into Shared::text (16-B loads)
//   strips    kLanes positions at a time: every lane looks up the candidate an EARLIER strip left in
//             the hash table for its 4 bytes and the distance-1 candidate, measures both with 4-byte
//             XOR compares, then the strip's positions go into the table (atomicMax: the highest
//             position wins a collision); greedy selection is the orbit of next(p) = p + max(1, len)
//             from where the previous strip's last token ended, found by pointer jumping (10 rounds);
//             chosen tokens go into the start / match bitmaps, the compact match list and the histograms
//   codes     CRC32 of 64-byte segments per lane, combined with x^(8 * bytes behind) mod P; two lanes
//             build the literal/length and distance Huffman trees (leaves rank-sorted by all lanes,
//             two-queue merge, lengths limited by moving Kraft units), then the 19-symbol code-length
//             code (limit 7); canonical codes assigned by all lanes
//   emit      token bit lengths per 64-position segment, an exclusive scan, then every lane packs its
//             tokens into 64-bit words of the zeroed output slot (OR for the shared edge words)
#pragma once
#include "gwa_layout.h"

namespace gwa {
namespace bgzf {

constexpr uint32_t kSlice = 0xff00;          // text bytes per block (htslib's choice)
constexpr uint32_t kLanes = 1024;            // lanes of a workgroup = positions of a strip
constexpr uint32_t kSeg = 64;                // positions per lane in the CRC and emission phases
constexpr uint32_t kHashBits = 13;
constexpr uint32_t kMaxMatches = 8192;       // compact match list; later matches go out as literals
constexpr uint32_t kMinMatch = 4;
constexpr uint32_t kMaxMatch = 258;
constexpr uint32_t kMaxDist = 32768;
constexpr uint32_t kSlotBytes = 65312;       // per-block output slot: slice + 31, rounded up to 8
constexpr uint32_t kMaxBlock = kSlice + 31;  // header 18 + stored payload (slice + 5) + trailer 8
constexpr uint32_t kRounds = 10;             // pointer-jumping rounds: 2^10 = kLanes
static_assert(kLanes * kSeg >= kSlice, "segments cover the slice");
static_assert((1u << kRounds) >= kLanes, "rounds cover a strip");

#if defined(__HIP_DEVICE_COMPILE__)
#define BGZF_LANES(...)                \
  {                                    \
    const uint32_t lane = threadIdx.x; \
    __VA_ARGS__                        \
  }                                    \
  __syncthreads();
#define BGZF_ADD(p, v) atomicAdd((p), (v))
#define BGZF_OR(p, v) atomicOr((p), (v))
#define BGZF_XOR(p, v) atomicXor((p), (v))
#define BGZF_MAX(p, v) atomicMax((p), (v))
#define BGZF_PEEK(p) atomicOr((p), 0u)
#define BGZF_OR64(p, v) atomicOr((unsigned long long *)(p), (unsigned long long)(v))
#else
#define BGZF_LANES(...) \
  for (uint32_t lane = 0; lane < kLanes; ++lane) { __VA_ARGS__ }
#define BGZF_ADD(p, v) (*(p) += (v))
#define BGZF_OR(p, v) (*(p) |= (v))
#define BGZF_XOR(p, v) (*(p) ^= (v))
#define BGZF_MAX(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#define BGZF_PEEK(p) (*(p))
#define BGZF_OR64(p, v) (*(p) |= (v))
#endif

// one Huffman tree under construction (a lane's serial work; leaves in ascending frequency order)
struct HuffWs {
  uint16_t order[288];  // symbols with a nonzero count, ascending by (count, symbol)
  uint32_t nodeF[288];  // internal nodes in creation order
  uint16_t parL[288], parN[288];
  uint16_t dep[288];
  uint32_t bl[17];        // codes per length
  uint32_t nextCode[17];  // first canonical code per length
  uint32_t nUsed;
};

struct Shared {
  uint32_t text[16384];        // the slice, zero padded
  uint32_t list[kMaxMatches];  // chosen matches in position order: (len - 3) | (dist - 1) << 8
  uint32_t startBits[2048];    // bit p: a token starts at p
  uint32_t matchBits[2048];    // bit p: that token is list[rank of p]
  union {
    uint32_t hash[1u << kHashBits];  // strips: 1 + the highest position with this hash in earlier strips
    struct {                         // after the strips
      uint32_t scan[kLanes + 32], scanTot[32];
      uint32_t matchBase[kLanes];
      uint32_t crcTab[256];
      HuffWs lit, dist, cl;
      uint16_t litCode[288], distCode[32], clCode[19];
      uint8_t litLen[288], distLen[32], clLen[19];
      uint8_t seq[320];  // the code lengths as the header sends them
    } c;
  } u;
  uint32_t cand[kLanes];  // strip: len | dist << 16 of the lane's match (0: none)
  uint16_t jump[2][kLanes];
  uint32_t reach[32], sel[32], wpre[33];
  uint32_t litHist[288], distHist[32], clHist[19];
  uint32_t hdrOff[kLanes];  // bit offset of the lane's code length in the block header
  uint32_t n, carry, nMatches, stripMatches;
  uint32_t crc, hlit, hdist, hclen, nSeq, hdrBits, tokBits, payloadBytes, stored;
};

GWA_HD uint32_t load4(const uint32_t *text, uint32_t p) {
  const uint32_t w = p >> 2;
  const uint64_t v = (uint64_t)text[w] | (uint64_t)text[w + 1] << 32;
  return (uint32_t)(v >> (8 * (p & 3)));
}
// the 16 bytes in[at, at + 16) as four little-endian words, bytes from n on read as zero
GWA_HD void loadChunk(const uint8_t *in, uint32_t at, uint32_t n, uint32_t *w) {
  w[0] = w[1] = w[2] = w[3] = 0;
  if (at + 16 <= n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 v = *reinterpret_cast<const uint4 *>(in + at);
    w[0] = v.x;
    w[1] = v.y;
    w[2] = v.z;
    w[3] = v.w;
#else
    for (uint32_t k = 0; k < 16; ++k) w[k >> 2] |= (uint32_t)in[at + k] << (8 * (k & 3));
#endif
  } else {
    for (uint32_t k = 0; at + k < n; ++k) w[k >> 2] |= (uint32_t)in[at + k] << (8 * (k & 3));
  }
}
GWA_HD uint32_t byteAt(const uint32_t *text, uint32_t p) { return (text[p >> 2] >> (8 * (p & 3))) & 0xff; }
GWA_HD uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - kHashBits); }

// length of the common prefix of text[q..] and text[p..], q < p, at most maxLen
GWA_HD uint32_t matchLen(const uint32_t *text, uint32_t q, uint32_t p, uint32_t maxLen) {
  uint32_t k = 0;
  while (k < maxLen) {
    const uint32_t x = load4(text, q + k) ^ load4(text, p + k);
    if (x) {
      k += (uint32_t)__builtin_ctz(x) >> 3;
      break;
    }
    k += 4;
  }
  return k < maxLen ? k : maxLen;
}

// whether a match pays for its length and distance codes: about 12 bits + the distance's extra bits (up
// to 13) against the literals it replaces, which in SAM text are often the 2-bit bases of SEQ
GWA_HD bool worth(uint32_t len, uint32_t dist) {
  if (len < kMinMatch) return false;
  if (dist == 1) return true;
  return len >= 6 + (dist > 2048 ? 2u : 0u) + (dist > 16384 ? 2u : 0u);
}

struct LenCode {
  uint32_t sym, eb, ev;
};
GWA_HD LenCode lenCode(uint32_t len) {  // 3..258
  const uint32_t l = len - 3;
  if (l < 8) return {257 + l, 0, 0};
  if (len == 258) return {285, 0, 0};
  const uint32_t hb = 31 - (uint32_t)__builtin_clz(l), eb = hb - 2;
  return {257 + 4 * (eb + 1) + ((l >> eb) & 3), eb, l & ((1u << eb) - 1)};
}
GWA_HD LenCode distCode(uint32_t dist) {  // 1..32768
  const uint32_t d = dist - 1;
  if (d < 4) return {d, 0, 0};
  const uint32_t hb = 31 - (uint32_t)__builtin_clz(d), eb = hb - 1;
  return {2 * hb + ((d >> eb) & 1), eb, d & ((1u << eb) - 1)};
}

// CRC-32 (reflected 0xedb88320): the product of two polynomials mod P, and x^(8 * len) mod P
GWA_HD uint32_t crcMul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 0x80000000u; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1) ? (b >> 1) ^ 0xedb88320u : b >> 1;
  }
  return p;
}
GWA_HD uint32_t crcXpow8(uint32_t len) {
  uint32_t r = 0x80000000u, sq = 0x00800000u;  // x^0, x^8
  for (; len; len >>= 1) {
    if (len & 1) r = crcMul(r, sq);
    sq = crcMul(sq, sq);
  }
  return r;
}

GWA_HD uint32_t bitrev(uint32_t v, uint32_t n) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < n; ++i) r |= ((v >> i) & 1) << (n - 1 - i);
  return r;
}

// the output slot as a bit string (zeroed before): bits go in with OR, so lanes may share words
struct BitWriter {
  uint64_t *slot;
  uint64_t word;  // index of the word being filled
  uint64_t acc;
  uint32_t fill;  // bits of acc in use
  bool edge;      // the word being filled may be shared with the lane before
  GWA_HD void start(uint64_t *s, uint64_t bitPos) {
    slot = s;
    word = bitPos >> 6;
    fill = (uint32_t)(bitPos & 63);
    acc = 0;
    edge = true;
  }
  GWA_HD void put(uint64_t v, uint32_t nb) {  // nb <= 57, v < 2^nb
    if (!nb) return;
    acc |= v << fill;
    if (fill + nb >= 64) {
#if defined(__HIP_DEVICE_COMPILE__)
      if (edge) BGZF_OR64(slot + word, acc);
      else slot[word] = acc;
#else
      BGZF_OR64(slot + word, acc);
#endif
      edge = false;
      ++word;
      acc = fill ? v >> (64 - fill) : 0;
      fill = fill + nb - 64;
    } else {
      fill += nb;
    }
  }
  GWA_HD void finish() {
    if (acc) BGZF_OR64(slot + word, acc);
  }
};

GWA_HD uint32_t sidx(uint32_t i) { return i + (i >> 5); }  // (scan array: 32 consecutive entries per lane, padded)

// ---- Huffman ---------------------------------------------------------------------------------------

// every lane: the rank of symbol `lane` among the used symbols
GWA_HD void huffRank(HuffWs &w, const uint32_t *freq, uint32_t nsym, uint32_t lane) {
  if (lane >= nsym || !freq[lane]) return;
  const uint32_t f = freq[lane];
  uint32_t r = 0;
  for (uint32_t j = 0; j < nsym; ++j) {
    const uint32_t g = freq[j];
    r += (g && (g < f || (g == f && j < lane))) ? 1u : 0u;
  }
  w.order[r] = (uint16_t)lane;
}

// one lane: code lengths of the used symbols (lens zeroed by the caller), at most maxBits
GWA_HD void huffLengths(HuffWs &w, const uint32_t *freq, uint32_t nsym, uint32_t maxBits, uint8_t *lens, bool twoCodes) {
  uint32_t nUsed = 0;
  for (uint32_t i = 0; i < nsym; ++i) nUsed += freq[i] ? 1u : 0u;
  w.nUsed = nUsed;
  for (uint32_t i = 0; i <= 16; ++i) w.bl[i] = 0;
  if (nUsed == 0) return;
  if (nUsed == 1) {
    lens[w.order[0]] = 1;
    w.bl[1] = 1;
    if (twoCodes) {  // (a code-length code must be complete: a second code of one bit)
      lens[w.order[0] ? 0 : 1] = 1;
      w.bl[1] = 2;
    }
  } else {
    uint32_t li = 0, ni = 0;
    for (uint32_t nn = 0; nn + 1 < nUsed; ++nn) {
      uint32_t f = 0;
      for (int k = 0; k < 2; ++k) {
        if (li < nUsed && (ni >= nn || freq[w.order[li]] <= w.nodeF[ni])) {
          f += freq[w.order[li]];
          w.parL[li++] = (uint16_t)nn;
        } else {
          f += w.nodeF[ni];
          w.parN[ni++] = (uint16_t)nn;
        }
      }
      w.nodeF[nn] = f;
    }
    w.dep[nUsed - 2] = 0;
    for (uint32_t k = nUsed - 2; k-- > 0;) w.dep[k] = (uint16_t)(w.dep[w.parN[k]] + 1);
    for (uint32_t i = 0; i < nUsed; ++i) {
      uint32_t d = w.dep[w.parL[i]] + 1u;
      w.bl[d > maxBits ? maxBits : d]++;
    }
    // length limit: the codes clipped to maxBits overfill the code space; take one unit out at a time
    // (one code less at maxBits, one code of the longest shorter length moved down beside a new sibling)
    uint32_t total = 0;
    for (uint32_t i = 1; i <= maxBits; ++i) total += w.bl[i] << (maxBits - i);
    while (total > (1u << maxBits)) {
      w.bl[maxBits]--;
      for (uint32_t i = maxBits - 1; i >= 1; --i)
        if (w.bl[i]) {
          w.bl[i]--;
          w.bl[i + 1] += 2;
          break;
        }
      --total;
    }
    uint32_t idx = 0;  // the least frequent symbols get the longest codes
    for (uint32_t len = maxBits; len >= 1; --len)
      for (uint32_t c = 0; c < w.bl[len]; ++c) lens[w.order[idx++]] = (uint8_t)len;
  }
  uint32_t code = 0;
  w.nextCode[0] = 0;
  for (uint32_t len = 1; len <= 16; ++len) {
    code = (code + w.bl[len - 1]) << 1;
    w.nextCode[len] = code;
  }
}

// every lane: the canonical code of symbol `lane`, bit-reversed (deflate sends codes from the top bit)
GWA_HD void huffCode(const HuffWs &w, const uint8_t *lens, uint32_t nsym, uint16_t *codes, uint32_t lane) {
  if (lane >= nsym) return;
  const uint32_t len = lens[lane];
  if (!len) {
    codes[lane] = 0;
    return;
  }
  uint32_t k = 0;
  for (uint32_t j = 0; j < lane; ++j) k += lens[j] == len ? 1u : 0u;
  codes[lane] = (uint16_t)bitrev(w.nextCode[len] + k, len);
}

// ---- scan ------------------------------------------------------------------------------------------
// exclusive scan of sh.u.c.scan[sidx(0 .. kLanes - 1)] in two levels (32 lanes scan 32 entries each, lane 0
// scans their sums): afterwards lane t's offset is scanAt(sh, t) and sh.totalField holds the total
#define BGZF_SCAN(sh, totalField)                            \
  BGZF_LANES(if (lane < 32) {                                \
    uint32_t s_ = 0;                                         \
    for (uint32_t i_ = 0; i_ < 32; ++i_) {                   \
      const uint32_t at_ = sidx(lane * 32 + i_);             \
      const uint32_t v_ = (sh).u.c.scan[at_];                \
      (sh).u.c.scan[at_] = s_;                               \
      s_ += v_;                                              \
    }                                                        \
    (sh).u.c.scanTot[lane] = s_;                             \
  })                                                         \
  BGZF_LANES(if (lane == 0) {                                \
    uint32_t s_ = 0;                                         \
    for (uint32_t c_ = 0; c_ < 32; ++c_) {                   \
      const uint32_t v_ = (sh).u.c.scanTot[c_];              \
      (sh).u.c.scanTot[c_] = s_;                             \
      s_ += v_;                                              \
    }                                                        \
    (sh).totalField = s_;                                    \
  })
GWA_HD uint32_t scanAt(const Shared &sh, uint32_t t) { return sh.u.c.scan[sidx(t)] + sh.u.c.scanTot[t >> 5]; }

// bits of the token that starts at p (mi: its index in the match list when it is a match)
GWA_HD uint32_t tokenBits(const Shared &sh, uint32_t p, bool isMatch, uint32_t mi) {
  if (!isMatch) return sh.u.c.litLen[byteAt(sh.text, p)];
  const uint32_t e = sh.list[mi];
  const LenCode lc = lenCode((e & 0xff) + 3), dc = distCode((e >> 8) + 1);
  return sh.u.c.litLen[lc.sym] + lc.eb + sh.u.c.distLen[dc.sym] + dc.eb;
}

// ---- one slice -------------------------------------------------------------------------------------
// in: the slice (device: 16-byte aligned; nothing past in + n is read); slot: kSlotBytes of zeroed,
// 8-byte aligned output.  Returns the block's size through *size (lane 0 writes it) and adds
// to *storedCount when the block is a stored one.  Uniform control flow: every lane of the workgroup
// calls it with the same arguments.
GWA_HD void compressSlice(Shared &sh, const uint8_t *in, uint32_t n, uint64_t *slot, uint32_t *size, uint32_t *storedCount) {
  // stage + zero
  BGZF_LANES(
    for (uint32_t c = lane; c < 4096; c += kLanes) {  // 16-byte chunks
      uint32_t w[4];
      loadChunk(in, c * 16, n, w);
      for (uint32_t k = 0; k < 4; ++k) sh.text[c * 4 + k] = w[k];
    }
    for (uint32_t i = lane; i < 2048; i += kLanes) sh.startBits[i] = sh.matchBits[i] = 0;
    for (uint32_t i = lane; i < (1u << kHashBits); i += kLanes) sh.u.hash[i] = 0;
    if (lane < 288) sh.litHist[lane] = 0;
    if (lane < 32) sh.distHist[lane] = 0;
    if (lane < 19) sh.clHist[lane] = 0;
    if (lane == 0) {
      sh.n = n;
      sh.carry = 0;
      sh.nMatches = 0;
      sh.stripMatches = 0;
      sh.crc = 0;
      sh.stored = 0;
    })

  // ---- strips
  const uint32_t nStrips = (n + kLanes - 1) / kLanes;
  for (uint32_t s = 0; s < nStrips; ++s) {
    const uint32_t base = s * kLanes;
    // S1: candidates
    BGZF_LANES(
      const uint32_t p = base + lane;
      uint32_t best = 0, bestDist = 0;
      if (p + kMinMatch <= n) {
        const uint32_t maxLen = n - p < kMaxMatch ? n - p : kMaxMatch;
        const uint32_t c = sh.u.hash[hash4(load4(sh.text, p))];
        if (c && p - (c - 1) <= kMaxDist) {
          const uint32_t l = matchLen(sh.text, c - 1, p, maxLen);
          if (worth(l, p - (c - 1))) {
            best = l;
            bestDist = p - (c - 1);
          }
        }
        if (p >= 1) {
          const uint32_t l = matchLen(sh.text, p - 1, p, maxLen);
          if (worth(l, 1) && l + 1 >= best) {
            best = l;
            bestDist = 1;
          }
        }
      }
      sh.cand[lane] = best | bestDist << 16;
      const uint32_t nx = lane + (best ? best : 1u);
      sh.jump[0][lane] = (uint16_t)(nx < kLanes ? nx : kLanes);
      if (lane < 32) {
        const uint32_t rel = sh.carry - base;  // (carry >= base: the previous strip's last token ended there or later)
        sh.reach[lane] = (sh.carry >= base && (rel >> 5) == lane) ? 1u << (rel & 31) : 0u;
        sh.sel[lane] = 0;
      }
      if (lane == 0) {
        sh.nMatches += sh.stripMatches;
        sh.stripMatches = 0;
      })
    // S2: the strip's positions into the table
    BGZF_LANES(
      const uint32_t p = base + lane;
      if (p + kMinMatch <= n) BGZF_MAX(&sh.u.hash[hash4(load4(sh.text, p))], p + 1);)
    // S3: the orbit of next() from the carry, by pointer jumping
    for (uint32_t r = 0; r < kRounds; ++r) {
      const uint32_t cur = r & 1;
      BGZF_LANES(
        const uint32_t j = sh.jump[cur][lane];
        if (j < kLanes && ((BGZF_PEEK(&sh.reach[lane >> 5]) >> (lane & 31)) & 1)) BGZF_OR(&sh.reach[j >> 5], 1u << (j & 31));
        sh.jump[cur ^ 1][lane] = j < kLanes ? sh.jump[cur][j] : (uint16_t)kLanes;)
    }
    // S4: the chosen tokens
    BGZF_LANES(
      const uint32_t p = base + lane;
      const bool chosen = p < n && ((sh.reach[lane >> 5] >> (lane & 31)) & 1);
      const uint32_t cd = sh.cand[lane];
      if (chosen) {
        const uint32_t len = cd & 0xffff;
        if (len) BGZF_OR(&sh.sel[lane >> 5], 1u << (lane & 31));
        if (lane + (len ? len : 1u) >= kLanes) sh.carry = p + (len ? len : 1u);  // (the orbit's last element of the strip: one lane)
      }
      if (lane < 32 && base + lane * 32 < n) {
        uint32_t w = sh.reach[lane];
        const uint32_t left = n - (base + lane * 32);
        if (left < 32) w &= (1u << left) - 1;
        if (w) BGZF_OR(&sh.startBits[(base >> 5) + lane], w);
      })
    // S5: matches before each word of the strip
    BGZF_LANES(if (lane < 32) {
      uint32_t c = 0;
      for (uint32_t v = 0; v < lane; ++v) c += (uint32_t)__builtin_popcount(sh.sel[v]);
      sh.wpre[lane] = c;
      if (lane == 31) sh.stripMatches = c + (uint32_t)__builtin_popcount(sh.sel[31]);
    })
    // S6: list, bitmaps, histograms
    BGZF_LANES(
      const uint32_t p = base + lane;
      const bool chosen = p < n && ((sh.reach[lane >> 5] >> (lane & 31)) & 1);
      if (chosen) {
        const uint32_t cd = sh.cand[lane], len = cd & 0xffff, dist = cd >> 16;
        if (!len) {
          BGZF_ADD(&sh.litHist[byteAt(sh.text, p)], 1u);
        } else {
          const uint32_t rank = sh.nMatches + sh.wpre[lane >> 5] +
                                (uint32_t)__builtin_popcount(sh.sel[lane >> 5] & ((1u << (lane & 31)) - 1));
          if (rank < kMaxMatches) {
            sh.list[rank] = (len - 3) | (dist - 1) << 8;
            BGZF_OR(&sh.matchBits[p >> 5], 1u << (p & 31));
            BGZF_ADD(&sh.litHist[lenCode(len).sym], 1u);
            BGZF_ADD(&sh.distHist[distCode(dist).sym], 1u);
          } else {  // the list is full: the match's bytes go out as literals
            for (uint32_t k = 0; k < len; ++k) {
              BGZF_ADD(&sh.litHist[byteAt(sh.text, p + k)], 1u);
              if (k) BGZF_OR(&sh.startBits[(p + k) >> 5], 1u << ((p + k) & 31));
            }
          }
        }
      })
  }

  // ---- CRC32 and the code tables (the hash table's space is reused from here on)
  BGZF_LANES(
    if (lane < 256) {
      uint32_t c = lane;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0xedb88320u : c >> 1;
      sh.u.c.crcTab[lane] = c;
    }
    if (lane == 0) sh.litHist[256] = 1;  // end of block
    if (lane < 288) sh.u.c.litLen[lane] = 0;
    if (lane < 32) sh.u.c.distLen[lane] = 0;
    if (lane < 19) sh.u.c.clLen[lane] = 0;)
  BGZF_LANES(
    const uint32_t b = lane * kSeg;
    if (b < n) {
      const uint32_t e = b + kSeg < n ? b + kSeg : n;
      uint32_t c = lane == 0 ? 0xffffffffu : 0u;
      for (uint32_t p = b; p < e; ++p) c = sh.u.c.crcTab[(c ^ byteAt(sh.text, p)) & 0xff] ^ (c >> 8);
      BGZF_XOR(&sh.crc, crcMul(c, crcXpow8(n - e)));
    }
    huffRank(sh.u.c.lit, sh.litHist, 286, lane);
    huffRank(sh.u.c.dist, sh.distHist, 30, lane);)
  BGZF_LANES(
    if (lane == 0) huffLengths(sh.u.c.lit, sh.litHist, 286, 15, sh.u.c.litLen, false);
    if (lane == 64) huffLengths(sh.u.c.dist, sh.distHist, 30, 15, sh.u.c.distLen, false);)
  // the header's code-length sequence (every length sent, no run-length symbols) and its histogram
  BGZF_LANES(
    huffCode(sh.u.c.lit, sh.u.c.litLen, 286, sh.u.c.litCode, lane);
    huffCode(sh.u.c.dist, sh.u.c.distLen, 30, sh.u.c.distCode, lane);
    if (lane == 0) {
      uint32_t hl = 286, hd = 30;
      while (hl > 257 && !sh.u.c.litLen[hl - 1]) --hl;
      while (hd > 1 && !sh.u.c.distLen[hd - 1]) --hd;
      sh.hlit = hl;
      sh.hdist = hd;
      sh.nSeq = hl + hd;
    })
  BGZF_LANES(
    if (lane < sh.nSeq) {
      const uint32_t v = lane < sh.hlit ? sh.u.c.litLen[lane] : sh.u.c.distLen[lane - sh.hlit];
      sh.u.c.seq[lane] = (uint8_t)v;
      BGZF_ADD(&sh.clHist[v], 1u);
    })
  BGZF_LANES(huffRank(sh.u.c.cl, sh.clHist, 19, lane);)
  BGZF_LANES(
    if (lane == 0) {
      huffLengths(sh.u.c.cl, sh.clHist, 19, 7, sh.u.c.clLen, true);
      const uint8_t ord[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
      uint32_t hc = 19;
      while (hc > 4 && !sh.u.c.clLen[ord[hc - 1]]) --hc;
      sh.hclen = hc;
    })
  // bit offsets of the header's code lengths, then of every lane's tokens
  BGZF_LANES(
    huffCode(sh.u.c.cl, sh.u.c.clLen, 19, sh.u.c.clCode, lane);
    sh.u.c.scan[sidx(lane)] = lane < sh.nSeq ? sh.u.c.clLen[sh.u.c.seq[lane]] : 0u;)
  BGZF_SCAN(sh, hdrBits)
  BGZF_LANES(
    sh.hdrOff[lane] = scanAt(sh, lane);  // (a lane reads and rewrites its own scan entry only)
    sh.u.c.scan[sidx(lane)] = (uint32_t)__builtin_popcount(sh.matchBits[2 * lane]) + (uint32_t)__builtin_popcount(sh.matchBits[2 * lane + 1]);)
  BGZF_SCAN(sh, tokBits)
  BGZF_LANES(
    uint32_t bits = 0, mi = scanAt(sh, lane);
    sh.u.c.matchBase[lane] = mi;
    for (uint32_t h = 0; h < 2; ++h) {
      uint32_t w = sh.startBits[2 * lane + h];
      const uint32_t m = sh.matchBits[2 * lane + h];
      while (w) {
        const uint32_t b = (uint32_t)__builtin_ctz(w);
        w &= w - 1;
        const bool isM = (m >> b) & 1;
        bits += tokenBits(sh, lane * kSeg + h * 32 + b, isM, mi);
        mi += isM ? 1u : 0u;
      }
    }
    sh.u.c.scan[sidx(lane)] = bits;)
  BGZF_SCAN(sh, tokBits)
  BGZF_LANES(
    if (lane == 0) {
      const uint32_t hb = 3 + 5 + 5 + 4 + 3 * sh.hclen + sh.hdrBits;
      sh.hdrBits = hb;
      const uint32_t bitsAll = hb + sh.tokBits + sh.u.c.litLen[256];
      uint32_t bytes = (bitsAll + 7) >> 3;
      if (bytes > sh.n + 5) {
        sh.stored = 1;
        bytes = sh.n + 5;
      }
      sh.payloadBytes = bytes;
    })

  // ---- emission
  BGZF_LANES(
    const uint32_t nn = sh.n;
    const uint64_t pay = 18 * 8;  // the payload's first bit
    BitWriter bw;
    if (lane == 0) {  // gzip header with the BC extra field, then the trailer
      const uint32_t total = 18 + sh.payloadBytes + 8;
      bw.start(slot, 0);
      bw.put(0x04088b1fu, 32);
      bw.put(0, 32);
      bw.put(0x0006ff00u, 32);
      bw.put(0x00024342u, 32);
      bw.put(total - 1, 16);
      bw.finish();
      bw.start(slot, (uint64_t)(18 + sh.payloadBytes) * 8);
      bw.put(sh.crc ^ 0xffffffffu, 32);
      bw.put(nn, 32);
      bw.finish();
      *size = total;
      if (sh.stored) BGZF_ADD(storedCount, 1u);
    }
    if (sh.stored) {
      if (lane == 0) {
        bw.start(slot, pay);
        bw.put(1, 8);
        bw.put(nn, 16);
        bw.put(nn ^ 0xffffu, 16);
        bw.finish();
      }
      const uint32_t b = lane * kSeg;
      if (b < nn) {
        const uint32_t e = b + kSeg < nn ? b + kSeg : nn;
        bw.start(slot, pay + 40 + (uint64_t)b * 8);
        for (uint32_t p = b; p < e; ++p) bw.put(byteAt(sh.text, p), 8);
        bw.finish();
      }
    } else {
      if (lane == 0) {
        bw.start(slot, pay);
        bw.put(1 | 2 << 1, 3);
        bw.put(sh.hlit - 257, 5);
        bw.put(sh.hdist - 1, 5);
        bw.put(sh.hclen - 4, 4);
        const uint8_t ord[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        for (uint32_t i = 0; i < sh.hclen; ++i) bw.put(sh.u.c.clLen[ord[i]], 3);
        bw.finish();
        bw.start(slot, pay + sh.hdrBits + sh.tokBits);  // end of block
        bw.put(sh.u.c.litCode[256], sh.u.c.litLen[256]);
        bw.finish();
      }
      if (lane < sh.nSeq) {
        const uint32_t v = sh.u.c.seq[lane];
        bw.start(slot, pay + 17 + 3 * sh.hclen + sh.hdrOff[lane]);
        bw.put(sh.u.c.clCode[v], sh.u.c.clLen[v]);
        bw.finish();
      }
      uint32_t mi = sh.u.c.matchBase[lane];
      bw.start(slot, pay + sh.hdrBits + scanAt(sh, lane));
      for (uint32_t h = 0; h < 2; ++h) {
        uint32_t w = sh.startBits[2 * lane + h];
        const uint32_t m = sh.matchBits[2 * lane + h];
        while (w) {
          const uint32_t b = (uint32_t)__builtin_ctz(w);
          w &= w - 1;
          const uint32_t p = lane * kSeg + h * 32 + b;
          if ((m >> b) & 1) {
            const uint32_t e = sh.list[mi++];
            const LenCode lc = lenCode((e & 0xff) + 3), dc = distCode((e >> 8) + 1);
            bw.put((uint64_t)sh.u.c.litCode[lc.sym] | (uint64_t)lc.ev << sh.u.c.litLen[lc.sym], sh.u.c.litLen[lc.sym] + lc.eb);
            bw.put((uint64_t)sh.u.c.distCode[dc.sym] | (uint64_t)dc.ev << sh.u.c.distLen[dc.sym], sh.u.c.distLen[dc.sym] + dc.eb);
          } else {
            const uint32_t c = byteAt(sh.text, p);
            bw.put(sh.u.c.litCode[c], sh.u.c.litLen[c]);
          }
        }
      }
      bw.finish();
    })
}

static_assert(sizeof(Shared) <= 160 * 1024, "one workgroup's LDS");

// the 28-byte end-of-file marker of the specification (an empty block)
GWA_HD void eofMarker(uint8_t *out28) {
  const uint8_t m[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 28; ++i) out28[i] = m[i];
}

}  // namespace bgzf
}  // namespace gwa
