// rank_check.cpp -- TEST-ONLY: exhaustive check of the rank on the midpoint Occ blocks
// (OccBlock in gwa_layout.h; loadBlock / finishBlock / rankOne / rankAll / kmerInterval in
// bsf_core.h) against naive counts over the BWT, on the host build of the index (host_index.cpp).
//
// For each text, in the flagged and in the forced plain mode, on both strands:
//   - rankOne(c), c = 0..4, and rankAll at EVERY i in [0, N], against the prefix counts of
//     BWT[p] = T[(SA[p] - 1) mod N];
//   - BsfLane::occOne and rank2 at i = N + 1 (they clamp to N);
//   - the has-N bit: set exactly on the blocks whose N bitmap is not empty (flagged), never (plain);
//   - kmerInterval for every key of K = 3 against step-by-step backward search on the naive counts.
// Texts: the lengths around the half-block and block edges, each as random ACGT, all A, N as the
// last character, and scattered N with an N run; the program checks that their blocks include
// every kind: N only in half 0, only in half 1, in both, in neither.
// Prints "rank_check ok ..." and exits 0, or the first mismatches and exits 1.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "bsf_core.h"
#include "host_index.h"

using namespace gwa;

static int g_fail = 0;
static int g_kinds[2][4];  // [mode][nothing, half 0 only, half 1 only, both]
static uint64_t g_ranks = 0, g_kmers = 0;

#define FAIL(...)                                   \
  do {                                              \
    if (g_fail < 20) { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } \
    ++g_fail;                                       \
  } while (0)

static uint64_t g_rng = 0x2545F4914F6CDD1DULL;
static uint32_t rnd(uint32_t n) {
  g_rng = g_rng * 6364136223846793005ULL + 1442695040888963407ULL;
  return (uint32_t)((g_rng >> 33) % n);
}

static void checkStrand(const char *name, int mode, int fm, const HostIndex &h, const std::vector<uint8_t> &T) {
  const uint64_t n = h.N;
  const OccBlock *occ = h.occ[fm].data();
  if (h.occ[fm].size() != n / 128 + 1) FAIL("%s mode %d fm %d: %zu blocks", name, mode, fm, h.occ[fm].size());
  // naive[c][i] = # of c in bwt[0, i)
  std::vector<uint64_t> naive[5];
  for (int c = 0; c < 5; ++c) naive[c].assign(n + 1, 0);
  for (uint64_t p = 0; p < n; ++p) {
    const uint32_t s = h.sa[fm][p];
    const uint8_t ch = T[s == 0 ? n - 1 : s - 1];
    for (int c = 0; c < 5; ++c) naive[c][p + 1] = naive[c][p] + (ch == c ? 1 : 0);
  }
  for (uint64_t b = 0; b < h.occ[fm].size(); ++b) {
    const OccBlock &B = occ[b];
    const bool flag = (B.cnt[0] & kOccHasN) != 0, hasN = (B.nmask[0] | B.nmask[1]) != 0;
    if (flag != (mode == kOccFlagged && hasN)) FAIL("%s mode %d fm %d block %llu: has-N bit %d, N bitmap %d", name, mode, fm, (unsigned long long)b, flag, hasN);
    ++g_kinds[mode][(B.nmask[0] ? 1 : 0) | (B.nmask[1] ? 2 : 0)];
  }
  for (uint64_t i = 0; i <= n; ++i) {
    Block B;
    loadBlock(occ, i, mode, B);
    finishBlock(occ, i, mode, B);
    uint64_t all[5];
    rankAll(B, i, all);
    for (int c = 0; c < 5; ++c) {
      const uint64_t one = rankOne(B, i, c);
      if (one != naive[c][i] || all[c] != naive[c][i])
        FAIL("%s mode %d fm %d i %llu c %d: rankOne %llu rankAll %llu expect %llu", name, mode, fm, (unsigned long long)i, c,
             (unsigned long long)one, (unsigned long long)all[c], (unsigned long long)naive[c][i]);
      ++g_ranks;
    }
  }
  // the clamp of the lane's primitives: i = N + 1 answers as i = N
  {
    IndexView v{};
    v.occ[0] = h.occ[0].data(); v.occ[1] = h.occ[1].data();
    v.N = n;
    v.occMode = mode;
    for (int c = 0; c < 5; ++c) v.C[c] = h.C[c];
    SearchConfig cfg{};
    StairTables st{};
    LaneMem<4> L{};
    Caps caps{};
    BsfLane<4, 4> lane(v, cfg, st, L, caps);
    lane.blocks = 0;
    uint64_t lo[5], hi[5];
    lane.rank2(fm, n + 1, n + 1, lo, hi);
    for (int c = 0; c < 5; ++c) {
      const uint64_t one = lane.occOne(fm, c, n + 1);
      if (one != naive[c][n] || lo[c] != naive[c][n] || hi[c] != naive[c][n])
        FAIL("%s mode %d fm %d clamp c %d: occOne %llu rank2 %llu %llu expect %llu", name, mode, fm, c, (unsigned long long)one,
             (unsigned long long)lo[c], (unsigned long long)hi[c], (unsigned long long)naive[c][n]);
    }
    if (lane.blocks != 1 + 5) FAIL("%s mode %d fm %d: blocks %d after rank2 in one window + 5 occOne", name, mode, fm, lane.blocks);
  }
  // k-mer intervals
  const int K = 3;
  for (uint32_t key = 0; key < (1u << (2 * K)); ++key) {
    uint64_t lb = 0, ub = n, exp = 0;
    bool empty = false;
    for (int j = 0; j < K && !empty; ++j) {
      const int ch = (int)((key >> (2 * j)) & 3);
      const uint64_t nlb = h.C[ch] + naive[ch][lb], nub = h.C[ch] + naive[ch][ub];
      if (nlb >= nub) empty = true;
      lb = nlb;
      ub = nub;
    }
    if (!empty) exp = (ub << 32) | lb;
    const uint64_t got = kmerInterval(occ, h.C, n, key, K);
    if (got != exp) FAIL("%s mode %d fm %d key %u: kmerInterval %llx expect %llx", name, mode, fm, key, (unsigned long long)got, (unsigned long long)exp);
    ++g_kmers;
  }
}

static void checkText(const std::string &name, const std::vector<uint8_t> &T) {
  const uint64_t n = T.size();
  std::vector<uint8_t> R(T.rbegin(), T.rend());
  for (int mode = 0; mode < 2; ++mode) {
    HostIndex h;
    h.T = T;
    h.N = n;
    h.names.push_back("t");
    h.lengths.push_back((int64_t)n);
    h.offsets.push_back(0);
    h.occMode = mode;
    if (!cyclicSAHost(T.data(), n, h.sa[0]) || !cyclicSAHost(R.data(), n, h.sa[1])) {
      // a periodic text (all A): its rotations tie, any order of them is a sorted one
      for (int f = 0; f < 2; ++f) {
        h.sa[f].resize(n);
        for (uint64_t i = 0; i < n; ++i) h.sa[f][i] = (uint32_t)i;
      }
    }
    finishIndex(h);
    if (h.occMode != mode) FAIL("%s: finishIndex changed occMode %d to %d", name.c_str(), mode, h.occMode);
    checkStrand(name.c_str(), mode, 0, h, T);
    checkStrand(name.c_str(), mode, 1, h, R);
  }
}

int main() {
  const int lens[] = {1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 1000};
  int texts = 0;
  for (int n : lens) {
    std::vector<uint8_t> T((size_t)n);
    const std::string ln = std::to_string(n);
    for (auto &c : T) c = (uint8_t)rnd(4);
    checkText("acgt" + ln, T);
    std::vector<uint8_t> E = T;
    E[(size_t)n - 1] = 4;
    checkText("endN" + ln, E);
    checkText("allA" + ln, std::vector<uint8_t>((size_t)n, 0));
    texts += 3;
    // scattered single N (each puts one N somewhere in the BWT) and one N run (an N run at the BWT's end)
    for (int v = 0; v < 3 && n >= 63; ++v) {
      std::vector<uint8_t> S = T;
      const int singles = 1 + (int)rnd(3), run = 2 + (int)rnd(n >= 1000 ? 70 : 12);
      for (int j = 0; j < singles; ++j) S[rnd((uint32_t)n)] = 4;
      const int at = (int)rnd((uint32_t)(n - run));
      for (int j = 0; j < run; ++j) S[(size_t)(at + j)] = 4;
      checkText("runN" + ln + "_" + std::to_string(v), S);
      ++texts;
    }
  }
  for (int mode = 0; mode < 2; ++mode)
    for (int kind = 0; kind < 4; ++kind)
      if (g_kinds[mode][kind] == 0) FAIL("mode %d: no block with N-bitmap kind %d among the texts", mode, kind);
  if (g_kinds[0][0] <= g_kinds[0][1] + g_kinds[0][2] + g_kinds[0][3]) FAIL("most blocks should hold no N");
  if (g_fail) {
    fprintf(stderr, "rank_check: %d mismatches\n", g_fail);
    return 1;
  }
  printf("rank_check ok: %d texts x 2 modes x 2 strands, %llu ranks, %llu k-mers; blocks without N / N in half 0 / half 1 / both: %d %d %d %d\n",
         texts, (unsigned long long)g_ranks, (unsigned long long)g_kmers, g_kinds[0][0], g_kinds[0][1], g_kinds[0][2], g_kinds[0][3]);
  return 0;
}
