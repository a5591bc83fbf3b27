// The regrouping rule of one-pass device bundles, defined once: the device step
// (csrc/hip/regroup.hip) and its host model (csrc/host/regroup.cpp) follow it step by
// step and give the same parents, extension lists and permutation.
//
// A candidate's count is the popcount of the AND of its k item rows, in any order: any
// (k-1)-subset may be the shared part of a piece and the remaining item its extension.
// The generator groups candidates under their lexicographic prefix; the deep levels of
// a run come from a few large patterns, whose prefix groups hold 1-2 candidates while
// the same candidates share other parents 6-8 ways.  The rule, per level (levels are
// independent), over the level's parent rows P [n][m] (sorted) and candidates (x, y):
//
//   par[c][j]   the row of P equal to candidate c without its j-th item (binary
//               search; -1: not a row of P).  par[c][m] is the prefix row itself.
//   rounds      for thr in 8, 6, 4, 3, 2, 1 (rg_thr), repeated while a round assigns anything:
//                 u[p]   = unassigned candidates with p among their parents
//                 every unassigned c votes for the parent with the largest u[p] >= thr
//                          (ties: the largest j, i.e. towards the prefix)
//                 a parent with >= thr votes takes all its voters
//               (at thr = 1 the prefix always qualifies: every candidate ends assigned)
//   fallback    a level whose regrouped piece count sum(ceil(children / 8)) is not below
//               the prefix plan's keeps the prefix plan (at one m per level the cost
//               pieces * (m + constant) compares as the piece counts do), and so does a
//               level of more than kRgMaxRows parent rows
//   numbering   parents in row order, a parent's children in candidate order:
//               new index = off'[p] + rank, perm[new] = old
//
// Every step is a sum or a maximum over a set: the result does not depend on the order
// in which threads run, and is the same on every rank.
#pragma once
#include <stdint.h>

namespace fa {

// the rounds' thresholds, in order (a function: host and device code both call it)
constexpr int kRgNThr = 6;
constexpr int rg_thr(int t) { return t == 0 ? 8 : t == 1 ? 6 : t == 2 ? 4 : t == 3 ? 3 : t == 4 ? 2 : 1; }
// parent rows of a level the device step regroups (its three counters per row are always in LDS)
constexpr int kRgMaxRows = 12288;

// LDS of the device step's rounds kernel (regroup.hip k_dl_rg_rounds), one workgroup per level:
//   counters   u, u2, v: 16 bits per parent row each, two rows to a word (a parent has at most
//              F1 - m <= kAgMaxF1 - 1 = 32,767 children, so a half never carries into the next)
//   lists      the level's parent lists, uint16 [m + 1][C] (0xFFFF: not a row), and the
//              unassigned candidates' indices, uint16 [C]
// The counters always fit (kRgMaxRows).  The lists are in LDS when rg_lds_fits says so, else
// the kernel reads them from its global scratch; the launcher sizes the launch and the
// kernel picks its path by these same functions.
constexpr int64_t kRgLdsMax = 160 * 1024 - 512;          // (minus the kernel's static scratch)
constexpr int64_t rg_al16(int64_t b) { return (b + 15) & ~(int64_t)15; }
constexpr int64_t rg_lds_counters(int64_t n) { return rg_al16(3 * 4 * ((n + 1) / 2)); }
constexpr int64_t rg_lds_par(int64_t C, int64_t m) { return rg_al16(2 * C * (m + 1)); }
constexpr int64_t rg_lds_all(int64_t n, int64_t C, int64_t m) {
  return rg_lds_counters(n) + rg_lds_par(C, m) + rg_al16(2 * C);
}
// cap: the LDS bytes the step may use (at most kRgLdsMax)
constexpr bool rg_lds_fits(int64_t n, int64_t C, int64_t m, int64_t cap) {
  return C < 0xFFFF && rg_lds_all(n, C, m) <= cap;
}
constexpr int64_t rg_lds_bytes(int64_t n, int64_t C, int64_t m, int64_t cap) {
  return rg_lds_fits(n, C, m, cap) ? rg_lds_all(n, C, m) : rg_lds_counters(n);
}
static_assert(rg_lds_counters(kRgMaxRows) <= kRgLdsMax, "the counters of any level fit");
// The statistics of the bundle the post step last regrouped, in the control block (fa_dl.h:
// slots free between kDlPiecesI32 and kDlBits): kRgStats + 4 l .. + 3 are level l's prefix
// pieces, the rule's pieces, rounds, 1 = the level kept the prefix plan.
constexpr int kRgStats = 224;
static_assert(kRgStats + 4 * 32 <= 512, "the statistics end before the control block's bitset");

// compare the m-row a with the (m + 1)-row s without position p (fa_hip.h cmp_skip)
inline int rg_cmp_skip(const int32_t* a, const int32_t* s, int k, int p) {
  for (int i = 0, j = 0; i < k - 1; ++i, ++j) {
    if (j == p) ++j;
    const int32_t x = a[i], y = s[j];
    if (x != y) return x < y ? -1 : 1;
  }
  return 0;
}

}  // namespace fa
