// The slab kernel's LDS capacity rule and the trimming estimate, defined once.
//
// k_count_slab_rec (csrc/hip/count.hip) keeps, per workgroup, a slab of sw bitmap
// words for each used item, one accumulator per candidate and (optionally) a copy
// of the rank -> slab-row map in LDS.  Every layer that bundles, plans or launches
// a level asks the same question -- which slab width holds the accumulators, and
// does the bundle fit one pass -- and answers it here: plan.cpp (host planner),
// gen.hip (host-loop chain, device chain, the bundle post step), count.hip (the
// launcher's footprint check) and, through libfa_host.so's fa_slab_* exports
// (plan.cpp), fastapriori_amd.ops.primitives.  The rows' layout inside the slab (where row
// u starts, which 16-B slot column it falls on) is defined here too, for the kernel's builds
// and reads and for the lane deal (levels.hip), and with it the tail rule that thins the
// rows' padding to keep a run's last bundle in one pass.
//
// Plain C++: no std::, no braced-list loops, so the same text compiles as host code
// (g++) and as __host__ __device__ code (hipcc).
//
// Width order 16, 32, 8, 4: measured per slab column on MI355X (T40I10D100M levels
// 7-10, k_count_slab_rec), 64-B rows read ~0.43x and 256-B rows ~0.55x as many
// columns per second as 128-B rows (the 256-B form holds 16 uint4 of prefix AND
// per thread: fewer waves, longer row scans per LDS bank).  (As the order stands the
// rule never returns 32: its capacity is below width 16's, which is asked first.)
//
// Known differences between the callers (kept as they are; `lds` below is always
// "the budget left for slab + accumulators", the caller decides what that is):
//   * plan.cpp subtracts slab_map_lds(F1) from the budget itself before it asks.
//   * The device loop (FastApriori device bundles, gen.hip fa_hip_dl_*, dl_post,
//     ops.primitives dl_plan / dl_count_multipass / dl_window_plan) passes
//     dl_lds_budget(F1) = TUNING.slab_lds_bytes - slab_map_lds(F1): map subtracted.
//   * The host loop (FastApriori._plan_bundle, _trim_worth_it, _trim, gen.hip
//     fa_hip_ag_chain / k_agd_setup) passes TUNING.slab_lds_bytes with NO map
//     subtraction: its bundling limit may exceed the planner's capacity by up to
//     16 KB of LDS (the planner then cuts the bundle into passes).
//   * Workgroup counts: the launcher charges slab_acc_words(n) accumulators and the
//     map (fa_hip_count_slab_rec_cls).  dl_post and dl_count do the same;
//     dl_count_multipass rounds but omits the map; count_level includes the map but
//     charges the unrounded accumulators (the same count whenever the budget is a
//     multiple of 32 B, as the default is).  (The launch's mode bits, and the rest of
//     what dl_post and dl_count share with the kernels -- control block, level
//     table, DlPost -- are fa_dl.h's; Python assembles the launch once, in
//     ops.primitives._slab_count, with each caller's charge.)
#pragma once
#include <math.h>
#include <stdint.h>

#include "fa_dl.h"

#if defined(__HIPCC__)
#define FA_SLAB_FN __host__ __device__ inline
#else
#define FA_SLAB_FN inline
#endif

namespace fa {

constexpr int kSlabBundleTarget = 8192;   // a width qualifies when it holds min(C, this) accumulators
constexpr int kSlabMinCap4 = 1024;        // ... or, at width 4, at least this many
constexpr int kSlabMapMaxF1 = 8192;       // largest F1 whose rank map is copied to LDS

// LDS bytes of one item's slab row: sw words + 2 of padding (an odd number of 16-B slots)
FA_SLAB_FN int64_t slab_row_bytes(int sw) { return (int64_t)(sw + 2) * 8; }

// LDS bytes of k_count_slab_rec's copy of the rank -> slab-row map (u16 per
// frequent item, rounded to 16 B); 0 = the map stays in global memory
FA_SLAB_FN int64_t slab_map_lds(int64_t F1) {
  return F1 <= kSlabMapMaxF1 ? ((F1 * 2 + 15) & ~(int64_t)15) : 0;
}

// ---- row layout, defined once -----------------------------------------------------------
// A row holds sw * 8 data bytes; one 16-B pad slot follows every 2^s rows (pad shift s,
// 0 .. kSlabPadMax).  s = 0 is the layout above: every row padded, stride (sw + 2) * 8, an
// odd number of 16-B slots, so rows start on all 16 slot columns of the 256-B bank row.
// s > 0 thins the padding: at sw = 16 row u starts on column (8u + (u >> s)) mod 16, which
// still reaches every column, for 16 / 2^s bytes of padding per row instead of 16.
// Every builder and reader of a slab (count.hip), the lane deal (levels.hip
// k_dl_lane_assign) and the CPU bank model (benchmarks/lds_bank_model.py, through the
// fa_slab_row_* exports) take a row's place from these two functions.
constexpr int kSlabPadMax = 3;

// byte offset of row u
FA_SLAB_FN int64_t slab_row_off(int sw, int s, int64_t u) { return u * sw * 8 + (u >> s) * 16; }
// 16-B slot column (0 .. 15) of row u's first slot in the 256-B bank row: (slab_row_off >> 4)
// mod 16 for the even widths the kernels have, in 32-bit arithmetic (the lane deal asks per
// record and read position)
FA_SLAB_FN int slab_row_col(int sw, int s, int u) {
  return (int)(((uint32_t)u * (uint32_t)(sw >> 1) + ((uint32_t)u >> s)) & 15u);
}
// bytes of n rows (the accumulators start here)
FA_SLAB_FN int64_t slab_rows_bytes(int sw, int s, int64_t n) {
  return n * sw * 8 + ((n + ((int64_t)1 << s) - 1) >> s) * 16;
}
// A layout in one int, for the arguments that used to carry the width alone (the count's
// launcher, the device plan's lane deal, fa_slab_workgroups): pad shift 0 is the bare width.
FA_SLAB_FN int slab_layout(int sw, int s) { return sw | (s << 8); }
FA_SLAB_FN int slab_layout_sw(int layout) { return layout & 0xFF; }
FA_SLAB_FN int slab_layout_pad(int layout) { return (layout >> 8) & 0xFF; }

// Slab width for n_used items and C candidates in lds bytes (accb: LDS bytes per
// accumulator: 4, 2 or 1): the first width in the measured order whose accumulator
// capacity holds min(C, kSlabBundleTarget), else width 4 from kSlabMinCap4.
// *cap = that capacity (candidates per pass).  Returns 0 (*cap = 0) when nothing fits.
FA_SLAB_FN int slab_width(int64_t n_used, int64_t C, double lds, double accb, int64_t* cap) {
  const int order[4] = {16, 32, 8, 4};
  const int64_t want = C < kSlabBundleTarget ? C : kSlabBundleTarget;
  for (int q = 0; q < 4; ++q) {
    const int sw = order[q];
    const int64_t c = (int64_t)((lds - (double)(n_used * slab_row_bytes(sw))) / accb);
    if (c >= want || (sw == 4 && c >= kSlabMinCap4)) { *cap = c; return sw; }
  }
  *cap = 0;
  return 0;
}

FA_SLAB_FN int64_t slab_cap(int64_t n_used, int64_t C, double lds, double accb) {
  int64_t cap = 0;
  slab_width(n_used, C, lds, accb, &cap);
  return cap;
}

// Largest bundle total t with t <= slab_cap(n_used, t) (monotone in t)
FA_SLAB_FN int64_t slab_total_limit(int64_t n_used, double lds, double accb) {
  int64_t lo = 0, hi = (int64_t)1 << 31;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) / 2;
    if (mid <= slab_cap(n_used, mid, lds, accb)) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Accumulator width of a slab count, defined once: accb (the LDS bytes per accumulator
// the rule above was asked with: 4, 2 or 1) selects the kernel's counters -- u32, two
// packed u16, or four single-writer bytes per word.  Weighted rows always count into u32.
// The mode bit rides in fa_hip_count_slab_rec_cls's cls argument: fa_dl.h's kSlabAcc16,
// or kSlabAcc8 beside it (private: no layer but this header and the launcher names it).
constexpr int kSlabAcc8 = 8;
static_assert((kSlabAcc8 & (kSlabCls | kSlabDense | kSlabAcc16)) == 0, "a mode bit of its own");

FA_SLAB_FN int slab_acc_bytes(double accb, bool weighted) {
  return weighted ? 4 : accb == 1.0 ? 1 : accb == 2.0 ? 2 : 4;
}
FA_SLAB_FN int slab_acc_mode(double accb, bool weighted) {
  const int b = slab_acc_bytes(accb, weighted);
  return b == 1 ? kSlabAcc8 : b == 2 ? kSlabAcc16 : 0;
}
FA_SLAB_FN int slab_mode_acc_bytes(int cls, bool weighted) {
  return weighted ? 4 : (cls & kSlabAcc8) ? 1 : (cls & kSlabAcc16) ? 2 : 4;
}
// u32 words that hold C counters of acc_bytes each (before slab_acc_words' rounding)
FA_SLAB_FN int64_t slab_acc_count(int64_t C, int acc_bytes) {
  return acc_bytes == 1 ? (C + 3) / 4 : acc_bytes == 2 ? (C + 1) / 2 : C;
}

// A one-pass bundle accepted by the rule at *accb bytes per accumulator (slab width *sw,
// capacity *cap) may count in narrower accumulators of accb_try bytes where that moves its
// slab up to width 16, the measured best, still in one pass; else it stays as it is.  The
// bundling itself (which levels share a launch) is the rule's at *accb either way.
FA_SLAB_FN bool slab_acc_upgrade(int64_t n_used, int64_t C, double lds, double accb_try, int* sw, int64_t* cap,
                                 double* accb) {
  if (*sw == 16 || accb_try >= *accb) return false;
  int64_t c = 0;
  if (slab_width(n_used, C, lds, accb_try, &c) != 16 || C > c) return false;
  *sw = 16;
  *cap = c;
  *accb = accb_try;
  return true;
}

// The kernel's accumulator words for n_acc accumulators (the map after them is 16-B aligned)
FA_SLAB_FN int64_t slab_acc_words(int64_t n_acc) { return (n_acc + 3) & ~(int64_t)3; }

// Dynamic LDS bytes of one workgroup: slab rows, n_acc_words u32 accumulators, map
FA_SLAB_FN int64_t slab_kernel_lds(int64_t n_used, int sw, int64_t n_acc_words, int64_t map_bytes) {
  return n_used * slab_row_bytes(sw) + n_acc_words * 4 + map_bytes;
}

// ... with the rows at pad shift s (s = 0: slab_kernel_lds)
FA_SLAB_FN int64_t slab_kernel_lds_pack(int64_t n_used, int sw, int s, int64_t n_acc_words, int64_t map_bytes) {
  return slab_rows_bytes(sw, s, n_used) + n_acc_words * 4 + map_bytes;
}

// ---- the tail rule (TUNING.dl_tail_bundle) ----------------------------------------------
// A bundle that holds every remaining level of the run is worth one pass at width 16 even
// where the rule above would split it: the split costs a second build of every slab.  The
// packed rule asks for all C candidates in ONE pass of 16-word slabs, with the smallest
// pad shift that leaves room for them: width 16 and *s, *cap = that capacity.  Where no
// shift fits, the answer is slab_width's own (*s = 0).
FA_SLAB_FN int slab_pack_width(int64_t n_used, int64_t C, double lds, double accb, int64_t* cap, int* s) {
  for (int q = 0; q <= kSlabPadMax; ++q) {
    const int64_t c = (int64_t)((lds - (double)slab_rows_bytes(16, q, n_used)) / accb);
    if (c >= C) { *cap = c; *s = q; return 16; }
  }
  *s = 0;
  return slab_width(n_used, C, lds, accb, cap);
}
// C candidates fit one packed pass
FA_SLAB_FN bool slab_pack_fits(int64_t n_used, int64_t C, double lds, double accb) {
  const int64_t c = (int64_t)((lds - (double)slab_rows_bytes(16, kSlabPadMax, n_used)) / accb);
  return C >= 1 && c >= C;
}
// The levels of a bundle (C[0 .. L) candidates each) that the rule above accepts at accb:
// level 0 stands (its own one-pass test is the generator's), level l joins while the total
// with it fits one pass -- the device chain's capacity test (gen.hip k_dl_decide), replayed.
// The chain's growth and bound tests do not depend on the capacity, so this is where a
// chain run without the tail rule would have stopped.
FA_SLAB_FN int slab_tail_cut(const int64_t* C, int L, int64_t n_used, double lds, double accb) {
  int64_t total = L > 0 ? C[0] : 0;
  int l = L > 0 ? 1 : 0;
  for (; l < L; ++l) {
    if (total + C[l] > slab_cap(n_used, total + C[l], lds, accb)) break;
    total += C[l];
  }
  return l;
}

// Workgroups of a slab count: one per slab, at most 256 CUs x the workgroups of
// kernel_lds bytes that fit a CU's budget (1 or 2)
FA_SLAB_FN int64_t slab_workgroups(int64_t nslabs, int64_t budget, int64_t kernel_lds) {
  int64_t per_cu = budget / (kernel_lds > 1 ? kernel_lds : 1);
  per_cu = per_cu < 1 ? 1 : per_cu > 2 ? 2 : per_cu;
  const int64_t n = nslabs < 256 * per_cu ? nslabs : 256 * per_cu;
  return n > 1 ? n : 1;
}

// ---- trimming estimate (host only) ----------------------------------------------------

// P[Binom(L, p) >= k] = I_p(k, L - k + 1): 1 - the k lowest terms, by the pmf's recurrence
inline double binom_tail(int64_t L, double p, int k) {
  if (L < k) return 0.0;
  if (p <= 0.0) return k <= 0 ? 1.0 : 0.0;
  if (p >= 1.0) return 1.0;
  double pmf = pow(1.0 - p, (double)L), below = 0.0;
  const double r = p / (1.0 - p);
  for (int i = 0; i < k; ++i) {
    below += pmf;
    pmf *= (double)(L - i) / (double)(i + 1) * r;
  }
  const double t = 1.0 - below;
  return t < 0.0 ? 0.0 : t > 1.0 ? 1.0 : t;
}

// Rows expected to keep >= k of the used items, and the item occurrences they keep:
// an occurrence survives with probability p, len_hist[L] rows have length L.
inline void trim_estimate(const int64_t* len_hist, int64_t n_bins, double p, int k, double* rows, double* nnz) {
  double est_rows = 0.0, est_nnz = 0.0;
  for (int64_t L = 0; L < n_bins; ++L) {
    const double h = (double)len_hist[L];
    if (h == 0.0) continue;
    est_rows += h * binom_tail(L, p, k);
    est_nnz += h * (double)L * p;
  }
  *rows = est_rows;
  *nnz = est_nnz;
}

}  // namespace fa
