// The slab kernel's LDS capacity rule and the trimming estimate, defined once.
//
// k_count_slab_rec (csrc/hip/count.hip) keeps, per workgroup, a slab of sw bitmap
// words for each used item, one accumulator per candidate and (optionally) a copy
// of the rank -> slab-row map in LDS.  Every layer that bundles, plans or launches
// a level asks the same question -- which slab width holds the accumulators, and
// does the bundle fit one pass -- and answers it here: plan.cpp (host planner),
// gen.hip (host-loop chain, device chain, the bundle post step), count.hip (the
// launcher's footprint check) and, through libfa_host.so's fa_slab_* exports
// (plan.cpp), fastapriori_amd.ops.primitives.
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
