// The measures of an exported association rule A -> c, defined once for the kernels
// (csrc/hip/rules.hip) and the C++ path (rules.cpp fa_rule_measures_cpu).
//
// cS = count(A + {c}), cA = count(A), cC = count({c}), N = the number of lines; all are
// at most 2^31 - 1 (the callers reject anything larger), so every product below stays
// under 2^62 and is exact in signed int64.  A measure is then two int64 -> double
// conversions and ONE division: no expression holds a multiply next to an add, so
// there is nothing a compiler could contract into an FMA, and the device, this file's
// host build and Python's float(a * b) / float(c * d) on ints agree bit for bit.
// Level-1 counts are occurrence counts, so cC may exceed N (a token repeated on a
// line): leverage and conviction then come out negative, which is why the arithmetic
// is signed.  cA == cS is tested first, so conviction never divides by zero.
//
// Plain C++ like fa_limits.h: g++ and hipcc both read it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FA_RM_HD __host__ __device__ __forceinline__
#else
#define FA_RM_HD inline
#endif

namespace fa {

// the sort measures, in the order of --rules-sort's choices (config.py RULE_SORTS)
enum RuleSort { kSortConfidence = 0, kSortLift = 1, kSortLeverage = 2, kSortConviction = 3, kSortSupport = 4 };

constexpr int64_t kRuleCountMax = 2147483647;      // N and every count: products stay below 2^62

FA_RM_HD double rm_confidence(int64_t cS, int64_t cA) { return (double)cS / (double)cA; }
FA_RM_HD double rm_support(int64_t cS, int64_t N) { return (double)cS / (double)N; }
FA_RM_HD double rm_lift(int64_t cS, int64_t cA, int64_t cC, int64_t N) {
  const int64_t num = cS * N, den = cA * cC;
  return (double)num / (double)den;
}
FA_RM_HD double rm_leverage(int64_t cS, int64_t cA, int64_t cC, int64_t N) {
  const int64_t num = cS * N - cA * cC, den = N * N;
  return (double)num / (double)den;
}
FA_RM_HD double rm_conviction(int64_t cS, int64_t cA, int64_t cC, int64_t N) {
  if (cA == cS) return __builtin_inf();
  const int64_t num = cA * (N - cC), den = N * (cA - cS);
  return (double)num / (double)den;
}

FA_RM_HD double rm_measure(int sort, int64_t cS, int64_t cA, int64_t cC, int64_t N) {
  switch (sort) {
    case kSortLift: return rm_lift(cS, cA, cC, N);
    case kSortLeverage: return rm_leverage(cS, cA, cC, N);
    case kSortConviction: return rm_conviction(cS, cA, cC, N);
    case kSortSupport: return rm_support(cS, N);
    default: return rm_confidence(cS, cA);
  }
}

// what selects a rule (fp64 comparisons, both bounds inclusive) and names its sort measure
struct RuleSel {
  double min_conf, min_lift;
  int64_t N;
  int32_t has_lift, sort;
};

FA_RM_HD bool rm_selected(const RuleSel& q, int64_t cS, int64_t cA, int64_t cC) {
  if (!(rm_confidence(cS, cA) >= q.min_conf)) return false;
  return !q.has_lift || rm_lift(cS, cA, cC, q.N) >= q.min_lift;
}

}  // namespace fa
