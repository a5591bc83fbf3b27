// The (itemset, split) enumeration of the multi-item rule export, defined once for the
// kernels (csrc/hip/rules.hip k_rs_count / k_rs_emit) and the C++ path (rules.cpp
// fa_rule_splits_cpu).
//
// A frequent S of k >= 2 items (ascending ranks at positions 0 .. k-1) and a cap M >= 1 on
// the consequent's size give one rule S \ B -> B per non-empty proper subset B of S with
// |B| = b <= min(M, k - 1).  The splits of one itemset are numbered j = 0 .. n_k - 1:
//   b ascending, and within one b the b-subsets of the positions in lexicographic order
//   (as ascending tuples: {0,1} {0,2} {1,2}),
// with n_k = sum_{b = 1 .. min(M, k-1)} C(k, b).  A split is a position mask: bit p set
// means S[p] belongs to the consequent.  k <= kSplitMaxK = 32, so a mask is one uint32 and
// n_k <= 2^32 - 2 fits one too.  The elements of a level are numbered s * n_k + j over its
// rows s, the levels follow each other in ascending order.
//
// Every function reads binomials from a Pascal table the caller hands over (33 x 33 words,
// C(n, r) at [n * kSplitStride + r]): the host uses kSplitPascal, a kernel the copy it staged
// in LDS, so no lane recomputes a binomial.
//
// Plain C++ like fa_rule_measures.h: g++ and hipcc both read it.
#pragma once
#include <stdint.h>

#include "fa_rule_measures.h"

namespace fa {

constexpr int kSplitMaxK = 32;                 // the deepest level: a position mask is one uint32
constexpr int kSplitStride = kSplitMaxK + 1;   // words per Pascal row (r = 0 .. 32)

// C(n, r) for 0 <= r <= n <= 32 (0 above the diagonal); the largest, C(32, 16) = 601080390
struct SplitPascal {
  uint32_t c[kSplitStride * kSplitStride];
  constexpr SplitPascal() : c{} {
    for (int n = 0; n <= kSplitMaxK; ++n) {
      c[n * kSplitStride] = 1;
      for (int r = 1; r <= n; ++r)
        c[n * kSplitStride + r] = c[(n - 1) * kSplitStride + r - 1] + (r < n ? c[(n - 1) * kSplitStride + r] : 0u);
    }
  }
};
inline constexpr SplitPascal kSplitPascal{};   // the host's table (rules.hip keeps a device copy)

// the consequent sizes of a level-k itemset: 1 .. split_bmax(k, M)
FA_RM_HD int split_bmax(int k, int M) { return M < k - 1 ? M : k - 1; }

// n_k: the splits of one level-k itemset (0 for k < 2 or M < 1)
FA_RM_HD uint32_t split_count(const uint32_t* pas, int k, int M) {
  uint32_t n = 0;
  for (int b = 1; b <= split_bmax(k, M); ++b) n += pas[k * kSplitStride + b];
  return n;
}

// level-local element index -> (row s, split j), nk = n_k > 0.  64-bit division only past
// 2^32 elements in one level (as rm_locate in rules.hip).
FA_RM_HD void split_decode(int64_t local, uint32_t nk, int64_t* s, uint32_t* j) {
  const int64_t row = (local >> 32) == 0 ? (int64_t)((uint32_t)local / nk) : local / (int64_t)nk;
  *s = row;
  *j = (uint32_t)(local - row * (int64_t)nk);
}

// split j < n_k of a level-k itemset -> (b, position mask); both loops are bounded by k
// whatever j is
FA_RM_HD void split_unrank(const uint32_t* pas, int k, uint32_t j, int* b_out, uint32_t* mask_out) {
  int b = 1;
  for (uint32_t c = pas[k * kSplitStride + 1]; b < k - 1 && j >= c; c = pas[k * kSplitStride + b]) {
    j -= c;
    ++b;
  }
  // the j-th b-subset of 0 .. k-1 in lexicographic order: position p leads C(k-1-p, r-1)
  // of the subsets that are left when r items are still to place
  uint32_t mask = 0;
  int r = b;
  for (int p = 0; r > 0 && p < k; ++p) {
    const uint32_t lead = pas[(k - 1 - p) * kSplitStride + r - 1];
    if (j < lead) {
      mask |= 1u << p;
      --r;
    } else {
      j -= lead;
    }
  }
  *b_out = b;
  *mask_out = mask;
}

// every position of a level-k itemset
FA_RM_HD uint32_t split_full(int k) { return k >= 32 ? 0xffffffffu : (1u << k) - 1u; }

// Compares the row `a` (as many items as `take` has bits) with the items of S at the
// positions in `take`, in ascending position: the generalisation of cmp_skip (fa_hip.h),
// which leaves out one position.  The items are walked bit by bit from S itself.
FA_RM_HD int split_cmp(const int32_t* a, const int32_t* S, uint32_t take) {
  for (int i = 0; take; ++i, take &= take - 1) {
    const int32_t x = a[i], y = S[__builtin_ctz(take)];
    if (x != y) return x < y ? -1 : 1;
  }
  return 0;
}

// row of S's items at the positions `take` in a sorted level of n rows of m = popcount(take)
// items, -1 when it is missing
FA_RM_HD int64_t split_find(const int32_t* rows, int64_t n, int m, const int32_t* S, uint32_t take) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const int c = split_cmp(rows + mid * m, S, take);
    if (c == 0) return mid;
    if (c < 0) lo = mid + 1; else hi = mid;
  }
  return -1;
}

// The element total of a result and its workgroups of `tpb` elements, with overflow-checked
// arithmetic: sizes[k-1] rows at level k, eoff[k] = first element of level k >= 2 (K + 2
// words, when eoff is not null).  -3: a level of >= 2^31 - 1 rows, K > kSplitMaxK, M < 1, or
// 2^31 - 1 workgroups or more.
inline int64_t split_total(const uint32_t* pas, const int64_t* sizes, int K, int M, int tpb, int64_t* blocks,
                           int64_t* eoff) {
  if (K > kSplitMaxK || M < 1) return -3;
  const int64_t cap = ((int64_t)2147483647 - 1) * tpb;      // the most elements a grid holds
  int64_t total = 0;
  if (eoff) eoff[0] = eoff[1] = 0;
  for (int k = 1; k <= K; ++k) {
    if (sizes[k - 1] < 0 || sizes[k - 1] >= (int64_t)2147483647) return -3;
    if (k < 2) continue;
    if (eoff) eoff[k] = total;
    const int64_t nk = (int64_t)split_count(pas, k, M);     // < 2^32, sizes < 2^31: the product fits
    const int64_t add = sizes[k - 1] * nk;
    if (add > cap - total) return -3;
    total += add;
  }
  if (eoff) eoff[K + 1] = total;
  *blocks = (total + tpb - 1) / tpb;
  return total;
}

}  // namespace fa
