// Closed and maximal frequent itemsets: the superset marks, on the CPU.  (No
// counterpart in the reference, which writes every frequent itemset.)
//
// Every frequent S of size k >= 2 and every position p name the (k-1)-subset
// T = S - {S[p]}, a row of the lexicographically sorted level k-1 by downward closure:
// T has a frequent superset (it is not maximal), and one of equal count when
// count(S) == count(T) (it is not closed).  Counts are anti-monotone, so supersets
// larger than |T| + 1 add nothing.  Device counterpart (same inputs, same marks, same
// error): csrc/hip/condense.hip k_sup_mark.
#include "fa_common.h"

namespace fa {

// row S minus position p against the (k-1)-row a, lexicographic
static inline int cmp_skip(const int32_t* a, const int32_t* s, int k, int p) {
  for (int i = 0, j = 0; i < k - 1; ++i, ++j) {
    if (j == p) ++j;
    const int32_t x = a[i], y = s[j];
    if (x != y) return x < y ? -1 : 1;
  }
  return 0;
}

}  // namespace fa

using namespace fa;

// rows_all: every level's int32 rows concatenated, base[m] the element offset of the
// size-m level (base[1] = 0); cnt_all: the int64 counts, cbase[m-1] the row offset of
// the size-m level (cbase[0] = 0, cbase[K] the number of itemsets).  sup / eq: one byte
// per itemset, indexed like cnt_all and zeroed by the caller; sup[t] = 1 when itemset t
// has a frequent superset, eq[t] = 1 when it has one of equal count.
// Returns 0, or the largest level k with a subset missing from level k-1 (the input is
// not downward closed or not sorted); such a pair marks nothing.
FA_API int fa_condense_cpu(const int32_t* rows_all, const int64_t* base, const int64_t* cnt_all,
                           const int64_t* cbase, int K, uint8_t* sup, uint8_t* eq, int nthreads) {
  std::atomic<int> bad{0};
  for (int k = 2; k <= K; ++k) {
    const int64_t rS = cbase[k - 1], rA = cbase[k - 2];
    const int64_t nS = cbase[k] - rS, nA = rS - rA;
    const int32_t* S = rows_all + base[k];
    const int32_t* A = rows_all + base[k - 1];
    parallel_for(nS, nthreads, 1024, [&](int64_t b, int64_t e, int) {
      for (int64_t s = b; s < e; ++s) {
        const int32_t* row = S + s * k;
        for (int p = 0; p < k; ++p) {
          int64_t lo = 0, hi = nA, found = -1;
          while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            const int c = cmp_skip(A + mid * (k - 1), row, k, p);
            if (c == 0) { found = mid; break; }
            if (c < 0) lo = mid + 1; else hi = mid;
          }
          if (found < 0) {
            int cur = bad.load(std::memory_order_relaxed);
            while (cur < k && !bad.compare_exchange_weak(cur, k, std::memory_order_relaxed)) {}
            continue;
          }
          // several threads may mark one row: relaxed atomic byte stores of the constant 1
          const int64_t t = rA + found;
          __atomic_store_n(&sup[t], (uint8_t)1, __ATOMIC_RELAXED);
          if (cnt_all[rS + s] == cnt_all[t]) __atomic_store_n(&eq[t], (uint8_t)1, __ATOMIC_RELAXED);
        }
      }
    });
  }
  return bad.load();
}
