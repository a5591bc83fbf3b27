// Closed and maximal frequent itemsets on the device: the superset marks of every level
// in one launch.  (No counterpart in the reference, which writes every frequent itemset.)
//
//   * T is maximal iff no proper superset of T is frequent;
//   * T is closed  iff no proper superset of T has T's count.
// Every (S, p) of level k names one (k-1)-subset T = S - {S[p]}, which by downward
// closure is a row of level k-1: T then has a frequent superset, and one of equal count
// when count(S) == count(T).  Counts are anti-monotone, so a larger superset of equal
// count implies a (k-1)+1 one, and one pass over all (S, p) of all levels marks every
// non-maximal and every non-closed itemset.  The lookup is k_rule_gen's subset index
// (rules.hip) read in the other direction: cmp_skip (fa_hip.h) is shared.
// Host counterpart (same inputs, same marks, same error): csrc/host/condense.cpp.
#include "fa_hip.h"

namespace fa {

constexpr int kSupTPB = 256;

// One thread per (itemset S, position p) over all levels k = 2..K, addressed by one
// int64 index: eoff[k] is the first index of level k (eoff[K+1] the total), so a result
// of 20 levels is one dispatch.  rows_all / base[m] (element offset of the size-m level)
// and cnt_all / cbase[m-1] (row offset of the size-m level) are rules_build_device's
// layout; the marks sup / eq are indexed like cnt_all and zeroed by the caller.
//   * The level table is searched in memory, not staged: it has K + 2 words, every lane
//     of a wave reads the same one or two of them, and it takes any K.
//   * Lanes of a wave share the same few itemsets, so their probes share the top of the
//     search tree and mostly the same rows of level k-1 (k_rule_gen's access argument).
//   * Many threads mark the same row: every write is a byte store of the constant 1, so
//     the result does not depend on their order.
//   * A subset that is not found means the input is not downward closed or not sorted:
//     the thread raises err to its level (atomicMax: the largest such level survives)
//     and stores nothing, so nothing is ever indexed with -1.
__global__ __launch_bounds__(kSupTPB) void k_sup_mark(
    const int32_t* __restrict__ rows_all, const int64_t* __restrict__ base, const int64_t* __restrict__ cnt_all,
    const int64_t* __restrict__ cbase, const int64_t* __restrict__ eoff, int K, int64_t total,
    uint8_t* __restrict__ sup, uint8_t* __restrict__ eq, int32_t* __restrict__ err) {
  const int64_t idx = (int64_t)blockIdx.x * kSupTPB + threadIdx.x;
  if (idx >= total) return;
  // the last k in [2, K] with eoff[k] <= idx (an empty level has eoff[k] == eoff[k+1])
  int klo = 2, khi = K;
  while (klo < khi) {
    const int mid = (klo + khi + 1) >> 1;
    if (eoff[mid] <= idx) klo = mid; else khi = mid - 1;
  }
  const int k = klo;
  const int64_t local = idx - eoff[k];
  // 64-bit division only past 2^32 elements in one level
  const int64_t s = (local >> 32) == 0 ? (int64_t)((uint32_t)local / (uint32_t)k) : local / k;
  const int p = (int)(local - s * k);
  const int64_t rS = cbase[k - 1], rA = cbase[k - 2];       // first rows of level k and of level k-1
  const int32_t* row = rows_all + base[k] + s * k;
  const int32_t* A = rows_all + base[k - 1];
  int64_t lo = 0, hi = rS - rA, found = -1;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const int c = cmp_skip(A + mid * (k - 1), row, k, p);
    if (c == 0) { found = mid; break; }
    if (c < 0) lo = mid + 1; else hi = mid;
  }
  if (found < 0) {
    atomicMax(err, k);
    return;
  }
  const int64_t t = rA + found;
  sup[t] = 1;
  if (cnt_all[rS + s] == cnt_all[t]) eq[t] = 1;             // full 64-bit compare
}

}  // namespace fa

using namespace fa;

// sizes: HOST array of the K levels' row counts (the launcher's checks and the grid);
// every other pointer is device memory.  0 with no launch when no level above the
// first has a row; 3 when a level has >= INT32_MAX rows (as fa_hip_rule_gen) or the
// grid would not fit.  err must be zero on entry; a non-zero word after the kernel is
// the largest level with a subset missing from the level below.
FA_API int fa_hip_sup_mark(const int32_t* rows_all, const int64_t* base, const int64_t* cnt_all,
                           const int64_t* cbase, const int64_t* eoff, const int64_t* sizes, int K, uint8_t* sup,
                           uint8_t* eq, int32_t* err, hipStream_t st) {
  if (K < 2 || sizes[1] <= 0) {
    // no level 2: nothing to mark -- unless a later level has rows, which the kernel reports
    bool later = false;
    for (int k = 3; k <= K; ++k) later = later || sizes[k - 1] > 0;
    if (!later) return 0;
  }
  int64_t total = 0;
  for (int k = 1; k <= K; ++k) {
    if (sizes[k - 1] >= (int64_t)INT32_MAX) return 3;
    if (k >= 2) total += sizes[k - 1] * k;
  }
  const int64_t blocks = (total + kSupTPB - 1) / kSupTPB;
  if (blocks >= (int64_t)INT32_MAX) return 3;
  hipLaunchKernelGGL(k_sup_mark, dim3((unsigned)blocks), dim3(kSupTPB), 0, st, rows_all, base, cnt_all, cbase, eoff,
                     K, total, sup, eq, err);
  FA_LAUNCH_RET();
}
