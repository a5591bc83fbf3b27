// Association rules on the device: subset index + confidence, level-wise
// redundancy cut, and emission of the sorted rule table.
//
// Reference behaviour (AssociationRules.scala):
//   * genRules (:122-145): every frequent S (|S| = k >= 2) and every position p
//     gives the rule (S - {S[p]}) -> S[p], conf = count(S).toDouble / count(S - {S[p]}).
//     The reference finds S - {S[p]} with a linear scan of all (k-1)-itemsets; here
//     one thread per (S, p) binary-searches the lexicographically sorted level k-1
//     (the "subset index" sub_k[S][p]).
//   * cut (:147-182): a rule A -> r with |A| >= 2 survives iff for every a in A the
//     rule (A - {a}) -> r survived one level down with strictly smaller confidence.
//     That child rule lives in itemset S - {a} = S - {S[q]}, whose index is the
//     subset index sub_k[S][q]; inside it the consequent r sits at position
//     p - (q < p).  So the cut is a dense lookup — no hash table of rules, unlike
//     the reference's per-level broadcast of a groupBy map (:158-160).
//   * order (:116-120): torch stable sorts on the device (conf desc, consequent
//     tie position asc, antecedent size asc, antecedent index asc: a total order);
//     k_rule_emit then writes the antecedent rows of the sorted rules.
// Host counterpart (same semantics, CPU runs and tests): csrc/host/rules.cpp.
#include "fa_hip.h"
#include "../host/fa_rule_measures.h"
#include "../host/fa_rule_splits.h"

namespace fa {

constexpr int kRuleTPB = 256;

// One thread per (itemset s, position p) of level k.  Rows of a wave share
// the same few itemsets, so the binary-search probes of neighbouring lanes
// mostly hit the same cache lines of level k-1.
// A subset that is not found (the input is not downward closed, or level k-1 is not
// sorted) stores sub = -1, conf = 0.0 and raises err to k (atomicMax, as k_sup_mark:
// the largest such level survives); the caller reads the word before it orders or
// emits anything, so no -1 is ever used as a row index.
__global__ __launch_bounds__(kRuleTPB) void k_rule_gen(
    const int32_t* __restrict__ S, int64_t nS, int k, const int32_t* __restrict__ A, int64_t nA,
    const int64_t* __restrict__ cS, const int64_t* __restrict__ cA, int32_t* __restrict__ sub,
    double* __restrict__ conf, int32_t* __restrict__ err) {
  const int64_t idx = (int64_t)blockIdx.x * kRuleTPB + threadIdx.x;
  if (idx >= nS * k) return;
  const int64_t s = idx / k;
  const int p = (int)(idx - s * k);
  const int32_t* row = S + s * k;
  int64_t lo = 0, hi = nA, found = -1;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const int c = cmp_skip(A + mid * (k - 1), row, k, p);
    if (c == 0) { found = mid; break; }
    if (c < 0) lo = mid + 1; else hi = mid;
  }
  sub[idx] = (int32_t)found;
  conf[idx] = found >= 0 ? (double)cS[s] / (double)cA[found] : 0.0;
  if (found < 0) atomicMax(err, k);
}

// Level-wise cut for level k >= 3 (antecedent size k-1 >= 2).  kept_prev /
// conf_prev: the level k-1 rules ([n_{k-1}][k-1]).
__global__ __launch_bounds__(kRuleTPB) void k_rule_cut(
    const int32_t* __restrict__ sub, const double* __restrict__ conf, int64_t nS, int k,
    const uint8_t* __restrict__ kept_prev, const double* __restrict__ conf_prev, uint8_t* __restrict__ kept) {
  const int64_t idx = (int64_t)blockIdx.x * kRuleTPB + threadIdx.x;
  if (idx >= nS * k) return;
  const int64_t s = idx / k;
  const int p = (int)(idx - s * k);
  const double c = conf[idx];
  const int32_t* srow = sub + s * k;
  bool ok = true;
  for (int q = 0; q < k && ok; ++q) {
    if (q == p) continue;
    const int32_t child = srow[q];
    if (child < 0) { ok = false; break; }
    const int64_t ci = (int64_t)child * (k - 1) + (p - (q < p ? 1 : 0));
    // strict: a child with equal (or higher) confidence makes this rule redundant
    ok = kept_prev[ci] && !(conf_prev[ci] >= c);
  }
  kept[idx] = ok ? 1 : 0;
}

// Antecedent rows of the sorted rules.  rows_all: every level's rows
// concatenated; base[m]: element offset of level m (antecedent size m).
__global__ __launch_bounds__(kRuleTPB) void k_rule_emit(
    const int32_t* __restrict__ rows_all, const int64_t* __restrict__ base, const int32_t* __restrict__ msz,
    const int32_t* __restrict__ ante_idx, const int64_t* __restrict__ ante_off, int64_t R,
    int32_t* __restrict__ ante) {
  const int64_t i = (int64_t)blockIdx.x * kRuleTPB + threadIdx.x;
  if (i >= R) return;
  const int m = msz[i];
  const int32_t* src = rows_all + base[m] + (int64_t)ante_idx[i] * m;
  int32_t* dst = ante + ante_off[i];
  for (int j = 0; j < m; ++j) dst[j] = src[j];
}

// ---------------------------------------------------------------------------
// Rule export (all_rules: no counterpart in the reference): EVERY rule A -> c of every
// frequent S = A + {c}, |S| >= 2, without the cut, selected on confidence (and lift)
// thresholds and compacted on the device.  Measures: ../host/fa_rule_measures.h.
//
// One thread per (S, p) over all levels k = 2..K, addressed as k_sup_mark (condense.hip)
// does: an int64 index over eoff (K + 2 words, searched in memory), the 32-bit division
// fast path, rows_all / base / cnt_all / cbase in rules_build_device's layout.
//   k_rm_count  finds A = S - {S[p]} in level k-1 and c = S[p] in level 1, tests the
//               thresholds, keeps sub[idx] = A's row (-1: not selected) and leaves the
//               workgroup's number of selected rules in wgtot (wg_sum);
//   k_rm_scan   one workgroup: exclusive scan of wgtot into wgoff (wg_scan_chunks), the
//               total R into ctl[0];
//   k_rm_emit   writes only the selected rules, at wgoff[workgroup] + the thread's rank
//               among its workgroup's selected threads (wg_scan_excl): stable in (level,
//               itemset, position) order and without atomics, so two runs place alike.
// ctl: two int64 words zeroed by the caller, [0] = R, [1] = the error word (the largest
// level k with an antecedent missing from level k-1 or a consequent missing from level
// 1: atomicMax as k_rule_gen); the caller reads both in one copy before it sizes, orders
// or emits anything.  A pair that raises the error selects nothing.
// ---------------------------------------------------------------------------
constexpr int kRmW = kRuleTPB / kWave;
constexpr int kRmScanTPB = 1024;

struct RmAt {
  int k, p;
  int64_t s;
  const int32_t* row;      // S
};

__device__ __forceinline__ RmAt rm_locate(const int32_t* __restrict__ rows_all, const int64_t* __restrict__ base,
                                          const int64_t* __restrict__ eoff, int K, int64_t idx) {
  // the last k in [2, K] with eoff[k] <= idx (an empty level has eoff[k] == eoff[k+1])
  int klo = 2, khi = K;
  while (klo < khi) {
    const int mid = (klo + khi + 1) >> 1;
    if (eoff[mid] <= idx) klo = mid; else khi = mid - 1;
  }
  RmAt a;
  a.k = klo;
  const int64_t local = idx - eoff[klo];
  // 64-bit division only past 2^32 elements in one level
  a.s = (local >> 32) == 0 ? (int64_t)((uint32_t)local / (uint32_t)klo) : local / klo;
  a.p = (int)(local - a.s * klo);
  a.row = rows_all + base[klo] + a.s * klo;
  return a;
}

// row of item c in level 1 (sorted single items), -1 when it is missing
__device__ __forceinline__ int64_t rm_find1(const int32_t* __restrict__ L1, int64_t n1, int32_t c) {
  int64_t lo = 0, hi = n1;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const int32_t x = L1[mid];
    if (x == c) return mid;
    if (x < c) lo = mid + 1; else hi = mid;
  }
  return -1;
}

__global__ __launch_bounds__(kRuleTPB) void k_rm_count(
    const int32_t* __restrict__ rows_all, const int64_t* __restrict__ base, const int64_t* __restrict__ cnt_all,
    const int64_t* __restrict__ cbase, const int64_t* __restrict__ eoff, int K, int64_t total, RuleSel q,
    int32_t* __restrict__ sub, int32_t* __restrict__ wgtot, unsigned long long* __restrict__ ctl) {
  __shared__ int scratch[kRmW];
  const int64_t idx = (int64_t)blockIdx.x * kRuleTPB + threadIdx.x;
  int sel = 0;
  if (idx < total) {
    const RmAt at = rm_locate(rows_all, base, eoff, K, idx);
    const int k = at.k;
    const int64_t rS = cbase[k - 1], rA = cbase[k - 2];       // first rows of level k and of level k-1
    const int32_t* A = rows_all + base[k - 1];
    int64_t lo = 0, hi = rS - rA, found = -1;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      const int c = cmp_skip(A + mid * (k - 1), at.row, k, at.p);
      if (c == 0) { found = mid; break; }
      if (c < 0) lo = mid + 1; else hi = mid;
    }
    const int64_t c1 = rm_find1(rows_all + base[1], cbase[1], at.row[at.p]);
    if (found < 0 || c1 < 0) {
      atomicMax(ctl + 1, (unsigned long long)k);
    } else {
      sel = rm_selected(q, cnt_all[rS + at.s], cnt_all[rA + found], cnt_all[c1]) ? 1 : 0;
    }
    sub[idx] = sel ? (int32_t)found : -1;
  }
  const int tot = wg_sum<kRmW>(sel, scratch);                 // every thread reaches it
  if (threadIdx.x == 0) wgtot[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kRmScanTPB) void k_rm_scan(const int32_t* __restrict__ wgtot, int64_t nwg,
                                                        int64_t* __restrict__ wgoff,
                                                        unsigned long long* __restrict__ ctl) {
  __shared__ int scratch[kRmScanTPB / kWave];
  const int64_t R = wg_scan_chunks<kRmScanTPB / kWave>(
      nwg, (int64_t)0, scratch, [&](int64_t i) { return (int)wgtot[i]; },
      [&](int64_t i, int64_t before, int) { wgoff[i] = before; });
  if (threadIdx.x == 0) ctl[0] = (unsigned long long)R;
}

// R: the total k_rm_scan left in ctl[0] (the outputs hold R rules; nothing is written past it)
__global__ __launch_bounds__(kRuleTPB) void k_rm_emit(
    const int32_t* __restrict__ rows_all, const int64_t* __restrict__ base, const int64_t* __restrict__ cnt_all,
    const int64_t* __restrict__ cbase, const int64_t* __restrict__ eoff, int K, int64_t total, int64_t N, int sort,
    const int32_t* __restrict__ sub, const int64_t* __restrict__ wgoff, int64_t R, int64_t* __restrict__ cntS,
    int64_t* __restrict__ cntA, int64_t* __restrict__ cntC, int32_t* __restrict__ msz, int32_t* __restrict__ aidx,
    int32_t* __restrict__ cons, double* __restrict__ conf, double* __restrict__ key) {
  __shared__ int scratch[kRmW];
  const int64_t idx = (int64_t)blockIdx.x * kRuleTPB + threadIdx.x;
  const int32_t found = idx < total ? sub[idx] : -1;
  const int sel = found >= 0 ? 1 : 0;
  int wg_total;
  const int before = wg_scan_excl<kRmW>(sel, scratch, wg_total);
  if (!sel) return;
  const int64_t o = wgoff[blockIdx.x] + before;
  if (o >= R) return;
  const RmAt at = rm_locate(rows_all, base, eoff, K, idx);
  const int k = at.k;
  const int32_t c = at.row[at.p];
  const int64_t c1 = rm_find1(rows_all + base[1], cbase[1], c);   // found by k_rm_count
  if (c1 < 0) return;
  const int64_t cS = cnt_all[cbase[k - 1] + at.s], cA = cnt_all[cbase[k - 2] + found], cC = cnt_all[c1];
  cntS[o] = cS;
  cntA[o] = cA;
  cntC[o] = cC;
  msz[o] = k - 1;
  aidx[o] = found;
  cons[o] = c;
  conf[o] = rm_confidence(cS, cA);
  key[o] = rm_measure(sort, cS, cA, cC, N);
}

// ---------------------------------------------------------------------------
// Rule export with multi-item consequents (all_rules(max_consequent = M); no counterpart in
// the reference): every rule S \ B -> B of every frequent S, |S| = k >= 2, for every
// non-empty proper subset B with |B| = b <= min(M, k - 1).  The enumeration -- element
// numbering, unranking of a split into (b, position mask), the masked row compare -- is
// ../host/fa_rule_splits.h, shared with rules.cpp fa_rule_splits_cpu.
//
// One thread per (itemset, split) element over all levels, an int64 index over eoff as
// k_rm_count; the element total grows as 2^k per itemset, so NOTHING wider than one bit per
// element lives between the passes:
//   k_rs_count  unranks its split, finds S \ B in level k - b and B in level b, tests the
//               thresholds, and stores one ballot word per wave and the workgroup's number
//               of selected rules in wgtot (wg_sum);
//   k_rm_scan   (above) the workgroup offsets, R into ctl[0];
//   k_rs_emit   reads its wave's ballot word, ranks the selected lanes (wg_scan_excl) and
//               redoes both searches for those only; placement as k_rm_emit: stable in
//               enumeration order, no atomics.
// Pascal rows 0 .. K and the n_k are staged in LDS once per workgroup (rs_stage); a mask's
// items are read bit by bit from the row in global memory, which neighbouring lanes share.
// ctl as k_rm_count: [1] = the largest level k with an antecedent or a consequent missing
// from its level.  The ballot, the sums and the barriers sit outside every divergent branch.
// ---------------------------------------------------------------------------
__device__ const SplitPascal d_split_pascal{};

struct RsAt {
  int k, b;
  uint32_t mask;           // positions of B in S
  int64_t s;
  const int32_t* row;      // S
};

// every thread of the workgroup calls it (it ends in a barrier); K <= kSplitMaxK
__device__ __forceinline__ void rs_stage(uint32_t* pas, uint32_t* nk, int K, int M) {
  for (int i = threadIdx.x; i < (K + 1) * kSplitStride; i += kRuleTPB) pas[i] = d_split_pascal.c[i];
  if ((int)threadIdx.x <= K) nk[threadIdx.x] = split_count(d_split_pascal.c, (int)threadIdx.x, M);
  __syncthreads();
}

__device__ __forceinline__ RsAt rs_locate(const int32_t* __restrict__ rows_all, const int64_t* __restrict__ base,
                                          const int64_t* __restrict__ eoff, int K, const uint32_t* pas,
                                          const uint32_t* nk, int64_t idx) {
  // the last k in [2, K] with eoff[k] <= idx (an empty level has eoff[k] == eoff[k+1])
  int klo = 2, khi = K;
  while (klo < khi) {
    const int mid = (klo + khi + 1) >> 1;
    if (eoff[mid] <= idx) klo = mid; else khi = mid - 1;
  }
  RsAt a;
  a.k = klo;
  uint32_t j;
  split_decode(idx - eoff[klo], nk[klo], &a.s, &j);
  split_unrank(pas, klo, j, &a.b, &a.mask);
  a.row = rows_all + base[klo] + a.s * klo;
  return a;
}

// rows of S \ B in level k - b and of B in level b (-1: missing)
__device__ __forceinline__ void rs_find(const int32_t* __restrict__ rows_all, const int64_t* __restrict__ base,
                                        const int64_t* __restrict__ cbase, const RsAt& at, int64_t& fa, int64_t& fb) {
  const int m = at.k - at.b;
  fa = split_find(rows_all + base[m], cbase[m] - cbase[m - 1], m, at.row, split_full(at.k) & ~at.mask);
  fb = split_find(rows_all + base[at.b], cbase[at.b] - cbase[at.b - 1], at.b, at.row, at.mask);
}

__global__ __launch_bounds__(kRuleTPB) void k_rs_count(
    const int32_t* __restrict__ rows_all, const int64_t* __restrict__ base, const int64_t* __restrict__ cnt_all,
    const int64_t* __restrict__ cbase, const int64_t* __restrict__ eoff, int K, int M, int64_t total, RuleSel q,
    unsigned long long* __restrict__ ballots, int32_t* __restrict__ wgtot, unsigned long long* __restrict__ ctl) {
  __shared__ uint32_t pas[kSplitStride * kSplitStride];
  __shared__ uint32_t nk[kSplitStride];
  __shared__ int scratch[kRmW];
  rs_stage(pas, nk, K, M);
  const int64_t idx = (int64_t)blockIdx.x * kRuleTPB + threadIdx.x;
  int sel = 0;
  if (idx < total) {
    const RsAt at = rs_locate(rows_all, base, eoff, K, pas, nk, idx);
    int64_t fa, fb;
    rs_find(rows_all, base, cbase, at, fa, fb);
    if (fa < 0 || fb < 0) {
      atomicMax(ctl + 1, (unsigned long long)at.k);
    } else {
      sel = rm_selected(q, cnt_all[cbase[at.k - 1] + at.s], cnt_all[cbase[at.k - at.b - 1] + fa],
                        cnt_all[cbase[at.b - 1] + fb]) ? 1 : 0;
    }
  }
  const unsigned long long word = __ballot(sel);              // every lane reaches it
  if (lane_id() == 0) ballots[(int64_t)blockIdx.x * kRmW + (threadIdx.x >> 6)] = word;
  const int tot = wg_sum<kRmW>(sel, scratch);
  if (threadIdx.x == 0) wgtot[blockIdx.x] = tot;
}

// R: the total k_rm_scan left in ctl[0] (the outputs hold R rules; nothing is written past it)
__global__ __launch_bounds__(kRuleTPB) void k_rs_emit(
    const int32_t* __restrict__ rows_all, const int64_t* __restrict__ base, const int64_t* __restrict__ cnt_all,
    const int64_t* __restrict__ cbase, const int64_t* __restrict__ eoff, int K, int M, int64_t total, int64_t N,
    int sort, const unsigned long long* __restrict__ ballots, const int64_t* __restrict__ wgoff, int64_t R,
    int64_t* __restrict__ cntS, int64_t* __restrict__ cntA, int64_t* __restrict__ cntC, int32_t* __restrict__ asz,
    int32_t* __restrict__ aidx, int32_t* __restrict__ csz, int32_t* __restrict__ cidx, double* __restrict__ conf,
    double* __restrict__ key) {
  __shared__ uint32_t pas[kSplitStride * kSplitStride];
  __shared__ uint32_t nk[kSplitStride];
  __shared__ int scratch[kRmW];
  const int64_t idx = (int64_t)blockIdx.x * kRuleTPB + threadIdx.x;
  const unsigned long long word = ballots[(int64_t)blockIdx.x * kRmW + (threadIdx.x >> 6)];
  const int sel = (int)((word >> lane_id()) & 1ull);          // a lane past the total never selected
  int wg_total;
  const int before = wg_scan_excl<kRmW>(sel, scratch, wg_total);
  if (wg_total == 0) return;                                  // the whole workgroup: before the barrier below
  rs_stage(pas, nk, K, M);
  if (!sel || idx >= total) return;
  const int64_t o = wgoff[blockIdx.x] + before;
  if (o >= R) return;
  const RsAt at = rs_locate(rows_all, base, eoff, K, pas, nk, idx);
  int64_t fa, fb;
  rs_find(rows_all, base, cbase, at, fa, fb);                 // found by k_rs_count
  if (fa < 0 || fb < 0) return;
  const int64_t cS = cnt_all[cbase[at.k - 1] + at.s], cA = cnt_all[cbase[at.k - at.b - 1] + fa],
                cC = cnt_all[cbase[at.b - 1] + fb];
  cntS[o] = cS;
  cntA[o] = cA;
  cntC[o] = cC;
  asz[o] = at.k - at.b;
  aidx[o] = (int32_t)fa;
  csz[o] = at.b;
  cidx[o] = (int32_t)fb;
  conf[o] = rm_confidence(cS, cA);
  key[o] = rm_measure(sort, cS, cA, cC, N);
}

// the five measures of the kept rules, from their three counts (after the sort and the limit)
__global__ __launch_bounds__(kRuleTPB) void k_rm_fin(
    const int64_t* __restrict__ cntS, const int64_t* __restrict__ cntA, const int64_t* __restrict__ cntC, int64_t R,
    int64_t N, double* __restrict__ support, double* __restrict__ conf, double* __restrict__ lift,
    double* __restrict__ leverage, double* __restrict__ conviction) {
  const int64_t i = (int64_t)blockIdx.x * kRuleTPB + threadIdx.x;
  if (i >= R) return;
  const int64_t cS = cntS[i], cA = cntA[i], cC = cntC[i];
  support[i] = rm_support(cS, N);
  conf[i] = rm_confidence(cS, cA);
  lift[i] = rm_lift(cS, cA, cC, N);
  leverage[i] = rm_leverage(cS, cA, cC, N);
  conviction[i] = rm_conviction(cS, cA, cC, N);
}

inline dim3 rule_grid(int64_t n) { return dim3((unsigned)((n + kRuleTPB - 1) / kRuleTPB)); }

}  // namespace fa

using namespace fa;

// err: one device int32, zero before a build's first level; non-zero after the kernels is
// the largest level k with a subset missing from level k-1.
FA_API int fa_hip_rule_gen(const int32_t* S, int64_t nS, int k, const int32_t* A, int64_t nA, const int64_t* cS,
                           const int64_t* cA, int32_t* sub, double* conf, int32_t* err, hipStream_t st) {
  if (nS <= 0 || k < 2) return 0;
  if (nA >= (int64_t)INT32_MAX) return 3;
  hipLaunchKernelGGL(k_rule_gen, rule_grid(nS * k), dim3(kRuleTPB), 0, st, S, nS, k, A, nA, cS, cA, sub, conf,
                     err);
  FA_LAUNCH_RET();
}

FA_API int fa_hip_rule_cut(const int32_t* sub, const double* conf, int64_t nS, int k, const uint8_t* kept_prev,
                           const double* conf_prev, uint8_t* kept, hipStream_t st) {
  if (nS <= 0 || k < 3) return 0;
  hipLaunchKernelGGL(k_rule_cut, rule_grid(nS * k), dim3(kRuleTPB), 0, st, sub, conf, nS, k, kept_prev,
                     conf_prev, kept);
  FA_LAUNCH_RET();
}

FA_API int fa_hip_rule_emit(const int32_t* rows_all, const int64_t* base, const int32_t* msz,
                            const int32_t* ante_idx, const int64_t* ante_off, int64_t R, int32_t* ante,
                            hipStream_t st) {
  if (R <= 0) return 0;
  hipLaunchKernelGGL(k_rule_emit, rule_grid(R), dim3(kRuleTPB), 0, st, rows_all, base, msz, ante_idx, ante_off,
                     R, ante);
  FA_LAUNCH_RET();
}

// The (S, p) elements of levels 2..K and their workgroups, by the launcher's rules (as
// fa_hip_sup_mark): 0 elements when no level above the first has a row, -3 for a level of
// >= INT32_MAX rows or a grid that does not fit.  sizes: HOST array of the K row counts.
static int64_t rm_total(const int64_t* sizes, int K, int64_t* blocks) {
  int64_t total = 0;
  for (int k = 1; k <= K; ++k) {
    if (sizes[k - 1] >= (int64_t)INT32_MAX) return -3;
    if (k >= 2) total += sizes[k - 1] * k;
  }
  *blocks = (total + kRuleTPB - 1) / kRuleTPB;
  if (*blocks >= (int64_t)INT32_MAX) return -3;
  return total;
}

// Selection and count of the exported rules: k_rm_count + k_rm_scan, whatever K.  sizes is a
// HOST array; every other pointer is device memory: sub int32 [elements], wgtot int32 and
// wgoff int64 [workgroups of 256 elements], ctl two int64 words that are zero on entry
// ([0] = R, [1] = error level on return).  0 with no launch when no level above the first
// has a row; 3 for a level of >= INT32_MAX rows or a grid that does not fit.
FA_API int fa_hip_rule_measures(const int32_t* rows_all, const int64_t* base, const int64_t* cnt_all,
                                const int64_t* cbase, const int64_t* eoff, const int64_t* sizes, int K, int64_t N,
                                double min_conf, int has_lift, double min_lift, int sort, int32_t* sub,
                                int32_t* wgtot, int64_t* wgoff, int64_t* ctl, hipStream_t st) {
  int64_t blocks = 0;
  const int64_t total = rm_total(sizes, K, &blocks);
  if (total < 0) return 3;
  if (total == 0) return 0;
  RuleSel q;
  q.min_conf = min_conf;
  q.min_lift = min_lift;
  q.N = N;
  q.has_lift = has_lift;
  q.sort = sort;
  hipLaunchKernelGGL(k_rm_count, dim3((unsigned)blocks), dim3(kRuleTPB), 0, st, rows_all, base, cnt_all, cbase, eoff,
                     K, total, q, sub, wgtot, (unsigned long long*)ctl);
  hipLaunchKernelGGL(k_rm_scan, dim3(1), dim3(kRmScanTPB), 0, st, wgtot, blocks, wgoff, (unsigned long long*)ctl);
  FA_LAUNCH_RET();
}

// The R selected rules of fa_hip_rule_measures' sub / wgoff, in (level, itemset, position)
// order: their three counts, the antecedent's size and row, the consequent, the confidence
// and the sort measure (each output holds R elements).
FA_API int fa_hip_rule_measures_emit(const int32_t* rows_all, const int64_t* base, const int64_t* cnt_all,
                                     const int64_t* cbase, const int64_t* eoff, const int64_t* sizes, int K,
                                     int64_t N, int sort, const int32_t* sub, const int64_t* wgoff, int64_t R,
                                     int64_t* cntS, int64_t* cntA, int64_t* cntC, int32_t* msz, int32_t* aidx,
                                     int32_t* cons, double* conf, double* key, hipStream_t st) {
  int64_t blocks = 0;
  const int64_t total = rm_total(sizes, K, &blocks);
  if (total < 0) return 3;
  if (total == 0 || R <= 0) return 0;
  hipLaunchKernelGGL(k_rm_emit, dim3((unsigned)blocks), dim3(kRuleTPB), 0, st, rows_all, base, cnt_all, cbase, eoff,
                     K, total, N, sort, sub, wgoff, R, cntS, cntA, cntC, msz, aidx, cons, conf, key);
  FA_LAUNCH_RET();
}

FA_API int fa_hip_rule_measures_fin(const int64_t* cntS, const int64_t* cntA, const int64_t* cntC, int64_t R,
                                    int64_t N, double* support, double* conf, double* lift, double* leverage,
                                    double* conviction, hipStream_t st) {
  if (R <= 0) return 0;
  if ((R + kRuleTPB - 1) / kRuleTPB >= (int64_t)INT32_MAX) return 3;
  hipLaunchKernelGGL(k_rm_fin, rule_grid(R), dim3(kRuleTPB), 0, st, cntS, cntA, cntC, R, N, support, conf, lift,
                     leverage, conviction);
  FA_LAUNCH_RET();
}

// The multi-item-consequent export's selection and count: k_rs_count + k_rm_scan, whatever K
// and M (consequents of up to M items; anything above K - 1 means every split).  Layout as
// fa_hip_rule_measures with eoff[k] = the first (itemset, split) element of level k
// (fa_rule_splits.h); ballots: one uint64 per wave of 64 elements, wgtot int32 and wgoff int64
// per workgroup of 256, ctl two zeroed int64 words ([0] = R, [1] = error level on return).
// 0 with no launch when no level above the first has a row; 3 for K > 32, M < 1, a level of
// >= INT32_MAX rows or an element total whose grid does not fit (overflow-checked).
FA_API int fa_hip_rule_splits(const int32_t* rows_all, const int64_t* base, const int64_t* cnt_all,
                              const int64_t* cbase, const int64_t* eoff, const int64_t* sizes, int K, int M, int64_t N,
                              double min_conf, int has_lift, double min_lift, int sort, uint64_t* ballots,
                              int32_t* wgtot, int64_t* wgoff, int64_t* ctl, hipStream_t st) {
  int64_t blocks = 0;
  const int64_t total = split_total(kSplitPascal.c, sizes, K, M, kRuleTPB, &blocks, nullptr);
  if (total < 0) return 3;
  if (total == 0) return 0;
  RuleSel q;
  q.min_conf = min_conf;
  q.min_lift = min_lift;
  q.N = N;
  q.has_lift = has_lift;
  q.sort = sort;
  hipLaunchKernelGGL(k_rs_count, dim3((unsigned)blocks), dim3(kRuleTPB), 0, st, rows_all, base, cnt_all, cbase, eoff,
                     K, M, total, q, (unsigned long long*)ballots, wgtot, (unsigned long long*)ctl);
  hipLaunchKernelGGL(k_rm_scan, dim3(1), dim3(kRmScanTPB), 0, st, wgtot, blocks, wgoff, (unsigned long long*)ctl);
  FA_LAUNCH_RET();
}

// The R selected rules of fa_hip_rule_splits' ballots / wgoff, in enumeration order: their
// three counts, the antecedent's size and row, the consequent's size and row (in level b; a
// level-1 row is its item's), the confidence and the sort measure (R elements each).
FA_API int fa_hip_rule_splits_emit(const int32_t* rows_all, const int64_t* base, const int64_t* cnt_all,
                                   const int64_t* cbase, const int64_t* eoff, const int64_t* sizes, int K, int M,
                                   int64_t N, int sort, const uint64_t* ballots, const int64_t* wgoff, int64_t R,
                                   int64_t* cntS, int64_t* cntA, int64_t* cntC, int32_t* asz, int32_t* aidx,
                                   int32_t* csz, int32_t* cidx, double* conf, double* key, hipStream_t st) {
  int64_t blocks = 0;
  const int64_t total = split_total(kSplitPascal.c, sizes, K, M, kRuleTPB, &blocks, nullptr);
  if (total < 0) return 3;
  if (total == 0 || R <= 0) return 0;
  hipLaunchKernelGGL(k_rs_emit, dim3((unsigned)blocks), dim3(kRuleTPB), 0, st, rows_all, base, cnt_all, cbase, eoff,
                     K, M, total, N, sort, (const unsigned long long*)ballots, wgoff, R, cntS, cntA, cntC, asz, aidx,
                     csz, cidx, conf, key);
  FA_LAUNCH_RET();
}
