// Association rules: generation, level-wise redundancy cut, ordering, and the
// CPU first-match recommender.
//
// Reference behaviour (AssociationRules.scala):
//   * genRules (:122-145): for every frequent S with |S| >= 2 and every s in S,
//     rule (S - {s}) -> s with conf = count(S).toDouble / count(S - {s}).
//     The reference finds S - {s} by a linear scan of all (|S|-1)-itemsets;
//     we binary-search the lexicographically sorted level instead (subset index).
//   * cut (:147-182): rules of the smallest antecedent size are all kept; a rule
//     A -> r at size i survives iff for EVERY a in A the rule (A - {a}) -> r was
//     kept at size i-1 and has strictly smaller confidence.
//   * order (:116-120): confidence descending, then consequent token as Int
//     ascending (tie positions are precomputed by the caller, see
//     fastapriori_amd/utils/jvm.py rule_tiebreak_key), then antecedent ranks.
//   * recommend (:80-106): first rule in that order with antecedent subset of the
//     basket and consequent not in the basket; otherwise "0".
#include <chrono>
#include <unordered_map>

#include "fa_combine.h"
#include "fa_common.h"
#include "fa_rule_measures.h"
#include "fa_rule_splits.h"

namespace fa {

struct RuleSet {
  std::vector<int64_t> ante_off;   // R+1
  std::vector<int32_t> ante;       // concatenated antecedent ranks (ascending)
  std::vector<int32_t> cons;
  std::vector<double> conf;
  std::vector<int64_t> stats;      // per antecedent level: before, after, cut microseconds
};

static inline int cmp_row(const int32_t* a, const int32_t* b, int m) {
  for (int i = 0; i < m; ++i)
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return 0;
}

static inline int64_t find_row(const int32_t* rows, int64_t n, int m, const int32_t* key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    int c = cmp_row(rows + mid * m, key, m);
    if (c == 0) return mid;
    if (c < 0) lo = mid + 1; else hi = mid;
  }
  return -1;
}

struct RawRule { int64_t ante; int32_t cons; double conf; };

}  // namespace fa

using namespace fa;

// rows[k-1]: level-k itemsets (sizes[k-1] rows of k ascending ranks, sorted);
// counts[k-1]: their supports.  levels_in = K.  tie_pos[r]: position of rank r's
// token in the consequent tiebreak order.
// The levels end at the first empty one: nothing is built, and no stats entry written,
// for it or for a level after it.  A level with rows above an empty one, or an itemset
// with a subset missing from the level below (the input is not downward closed or not
// sorted), is an error: *n_rules = -k for the largest such level k, the RuleSet is empty,
// and no antecedent index of -1 reaches the cut or the sort.
FA_API RuleSet* fa_rules_build(const int32_t* const* rows, const int64_t* const* counts,
                               const int64_t* sizes, int levels_in, const int64_t* tie_pos,
                               int nthreads, int64_t* n_rules) {
  auto* rs = new RuleSet();
  int levels = 0, gap = 0;
  while (levels < levels_in && sizes[levels] > 0) ++levels;
  for (int k = 2; k <= levels_in; ++k)
    if (sizes[k - 1] > 0 && sizes[k - 2] == 0) gap = k;
  if (gap) {
    *n_rules = -(int64_t)gap;
    return rs;
  }
  std::atomic<int> bad{0};
  // raw[L] = rules with antecedent size L (L = 1..levels-1), stored at raw[L-1]
  std::vector<std::vector<RawRule>> raw(std::max(0, levels - 1));
  for (int k = 2; k <= levels; ++k) {
    const int32_t* S = rows[k - 1];
    const int64_t nS = sizes[k - 1];
    const int32_t* A = rows[k - 2];
    const int64_t nA = sizes[k - 2];
    std::vector<RawRule>& out = raw[k - 2];
    out.resize((size_t)(nS * k));
    parallel_for(nS, nthreads, 1024, [&](int64_t b, int64_t e, int) {
      std::vector<int32_t> key(k - 1);
      for (int64_t s = b; s < e; ++s) {
        const int32_t* row = S + s * k;
        for (int p = 0; p < k; ++p) {
          int w = 0;
          for (int q = 0; q < k; ++q) if (q != p) key[w++] = row[q];
          int64_t a = find_row(A, nA, k - 1, key.data());
          // a >= 0 always holds for a complete miner (anti-monotonicity)
          if (a < 0) {
            int cur = bad.load(std::memory_order_relaxed);
            while (cur < k && !bad.compare_exchange_weak(cur, k, std::memory_order_relaxed)) {}
          }
          double c = a >= 0 ? (double)counts[k - 1][s] / (double)counts[k - 2][a] : 0.0;
          out[(size_t)(s * k + p)] = RawRule{a, row[p], c};
        }
      }
    });
  }
  if (bad.load()) {
    *n_rules = -(int64_t)bad.load();
    return rs;
  }
  // level-wise cut
  std::vector<std::vector<char>> keep(raw.size());
  for (size_t L = 0; L < raw.size(); ++L) {
    const auto t_cut = std::chrono::steady_clock::now();
    keep[L].assign(raw[L].size(), L == 0 ? 1 : 0);
    if (L == 0) {
      rs->stats.push_back((int64_t)raw[0].size()); rs->stats.push_back((int64_t)raw[0].size());
      rs->stats.push_back(0);
      continue;
    }
    // kept rules of the level below, keyed by (antecedent index, consequent)
    std::unordered_map<uint64_t, double> low;
    low.reserve(raw[L - 1].size() * 2);
    for (size_t i = 0; i < raw[L - 1].size(); ++i)
      if (keep[L - 1][i]) low.emplace(((uint64_t)raw[L - 1][i].ante << 32) | (uint32_t)raw[L - 1][i].cons,
                                      raw[L - 1][i].conf);
    const int m = (int)L + 1;          // antecedent size at this level
    const int32_t* Arows = rows[m - 1];
    const int32_t* Brows = rows[m - 2];
    const int64_t nB = sizes[m - 2];
    int64_t kept = 0;
    std::vector<int64_t> kept_t(std::max(1, nthreads), 0);
    parallel_for((int64_t)raw[L].size(), nthreads, 4096, [&](int64_t b, int64_t e, int tid) {
      std::vector<int32_t> key(m - 1);
      for (int64_t i = b; i < e; ++i) {
        const RawRule& r = raw[L][i];
        const int32_t* a = Arows + r.ante * m;
        bool ok = true;
        for (int p = 0; p < m && ok; ++p) {
          int w = 0;
          for (int q = 0; q < m; ++q) if (q != p) key[w++] = a[q];
          int64_t bi = find_row(Brows, nB, m - 1, key.data());
          if (bi < 0) { ok = false; break; }
          auto it = low.find(((uint64_t)bi << 32) | (uint32_t)r.cons);
          if (it == low.end() || it->second >= r.conf) ok = false;
        }
        keep[L][i] = ok ? 1 : 0;
        kept_t[tid] += ok;
      }
    });
    for (auto v : kept_t) kept += v;
    rs->stats.push_back((int64_t)raw[L].size());
    rs->stats.push_back(kept);
    rs->stats.push_back((int64_t)std::chrono::duration_cast<std::chrono::microseconds>(
        std::chrono::steady_clock::now() - t_cut).count());
  }
  // gather kept rules and sort
  struct Ref { int32_t level; int64_t idx; };
  std::vector<Ref> refs;
  for (size_t L = 0; L < raw.size(); ++L)
    for (size_t i = 0; i < raw[L].size(); ++i)
      if (keep[L][i]) refs.push_back(Ref{(int32_t)L, (int64_t)i});
  auto ante_ptr = [&](const Ref& r) { return rows[r.level] + raw[r.level][r.idx].ante * (r.level + 1); };
  std::stable_sort(refs.begin(), refs.end(), [&](const Ref& x, const Ref& y) {
    const RawRule& a = raw[x.level][x.idx];
    const RawRule& b = raw[y.level][y.idx];
    if (a.conf != b.conf) return a.conf > b.conf;
    int64_t ta = tie_pos[a.cons], tb = tie_pos[b.cons];
    if (ta != tb) return ta < tb;
    if (x.level != y.level) return x.level < y.level;
    return cmp_row(ante_ptr(x), ante_ptr(y), x.level + 1) < 0;
  });
  rs->ante_off.push_back(0);
  for (auto& r : refs) {
    const RawRule& rr = raw[r.level][r.idx];
    const int32_t* a = ante_ptr(r);
    rs->ante.insert(rs->ante.end(), a, a + r.level + 1);
    rs->ante_off.push_back((int64_t)rs->ante.size());
    rs->cons.push_back(rr.cons);
    rs->conf.push_back(rr.conf);
  }
  *n_rules = (int64_t)refs.size();
  return rs;
}

FA_API int64_t fa_rules_nante(RuleSet* rs) { return (int64_t)rs->ante.size(); }
FA_API int64_t fa_rules_nstats(RuleSet* rs) { return (int64_t)rs->stats.size(); }

FA_API void fa_rules_export(RuleSet* rs, int64_t* ante_off, int32_t* ante, int32_t* cons,
                            double* conf, int64_t* stats) {
  std::memcpy(ante_off, rs->ante_off.data(), rs->ante_off.size() * 8);
  if (!rs->ante.empty()) std::memcpy(ante, rs->ante.data(), rs->ante.size() * 4);
  if (!rs->cons.empty()) std::memcpy(cons, rs->cons.data(), rs->cons.size() * 4);
  if (!rs->conf.empty()) std::memcpy(conf, rs->conf.data(), rs->conf.size() * 8);
  if (!rs->stats.empty()) std::memcpy(stats, rs->stats.data(), rs->stats.size() * 8);
}

FA_API void fa_rules_free(RuleSet* rs) { delete rs; }

// First-match recommendation on the CPU.  Baskets are CSR of distinct ranks.
// out[i] = recommended rank, or -1 for "0".
FA_API void fa_recommend_cpu(const int64_t* ante_off, const int32_t* ante, const int32_t* cons,
                             int64_t R, int32_t F1, const int64_t* bask_off, const int32_t* bask,
                             int64_t M, int32_t* out, int nthreads) {
  const int64_t words = ((int64_t)F1 + 63) / 64;
  parallel_for(M, nthreads, 256, [&](int64_t b, int64_t e, int) {
    std::vector<uint64_t> bits((size_t)std::max<int64_t>(1, words), 0);
    for (int64_t u = b; u < e; ++u) {
      const int64_t s = bask_off[u], t = bask_off[u + 1];
      for (int64_t i = s; i < t; ++i) bits[bask[i] >> 6] |= 1ull << (bask[i] & 63);
      const int64_t usz = t - s;
      int32_t rec = -1;
      for (int64_t r = 0; r < R && usz > 0; ++r) {
        int32_t c = cons[r];
        if ((bits[c >> 6] >> (c & 63)) & 1) continue;
        const int64_t a0 = ante_off[r], a1 = ante_off[r + 1];
        if (a1 - a0 > usz) continue;
        bool sub = true;
        for (int64_t i = a0; i < a1; ++i)
          if (!((bits[ante[i] >> 6] >> (ante[i] & 63)) & 1)) { sub = false; break; }
        if (sub) { rec = c; break; }
      }
      out[u] = rec;
      for (int64_t i = s; i < t; ++i) bits[bask[i] >> 6] = 0;
    }
  });
}

// Ranked top-n on the CPU (an extension; the reference stops at the first match): the
// first n firing rules, in table order, whose consequents are pairwise distinct.
// out[u * n + j] = rule id of entry j, -1 past the last one.  1 <= n; R < 2^31.
FA_API void fa_recommend_topn_cpu(const int64_t* ante_off, const int32_t* ante, const int32_t* cons,
                                  int64_t R, int32_t F1, const int64_t* bask_off, const int32_t* bask,
                                  int64_t M, int32_t n, int32_t* out, int nthreads) {
  const int64_t words = ((int64_t)F1 + 63) / 64;
  parallel_for(M, nthreads, 256, [&](int64_t b, int64_t e, int) {
    std::vector<uint64_t> bits((size_t)std::max<int64_t>(1, words), 0), taken(bits.size(), 0);
    for (int64_t u = b; u < e; ++u) {
      const int64_t s = bask_off[u], t = bask_off[u + 1];
      for (int64_t i = s; i < t; ++i) bits[bask[i] >> 6] |= 1ull << (bask[i] & 63);
      const int64_t usz = t - s;
      int32_t* o = out + u * n;
      int32_t cnt = 0;
      for (int64_t r = 0; r < R && usz > 0 && cnt < n; ++r) {
        int32_t c = cons[r];
        if (((bits[c >> 6] | taken[c >> 6]) >> (c & 63)) & 1) continue;
        const int64_t a0 = ante_off[r], a1 = ante_off[r + 1];
        if (a1 - a0 > usz) continue;
        bool sub = true;
        for (int64_t i = a0; i < a1; ++i)
          if (!((bits[ante[i] >> 6] >> (ante[i] & 63)) & 1)) { sub = false; break; }
        if (!sub) continue;
        taken[c >> 6] |= 1ull << (c & 63);
        o[cnt++] = (int32_t)r;
      }
      for (int32_t j = 0; j < cnt; ++j) taken[cons[o[j]] >> 6] = 0;
      for (int32_t j = cnt; j < n; ++j) o[j] = -1;
      for (int64_t i = s; i < t; ++i) bits[bask[i] >> 6] = 0;
    }
  });
}

// Leave-one-out rank on the CPU (an extension, AssociationRules.evaluate): trial t is
// element t of the basket CSR, trow[t] its row.  out[t] = the 1-based place of h = bask[t]
// in the top-n list (fa_recommend_topn_cpu's) of its basket without h, 0 when it is not in
// it.  Written as the definition: clear h's bit, walk the table in order, restore the bit.
// 1 <= n.  Device counterpart: csrc/hip/recommend.hip k_holdout_rank(_indexed).
FA_API void fa_holdout_rank_cpu(const int64_t* ante_off, const int32_t* ante, const int32_t* cons,
                                int64_t R, int32_t F1, const int64_t* bask_off, const int32_t* bask,
                                const int64_t* trow, int64_t T, int32_t n, int32_t* out, int nthreads) {
  const int64_t words = ((int64_t)F1 + 63) / 64;
  parallel_for(T, nthreads, 256, [&](int64_t b, int64_t e, int) {
    std::vector<uint64_t> bits((size_t)std::max<int64_t>(1, words), 0), taken(bits.size(), 0);
    std::vector<int32_t> got;
    int64_t cur = -1;                                  // the row whose bits are set
    auto unset = [&]() {
      if (cur >= 0)
        for (int64_t i = bask_off[cur]; i < bask_off[cur + 1]; ++i) bits[bask[i] >> 6] = 0;
    };
    for (int64_t t = b; t < e; ++t) {
      const int64_t u = trow[t];
      if (u != cur) {
        unset();
        cur = u;
        for (int64_t i = bask_off[u]; i < bask_off[u + 1]; ++i) bits[bask[i] >> 6] |= 1ull << (bask[i] & 63);
      }
      const int32_t h = bask[t];
      const int64_t usz = bask_off[u + 1] - bask_off[u] - 1;
      bits[h >> 6] &= ~(1ull << (h & 63));
      int32_t rank = 0;
      got.clear();
      for (int64_t r = 0; r < R && usz > 0 && (int32_t)got.size() < n; ++r) {
        const int32_t c = cons[r];
        if (((bits[c >> 6] | taken[c >> 6]) >> (c & 63)) & 1) continue;
        const int64_t a0 = ante_off[r], a1 = ante_off[r + 1];
        if (a1 - a0 > usz) continue;
        bool sub = true;
        for (int64_t i = a0; i < a1; ++i)
          if (!((bits[ante[i] >> 6] >> (ante[i] & 63)) & 1)) { sub = false; break; }
        if (!sub) continue;
        taken[c >> 6] |= 1ull << (c & 63);
        got.push_back(c);
        if (c == h) { rank = (int32_t)got.size(); break; }
      }
      for (int32_t c : got) taken[c >> 6] = 0;
      bits[h >> 6] |= 1ull << (h & 63);
      out[t] = rank;
    }
    unset();
  });
}

// ---------------------------------------------------------------------------
// Combined scoring on the CPU (an extension, --combine sum|votes; docs/PARITY.md): every
// firing rule r of a basket (antecedent inside, consequent outside) adds weight[r] (int64,
// 1 .. 2^32) to the score S of its consequent, f is the consequent's smallest firing rule
// id, and the list is the consequents with S > 0 by S descending, then f ascending, cut to
// n.  Sums are exact: R < 2^31 rules of at most 2^32 stay below 2^63.  Device counterpart:
// csrc/hip/recommend.hip k_recommend_combined / k_holdout_rank_combined.
// ---------------------------------------------------------------------------
namespace fa {

// Per-thread state of the walk.  A rule is listed under the last item of its antecedent
// (built here, by counting), so a basket visits the lists of its own items only.
struct CombineWalk {
  const int64_t* ante_off; const int32_t* ante; const int32_t* cons; const int64_t* weight;
  const std::vector<int64_t>* list_off; const std::vector<int32_t>* list_rule;
  std::vector<uint64_t> bits;
  std::vector<int64_t> score;
  std::vector<int32_t> first, touched;

  CombineWalk(int32_t F1) : bits((size_t)std::max<int64_t>(1, ((int64_t)F1 + 63) / 64), 0),
                            score((size_t)std::max(F1, 1), 0), first((size_t)std::max(F1, 1), INT32_MAX) {}
  bool has(int32_t x) const { return (bits[x >> 6] >> (x & 63)) & 1; }
  // adds up the firing rules of the set in `bits` (usz items), visiting the lists of b[0 .. nb) except h
  void walk(const int32_t* b, int64_t nb, int32_t h, int64_t usz) {
    for (int64_t j = 0; j < nb; ++j) {
      if (b[j] == h) continue;
      for (int64_t q = (*list_off)[b[j]]; q < (*list_off)[b[j] + 1]; ++q) {
        const int32_t r = (*list_rule)[q], c = cons[r];
        const int64_t a0 = ante_off[r], a1 = ante_off[r + 1];
        if (has(c) || a1 - a0 > usz) continue;
        bool sub = true;
        for (int64_t i = a0; i < a1; ++i)
          if (!has(ante[i])) { sub = false; break; }
        if (!sub) continue;
        if (score[c] == 0) touched.push_back(c);
        score[c] += weight[r];
        first[c] = std::min(first[c], r);
      }
    }
  }
  bool beats(int32_t a, int32_t b) const { return score[a] != score[b] ? score[a] > score[b] : first[a] < first[b]; }
  void reset() {
    for (int32_t c : touched) { score[c] = 0; first[c] = INT32_MAX; }
    touched.clear();
  }
};

static void combine_lists(const int64_t* ante_off, const int32_t* ante, int64_t R, int32_t F1,
                          std::vector<int64_t>& list_off, std::vector<int32_t>& list_rule) {
  list_off.assign((size_t)F1 + 1, 0);
  list_rule.resize((size_t)R);
  for (int64_t r = 0; r < R; ++r) ++list_off[(size_t)ante[ante_off[r + 1] - 1] + 1];
  for (int32_t i = 0; i < F1; ++i) list_off[(size_t)i + 1] += list_off[i];
  std::vector<int64_t> at(list_off.begin(), list_off.end() - 1);
  for (int64_t r = 0; r < R; ++r) list_rule[(size_t)at[ante[ante_off[r + 1] - 1]]++] = (int32_t)r;
}

}  // namespace fa

// out_rule[u * n + j] = f of entry j, -1 past the last one; out_score[u * n + j] = its S, 0
// there.  1 <= n; R < 2^31.
FA_API void fa_recommend_combined_cpu(const int64_t* ante_off, const int32_t* ante, const int32_t* cons,
                                      const int64_t* weight, int64_t R, int32_t F1, const int64_t* bask_off,
                                      const int32_t* bask, int64_t M, int32_t n, int32_t* out_rule,
                                      int64_t* out_score, int nthreads) {
  std::vector<int64_t> list_off;
  std::vector<int32_t> list_rule;
  combine_lists(ante_off, ante, R, F1, list_off, list_rule);
  parallel_for(M, nthreads, 256, [&](int64_t b, int64_t e, int) {
    CombineWalk w(F1);
    w.ante_off = ante_off; w.ante = ante; w.cons = cons; w.weight = weight;
    w.list_off = &list_off; w.list_rule = &list_rule;
    for (int64_t u = b; u < e; ++u) {
      const int64_t s = bask_off[u], t = bask_off[u + 1];
      for (int64_t i = s; i < t; ++i) w.bits[bask[i] >> 6] |= 1ull << (bask[i] & 63);
      w.walk(bask + s, t - s, -1, t - s);
      std::sort(w.touched.begin(), w.touched.end(), [&](int32_t x, int32_t y) { return w.beats(x, y); });
      const int32_t cnt = (int32_t)std::min<size_t>(w.touched.size(), (size_t)n);
      for (int32_t j = 0; j < n; ++j) {
        out_rule[u * n + j] = j < cnt ? w.first[w.touched[j]] : -1;
        out_score[u * n + j] = j < cnt ? w.score[w.touched[j]] : 0;
      }
      w.reset();
      for (int64_t i = s; i < t; ++i) w.bits[bask[i] >> 6] = 0;
    }
  });
}

// Trial t is element t of the basket CSR, trow[t] its row: out[t] = the place of h = bask[t]
// in the combined list of its basket without h, 0 when S(h) = 0 or the place exceeds n.
FA_API void fa_holdout_rank_combined_cpu(const int64_t* ante_off, const int32_t* ante, const int32_t* cons,
                                         const int64_t* weight, int64_t R, int32_t F1, const int64_t* bask_off,
                                         const int32_t* bask, const int64_t* trow, int64_t T, int32_t n,
                                         int32_t* out, int nthreads) {
  std::vector<int64_t> list_off;
  std::vector<int32_t> list_rule;
  combine_lists(ante_off, ante, R, F1, list_off, list_rule);
  parallel_for(T, nthreads, 256, [&](int64_t b, int64_t e, int) {
    CombineWalk w(F1);
    w.ante_off = ante_off; w.ante = ante; w.cons = cons; w.weight = weight;
    w.list_off = &list_off; w.list_rule = &list_rule;
    for (int64_t t = b; t < e; ++t) {
      const int64_t u = trow[t], s = bask_off[u], z = bask_off[u + 1];
      const int32_t h = bask[t];
      for (int64_t i = s; i < z; ++i)
        if (bask[i] != h) w.bits[bask[i] >> 6] |= 1ull << (bask[i] & 63);
      w.walk(bask + s, z - s, h, z - s - 1);
      int32_t place = 0;
      if (w.score[h] > 0) {
        place = 1;
        for (int32_t c : w.touched) place += w.beats(c, h);
      }
      out[t] = place <= n ? place : 0;
      w.reset();
      for (int64_t i = s; i < z; ++i) w.bits[bask[i] >> 6] = 0;
    }
  });
}

// fa_combine.h's LDS rule by name: one wave's bytes, the waves per workgroup (0: no wave
// fits, the launchers return 2) and the LDS limit
FA_API int64_t fa_combine_wave_bytes(int64_t F1) { return combine_wave_bytes(F1); }
FA_API int fa_combine_waves(int64_t F1) { return combine_waves(F1); }
FA_API int64_t fa_combine_lds_max() { return kCombLdsMax; }

// ---------------------------------------------------------------------------
// Rule export (AssociationRules.all_rules; no counterpart in the reference): every rule
// A -> c of every frequent S = A + {c}, |S| >= 2, WITHOUT the cut, with the measures of
// fa_rule_measures.h.  Device counterpart (same inputs, selection, order and error):
// csrc/hip/rules.hip k_rm_count / k_rm_scan / k_rm_emit / k_rm_fin.
// ---------------------------------------------------------------------------
namespace fa {

struct RuleMeasureSet {
  std::vector<int64_t> ante_off, cS, cA, cC;       // R+1, R, R, R
  std::vector<int32_t> ante, cons;
  std::vector<double> support, conf, lift, leverage, conviction;
};

}  // namespace fa

// rows_all / base / cnt_all / cbase: condense.cpp's layout (base[m]: element offset of the
// size-m level, cbase[m-1]: its first row).  The levels end at the first empty one (the
// caller rejects rows above an empty level).  Selection: confidence >= min_conf and, with
// has_lift, lift >= min_lift, in fp64.  Order: the sort measure descending (+inf first),
// confidence descending, tie_pos[consequent], antecedent size, antecedent row -- a total
// order; limit >= 0 keeps that many rules.  *n_rules: the rules kept, or -k for the
// largest level k with an antecedent missing from level k-1 or a consequent missing from
// level 1 (nothing is built then).  N and every count are at most kRuleCountMax (the
// caller checks).
FA_API RuleMeasureSet* fa_rule_measures_cpu(const int32_t* rows_all, const int64_t* base, const int64_t* cnt_all,
                                            const int64_t* cbase, int K, int64_t N, double min_conf, int has_lift,
                                            double min_lift, int sort, int64_t limit, const int64_t* tie_pos,
                                            int nthreads, int64_t* n_rules) {
  auto* out = new RuleMeasureSet();
  out->ante_off.push_back(0);
  *n_rules = 0;
  int levels = 0;
  while (levels < K && cbase[levels + 1] > cbase[levels]) ++levels;
  if (levels < 2) return out;
  RuleSel q;
  q.min_conf = min_conf;
  q.min_lift = min_lift;
  q.N = N;
  q.has_lift = has_lift;
  q.sort = sort;
  // (S, p) elements in (level, itemset, position) order, in fixed chunks of itemsets:
  // pass 1 finds and selects (sub: the antecedent's row, -1 when not selected) and counts
  // per chunk, a scan places the chunks, pass 2 writes the selected rules
  constexpr int64_t kChunk = 1024;
  struct Chunk { int k; int64_t s0, s1, e0; };
  std::vector<Chunk> chunks;
  int64_t total = 0;
  for (int k = 2; k <= levels; ++k) {
    const int64_t nS = cbase[k] - cbase[k - 1];
    for (int64_t s0 = 0; s0 < nS; s0 += kChunk) {
      const int64_t s1 = std::min(nS, s0 + kChunk);
      chunks.push_back(Chunk{k, s0, s1, total + s0 * k});
    }
    total += nS * k;
  }
  std::vector<int32_t> sub((size_t)total);
  std::vector<int64_t> coff(chunks.size() + 1, 0);
  std::atomic<int> bad{0};
  const int32_t* L1 = rows_all + base[1];
  const int64_t n1 = cbase[1];
  parallel_for((int64_t)chunks.size(), nthreads, 1, [&](int64_t b, int64_t e, int) {
    std::vector<int32_t> key;
    for (int64_t ci = b; ci < e; ++ci) {
      const Chunk& c = chunks[(size_t)ci];
      const int k = c.k;
      key.resize((size_t)k - 1);
      const int32_t* S = rows_all + base[k];
      const int32_t* A = rows_all + base[k - 1];
      const int64_t rS = cbase[k - 1], rA = cbase[k - 2], nA = rS - rA;
      int64_t kept = 0;
      for (int64_t s = c.s0; s < c.s1; ++s) {
        const int32_t* row = S + s * k;
        for (int p = 0; p < k; ++p) {
          int w = 0;
          for (int j = 0; j < k; ++j) if (j != p) key[w++] = row[j];
          const int64_t a = find_row(A, nA, k - 1, key.data());
          const int64_t c1 = find_row(L1, n1, 1, row + p);
          bool sel = false;
          if (a < 0 || c1 < 0) {
            int cur = bad.load(std::memory_order_relaxed);
            while (cur < k && !bad.compare_exchange_weak(cur, k, std::memory_order_relaxed)) {}
          } else {
            sel = rm_selected(q, cnt_all[rS + s], cnt_all[rA + a], cnt_all[c1]);
          }
          sub[(size_t)(c.e0 + (s - c.s0) * k + p)] = sel ? (int32_t)a : -1;
          kept += sel;
        }
      }
      coff[(size_t)ci + 1] = kept;
    }
  });
  if (bad.load()) {
    *n_rules = -(int64_t)bad.load();
    return out;
  }
  for (size_t i = 0; i < chunks.size(); ++i) coff[i + 1] += coff[i];
  const int64_t R = coff[chunks.size()];
  struct Sel { double key, conf; int64_t tie, cS, cA, cC; int32_t msz, aidx, cons; };
  std::vector<Sel> sel((size_t)R);
  parallel_for((int64_t)chunks.size(), nthreads, 1, [&](int64_t b, int64_t e, int) {
    for (int64_t ci = b; ci < e; ++ci) {
      const Chunk& c = chunks[(size_t)ci];
      const int k = c.k;
      const int32_t* S = rows_all + base[k];
      const int64_t rS = cbase[k - 1], rA = cbase[k - 2];
      int64_t o = coff[(size_t)ci];
      for (int64_t s = c.s0; s < c.s1; ++s)
        for (int p = 0; p < k; ++p) {
          const int32_t a = sub[(size_t)(c.e0 + (s - c.s0) * k + p)];
          if (a < 0) continue;
          const int32_t item = S[s * k + p];
          const int64_t cS = cnt_all[rS + s], cA = cnt_all[rA + a], cC = cnt_all[find_row(L1, n1, 1, &item)];
          sel[(size_t)o++] = Sel{rm_measure(sort, cS, cA, cC, N), rm_confidence(cS, cA), tie_pos[item], cS, cA, cC,
                                 k - 1, a, item};
        }
    }
  });
  // the order: sorted chunks merged pairwise, as the itemset writer's lines
  auto less = [](const Sel& x, const Sel& y) {
    if (x.key != y.key) return x.key > y.key;
    if (x.conf != y.conf) return x.conf > y.conf;
    if (x.tie != y.tie) return x.tie < y.tie;
    if (x.msz != y.msz) return x.msz < y.msz;
    return x.aidx < y.aidx;
  };
  {
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>(nthreads, R / 4096));
    std::vector<int64_t> cut((size_t)T + 1);
    for (int t = 0; t <= T; ++t) cut[t] = R * t / T;
    parallel_for_threads(T, [&](int t) { std::sort(sel.begin() + cut[t], sel.begin() + cut[t + 1], less); });
    for (int w = 1; w < T; w *= 2) {
      const int nm = (T + 2 * w - 1) / (2 * w), nt = std::min(nm, std::max(nthreads, 1));
      parallel_for_threads(nt, [&](int tid) {
        for (int m = tid; m < nm; m += nt) {
          const int a0 = 2 * w * m, a1 = std::min(T, a0 + w), a2 = std::min(T, a0 + 2 * w);
          if (a1 < a2) std::inplace_merge(sel.begin() + cut[a0], sel.begin() + cut[a1], sel.begin() + cut[a2], less);
        }
      });
    }
  }
  const int64_t keep = limit >= 0 ? std::min(limit, R) : R;
  out->ante_off.resize((size_t)keep + 1);
  for (int64_t i = 0; i < keep; ++i) out->ante_off[(size_t)i + 1] = out->ante_off[(size_t)i] + sel[(size_t)i].msz;
  out->ante.resize((size_t)out->ante_off[(size_t)keep]);
  for (auto* v : {&out->cS, &out->cA, &out->cC}) v->resize((size_t)keep);
  for (auto* v : {&out->support, &out->conf, &out->lift, &out->leverage, &out->conviction}) v->resize((size_t)keep);
  out->cons.resize((size_t)keep);
  parallel_for(keep, nthreads, 4096, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; ++i) {
      const Sel& r = sel[(size_t)i];
      const int32_t* a = rows_all + base[r.msz] + (int64_t)r.aidx * r.msz;
      std::copy(a, a + r.msz, out->ante.begin() + out->ante_off[(size_t)i]);
      out->cons[i] = r.cons;
      out->cS[i] = r.cS; out->cA[i] = r.cA; out->cC[i] = r.cC;
      out->support[i] = rm_support(r.cS, N);
      out->conf[i] = rm_confidence(r.cS, r.cA);
      out->lift[i] = rm_lift(r.cS, r.cA, r.cC, N);
      out->leverage[i] = rm_leverage(r.cS, r.cA, r.cC, N);
      out->conviction[i] = rm_conviction(r.cS, r.cA, r.cC, N);
    }
  });
  *n_rules = keep;
  return out;
}

FA_API int64_t fa_rule_measures_nante(RuleMeasureSet* h) { return (int64_t)h->ante.size(); }

// every array holds R elements (ante_off R+1, ante fa_rule_measures_nante)
FA_API void fa_rule_measures_export(RuleMeasureSet* h, int64_t* ante_off, int32_t* ante, int32_t* cons, int64_t* cS,
                                    int64_t* cA, int64_t* cC, double* support, double* conf, double* lift,
                                    double* leverage, double* conviction) {
  auto put = [](auto* dst, const auto& v) {
    if (!v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(v[0]));
  };
  put(ante_off, h->ante_off); put(ante, h->ante); put(cons, h->cons);
  put(cS, h->cS); put(cA, h->cA); put(cC, h->cC);
  put(support, h->support); put(conf, h->conf); put(lift, h->lift);
  put(leverage, h->leverage); put(conviction, h->conviction);
}

FA_API void fa_rule_measures_free(RuleMeasureSet* h) { delete h; }

// ---------------------------------------------------------------------------
// Rule export with multi-item consequents (AssociationRules.all_rules(max_consequent = M); no
// counterpart in the reference): every rule S \ B -> B of every frequent S, |S| = k >= 2, for
// every non-empty proper subset B with |B| <= min(M, k - 1), with fa_rule_measures.h's
// measures on cS = count(S), cA = count(S \ B) and cC = count(B).  The enumeration is
// fa_rule_splits.h's.  Device counterpart (same inputs, selection, order and error):
// csrc/hip/rules.hip k_rs_count / k_rm_scan / k_rs_emit / k_rm_fin.
// ---------------------------------------------------------------------------
namespace fa {

struct RuleSplitSet {
  std::vector<int64_t> ante_off, cons_off, cS, cA, cC;       // R+1, R+1, R, R, R
  std::vector<int32_t> ante, cons;
  std::vector<double> support, conf, lift, leverage, conviction;
};

}  // namespace fa

// the enumeration by name, for the tests: n_k, the unranking (1: k, M or j out of range) and
// the decode of a level-local index
FA_API uint64_t fa_rule_split_count(int k, int M) {
  return (k < 2 || k > kSplitMaxK || M < 1) ? 0 : (uint64_t)split_count(kSplitPascal.c, k, M);
}
FA_API int fa_rule_split_unrank(int k, int M, uint64_t j, int32_t* b, uint32_t* mask) {
  if (j >= fa_rule_split_count(k, M)) return 1;
  int bb;
  split_unrank(kSplitPascal.c, k, (uint32_t)j, &bb, mask);
  *b = bb;
  return 0;
}
FA_API int fa_rule_split_decode(int64_t local, uint64_t nk, int64_t* s, uint64_t* j) {
  if (local < 0 || nk == 0 || nk > 0xfffffffeull) return 1;
  uint32_t jj;
  split_decode(local, (uint32_t)nk, s, &jj);
  *j = jj;
  return 0;
}

// Layout, selection and limits as fa_rule_measures_cpu; M >= 1 caps the consequent's size
// (anything above K - 1 means every split).  Order: the sort measure descending (+inf first),
// confidence descending, consequent size, the consequent key (tie_pos[item] for one item,
// else the consequent's row in its level), antecedent size, antecedent row -- a total order;
// limit >= 0 keeps that many rules.  *n_rules: the rules kept, -k for the largest level k
// with an antecedent or a consequent missing from its level, or INT64_MIN for K > 32, M < 1
// or an element total past the device grid's (the caller checks all three first).
FA_API RuleSplitSet* fa_rule_splits_cpu(const int32_t* rows_all, const int64_t* base, const int64_t* cnt_all,
                                        const int64_t* cbase, int K, int M, int64_t N, double min_conf, int has_lift,
                                        double min_lift, int sort, int64_t limit, const int64_t* tie_pos,
                                        int nthreads, int64_t* n_rules) {
  auto* out = new RuleSplitSet();
  out->ante_off.push_back(0);
  out->cons_off.push_back(0);
  *n_rules = 0;
  int levels = 0;
  while (levels < K && cbase[levels + 1] > cbase[levels]) ++levels;
  {
    std::vector<int64_t> sizes((size_t)std::max(levels, 1), 0);
    for (int k = 1; k <= levels; ++k) sizes[(size_t)k - 1] = cbase[k] - cbase[k - 1];
    int64_t blocks = 0;
    if (split_total(kSplitPascal.c, sizes.data(), levels, M, 256, &blocks, nullptr) < 0) {
      *n_rules = INT64_MIN;
      return out;
    }
  }
  if (levels < 2) return out;
  RuleSel q;
  q.min_conf = min_conf;
  q.min_lift = min_lift;
  q.N = N;
  q.has_lift = has_lift;
  q.sort = sort;
  const uint32_t* pas = kSplitPascal.c;
  // elements in enumeration order, in chunks of about kChunk of them (whole itemsets): every
  // chunk collects its selected rules, the chunks are joined in order
  constexpr int64_t kChunk = 1 << 16;
  struct Chunk { int k; int64_t s0, s1; };
  std::vector<Chunk> chunks;
  for (int k = 2; k <= levels; ++k) {
    const int64_t nS = cbase[k] - cbase[k - 1];
    const int64_t per = std::max<int64_t>(1, kChunk / (int64_t)split_count(pas, k, M));
    for (int64_t s0 = 0; s0 < nS; s0 += per) chunks.push_back(Chunk{k, s0, std::min(nS, s0 + per)});
  }
  struct Sel { double key, conf; int64_t ckey, cS, cA, cC; int32_t csz, cidx, asz, aidx; };
  std::vector<std::vector<Sel>> found(chunks.size());
  std::atomic<int> bad{0};
  parallel_for((int64_t)chunks.size(), nthreads, 1, [&](int64_t b0, int64_t e0, int) {
    for (int64_t ci = b0; ci < e0; ++ci) {
      const Chunk& c = chunks[(size_t)ci];
      const int k = c.k;
      const uint32_t nk = split_count(pas, k, M), full = split_full(k);
      const int32_t* S = rows_all + base[k];
      std::vector<Sel>& dst = found[(size_t)ci];
      for (int64_t s = c.s0; s < c.s1; ++s) {
        const int32_t* row = S + s * k;
        const int64_t cS = cnt_all[cbase[k - 1] + s];
        for (uint32_t j = 0; j < nk; ++j) {
          int b;
          uint32_t mask;
          split_unrank(pas, k, j, &b, &mask);
          const int m = k - b;
          const int64_t fa = split_find(rows_all + base[m], cbase[m] - cbase[m - 1], m, row, full & ~mask);
          const int64_t fb = split_find(rows_all + base[b], cbase[b] - cbase[b - 1], b, row, mask);
          if (fa < 0 || fb < 0) {
            int cur = bad.load(std::memory_order_relaxed);
            while (cur < k && !bad.compare_exchange_weak(cur, k, std::memory_order_relaxed)) {}
            continue;
          }
          const int64_t cA = cnt_all[cbase[m - 1] + fa], cC = cnt_all[cbase[b - 1] + fb];
          if (!rm_selected(q, cS, cA, cC)) continue;
          const int64_t ckey = b == 1 ? tie_pos[rows_all[base[1] + fb]] : fb;
          dst.push_back(Sel{rm_measure(sort, cS, cA, cC, N), rm_confidence(cS, cA), ckey, cS, cA, cC, b, (int32_t)fb,
                            m, (int32_t)fa});
        }
      }
    }
  });
  if (bad.load()) {
    *n_rules = -(int64_t)bad.load();
    return out;
  }
  std::vector<int64_t> coff(chunks.size() + 1, 0);
  for (size_t i = 0; i < chunks.size(); ++i) coff[i + 1] = coff[i] + (int64_t)found[i].size();
  const int64_t R = coff[chunks.size()];
  std::vector<Sel> sel((size_t)R);
  parallel_for((int64_t)chunks.size(), nthreads, 1, [&](int64_t b0, int64_t e0, int) {
    for (int64_t ci = b0; ci < e0; ++ci) {
      std::copy(found[(size_t)ci].begin(), found[(size_t)ci].end(), sel.begin() + coff[(size_t)ci]);
      std::vector<Sel>().swap(found[(size_t)ci]);
    }
  });
  auto less = [](const Sel& x, const Sel& y) {
    if (x.key != y.key) return x.key > y.key;
    if (x.conf != y.conf) return x.conf > y.conf;
    if (x.csz != y.csz) return x.csz < y.csz;
    if (x.ckey != y.ckey) return x.ckey < y.ckey;
    if (x.asz != y.asz) return x.asz < y.asz;
    return x.aidx < y.aidx;
  };
  {
    // sorted parts merged pairwise, as fa_rule_measures_cpu
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>(nthreads, R / 4096));
    std::vector<int64_t> cut((size_t)T + 1);
    for (int t = 0; t <= T; ++t) cut[t] = R * t / T;
    parallel_for_threads(T, [&](int t) { std::sort(sel.begin() + cut[t], sel.begin() + cut[t + 1], less); });
    for (int w = 1; w < T; w *= 2) {
      const int nm = (T + 2 * w - 1) / (2 * w), nt = std::min(nm, std::max(nthreads, 1));
      parallel_for_threads(nt, [&](int tid) {
        for (int mi = tid; mi < nm; mi += nt) {
          const int a0 = 2 * w * mi, a1 = std::min(T, a0 + w), a2 = std::min(T, a0 + 2 * w);
          if (a1 < a2) std::inplace_merge(sel.begin() + cut[a0], sel.begin() + cut[a1], sel.begin() + cut[a2], less);
        }
      });
    }
  }
  const int64_t keep = limit >= 0 ? std::min(limit, R) : R;
  out->ante_off.resize((size_t)keep + 1);
  out->cons_off.resize((size_t)keep + 1);
  for (int64_t i = 0; i < keep; ++i) {
    out->ante_off[(size_t)i + 1] = out->ante_off[(size_t)i] + sel[(size_t)i].asz;
    out->cons_off[(size_t)i + 1] = out->cons_off[(size_t)i] + sel[(size_t)i].csz;
  }
  out->ante.resize((size_t)out->ante_off[(size_t)keep]);
  out->cons.resize((size_t)out->cons_off[(size_t)keep]);
  for (auto* v : {&out->cS, &out->cA, &out->cC}) v->resize((size_t)keep);
  for (auto* v : {&out->support, &out->conf, &out->lift, &out->leverage, &out->conviction}) v->resize((size_t)keep);
  parallel_for(keep, nthreads, 4096, [&](int64_t b0, int64_t e0, int) {
    for (int64_t i = b0; i < e0; ++i) {
      const Sel& r = sel[(size_t)i];
      const int32_t* a = rows_all + base[r.asz] + (int64_t)r.aidx * r.asz;
      const int32_t* c = rows_all + base[r.csz] + (int64_t)r.cidx * r.csz;
      std::copy(a, a + r.asz, out->ante.begin() + out->ante_off[(size_t)i]);
      std::copy(c, c + r.csz, out->cons.begin() + out->cons_off[(size_t)i]);
      out->cS[i] = r.cS; out->cA[i] = r.cA; out->cC[i] = r.cC;
      out->support[i] = rm_support(r.cS, N);
      out->conf[i] = rm_confidence(r.cS, r.cA);
      out->lift[i] = rm_lift(r.cS, r.cA, r.cC, N);
      out->leverage[i] = rm_leverage(r.cS, r.cA, r.cC, N);
      out->conviction[i] = rm_conviction(r.cS, r.cA, r.cC, N);
    }
  });
  *n_rules = keep;
  return out;
}

FA_API int64_t fa_rule_splits_nante(RuleSplitSet* h) { return (int64_t)h->ante.size(); }
FA_API int64_t fa_rule_splits_ncons(RuleSplitSet* h) { return (int64_t)h->cons.size(); }

// every array holds R elements (ante_off / cons_off R+1, ante / cons the two totals above)
FA_API void fa_rule_splits_export(RuleSplitSet* h, int64_t* ante_off, int32_t* ante, int64_t* cons_off, int32_t* cons,
                                  int64_t* cS, int64_t* cA, int64_t* cC, double* support, double* conf, double* lift,
                                  double* leverage, double* conviction) {
  auto put = [](auto* dst, const auto& v) {
    if (!v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(v[0]));
  };
  put(ante_off, h->ante_off); put(ante, h->ante); put(cons_off, h->cons_off); put(cons, h->cons);
  put(cS, h->cS); put(cA, h->cA); put(cC, h->cC);
  put(support, h->support); put(conf, h->conf); put(lift, h->lift);
  put(leverage, h->leverage); put(conviction, h->conviction);
}

FA_API void fa_rule_splits_free(RuleSplitSet* h) { delete h; }
