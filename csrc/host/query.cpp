// The query counter's host side (no counterpart in the reference): the window plan of
// csrc/hip/query.hip k_query_slab and the C++ reference that counts the same plan over
// the same raw rows.  Limits and the LDS rule: fa_query.h.
#include <memory>

#include "fa_common.h"
#include "fa_query.h"

namespace fa {

struct QueryPlan {
  int err = 0;                   // 0, or 1: a single query does not fit a window at width 1
  int64_t bad_query = -1, bad_len = 0, cap1 = 0;
  int64_t n_used = 0, n_live = 0;
  std::vector<QWin> wins;
  std::vector<uint16_t> tab;     // [W][n_used]: used index -> slab row, kQAbsent outside the window
  std::vector<int32_t> qoff;     // per window n_q + 1 entries, relative to the window's qrow slice
  std::vector<uint16_t> qrow;
  std::vector<int64_t> perm;     // plan order -> the caller's query index
};

// the most items of a window of n_q queries at width 1 within lds bytes
static int64_t item_cap(int64_t n_q, int64_t lds) {
  const int64_t fixed = query_lds_bytes(0, 1, n_q);
  if (fixed > lds) return 0;
  return std::min<int64_t>(kQMaxItems, (lds - fixed) / 8);
}

}  // namespace fa

using namespace fa;

// The limits by name (fa_query.h), entry i; nullptr past the end.
FA_API const char* fa_query_limits(int i, int64_t* value) {
  struct Entry { const char* name; int64_t value; };
  static const Entry table[] = {
#define FA_QUERY_X(name, value) {#name, value},
      FA_QUERY_LIMITS(FA_QUERY_X)
#undef FA_QUERY_X
  };
  if (i < 0 || i >= (int)(sizeof(table) / sizeof(table[0]))) return nullptr;
  *value = table[i].value;
  return table[i].name;
}

// fa_query.h's LDS footprint of a window and the width the rule gives it (0: none fits)
FA_API int64_t fa_query_lds_bytes(int64_t n_items, int64_t sw, int64_t n_q) {
  return query_lds_bytes(n_items, sw, n_q);
}
FA_API int fa_query_width(int64_t n_items, int64_t n_q, int64_t lds) { return query_width(n_items, n_q, lds); }

// The window cut.  Input: Q live queries as a CSR (off int64 [Q + 1], idx int32) of used
// indices in [0, n_used), distinct and ASCENDING inside a query, every query with at
// least one; index[i] is query i's place in the caller's count vector.  Queries are
// sorted lexicographically by their index lists, so neighbours share items, and cut
// greedily: a window closes when the next query would make it exceed `acc` queries
// (1 .. kQAcc) or the item capacity at width 1 within `lds` bytes.  A closed window takes
// the widest slab that fits (query_width), its items in ascending order are its slab rows.
// A query that does not fit a window alone sets the plan's error (fa_query_plan_info).
FA_API void* fa_query_plan(const int64_t* off, const int32_t* idx, const int64_t* index, int64_t Q, int64_t n_used,
                           int64_t acc, int64_t lds) {
  auto P = std::make_unique<QueryPlan>();
  P->n_used = n_used;
  P->n_live = Q;
  acc = std::max<int64_t>(1, std::min<int64_t>(acc, kQAcc));
  lds = std::min<int64_t>(lds, kQLdsMax);
  std::vector<int64_t> order(Q);
  for (int64_t i = 0; i < Q; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
    const bool lt = std::lexicographical_compare(idx + off[a], idx + off[a + 1], idx + off[b], idx + off[b + 1]);
    if (lt) return true;
    const bool gt = std::lexicographical_compare(idx + off[b], idx + off[b + 1], idx + off[a], idx + off[a + 1]);
    return !gt && a < b;
  });
  const int64_t cap1 = item_cap(1, lds);
  P->cap1 = cap1;
  std::vector<int64_t> stamp(std::max<int64_t>(n_used, 1), -1);   // the window that last took the item
  std::vector<int32_t> win_items;
  int64_t w0 = 0;                                                  // first query (in order) of the open window
  auto close = [&](int64_t w1) {
    if (w1 == w0) return;
    QWin w{};
    w.n_q = w1 - w0;
    w.n_items = (int64_t)win_items.size();
    w.sw = query_width(w.n_items, w.n_q, lds);
    w.tab_off = (int64_t)P->tab.size();
    w.qoff_off = (int64_t)P->qoff.size();
    w.qrow_off = (int64_t)P->qrow.size();
    w.q_base = (int64_t)P->perm.size();
    std::sort(win_items.begin(), win_items.end());
    P->tab.resize(P->tab.size() + n_used, (uint16_t)kQAbsent);
    uint16_t* tab = P->tab.data() + w.tab_off;
    for (size_t r = 0; r < win_items.size(); ++r) tab[win_items[r]] = (uint16_t)r;
    int32_t o = 0;
    for (int64_t s = w0; s < w1; ++s) {
      const int64_t q = order[s];
      P->qoff.push_back(o);
      for (int64_t x = off[q]; x < off[q + 1]; ++x) P->qrow.push_back(tab[idx[x]]);
      o += (int32_t)(off[q + 1] - off[q]);
      P->perm.push_back(index[q]);
    }
    P->qoff.push_back(o);
    P->wins.push_back(w);
    win_items.clear();
    w0 = w1;
  };
  for (int64_t s = 0; s < Q; ++s) {
    const int64_t q = order[s], len = off[q + 1] - off[q];
    if (len < 1 || len > cap1) {
      P->err = 1;
      P->bad_query = index[q];
      P->bad_len = len;
      return P.release();
    }
    const int64_t wid = (int64_t)P->wins.size();
    int64_t fresh = 0;
    for (int64_t x = off[q]; x < off[q + 1]; ++x) fresh += stamp[idx[x]] != wid;
    const int64_t nq = s - w0 + 1;
    if (nq > acc || (int64_t)win_items.size() + fresh > item_cap(nq, lds)) close(s);
    const int64_t cur = (int64_t)P->wins.size();
    for (int64_t x = off[q]; x < off[q + 1]; ++x)
      if (stamp[idx[x]] != cur) {
        stamp[idx[x]] = cur;
        win_items.push_back(idx[x]);
      }
  }
  close(Q);
  return P.release();
}

// info[0..8): error, the offending query and its length, the item capacity of a lone
// query, windows, and the lengths of tab, qoff, qrow (perm has the live queries' count)
FA_API void fa_query_plan_info(const void* h, int64_t* info) {
  const QueryPlan* P = (const QueryPlan*)h;
  info[0] = P->err;
  info[1] = P->bad_query;
  info[2] = P->bad_len;
  info[3] = P->cap1;
  info[4] = (int64_t)P->wins.size();
  info[5] = (int64_t)P->tab.size();
  info[6] = (int64_t)P->qoff.size();
  info[7] = (int64_t)P->qrow.size();
}

FA_API void fa_query_plan_export(const void* h, int64_t* wins, uint16_t* tab, int32_t* qoff, uint16_t* qrow,
                                 int64_t* perm) {
  const QueryPlan* P = (const QueryPlan*)h;
  if (!P->wins.empty()) memcpy(wins, P->wins.data(), P->wins.size() * sizeof(QWin));
  if (!P->tab.empty()) memcpy(tab, P->tab.data(), P->tab.size() * sizeof(uint16_t));
  if (!P->qoff.empty()) memcpy(qoff, P->qoff.data(), P->qoff.size() * sizeof(int32_t));
  if (!P->qrow.empty()) memcpy(qrow, P->qrow.data(), P->qrow.size() * sizeof(uint16_t));
  if (!P->perm.empty()) memcpy(perm, P->perm.data(), P->perm.size() * sizeof(int64_t));
}

FA_API void fa_query_plan_free(void* h) { delete (QueryPlan*)h; }

// The C++ reference on the device launcher's inputs (all in host memory): counts of every
// window's queries over the rows [0, n_rows), added into out.  Per window: the queries
// hang on the smallest of their slab rows; a thread marks a line's items of the window in
// its own array (the line's index + 1 as the mark, so nothing is cleared between lines)
// and, for every marked item, tests the queries hanging on it against the marks.  Rows go
// to the pool in chunks; every thread keeps its own counts and adds them at the end.
// Returns 0, or 3 for a window outside fa_query.h's limits (lds as the launcher's).
FA_API int fa_query_count_cpu(const int64_t* offsets, const int32_t* items, int64_t n_rows, const int32_t* lut,
                              int64_t lut_n, const int64_t* wins, int64_t W, const uint16_t* tab,
                              const int32_t* qoff, const uint16_t* qrow, const int64_t* perm, uint64_t* out,
                              int64_t lds, int nthreads) {
  if (W < 0 || n_rows < 0 || lut_n < 0 || lds < 0 || lds > kQLdsMax) return 3;
  for (int64_t i = 0; i < W; ++i) {
    const QWin* w = (const QWin*)wins + i;
    if (!query_window_ok(w->n_q, w->n_items, w->sw, lds)) return 3;
  }
  nthreads = std::max(1, nthreads);
  for (int64_t wi = 0; wi < W; ++wi) {
    const QWin w = ((const QWin*)wins)[wi];
    const uint16_t* wtab = tab + w.tab_off;
    const int32_t* wqoff = qoff + w.qoff_off;
    const uint16_t* wqrow = qrow + w.qrow_off;
    // queries by their smallest slab row: head[r] .. head[r + 1] in byrow
    std::vector<int32_t> head(w.n_items + 1, 0), byrow(w.n_q), first(w.n_q);
    for (int64_t q = 0; q < w.n_q; ++q) {
      uint16_t m = wqrow[wqoff[q]];
      for (int32_t x = wqoff[q]; x < wqoff[q + 1]; ++x) m = std::min(m, wqrow[x]);
      first[q] = m;
      ++head[m + 1];
    }
    for (int64_t r = 0; r < w.n_items; ++r) head[r + 1] += head[r];
    {
      std::vector<int32_t> fill(head.begin(), head.end() - 1);
      for (int64_t q = 0; q < w.n_q; ++q) byrow[fill[first[q]]++] = (int32_t)q;
    }
    std::vector<std::vector<int64_t>> mark(nthreads), cnt(nthreads);
    parallel_for(n_rows, nthreads, 4096, [&](int64_t b, int64_t e, int tid) {
      std::vector<int64_t>& mk = mark[tid];
      std::vector<int64_t>& c = cnt[tid];
      if (mk.empty()) {
        mk.assign(w.n_items, 0);
        c.assign(w.n_q, 0);
      }
      for (int64_t row = b; row < e; ++row) {
        const int64_t m = row + 1;
        for (int64_t p = offsets[row]; p < offsets[row + 1]; ++p) {
          const int64_t id = items[p];
          if (id < 0 || id >= lut_n || lut[id] < 0) continue;
          const uint16_t r = wtab[lut[id]];
          if (r != (uint16_t)kQAbsent) mk[r] = m;
        }
        for (int64_t p = offsets[row]; p < offsets[row + 1]; ++p) {
          const int64_t id = items[p];
          if (id < 0 || id >= lut_n || lut[id] < 0) continue;
          const uint16_t r = wtab[lut[id]];
          if (r == (uint16_t)kQAbsent) continue;
          for (int32_t j = head[r]; j < head[r + 1]; ++j) {
            const int32_t q = byrow[j];
            bool all = true;
            for (int32_t x = wqoff[q]; x < wqoff[q + 1] && all; ++x) all = mk[wqrow[x]] == m;
            c[q] += all;
          }
        }
      }
    });
    for (int t = 0; t < nthreads; ++t)
      if (!cnt[t].empty())
        for (int64_t q = 0; q < w.n_q; ++q) out[perm[w.q_base + q]] += (uint64_t)cnt[t][q];
  }
  return 0;
}
