// Host model of the device bundles' regrouping step (the rule: fa_regroup.h; the device
// step: csrc/hip/regroup.hip, which must give exactly these parents, extension lists and
// permutation).  Sequential and plain: it is the statement of the rule that the tests
// hold the kernels to, not a fast path.
#include <algorithm>
#include <vector>

#include "fa_common.h"
#include "fa_dl.h"
#include "fa_regroup.h"

namespace fa {

// One level of a bundle in the generator's form (DlDesc: parent rows, extensions per
// row, their offsets, the extension ids in row order) and the regrouped level's.
struct RgLevel {
  const int32_t* P;      // parent rows [n][m]
  const int32_t* cnt;    // extensions per parent row [n]
  const int64_t* off;    // exclusive offsets of cnt [n + 1]
  const int32_t* ex;     // extension ids [C]
  int64_t n, C, m;
  int32_t* cnt_out;      // [n]
  int64_t* off_out;      // [n + 1]
  int32_t* ex_out;       // [C]
  int32_t* perm;         // [C]: perm[new index] = old index (both level-local)
  // out: prefix plan's pieces, the rule's pieces (before the fallback), rounds, 1 = the
  // level keeps the prefix plan
  int64_t pieces_prefix, pieces_rule, rounds, kept_prefix;
};
static_assert(sizeof(RgLevel) == 15 * 8, "RgLevel layout (ops.host.RgLevelC)");

static int64_t rg_find(const int32_t* P, int64_t n, int m, const int32_t* s, int j) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const int r = rg_cmp_skip(P + mid * m, s, m + 1, j);
    if (r == 0) return mid;
    if (r < 0) lo = mid + 1; else hi = mid;
  }
  return -1;
}

static int64_t rg_pieces(const std::vector<int32_t>& a) {
  int64_t p = 0;
  for (int32_t c : a) p += (c + 7) / 8;
  return p;
}

// regroup: false = only the prefix plan in the output form (the bundle's fallback)
static void rg_level(RgLevel& lv, bool regroup) {
  const int64_t n = lv.n, C = lv.C;
  const int m = (int)lv.m, k = m + 1;
  std::vector<int64_t> pre(C), asg(C, -1), par;
  for (int64_t i = 0; i < n; ++i)
    for (int64_t c = lv.off[i]; c < lv.off[i] + lv.cnt[i]; ++c) pre[c] = i;
  std::vector<int32_t> a_pre(lv.cnt, lv.cnt + n);
  lv.pieces_prefix = lv.pieces_rule = rg_pieces(a_pre);
  lv.rounds = 0;
  lv.kept_prefix = 1;
  if (regroup && n <= kRgMaxRows) {
    par.assign(C * k, -1);
    std::vector<int32_t> row(k);
    for (int64_t c = 0; c < C; ++c) {
      std::copy(lv.P + pre[c] * m, lv.P + pre[c] * m + m, row.begin());
      row[m] = lv.ex[c];
      for (int j = 0; j < m; ++j) par[c * k + j] = rg_find(lv.P, n, m, row.data(), j);
      par[c * k + m] = pre[c];
    }
    std::vector<int32_t> u(n), v(n);
    std::vector<int64_t> cho(C);
    for (int t = 0; t < kRgNThr; ++t) {
      const int thr = rg_thr(t);
      for (;;) {
        ++lv.rounds;
        std::fill(u.begin(), u.end(), 0);
        std::fill(v.begin(), v.end(), 0);
        for (int64_t c = 0; c < C; ++c)
          if (asg[c] < 0)
            for (int j = 0; j < k; ++j)
              if (par[c * k + j] >= 0) ++u[par[c * k + j]];
        for (int64_t c = 0; c < C; ++c) {
          if (asg[c] >= 0) continue;
          int best = -1;
          int64_t bp = -1;
          for (int j = k - 1; j >= 0; --j) {
            const int64_t p = par[c * k + j];
            if (p >= 0 && u[p] >= thr && u[p] > best) { best = u[p]; bp = p; }
          }
          cho[c] = bp;
          if (bp >= 0) ++v[bp];
        }
        bool fired = false;
        for (int64_t c = 0; c < C; ++c)
          if (asg[c] < 0 && cho[c] >= 0 && v[cho[c]] >= thr) { asg[c] = cho[c]; fired = true; }
        if (!fired) break;
      }
    }
    std::vector<int32_t> a(n, 0);
    for (int64_t c = 0; c < C; ++c) ++a[asg[c]];
    lv.pieces_rule = rg_pieces(a);
    lv.kept_prefix = lv.pieces_rule < lv.pieces_prefix ? 0 : 1;
  }
  if (lv.kept_prefix) asg = pre;
  std::fill(lv.cnt_out, lv.cnt_out + n, 0);
  for (int64_t c = 0; c < C; ++c) ++lv.cnt_out[asg[c]];
  lv.off_out[0] = 0;
  for (int64_t i = 0; i < n; ++i) lv.off_out[i + 1] = lv.off_out[i] + lv.cnt_out[i];
  std::vector<int64_t> cur(lv.off_out, lv.off_out + n);
  for (int64_t c = 0; c < C; ++c) {      // candidate order inside every parent
    const int64_t p = asg[c], at = cur[p]++;
    int j = m;                           // the item left out: the prefix's is the extension
    if (!lv.kept_prefix)
      for (j = k - 1; j > 0 && par[c * k + j] != p; --j) {}
    lv.ex_out[at] = j == m ? lv.ex[c] : lv.P[pre[c] * m + j];
    lv.perm[at] = (int32_t)c;
  }
}

}  // namespace fa

using namespace fa;

// The regrouped plan of a bundle's L levels.  Returns 1 when the bundle regroups, 0 when
// it keeps the prefix plan as a whole (a level with a prefix past kDlInline ids); the
// outputs are filled either way.
FA_API int fa_dl_regroup(RgLevel* lv, int L) {
  bool ok = true;
  for (int l = 0; l < L; ++l) ok = ok && lv[l].m <= kDlInline;
  for (int l = 0; l < L; ++l) rg_level(lv[l], ok);
  return ok ? 1 : 0;
}

// the rule's constants for Python: 0 kRgMaxRows, 1 kRgStats
FA_API int64_t fa_dl_regroup_const(int i) { return i == 0 ? kRgMaxRows : i == 1 ? kRgStats : -1; }
