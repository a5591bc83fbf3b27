// Regrouping of a one-pass device bundle: every candidate under its best parent, not its
// lexicographic prefix (the rule and its reasons: ../host/fa_regroup.h; the host model the
// tests hold this file to: ../host/regroup.cpp).
//
// It sits between the generator chain (gen.hip fa_hip_dl_more) and the piece plan
// (levels.hip fa_hip_dl_plan): per level it rewrites the generator's extension lists
// (cnt, off, ext ids) over the SAME parent rows P -- a parent is a (k-1)-subset that is a
// row of P, and rows that end without children simply have cnt 0 -- so the plan kernels,
// their row order, their size buckets and the lane deal run on the regrouped level table
// unchanged.  Candidates are renumbered off'[p] + rank: contiguous per parent, hence per
// piece (count.hip's single-writer byte accumulators), and perm[new] = old lets
// k_dl_unpermute put the counts back in the generator's order before anything downstream
// reads them.
//
// One workgroup per level (levels are independent), the rounds' counters in LDS, ordinary
// barriers only: no workgroup waits for another.
#include "fa_hip.h"
#include "../host/fa_dl.h"
#include "../host/fa_regroup.h"

namespace fa {

constexpr int kRgThreads = 1024;
constexpr int kRgW = kRgThreads / 64;

// One level: the generator's table and the level's scratch (rg_scratch_bytes):
//   par int32 [C][m + 1], asg [C], cho [C], tmp [C], cnt_out [n + C] (ext ids at
//   cnt_out + n, as DlDesc.cnt), then off_out int64 [n + 1]
struct RgLv {
  const int32_t* P;
  const int32_t* cnt;
  const int64_t* off;
  const int32_t* rows;
  char* scr;
  int64_t n, C, base;
  int64_t m;
};
struct RgArgs {
  RgLv lv[kDlMaxL];
  int32_t* perm;          // [bundle candidates]
  long long* stats;       // [L][4]: prefix pieces, the rule's pieces, rounds, 1 = kept the prefix plan
};

__host__ __device__ inline int64_t rg_scratch_ints(int64_t n, int64_t C, int64_t m) {
  return ((C * (m + 5) + n) + 1) & ~(int64_t)1;
}
__host__ __device__ inline int64_t rg_scratch_bytes(int64_t n, int64_t C, int64_t m) {
  return (4 * rg_scratch_ints(n, C, m) + 8 * (n + 1) + 255) & ~(int64_t)255;
}

__device__ __forceinline__ int rg_find(const int32_t* __restrict__ P, int n, int m, const int32_t* __restrict__ s,
                                       int j) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const int r = cmp_skip(P + (int64_t)mid * m, s, m + 1, j);
    if (r == 0) return mid;
    if (r < 0) lo = mid + 1; else hi = mid;
  }
  return -1;
}

__global__ __launch_bounds__(kRgThreads) void k_dl_regroup(const RgArgs A) {
  extern __shared__ int rg_lds[];          // u, u2, v: [n] each
  __shared__ int sh[2 * kRgW];
  __shared__ int fired;
  const RgLv& V = A.lv[blockIdx.x];
  const int tid = threadIdx.x;
  const int64_t C = V.C, base = V.base;
  if (V.n > kRgMaxRows) {                  // (the launcher keeps this level's table)
    for (int64_t c = tid; c < C; c += kRgThreads) A.perm[base + c] = (int32_t)(base + c);
    int pp = 0;
    for (int64_t i = tid; i < V.n; i += kRgThreads) pp += (V.cnt[i] + 7) >> 3;
    pp = wg_sum<kRgW>(pp, sh);
    if (tid == 0) {
      long long* s = A.stats + 4 * blockIdx.x;
      s[0] = s[1] = pp; s[2] = 0; s[3] = 1;
    }
    return;
  }
  const int n = (int)V.n, m = (int)V.m, k = m + 1;
  int32_t* const par = reinterpret_cast<int32_t*>(V.scr);
  int32_t* const asg = par + C * k;
  int32_t* const cho = asg + C;
  int32_t* const tmp = cho + C;
  int32_t* const cnt_out = tmp + C;
  int32_t* const ex_out = cnt_out + n;
  int64_t* const off_out = reinterpret_cast<int64_t*>(V.scr + 4 * rg_scratch_ints(n, C, m));
  int* u = rg_lds;
  int* u2 = rg_lds + n;
  int* const v = rg_lds + 2 * n;
  for (int i = tid; i < 3 * n; i += kRgThreads) rg_lds[i] = 0;
  if (tid == 0) fired = 0;
  __syncthreads();
  // Candidate c is always handled by thread c mod kRgThreads: par, asg and cho are that
  // thread's own data; only the LDS counters are shared.
  for (int64_t c = tid; c < C; c += kRgThreads) {
    const int32_t* s = V.rows + c * k;
    int lo = 0, hi = n;                    // the prefix row: the last i with off[i] <= c
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (V.off[mid] <= c) lo = mid + 1; else hi = mid;
    }
    for (int j = 0; j < m; ++j) par[c * k + j] = rg_find(V.P, n, m, s, j);
    par[c * k + m] = lo - 1;
    asg[c] = -1;
    for (int j = 0; j < k; ++j) {
      const int p = par[c * k + j];
      if (p >= 0) atomicAdd(&u[p], 1);
    }
  }
  __syncthreads();
  int rounds = 0;
  for (int t = 0; t < kRgNThr; ++t) {
    const int thr = rg_thr(t);
    for (;;) {
      ++rounds;
      // votes: the parent with the most unassigned children, at least thr of them
      for (int64_t c = tid; c < C; c += kRgThreads) {
        if (asg[c] >= 0) continue;
        int best = -1, bp = -1;
        for (int j = k - 1; j >= 0; --j) {
          const int p = par[c * k + j];
          if (p < 0) continue;
          const int uu = u[p];
          if (uu >= thr && uu > best) { best = uu; bp = p; }
        }
        cho[c] = bp;
        if (bp >= 0) atomicAdd(&v[bp], 1);
      }
      __syncthreads();
      // a parent with >= thr votes takes its voters; the others are counted again (u2)
      for (int64_t c = tid; c < C; c += kRgThreads) {
        if (asg[c] >= 0) continue;
        const int bp = cho[c];
        if (bp >= 0 && v[bp] >= thr) {
          asg[c] = bp;
          fired = 1;
          continue;
        }
        for (int j = 0; j < k; ++j) {
          const int p = par[c * k + j];
          if (p >= 0) atomicAdd(&u2[p], 1);
        }
      }
      __syncthreads();
      const int f = fired;
      __syncthreads();
      if (tid == 0) fired = 0;
      if (f) { int* x = u; u = u2; u2 = x; }       // (nothing assigned: u still holds)
      for (int i = tid; i < n; i += kRgThreads) { u2[i] = 0; v[i] = 0; }
      __syncthreads();
      if (!f) break;
    }
  }
  // children per parent, and the piece counts of the two plans
  for (int64_t c = tid; c < C; c += kRgThreads) atomicAdd(&v[asg[c]], 1);
  __syncthreads();
  int pc[2] = {0, 0}, tot[2];
  for (int i = tid; i < n; i += kRgThreads) {
    pc[0] += (v[i] + 7) >> 3;
    pc[1] += (V.cnt[i] + 7) >> 3;
  }
  wg_sum<kRgW>(pc, sh, tot);
  const bool keep = tot[0] >= tot[1];              // not cheaper: the level keeps the prefix plan
  __syncthreads();
  if (keep) {
    for (int i = tid; i < n; i += kRgThreads) v[i] = 0;
    __syncthreads();
    for (int64_t c = tid; c < C; c += kRgThreads) {
      asg[c] = par[c * k + m];
      atomicAdd(&v[asg[c]], 1);
    }
    __syncthreads();
  }
  for (int i = tid; i < n; i += kRgThreads) cnt_out[i] = v[i];
  wg_scan_chunks<kRgW>(
      (int64_t)n, (int64_t)0, sh, [&](int64_t i) { return v[i]; },
      [&](int64_t i, int64_t before, int) { off_out[i] = before; });
  if (tid == 0) off_out[n] = C;
  // a parent's children in any order (u2 is all zero: the cursors), then every child's
  // rank among them by candidate index: the numbering does not depend on that order
  for (int64_t c = tid; c < C; c += kRgThreads) {
    const int p = asg[c];
    tmp[off_out[p] + atomicAdd(&u2[p], 1)] = (int32_t)c;
  }
  __syncthreads();
  for (int64_t c = tid; c < C; c += kRgThreads) {
    const int p = asg[c];
    const int64_t o = off_out[p];
    const int a = v[p];
    int r = 0;
    for (int q = 0; q < a; ++q) r += tmp[o + q] < (int32_t)c ? 1 : 0;
    int j = m;                                     // the item left out of the parent
    if (!keep)
      for (j = k - 1; j > 0 && par[c * k + j] != p; --j) {}
    ex_out[o + r] = V.rows[c * k + j];
    A.perm[base + o + r] = (int32_t)(base + c);
  }
  if (tid == 0) {
    long long* s = A.stats + 4 * blockIdx.x;
    s[0] = tot[1]; s[1] = tot[0]; s[2] = rounds; s[3] = keep ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void k_dl_unpermute(const uint32_t* __restrict__ in, const int32_t* __restrict__ perm,
                                                      int64_t C, uint32_t* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < C) out[perm[e]] = in[e];
}

static inline int64_t rg_al(int64_t b) { return (b + 255) & ~(int64_t)255; }

static bool rg_eligible(const DlDesc* desc, int L) {
  if (L < 1 || L > kDlMaxL) return false;
  for (int l = 0; l < L; ++l)
    if (desc[l].m < 1 || desc[l].m > kDlInline || desc[l].n < 1 || desc[l].C < 1 || desc[l].C > INT32_MAX / 64)
      return false;
  return true;
}

}  // namespace fa

using namespace fa;

// Scratch bytes of fa_hip_dl_regroup for these levels; 0: the bundle does not regroup
// (a prefix past kDlInline ids).
FA_API int64_t fa_hip_dl_regroup_need(const DlDesc* desc, int L) {
  if (!rg_eligible(desc, L)) return 0;
  int64_t C = 0, b = 0;
  for (int l = 0; l < L; ++l) {
    C += desc[l].C;
    if (desc[l].n <= kRgMaxRows) b += rg_scratch_bytes(desc[l].n, desc[l].C, desc[l].m);
  }
  return rg_al(4 * C) + b;
}

// Regroups the bundle desc [L] into out [L] (the same parent rows, candidate rows, m, n, C
// and base; cnt and off in scratch) and perm (device int32 [C] at the start of scratch:
// perm[new bundle index] = the generator's).  stats: device int64 [L][4] out, per level the
// prefix plan's pieces, the rule's, rounds, 1 = the level kept the prefix plan (the post
// step: the control block's kRgStats slots).  Returns 0, 1 (not eligible, or scratch too
// small) or the launch's error.
FA_API int fa_hip_dl_regroup(const DlDesc* desc, int L, void* scratch, int64_t bytes, DlDesc* out, long long* stats,
                             hipStream_t st) {
  const int64_t need = fa_hip_dl_regroup_need(desc, L);
  if (need == 0 || scratch == nullptr || stats == nullptr || bytes < need) return 1;
  int64_t C = 0;
  for (int l = 0; l < L; ++l) C += desc[l].C;
  RgArgs A{};
  char* w = static_cast<char*>(scratch);
  A.perm = reinterpret_cast<int32_t*>(w);
  w += rg_al(4 * C);
  A.stats = stats;
  int64_t n_max = 1;
  for (int l = 0; l < L; ++l) {
    const DlDesc& d = desc[l];
    RgLv& V = A.lv[l];
    V.P = reinterpret_cast<const int32_t*>((intptr_t)d.P);
    V.cnt = reinterpret_cast<const int32_t*>((intptr_t)d.cnt);
    V.off = reinterpret_cast<const int64_t*>((intptr_t)d.off);
    V.rows = reinterpret_cast<const int32_t*>((intptr_t)d.rows);
    V.n = d.n; V.C = d.C; V.base = d.base; V.m = d.m;
    V.scr = w;
    out[l] = d;
    if (d.n > kRgMaxRows) continue;
    n_max = std::max(n_max, d.n);
    int32_t* cnt_out = reinterpret_cast<int32_t*>(w) + d.C * (d.m + 1) + 3 * d.C;
    out[l].cnt = (int64_t)(intptr_t)cnt_out;
    out[l].off = (int64_t)(intptr_t)(w + 4 * rg_scratch_ints(d.n, d.C, d.m));
    w += rg_scratch_bytes(d.n, d.C, d.m);
  }
  const size_t lds = 3 * sizeof(int) * (size_t)n_max;
  static bool lds_set = false;               // once: the most a level may take
  if (!lds_set) {
    const hipError_t e = hipFuncSetAttribute((const void*)k_dl_regroup, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(3 * sizeof(int) * kRgMaxRows));
    if (e != hipSuccess) return (int)e;
    lds_set = true;
  }
  hipLaunchKernelGGL(k_dl_regroup, dim3((unsigned)L), dim3(kRgThreads), lds, st, A);
  FA_LAUNCH_RET();
}

// out[perm[e]] = in[e], e < C: the counts of a regrouped plan back in the generator's order
FA_API int fa_hip_dl_unpermute(const uint32_t* in, const int32_t* perm, int64_t C, uint32_t* out, hipStream_t st) {
  if (C < 1) return 1;
  hipLaunchKernelGGL(k_dl_unpermute, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, in, perm, C, out);
  FA_LAUNCH_RET();
}
