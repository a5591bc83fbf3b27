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
// Two kernels:
//   k_dl_rg_parents   the parent search, one thread per (candidate, position) of every level
//                     of the bundle: independent binary searches spread over the whole chip
//   k_dl_rg_rounds    the rounds and the numbering, one workgroup per level (levels are
//                     independent), ordinary barriers only: no workgroup waits for another.
//                     Counters, parent lists and the list of unassigned candidates in LDS
//                     (fa_regroup.h rg_lds_fits; a level whose lists do not fit reads them
//                     from its global scratch, with the same result).
#include <algorithm>
#include <type_traits>

#include "fa_hip.h"
#include "../host/fa_dl.h"
#include "../host/fa_regroup.h"

namespace fa {

constexpr int kRgThreads = 1024;
constexpr int kRgW = kRgThreads / 64;
constexpr int kRgPThreads = 256;           // k_dl_rg_parents
constexpr uint16_t kRgNone = 0xFFFF;       // par: not a row of P

// One level: the generator's table and the level's scratch (rg_scratch_bytes):
//   cnt_out int32 [n], ext ids int32 [C] (at cnt_out + n, as DlDesc.cnt), off_out int64 [n + 1],
//   par uint16 [m + 1][C] (position-major: a wave reads consecutive candidates), list int32 [C + 7]
//   (the unassigned candidates, then a parent's children, of a level whose lists are not in LDS)
struct RgLv {
  const int32_t* P;
  const int32_t* cnt;
  const int64_t* off;
  const int32_t* rows;
  char* scr;
  int64_t n, C, base;
  int32_t m;
  uint32_t blk0;          // k_dl_rg_parents: the level's first workgroup
};
struct RgArgs {
  RgLv lv[kDlMaxL];
  int32_t* perm;          // [bundle candidates]
  long long* stats;       // [L][4]: prefix pieces, the rule's pieces, rounds, 1 = kept the prefix plan
  int64_t lds_cap;        // rg_lds_fits' cap
  long long* phase;       // a probe's phase timers, [L][4] (or null): wall_clock64 at a level's start, after
                          // the setup, after the rounds and at the end of k_dl_rg_rounds
  int32_t L;
};
static_assert(sizeof(RgArgs) <= 4096, "kernel arguments");

__host__ __device__ inline int64_t rg_off_at(int64_t n, int64_t C) { return (4 * (n + C) + 7) & ~(int64_t)7; }
__host__ __device__ inline int64_t rg_par_at(int64_t n, int64_t C) { return rg_al16(rg_off_at(n, C) + 8 * (n + 1)); }
__host__ __device__ inline int64_t rg_list_at(int64_t n, int64_t C, int64_t m) {
  return rg_al16(rg_par_at(n, C) + 2 * C * (m + 1));
}
__host__ __device__ inline int64_t rg_scratch_bytes(int64_t n, int64_t C, int64_t m) {
  return (rg_list_at(n, C, m) + 4 * ((C + 7) & ~(int64_t)7) + 255) & ~(int64_t)255;   // (read 8 entries at a time)
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

// par[j][c] of every level with at most kRgMaxRows parent rows; element e = j C + c of a
// level is thread e of the level's workgroups (blk0 ..).
__global__ __launch_bounds__(kRgPThreads) void k_dl_rg_parents(const RgArgs A) {
  int l = 0;
  while (l + 1 < A.L && blockIdx.x >= A.lv[l + 1].blk0) ++l;   // (a level without workgroups shares its blk0 with the next)
  const RgLv& V = A.lv[l];
  const int n = (int)V.n, m = V.m, C = (int)V.C;
  if (V.n > kRgMaxRows) return;
  const int64_t e = (int64_t)(blockIdx.x - V.blk0) * kRgPThreads + threadIdx.x;
  if (e >= (int64_t)C * (m + 1)) return;
  const int j = (int)((uint32_t)e / (uint32_t)C), c = (int)e - j * C;   // (C (m + 1) < 2^31: rg_eligible)
  int r;
  if (j < m) {
    r = rg_find(V.P, n, m, V.rows + (int64_t)c * (m + 1), j);
  } else {                                   // the prefix row: the last i with off[i] <= c
    int lo = 0, hi = n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (V.off[mid] <= c) lo = mid + 1; else hi = mid;
    }
    r = lo - 1;
  }
  reinterpret_cast<uint16_t*>(V.scr + rg_par_at(n, C))[e] = r < 0 ? kRgNone : (uint16_t)r;
}

// 16-bit counters, two to a word: counter p is half p & 1 of word p >> 1
__device__ __forceinline__ void pk_inc(uint32_t* a, int p) { atomicAdd(&a[p >> 1], 1u << (16 * (p & 1))); }
__device__ __forceinline__ int pk_get(const uint32_t* a, int p) {
  return (int)reinterpret_cast<const uint16_t*>(a)[p];
}

// The vote of candidate c: the parent with the most unassigned children, at least thr of them
// (ties: the largest j; -1: none).  All of c's parents are read before any of their counters:
// two LDS latencies per candidate, not two per position.  ps: c's parents.  K = m + 1 is a
// template parameter (2 .. kRgMaxK): the loops unroll to what the level needs.
constexpr int kRgMaxK = kDlInline + 1;
template <int K>
__device__ __forceinline__ int rg_vote(const uint16_t* par, const uint32_t* u, int C, int thr, int c, int (&ps)[K]) {
#pragma unroll
  for (int j = 0; j < K; ++j) ps[j] = (int)par[j * C + c];
  int us[K];
#pragma unroll
  for (int j = 0; j < K; ++j) us[j] = ps[j] != kRgNone ? pk_get(u, ps[j]) : -1;
  int best = -1, bp = -1;
#pragma unroll
  for (int j = K - 1; j >= 0; --j)
    if (us[j] >= thr && us[j] > best) { best = us[j]; bp = ps[j]; }
  return bp;
}

// 8 consecutive list entries (16-byte aligned)
__device__ __forceinline__ void rg_load8(const uint16_t* p, int (&it)[8]) {
  const uint4 q = *reinterpret_cast<const uint4*>(p);
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int h = 0; h < 8; ++h) it[h] = (int)((w[h >> 1] >> (16 * (h & 1))) & 0xFFFFu);
}
__device__ __forceinline__ void rg_load8(const int32_t* p, int (&it)[8]) {
  const int4 a = reinterpret_cast<const int4*>(p)[0], b = reinterpret_cast<const int4*>(p)[1];
  it[0] = a.x; it[1] = a.y; it[2] = a.z; it[3] = a.w;
  it[4] = b.x; it[5] = b.y; it[6] = b.z; it[7] = b.w;
}

// The rounds, the fallback and the numbering of one level.  kLds: par and list in LDS
// (uint16 indices: C < 0xFFFF), else in the level's global scratch.
template <bool kLds, int K>
__device__ __forceinline__ void rg_level(const RgArgs& A, const RgLv& V, uint32_t* lds, int* sh, int* fired) {
  using Li = typename std::conditional<kLds, uint16_t, int32_t>::type;
  const int tid = threadIdx.x;
  constexpr int k = K, m = K - 1;
  const int n = (int)V.n, C = (int)V.C, nh = (n + 1) >> 1;
  const int64_t base = V.base;
  int32_t* const cnt_out = reinterpret_cast<int32_t*>(V.scr);
  int32_t* const ex_out = cnt_out + n;
  int64_t* const off_out = reinterpret_cast<int64_t*>(V.scr + rg_off_at(n, C));
  uint16_t* const gpar = reinterpret_cast<uint16_t*>(V.scr + rg_par_at(n, C));
  uint32_t* u = lds;
  uint32_t* u2 = lds + nh;
  uint32_t* const v = lds + 2 * nh;
  char* const lists = reinterpret_cast<char*>(lds) + rg_lds_counters(n);
  uint16_t* const par = kLds ? reinterpret_cast<uint16_t*>(lists) : gpar;
  Li* const list = kLds ? reinterpret_cast<Li*>(lists + rg_lds_par(C, m))
                        : reinterpret_cast<Li*>(V.scr + rg_list_at(n, C, m));
  auto mark = [&](int i) {
    if (A.phase != nullptr && tid == 0) A.phase[4 * blockIdx.x + i] = (long long)wall_clock64();
  };
  mark(0);
  for (int i = tid; i < 3 * nh; i += kRgThreads) lds[i] = 0;
  __syncthreads();
  // u of the first round (every candidate is unassigned), the lists into LDS
  const int E = k * C, nv = E >> 3;
  for (int i = tid; i < nv; i += kRgThreads) {
    const uint4 q = reinterpret_cast<const uint4*>(gpar)[i];
    if (kLds) reinterpret_cast<uint4*>(par)[i] = q;
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      const int p = (int)((w[h >> 1] >> (16 * (h & 1))) & 0xFFFFu);
      if (p != kRgNone) pk_inc(u, p);
    }
  }
  for (int e = 8 * nv + tid; e < E; e += kRgThreads) {
    const uint16_t p = gpar[e];
    if (kLds) par[e] = p;
    if (p != kRgNone) pk_inc(u, p);
  }
  for (int c = tid; c < C; c += kRgThreads) list[c] = (Li)c;
  __syncthreads();
  mark(1);
  // An assigned candidate leaves the list and keeps its parent in par[0][c]: position 0 is
  // read again only by the "item left out" search below, which ends there anyway.
  constexpr int kDead = kLds ? 0xFFFF : -1;        // a list entry that was assigned in this round
  int left = C, rounds = 0;
  for (int t = 0; t < kRgNThr; ++t) {
    const int thr = rg_thr(t);
    for (;;) {
      ++rounds;
#pragma unroll 2
      for (int i = tid; i < left; i += kRgThreads) {
        int ps[K];
        const int bp = rg_vote<K>(par, u, C, thr, (int)list[i], ps);
        if (bp >= 0) pk_inc(v, bp);
      }
      __syncthreads();
      // a parent with >= thr votes takes its voters (u is unchanged: the vote comes out the
      // same); the others are counted again (u2) and stay on the list
#pragma unroll 2
      for (int i = tid; i < left; i += kRgThreads) {
        const int c = (int)list[i];
        int ps[K];
        const int bp = rg_vote<K>(par, u, C, thr, c, ps);
        if (bp >= 0 && pk_get(v, bp) >= thr) {
          par[c] = (uint16_t)bp;
          list[i] = (Li)kDead;
          *fired = 1;
          continue;
        }
#pragma unroll
        for (int j = 0; j < K; ++j)
          if (ps[j] != kRgNone) pk_inc(u2, ps[j]);
      }
      __syncthreads();
      // a round that assigned something: the list without the assigned, in place.  One scan
      // element is a thread's 8 consecutive entries, which move to positions at or before
      // their own, inside chunks already read.
      const bool f = *fired != 0;
      if (f) {
      int it[8];
      left = (int)wg_scan_chunks<kRgW>(
          (int64_t)((left + 7) >> 3), (int64_t)0, sh,
          [&](int64_t g) {
            rg_load8(list + 8 * g, it);
            int kept = 0;
#pragma unroll
            for (int h = 0; h < 8; ++h) {
              if (8 * (int)g + h >= left) it[h] = kDead;
              kept += it[h] != kDead ? 1 : 0;
            }
            return kept;
          },
          [&](int64_t, int64_t before, int) {
            int r = (int)before;
#pragma unroll
            for (int h = 0; h < 8; ++h)
              if (it[h] != kDead) list[r++] = (Li)it[h];
          });
      if (tid == 0) *fired = 0;                      // (every thread has read it: the scan's barriers)
      uint32_t* x = u; u = u2; u2 = x;               // (nothing assigned: u still holds)
      }
      for (int i = tid; i < nh; i += kRgThreads) { u2[i] = 0; v[i] = 0; }
      __syncthreads();
      if (!f) break;
    }
  }
  mark(2);
  // children per parent, and the piece counts of the two plans
  for (int c = tid; c < C; c += kRgThreads) pk_inc(v, par[c]);
  __syncthreads();
  int pc[2] = {0, 0}, tot[2];
  for (int i = tid; i < n; i += kRgThreads) {
    pc[0] += (pk_get(v, i) + 7) >> 3;
    pc[1] += (V.cnt[i] + 7) >> 3;
  }
  wg_sum<kRgW>(pc, sh, tot);
  const bool keep = tot[0] >= tot[1];              // not cheaper: the level keeps the prefix plan
  __syncthreads();
  if (keep) {
    for (int i = tid; i < nh; i += kRgThreads) v[i] = 0;
    __syncthreads();
    for (int c = tid; c < C; c += kRgThreads) {
      const uint16_t p = par[m * C + c];
      par[c] = p;
      pk_inc(v, p);
    }
    __syncthreads();
  }
  // offsets: also as int32 cursors over u and u2 (2 nh >= n words, free now)
  int32_t* const cur = reinterpret_cast<int32_t*>(lds);
  wg_scan_chunks<kRgW>(
      (int64_t)n, (int64_t)0, sh, [&](int64_t i) { return pk_get(v, (int)i); },
      [&](int64_t i, int64_t before, int a) {
        cnt_out[i] = a;
        off_out[i] = before;
        cur[i] = (int32_t)before;
      });
  if (tid == 0) off_out[n] = C;
  // a parent's children in any order, then every child's rank among them by candidate index:
  // the numbering does not depend on that order.  The cursors end at the parents' ends.
  for (int c = tid; c < C; c += kRgThreads) list[atomicAdd(&cur[par[c]], 1)] = (Li)c;
  __syncthreads();
  for (int c = tid; c < C; c += kRgThreads) {
    const int p = par[c];
    const int a = pk_get(v, p), o = cur[p] - a;
    int r = 0;
    for (int q = 0; q < a; ++q) r += (int)list[o + q] < c ? 1 : 0;
    int j = m;                                     // the item left out of the parent
    if (!keep)
      for (j = k - 1; j > 0 && par[j * C + c] != p; --j) {}
    ex_out[o + r] = V.rows[(int64_t)c * k + j];
    A.perm[base + o + r] = (int32_t)(base + c);
  }
  if (tid == 0) {
    long long* s = A.stats + 4 * blockIdx.x;
    s[0] = tot[1]; s[1] = tot[0]; s[2] = rounds; s[3] = keep ? 1 : 0;
  }
  mark(3);
}

__global__ __launch_bounds__(kRgThreads) void k_dl_rg_rounds(const RgArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t rg_lds[];
  __shared__ int sh[2 * kRgW];
  __shared__ int fired;
  const RgLv& V = A.lv[blockIdx.x];
  const int tid = threadIdx.x;
  if (V.n > kRgMaxRows) {                  // (the launcher keeps this level's table)
    for (int64_t c = tid; c < V.C; c += kRgThreads) A.perm[V.base + c] = (int32_t)(V.base + c);
    int pp = 0;
    for (int64_t i = tid; i < V.n; i += kRgThreads) pp += (V.cnt[i] + 7) >> 3;
    pp = wg_sum<kRgW>(pp, sh);
    if (tid == 0) {
      long long* s = A.stats + 4 * blockIdx.x;
      s[0] = s[1] = pp; s[2] = 0; s[3] = 1;
    }
    return;
  }
  if (tid == 0) fired = 0;                 // (read after the barriers of the level's setup)
  const bool fits = rg_lds_fits(V.n, V.C, V.m, A.lds_cap);
#define FA_RG_K(K)                                         \
  case K:                                                  \
    if (fits) rg_level<true, K>(A, V, rg_lds, sh, &fired); \
    else rg_level<false, K>(A, V, rg_lds, sh, &fired);     \
    break;
  static_assert(kRgMaxK == 13, "one case per k = m + 1 (rg_eligible: 1 <= m <= kDlInline)");
  switch (V.m + 1) {
    FA_RG_K(2) FA_RG_K(3) FA_RG_K(4) FA_RG_K(5) FA_RG_K(6) FA_RG_K(7)
    FA_RG_K(8) FA_RG_K(9) FA_RG_K(10) FA_RG_K(11) FA_RG_K(12) FA_RG_K(13)
  }
#undef FA_RG_K
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

static int64_t g_rg_lds_cap = kRgLdsMax;
static long long* g_rg_phase = nullptr;

}  // namespace fa

using namespace fa;

// The LDS bytes the rounds kernel's fit rule may use (fa_regroup.h rg_lds_fits); < 0: the
// device's (the default).  A debug knob: tests reach the global-memory lists at tiny shapes.
FA_API void fa_hip_set_dl_regroup_lds(int64_t bytes) {
  g_rg_lds_cap = bytes < 0 ? kRgLdsMax : std::min<int64_t>(bytes, kRgLdsMax);
}

// A probe's phase timers: device int64 [kDlMaxL][4] that every later step writes (RgArgs.phase;
// the clock is wall_clock64's, 100 MHz), or null (the default): none.
FA_API void fa_hip_debug_dl_regroup_phases(long long* buf) { g_rg_phase = buf; }

// LDS bytes at which a level's lists are in LDS (rg_lds_fits; -1: never, C past 16-bit indices)
FA_API int64_t fa_hip_dl_regroup_lds(int64_t n, int64_t C, int64_t m) {
  return rg_lds_fits(n, C, m, INT64_MAX) ? rg_lds_all(n, C, m) : -1;
}

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
  if ((intptr_t)scratch & 15) return 1;      // (par is read 16 bytes at a time)
  int64_t C = 0;
  for (int l = 0; l < L; ++l) C += desc[l].C;
  RgArgs A{};
  char* w = static_cast<char*>(scratch);
  A.perm = reinterpret_cast<int32_t*>(w);
  w += rg_al(4 * C);
  A.stats = stats;
  A.lds_cap = g_rg_lds_cap;
  A.phase = g_rg_phase;
  A.L = L;
  int64_t lds = 16, blocks = 0;
  for (int l = 0; l < L; ++l) {
    const DlDesc& d = desc[l];
    RgLv& V = A.lv[l];
    V.P = reinterpret_cast<const int32_t*>((intptr_t)d.P);
    V.cnt = reinterpret_cast<const int32_t*>((intptr_t)d.cnt);
    V.off = reinterpret_cast<const int64_t*>((intptr_t)d.off);
    V.rows = reinterpret_cast<const int32_t*>((intptr_t)d.rows);
    V.n = d.n; V.C = d.C; V.base = d.base; V.m = (int32_t)d.m;
    V.scr = w;
    V.blk0 = (uint32_t)blocks;
    out[l] = d;
    if (d.n > kRgMaxRows) continue;
    lds = std::max(lds, rg_lds_bytes(d.n, d.C, d.m, A.lds_cap));
    blocks += (d.C * (d.m + 1) + kRgPThreads - 1) / kRgPThreads;
    out[l].cnt = (int64_t)(intptr_t)w;
    out[l].off = (int64_t)(intptr_t)(w + rg_off_at(d.n, d.C));
    w += rg_scratch_bytes(d.n, d.C, d.m);
  }
  static bool lds_set = false;               // once: the most a level may take
  if (!lds_set) {
    const hipError_t e =
        hipFuncSetAttribute((const void*)k_dl_rg_rounds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRgLdsMax);
    if (e != hipSuccess) return (int)e;
    lds_set = true;
  }
  if (blocks > 0) {
    hipLaunchKernelGGL(k_dl_rg_parents, dim3((unsigned)blocks), dim3(kRgPThreads), 0, st, A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(k_dl_rg_rounds, dim3((unsigned)L), dim3(kRgThreads), (size_t)lds, st, A);
  FA_LAUNCH_RET();
}

// out[perm[e]] = in[e], e < C: the counts of a regrouped plan back in the generator's order
FA_API int fa_hip_dl_unpermute(const uint32_t* in, const int32_t* perm, int64_t C, uint32_t* out, hipStream_t st) {
  if (C < 1) return 1;
  hipLaunchKernelGGL(k_dl_unpermute, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, in, perm, C, out);
  FA_LAUNCH_RET();
}
