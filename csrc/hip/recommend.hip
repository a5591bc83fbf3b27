// First-match recommendation (AssociationRules.scala:80-106): for each distinct
// basket U, the consequent of the first rule (in confidence order) whose
// antecedent is a subset of U and whose consequent is not in U.
//
// One wavefront per basket.  The basket is a bitset over ranks in LDS; each
// step tests 64 consecutive rules, one per lane, and __ballot + ffs picks the
// earliest match, so the scan stops at the first 64-rule chunk that hits.
#include "fa_hip.h"

namespace fa {

constexpr int kRecWaves = 4;

__global__ __launch_bounds__(256) void k_recommend(
    const int64_t* __restrict__ ante_off, const int32_t* __restrict__ ante, const int32_t* __restrict__ cons,
    int64_t R, int32_t F1, const int64_t* __restrict__ boff, const int32_t* __restrict__ bask, int64_t M,
    int32_t* __restrict__ out) {
  extern __shared__ uint32_t bits[];   // [kRecWaves][words]
  const int words = (F1 + 31) >> 5;
  const int wv = threadIdx.x >> 6, lane = lane_id();
  uint32_t* bs = bits + wv * words;
  const int64_t u = (int64_t)blockIdx.x * kRecWaves + wv;
  for (int i = lane; i < words; i += kWave) bs[i] = 0;
  __syncthreads();
  if (u < M) {
    const int64_t s = boff[u], e = boff[u + 1];
    for (int64_t i = s + lane; i < e; i += kWave) atomicOr(&bs[bask[i] >> 5], 1u << (bask[i] & 31));
  }
  __syncthreads();
  if (u >= M) return;
  const int64_t usz = boff[u + 1] - boff[u];
  int32_t rec = -1;
  if (usz > 0) {
    for (int64_t base = 0; base < R; base += kWave) {
      const int64_t r = base + lane;
      bool ok = false;
      if (r < R) {
        const int32_t c = cons[r];
        const int64_t a0 = ante_off[r], a1 = ante_off[r + 1];
        ok = !((bs[c >> 5] >> (c & 31)) & 1u) && (a1 - a0) <= usz;
        for (int64_t i = a0; ok && i < a1; ++i) {
          const int32_t a = ante[i];
          ok = (bs[a >> 5] >> (a & 31)) & 1u;
        }
      }
      const unsigned long long mask = __ballot(ok);
      if (mask) {
        const int first = __ffsll((long long)mask) - 1;
        rec = cons[base + first];
        break;
      }
    }
  }
  if (lane == 0) out[u] = rec;
}

// Indexed first match for large rule tables.  Rule r is listed under the
// last (highest-rank, i.e. least frequent) item of its antecedent; ante ⊆ U
// needs that item in U, so a basket only visits the lists of its own items.
// Lists hold rule ids in ascending (= recommendation) order: a list is scanned
// 64 rules per step until its first hit or until its ids pass the best hit so
// far, and the smallest hit over the basket's lists is the first match of the
// full ordered scan.
__global__ __launch_bounds__(256) void k_recommend_indexed(
    const int64_t* __restrict__ list_off, const int32_t* __restrict__ list_rule,
    const int64_t* __restrict__ ante_off, const int32_t* __restrict__ ante, const int32_t* __restrict__ cons,
    int64_t R, int32_t F1, const int64_t* __restrict__ boff, const int32_t* __restrict__ bask, int64_t M,
    int32_t* __restrict__ out) {
  extern __shared__ uint32_t bits[];   // [kRecWaves][words]
  const int words = (F1 + 31) >> 5;
  const int wv = threadIdx.x >> 6, lane = lane_id();
  uint32_t* bs = bits + wv * words;
  const int64_t u = (int64_t)blockIdx.x * kRecWaves + wv;
  for (int i = lane; i < words; i += kWave) bs[i] = 0;
  __syncthreads();
  if (u < M) {
    const int64_t s = boff[u], e = boff[u + 1];
    for (int64_t i = s + lane; i < e; i += kWave) atomicOr(&bs[bask[i] >> 5], 1u << (bask[i] & 31));
  }
  __syncthreads();
  if (u >= M) return;
  const int64_t s = boff[u], e = boff[u + 1];
  const int64_t usz = e - s;
  int32_t best = (int32_t)R;
  for (int64_t j = s; j < e; ++j) {
    const int32_t item = bask[j];
    const int64_t lo = list_off[item], hi = list_off[item + 1];
    for (int64_t base = lo; base < hi; base += kWave) {
      if (list_rule[base] >= best) break;            // wave-uniform: the rest of the list is later
      const int64_t q = base + lane;
      const int32_t r = q < hi ? list_rule[q] : INT32_MAX;
      bool ok = false;
      if (r < best) {
        const int32_t c = cons[r];
        const int64_t a0 = ante_off[r], a1 = ante_off[r + 1];
        ok = !((bs[c >> 5] >> (c & 31)) & 1u) && (a1 - a0) <= usz;
        for (int64_t i = a0; ok && i < a1 - 1; ++i) {   // the last item is `item`, in U
          const int32_t a = ante[i];
          ok = (bs[a >> 5] >> (a & 31)) & 1u;
        }
      }
      const unsigned long long mask = __ballot(ok);
      if (mask) {
        best = __builtin_amdgcn_readlane(r, __ffsll((long long)mask) - 1);
        break;
      }
    }
  }
  if (lane == 0) out[u] = best < R ? cons[best] : -1;
}

// ---------------------------------------------------------------------------
// Ranked top-N (an extension: the reference stops at the first match).  Walking
// the rule table in its order, the list of a basket is the first n firing rules
// with pairwise distinct consequents; out[u][0 .. n) holds their rule ids, -1
// padded, so cons[id] is the item and conf[id] its score.
//
// Both kernels keep the result in registers, entry j in lane j of the basket's
// wave (n <= 64), with `cnt` entries filled.  cnt, the step masks and everything
// a loop exit depends on come from __ballot / readlane values, so every branch
// below is wave-uniform.  Taken consequents are never set in the basket bitset:
// an antecedent holding one must not start to match.
// ---------------------------------------------------------------------------

// The basket of wave wv as a bitset in LDS (as in k_recommend); false for the idle
// waves of the last workgroup.  Every thread of the workgroup reaches both barriers.
__device__ __forceinline__ bool rec_load_basket(uint32_t* bs, int words, const int64_t* __restrict__ boff,
                                                const int32_t* __restrict__ bask, int64_t u, int64_t M) {
  const int lane = lane_id();
  for (int i = lane; i < words; i += kWave) bs[i] = 0;
  __syncthreads();
  if (u < M) {
    const int64_t s = boff[u], e = boff[u + 1];
    for (int64_t i = s + lane; i < e; i += kWave) atomicOr(&bs[bask[i] >> 5], 1u << (bask[i] & 31));
  }
  __syncthreads();
  return u < M;
}

// Ordered scan: 64 rules per step.  A lane's rule is dropped when its consequent is
// in one of the cnt filled slots (taken in an earlier step); the step's remaining
// lanes are consumed in lane (= rule) order, each accepted consequent clearing the
// later lanes that share it.
__global__ __launch_bounds__(256) void k_recommend_topn(
    const int64_t* __restrict__ ante_off, const int32_t* __restrict__ ante, const int32_t* __restrict__ cons,
    int64_t R, int32_t F1, const int64_t* __restrict__ boff, const int32_t* __restrict__ bask, int64_t M,
    int32_t n, int32_t* __restrict__ out) {
  extern __shared__ uint32_t bits[];   // [kRecWaves][words]
  const int words = (F1 + 31) >> 5;
  const int wv = threadIdx.x >> 6, lane = lane_id();
  uint32_t* bs = bits + wv * words;
  const int64_t u = (int64_t)blockIdx.x * kRecWaves + wv;
  if (!rec_load_basket(bs, words, boff, bask, u, M)) return;
  const int64_t usz = boff[u + 1] - boff[u];
  int32_t sr = -1, sc = -1;            // slot `lane`: accepted rule id, its consequent
  int cnt = 0;
  if (usz > 0) {
    for (int64_t base = 0; base < R && cnt < n; base += kWave) {
      const int64_t r = base + lane;
      bool ok = false;
      int32_t c = -1;
      if (r < R) {
        c = cons[r];
        const int64_t a0 = ante_off[r], a1 = ante_off[r + 1];
        ok = !((bs[c >> 5] >> (c & 31)) & 1u) && (a1 - a0) <= usz;
        for (int64_t i = a0; ok && i < a1; ++i) {
          const int32_t a = ante[i];
          ok = (bs[a >> 5] >> (a & 31)) & 1u;
        }
      }
      unsigned long long mask = __ballot(ok);
      if (!mask) continue;
      for (int j = 0; j < cnt; ++j) {
        const int32_t tc = __builtin_amdgcn_readlane(sc, j);
        ok = ok && c != tc;
      }
      mask = __ballot(ok);
      while (mask && cnt < n) {
        const int first = __ffsll((long long)mask) - 1;
        const int32_t ac = __builtin_amdgcn_readlane(c, first);
        if (lane == cnt) {
          sr = (int32_t)(base + first);
          sc = ac;
        }
        ++cnt;
        ok = ok && c != ac;              // the accepted lane and every later one with its consequent
        mask = __ballot(ok);
      }
    }
  }
  if (lane < n) out[u * n + lane] = sr;
}

// Per-item rule lists (see k_recommend_indexed).  Lists are visited in basket order,
// not rule order, so the wave keeps the best n (rule id, consequent) entries seen so
// far, sorted by rule id with distinct consequents (empty slots: INT32_MAX, -1).
// A firing rule (r, c) replaces the entry of c when it has a larger id, else an empty
// slot, else the worst entry when r is below it.  Kept ids only decrease, so once the
// buffer is full nothing at or past its worst id can enter: that id (R before) is the
// bound that ends a list, whose ids ascend.
__global__ __launch_bounds__(256) void k_recommend_topn_indexed(
    const int64_t* __restrict__ list_off, const int32_t* __restrict__ list_rule,
    const int64_t* __restrict__ ante_off, const int32_t* __restrict__ ante, const int32_t* __restrict__ cons,
    int64_t R, int32_t F1, const int64_t* __restrict__ boff, const int32_t* __restrict__ bask, int64_t M,
    int32_t n, int32_t* __restrict__ out) {
  extern __shared__ uint32_t bits[];   // [kRecWaves][words]
  const int words = (F1 + 31) >> 5;
  const int wv = threadIdx.x >> 6, lane = lane_id();
  uint32_t* bs = bits + wv * words;
  const int64_t u = (int64_t)blockIdx.x * kRecWaves + wv;
  if (!rec_load_basket(bs, words, boff, bask, u, M)) return;
  const int64_t s = boff[u], e = boff[u + 1];
  const int64_t usz = e - s;
  int32_t sr = INT32_MAX, sc = -1;     // slot `lane`
  int cnt = 0;
  int32_t bound = (int32_t)R;
  for (int64_t j = s; j < e; ++j) {
    const int32_t item = bask[j];
    const int64_t lo = list_off[item], hi = list_off[item + 1];
    for (int64_t base = lo; base < hi; base += kWave) {
      if (list_rule[base] >= bound) break;            // wave-uniform: the rest of the list is later
      const int64_t q = base + lane;
      const int32_t r = q < hi ? list_rule[q] : INT32_MAX;
      bool ok = false;
      int32_t c = -1;
      if (r < bound) {
        c = cons[r];
        const int64_t a0 = ante_off[r], a1 = ante_off[r + 1];
        ok = !((bs[c >> 5] >> (c & 31)) & 1u) && (a1 - a0) <= usz;
        for (int64_t i = a0; ok && i < a1 - 1; ++i) {   // the last item is `item`, in U
          const int32_t a = ante[i];
          ok = (bs[a >> 5] >> (a & 31)) & 1u;
        }
      }
      // the step's firing lanes in lane order: ids ascend along a list
      for (unsigned long long mask = __ballot(ok); mask; mask &= mask - 1) {
        const int f = __ffsll((long long)mask) - 1;
        const int32_t rr = __builtin_amdgcn_readlane(r, f), cc = __builtin_amdgcn_readlane(c, f);
        if (rr >= bound) break;                         // so are the lanes after it
        // p: the slot that leaves (the entry of cc, a free slot, or the worst entry)
        const unsigned long long hit = __ballot(sc == cc);
        int p;
        if (hit) {
          p = __ffsll((long long)hit) - 1;
          if (__builtin_amdgcn_readlane(sr, p) < rr) continue;
        } else if (cnt < n) {
          p = cnt++;
        } else {
          p = n - 1;
        }
        // rr is below slot p's id, so its place pos is at or before p: slots [pos, p) move up one
        const int pos = __popcll(__ballot(sr < rr));
        const int32_t ur = __shfl_up(sr, 1, kWave), uc = __shfl_up(sc, 1, kWave);
        if (lane > pos && lane <= p) {
          sr = ur;
          sc = uc;
        } else if (lane == pos) {
          sr = rr;
          sc = cc;
        }
        if (cnt == n) bound = __builtin_amdgcn_readlane(sr, n - 1);
      }
    }
  }
  if (lane < n) out[u * n + lane] = sr == INT32_MAX ? -1 : sr;
}

// ---------------------------------------------------------------------------
// Leave-one-out rank (an extension, AssociationRules.evaluate): trial t is element t of
// the basket CSR.  Its basket is row trow[t] WITHOUT the hidden item h = bask[t], and
// out[t] is the 1-based place of h in the top-n list of that basket, 0 when it is not in
// it.  One wave per trial; the walks are those of the top-n kernels above, cut short where
// h's place is settled.  As there, every loop exit and every branch a lane count depends on
// comes from a __ballot / readlane / readfirstlane value.
// ---------------------------------------------------------------------------

// The trial's basket minus h as a bitset in LDS; false for the idle waves of the last
// workgroup.  Every thread of the workgroup reaches both barriers.
__device__ __forceinline__ bool holdout_load_basket(uint32_t* bs, int words, const int64_t* __restrict__ boff,
                                                    const int32_t* __restrict__ bask,
                                                    const int64_t* __restrict__ trow, int64_t t, int64_t T) {
  const int lane = lane_id();
  for (int i = lane; i < words; i += kWave) bs[i] = 0;
  __syncthreads();
  if (t < T) {
    const int64_t u = trow[t];
    const int32_t h = bask[t];
    const int64_t s = boff[u], e = boff[u + 1];
    for (int64_t i = s + lane; i < e; i += kWave) {
      const int32_t b = bask[i];
      if (b != h) atomicOr(&bs[b >> 5], 1u << (b & 31));
    }
  }
  __syncthreads();
  return t < T;
}

// Ordered scan (k_recommend_topn's): only the taken consequents are kept, slot j in lane j.
// Ends when h is accepted (its place is the slots filled, counting it), when n slots are
// full or when the table ends (0).
__global__ __launch_bounds__(256) void k_holdout_rank(
    const int64_t* __restrict__ ante_off, const int32_t* __restrict__ ante, const int32_t* __restrict__ cons,
    int64_t R, int32_t F1, const int64_t* __restrict__ boff, const int32_t* __restrict__ bask,
    const int64_t* __restrict__ trow, int64_t T, int32_t n, int32_t* __restrict__ out) {
  extern __shared__ uint32_t bits[];   // [kRecWaves][words]
  const int words = (F1 + 31) >> 5;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = lane_id();
  uint32_t* bs = bits + wv * words;
  const int64_t t = (int64_t)blockIdx.x * kRecWaves + wv;
  if (!holdout_load_basket(bs, words, boff, bask, trow, t, T)) return;
  const int64_t u = trow[t];
  const int32_t h = __builtin_amdgcn_readfirstlane(bask[t]);
  const int64_t usz = boff[u + 1] - boff[u] - 1;     // without h
  int32_t sc = -1;                     // slot `lane`: a taken consequent
  int cnt = 0, rank = 0;
  if (usz > 0) {
    for (int64_t base = 0; base < R && cnt < n; base += kWave) {
      const int64_t r = base + lane;
      bool ok = false;
      int32_t c = -1;
      if (r < R) {
        c = cons[r];
        const int64_t a0 = ante_off[r], a1 = ante_off[r + 1];
        ok = !((bs[c >> 5] >> (c & 31)) & 1u) && (a1 - a0) <= usz;
        for (int64_t i = a0; ok && i < a1; ++i) {
          const int32_t a = ante[i];
          ok = (bs[a >> 5] >> (a & 31)) & 1u;
        }
      }
      unsigned long long mask = __ballot(ok);
      if (!mask) continue;
      for (int j = 0; j < cnt; ++j) {
        const int32_t tc = __builtin_amdgcn_readlane(sc, j);
        ok = ok && c != tc;
      }
      mask = __ballot(ok);
      while (mask && cnt < n) {
        const int first = __ffsll((long long)mask) - 1;
        const int32_t ac = __builtin_amdgcn_readlane(c, first);
        if (lane == cnt) sc = ac;
        ++cnt;
        if (ac == h) {                   // settled: a full list ends both loops
          rank = cnt;
          cnt = n;
        }
        ok = ok && c != ac;              // the accepted lane and every later one with its consequent
        mask = __ballot(ok);
      }
    }
  }
  if (lane == 0) out[t] = rank;
}

// Per-item rule lists (k_recommend_topn_indexed's buffer and bound).  h's own list is not
// visited: every rule in it has h in its antecedent.  Once a rule with consequent h is in
// the buffer, entries past it cannot change h's place, so its id bounds every later list,
// too.  At the end the place of h is its slot in the buffer.
__global__ __launch_bounds__(256) void k_holdout_rank_indexed(
    const int64_t* __restrict__ list_off, const int32_t* __restrict__ list_rule,
    const int64_t* __restrict__ ante_off, const int32_t* __restrict__ ante, const int32_t* __restrict__ cons,
    int64_t R, int32_t F1, const int64_t* __restrict__ boff, const int32_t* __restrict__ bask,
    const int64_t* __restrict__ trow, int64_t T, int32_t n, int32_t* __restrict__ out) {
  extern __shared__ uint32_t bits[];   // [kRecWaves][words]
  const int words = (F1 + 31) >> 5;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = lane_id();
  uint32_t* bs = bits + wv * words;
  const int64_t t = (int64_t)blockIdx.x * kRecWaves + wv;
  if (!holdout_load_basket(bs, words, boff, bask, trow, t, T)) return;
  const int64_t u = trow[t];
  const int32_t h = __builtin_amdgcn_readfirstlane(bask[t]);
  const int64_t s = boff[u], e = boff[u + 1];
  const int64_t usz = e - s - 1;       // without h
  int32_t sr = INT32_MAX, sc = -1;     // slot `lane`
  int cnt = 0;
  int32_t bound = (int32_t)R;
  for (int64_t j = s; j < e; ++j) {
    const int32_t item = __builtin_amdgcn_readfirstlane(bask[j]);
    if (item == h) continue;
    const int64_t lo = list_off[item], hi = list_off[item + 1];
    for (int64_t base = lo; base < hi; base += kWave) {
      if (__builtin_amdgcn_readfirstlane(list_rule[base]) >= bound) break;   // the rest of the list is later
      const int64_t q = base + lane;
      const int32_t r = q < hi ? list_rule[q] : INT32_MAX;
      bool ok = false;
      int32_t c = -1;
      if (r < bound) {
        c = cons[r];
        const int64_t a0 = ante_off[r], a1 = ante_off[r + 1];
        ok = !((bs[c >> 5] >> (c & 31)) & 1u) && (a1 - a0) <= usz;
        for (int64_t i = a0; ok && i < a1 - 1; ++i) {   // the last item is `item`, in the basket
          const int32_t a = ante[i];
          ok = (bs[a >> 5] >> (a & 31)) & 1u;
        }
      }
      // the step's firing lanes in lane order: ids ascend along a list
      for (unsigned long long mask = __ballot(ok); mask; mask &= mask - 1) {
        const int f = __ffsll((long long)mask) - 1;
        const int32_t rr = __builtin_amdgcn_readlane(r, f), cc = __builtin_amdgcn_readlane(c, f);
        if (rr >= bound) break;                         // so are the lanes after it
        // p: the slot that leaves (the entry of cc, a free slot, or the worst entry)
        const unsigned long long hit = __ballot(sc == cc);
        int p;
        if (hit) {
          p = __ffsll((long long)hit) - 1;
          if (__builtin_amdgcn_readlane(sr, p) < rr) continue;
        } else if (cnt < n) {
          p = cnt++;
        } else {
          p = n - 1;
        }
        // rr is below slot p's id, so its place pos is at or before p: slots [pos, p) move up one
        const int pos = __popcll(__ballot(sr < rr));
        const int32_t ur = __shfl_up(sr, 1, kWave), uc = __shfl_up(sc, 1, kWave);
        if (lane > pos && lane <= p) {
          sr = ur;
          sc = uc;
        } else if (lane == pos) {
          sr = rr;
          sc = cc;
        }
        // bound only falls: rr < bound, and a full buffer's worst id never grows
        if (cc == h) bound = rr;
        if (cnt == n) bound = min(bound, __builtin_amdgcn_readlane(sr, n - 1));
      }
    }
  }
  const unsigned long long at = __ballot(sc == h);
  if (lane == 0) out[t] = at ? __ffsll((long long)at) : 0;
}

}  // namespace fa

using namespace fa;

FA_API int fa_hip_recommend(const int64_t* ante_off, const int32_t* ante, const int32_t* cons, int64_t R,
                            int32_t F1, const int64_t* boff, const int32_t* bask, int64_t M, int32_t* out,
                            hipStream_t st) {
  if (M <= 0) return 0;
  const size_t words = (size_t)((F1 + 31) / 32);
  const size_t lds = std::max<size_t>(4, words * 4 * kRecWaves);
  if (lds > 64 * 1024) return 2;   // caller falls back to the host path
  dim3 g((unsigned)((M + kRecWaves - 1) / kRecWaves));
  hipLaunchKernelGGL(k_recommend, g, dim3(256), lds, st, ante_off, ante, cons, R, F1, boff, bask, M, out);
  FA_LAUNCH_RET();
}

FA_API int fa_hip_recommend_indexed(const int64_t* list_off, const int32_t* list_rule, const int64_t* ante_off,
                                    const int32_t* ante, const int32_t* cons, int64_t R, int32_t F1,
                                    const int64_t* boff, const int32_t* bask, int64_t M, int32_t* out,
                                    hipStream_t st) {
  if (M <= 0) return 0;
  if (R >= (int64_t)INT32_MAX) return 3;
  const size_t words = (size_t)((F1 + 31) / 32);
  const size_t lds = std::max<size_t>(4, words * 4 * kRecWaves);
  if (lds > 64 * 1024) return 2;   // caller falls back to the host path
  dim3 g((unsigned)((M + kRecWaves - 1) / kRecWaves));
  hipLaunchKernelGGL(k_recommend_indexed, g, dim3(256), lds, st, list_off, list_rule, ante_off, ante, cons, R, F1,
                     boff, bask, M, out);
  FA_LAUNCH_RET();
}

// out: int32 [M, n] rule ids, -1 padded; 1 <= n <= 64 (one result slot per lane)
FA_API int fa_hip_recommend_topn(const int64_t* ante_off, const int32_t* ante, const int32_t* cons, int64_t R,
                                 int32_t F1, const int64_t* boff, const int32_t* bask, int64_t M, int32_t n,
                                 int32_t* out, hipStream_t st) {
  if (n < 1 || n > kWave) return (int)hipErrorInvalidValue;
  if (M <= 0) return 0;
  if (R >= (int64_t)INT32_MAX) return 3;
  const size_t words = (size_t)((F1 + 31) / 32);
  const size_t lds = std::max<size_t>(4, words * 4 * kRecWaves);
  if (lds > 64 * 1024) return 2;   // caller falls back to the host path
  dim3 g((unsigned)((M + kRecWaves - 1) / kRecWaves));
  hipLaunchKernelGGL(k_recommend_topn, g, dim3(256), lds, st, ante_off, ante, cons, R, F1, boff, bask, M, n, out);
  FA_LAUNCH_RET();
}

FA_API int fa_hip_recommend_topn_indexed(const int64_t* list_off, const int32_t* list_rule, const int64_t* ante_off,
                                         const int32_t* ante, const int32_t* cons, int64_t R, int32_t F1,
                                         const int64_t* boff, const int32_t* bask, int64_t M, int32_t n,
                                         int32_t* out, hipStream_t st) {
  if (n < 1 || n > kWave) return (int)hipErrorInvalidValue;
  if (M <= 0) return 0;
  if (R >= (int64_t)INT32_MAX) return 3;
  const size_t words = (size_t)((F1 + 31) / 32);
  const size_t lds = std::max<size_t>(4, words * 4 * kRecWaves);
  if (lds > 64 * 1024) return 2;   // caller falls back to the host path
  dim3 g((unsigned)((M + kRecWaves - 1) / kRecWaves));
  hipLaunchKernelGGL(k_recommend_topn_indexed, g, dim3(256), lds, st, list_off, list_rule, ante_off, ante, cons, R,
                     F1, boff, bask, M, n, out);
  FA_LAUNCH_RET();
}

// out: int32 [T] places 1..n or 0, one per element of the basket CSR; trow: its row
FA_API int fa_hip_holdout_rank(const int64_t* ante_off, const int32_t* ante, const int32_t* cons, int64_t R,
                               int32_t F1, const int64_t* boff, const int32_t* bask, const int64_t* trow, int64_t T,
                               int32_t n, int32_t* out, hipStream_t st) {
  if (n < 1 || n > kWave) return (int)hipErrorInvalidValue;
  if (T <= 0) return 0;
  if (R >= (int64_t)INT32_MAX || T >= (int64_t)INT32_MAX) return 3;
  const size_t words = (size_t)((F1 + 31) / 32);
  const size_t lds = std::max<size_t>(4, words * 4 * kRecWaves);
  if (lds > 64 * 1024) return 2;   // caller falls back to the host path
  dim3 g((unsigned)((T + kRecWaves - 1) / kRecWaves));
  hipLaunchKernelGGL(k_holdout_rank, g, dim3(256), lds, st, ante_off, ante, cons, R, F1, boff, bask, trow, T, n, out);
  FA_LAUNCH_RET();
}

FA_API int fa_hip_holdout_rank_indexed(const int64_t* list_off, const int32_t* list_rule, const int64_t* ante_off,
                                       const int32_t* ante, const int32_t* cons, int64_t R, int32_t F1,
                                       const int64_t* boff, const int32_t* bask, const int64_t* trow, int64_t T,
                                       int32_t n, int32_t* out, hipStream_t st) {
  if (n < 1 || n > kWave) return (int)hipErrorInvalidValue;
  if (T <= 0) return 0;
  if (R >= (int64_t)INT32_MAX || T >= (int64_t)INT32_MAX) return 3;
  const size_t words = (size_t)((F1 + 31) / 32);
  const size_t lds = std::max<size_t>(4, words * 4 * kRecWaves);
  if (lds > 64 * 1024) return 2;   // caller falls back to the host path
  dim3 g((unsigned)((T + kRecWaves - 1) / kRecWaves));
  hipLaunchKernelGGL(k_holdout_rank_indexed, g, dim3(256), lds, st, list_off, list_rule, ante_off, ante, cons, R,
                     F1, boff, bask, trow, T, n, out);
  FA_LAUNCH_RET();
}
