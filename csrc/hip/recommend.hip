// First-match recommendation (AssociationRules.scala:80-106): for each distinct
// basket U, the consequent of the first rule (in confidence order) whose
// antecedent is a subset of U and whose consequent is not in U.
//
// One wavefront per basket.  The basket is a bitset over ranks in LDS; each
// step tests 64 consecutive rules, one per lane, and __ballot + ffs picks the
// earliest match, so the scan stops at the first 64-rule chunk that hits.
#include "fa_hip.h"
#include "../host/fa_combine.h"

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

// ---------------------------------------------------------------------------
// Combined scoring (an extension, --combine sum|votes; docs/PARITY.md): EVERY firing rule
// of a basket adds its weight w[r] (int64, 1 .. 2^32) to the score S(c) of its consequent,
// f(c) is the smallest firing rule id of c, and the list is the consequents with S > 0 by
// S descending, then f ascending (f is distinct per consequent, so the order is strict),
// cut to n.  There is no early exit, so both kernels are indexed: a basket visits the
// per-item rule lists of its own items (k_recommend_indexed's), every firing rule once.
//
// One wave per basket or trial, persistent over them.  Each wave owns four LDS rows over
// the F1 items (../host/fa_combine.h: size, order and the waves per workgroup): scores,
// first rules, the list of touched consequents and the basket bitset.  A firing lane adds
// its weight with a 64-bit LDS atomic and takes the min of its id; the lane whose add
// returns 0 appends the consequent to the touched list (weights are >= 1 and the sums stay
// below 2^63, so exactly one add per consequent returns 0).  Integer adds and mins do not
// depend on their order: two runs give the same output.  After the walk a consequent's
// place is 1 + the number of touched consequents that beat it -- no sort.  Only the
// touched entries and the basket's words are cleared before the next basket.
//
// A wave touches its own rows only, so the kernels hold no workgroup barrier (idle waves
// simply leave): wave_lds_sync orders a wave's LDS accesses.  As above, every loop exit
// and every lane count comes from a __ballot / readlane / readfirstlane value.
// ---------------------------------------------------------------------------
struct CombRows {
  unsigned long long* score;   // [F1] S(c), 0 = untouched
  int32_t* first;              // [F1] f(c), INT32_MAX = untouched
  int32_t* touched;            // [F1] the consequents with S > 0, in no particular order
  uint32_t* bs;                // basket bitset
};

__device__ __forceinline__ int64_t uniform_i64(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int l) {
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, l);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}

// wave wv's rows, all cleared
__device__ __forceinline__ CombRows comb_rows(unsigned char* lds, int wv, int32_t F1) {
  unsigned char* p = lds + (size_t)wv * (size_t)combine_wave_bytes(F1);
  CombRows w;
  w.score = (unsigned long long*)p;
  p += combine_score_bytes(F1);
  w.first = (int32_t*)p;
  p += combine_first_bytes(F1);
  w.touched = (int32_t*)p;
  p += combine_touched_bytes(F1);
  w.bs = (uint32_t*)p;
  const int lane = lane_id();
  for (int i = lane; i < F1; i += kWave) {
    w.score[i] = 0ull;
    w.first[i] = INT32_MAX;
  }
  for (int i = lane; i < (F1 + 31) >> 5; i += kWave) w.bs[i] = 0u;
  wave_lds_sync();
  return w;
}

// The walk over the lists of basket elements [s, e) except item h (-1: none), whose bits
// (without h) are set in w.bs; usz: the basket's size without h.  Returns the number of
// touched consequents.
__device__ __forceinline__ int comb_walk(const CombRows& w, const int64_t* __restrict__ list_off,
                                         const int32_t* __restrict__ list_rule, const int64_t* __restrict__ ante_off,
                                         const int32_t* __restrict__ ante, const int32_t* __restrict__ cons,
                                         const int64_t* __restrict__ weight, const int32_t* __restrict__ bask,
                                         int64_t s, int64_t e, int32_t h, int64_t usz) {
  const int lane = lane_id();
  const unsigned long long below = (1ull << lane) - 1;
  int nt = 0;
  for (int64_t j = s; j < e; ++j) {
    const int32_t item = __builtin_amdgcn_readfirstlane(bask[j]);
    if (item == h) continue;                 // every rule listed there has h in its antecedent
    const int64_t lo = uniform_i64(list_off[item]), hi = uniform_i64(list_off[item + 1]);
    for (int64_t base = lo; base < hi; base += kWave) {
      const int64_t q = base + lane;
      bool ok = false;
      int32_t r = -1, c = -1;
      if (q < hi) {
        r = list_rule[q];
        c = cons[r];
        const int64_t a0 = ante_off[r], a1 = ante_off[r + 1];
        ok = !((w.bs[c >> 5] >> (c & 31)) & 1u) && (a1 - a0) <= usz;
        for (int64_t i = a0; ok && i < a1 - 1; ++i) {   // the last item is `item`, in the basket
          const int32_t a = ante[i];
          ok = (w.bs[a >> 5] >> (a & 31)) & 1u;
        }
      }
      bool fresh = false;
      if (ok) {
        fresh = atomicAdd(&w.score[c], (unsigned long long)weight[r]) == 0ull;
        atomicMin(&w.first[c], r);
      }
      const unsigned long long mask = __ballot(fresh);
      if (fresh) w.touched[nt + __popcll(mask & below)] = c;
      nt += __popcll(mask);
    }
  }
  wave_lds_sync();
  return nt;
}

// back to the cleared state: the nt touched entries and the words of basket elements [s, e)
__device__ __forceinline__ void comb_reset(const CombRows& w, int nt, const int32_t* __restrict__ bask, int64_t s,
                                           int64_t e) {
  const int lane = lane_id();
  for (int i = lane; i < nt; i += kWave) {
    const int32_t c = w.touched[i];
    w.score[c] = 0ull;
    w.first[c] = INT32_MAX;
  }
  for (int64_t i = s + lane; i < e; i += kWave) w.bs[bask[i] >> 5] = 0u;
  wave_lds_sync();
}

// out_rule[u][j] = f of the j-th entry (-1 padded), out_score[u][j] = its S (0 padded).
// Touched consequent i (lane i of its 64-chunk) counts the touched consequents that beat it,
// chunk by chunk: a chunk's (S, f) sit in registers, one per lane, and are read by readlane.
__global__ __launch_bounds__(256) void k_recommend_combined(
    const int64_t* __restrict__ list_off, const int32_t* __restrict__ list_rule,
    const int64_t* __restrict__ ante_off, const int32_t* __restrict__ ante, const int32_t* __restrict__ cons,
    const int64_t* __restrict__ weight, int32_t F1, const int64_t* __restrict__ boff,
    const int32_t* __restrict__ bask, int64_t M, int32_t n, int32_t* __restrict__ out_rule,
    int64_t* __restrict__ out_score) {
  extern __shared__ __attribute__((aligned(16))) unsigned char comb_lds[];
  const int W = (int)(blockDim.x >> 6);
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = lane_id();
  if ((int64_t)blockIdx.x * W + wv >= M) return;
  const CombRows w = comb_rows(comb_lds, wv, F1);
  for (int64_t u = (int64_t)blockIdx.x * W + wv; u < M; u += (int64_t)gridDim.x * W) {
    const int64_t s = uniform_i64(boff[u]), e = uniform_i64(boff[u + 1]);
    for (int64_t i = s + lane; i < e; i += kWave) atomicOr(&w.bs[bask[i] >> 5], 1u << (bask[i] & 31));
    wave_lds_sync();
    const int nt = comb_walk(w, list_off, list_rule, ante_off, ante, cons, weight, bask, s, e, -1, e - s);
    int32_t* orule = out_rule + u * n;
    int64_t* oscore = out_score + u * n;
    for (int t0 = 0; t0 < nt; t0 += kWave) {
      const int i = t0 + lane;
      unsigned long long S = 0ull;
      int32_t f = INT32_MAX;
      if (i < nt) {
        const int32_t c = w.touched[i];
        S = w.score[c];
        f = w.first[c];
      }
      int beat = 0;
      for (int k0 = 0; k0 < nt; k0 += kWave) {
        const int k = k0 + lane;
        unsigned long long So = 0ull;
        int32_t fo = INT32_MAX;
        if (k < nt) {
          const int32_t co = w.touched[k];
          So = w.score[co];
          fo = w.first[co];
        }
        const int m = min(kWave, nt - k0);
        for (int x = 0; x < m; ++x) {
          const unsigned long long Sx = readlane_u64(So, x);
          const int32_t fx = __builtin_amdgcn_readlane(fo, x);
          beat += (Sx > S || (Sx == S && fx < f)) ? 1 : 0;
        }
      }
      if (i < nt && beat < n) {
        orule[beat] = f;
        oscore[beat] = (int64_t)S;
      }
    }
    if (lane >= min(nt, (int)n) && lane < n) {
      orule[lane] = -1;
      oscore[lane] = 0;
    }
    comb_reset(w, nt, bask, s, e);
  }
}

// Trial t is element t of the basket CSR (k_holdout_rank's): the walk runs over row trow[t]
// without h = bask[t], and out[t] is the place of h among the touched consequents, 0 when
// S(h) = 0 or the place exceeds n.
__global__ __launch_bounds__(256) void k_holdout_rank_combined(
    const int64_t* __restrict__ list_off, const int32_t* __restrict__ list_rule,
    const int64_t* __restrict__ ante_off, const int32_t* __restrict__ ante, const int32_t* __restrict__ cons,
    const int64_t* __restrict__ weight, int32_t F1, const int64_t* __restrict__ boff,
    const int32_t* __restrict__ bask, const int64_t* __restrict__ trow, int64_t T, int32_t n,
    int32_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char comb_lds[];
  const int W = (int)(blockDim.x >> 6);
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = lane_id();
  if ((int64_t)blockIdx.x * W + wv >= T) return;
  const CombRows w = comb_rows(comb_lds, wv, F1);
  for (int64_t t = (int64_t)blockIdx.x * W + wv; t < T; t += (int64_t)gridDim.x * W) {
    const int64_t u = uniform_i64(trow[t]);
    const int32_t h = __builtin_amdgcn_readfirstlane(bask[t]);
    const int64_t s = uniform_i64(boff[u]), e = uniform_i64(boff[u + 1]);
    for (int64_t i = s + lane; i < e; i += kWave) {
      const int32_t b = bask[i];
      if (b != h) atomicOr(&w.bs[b >> 5], 1u << (b & 31));
    }
    wave_lds_sync();
    const int nt = comb_walk(w, list_off, list_rule, ante_off, ante, cons, weight, bask, s, e, h, e - s - 1);
    const unsigned long long Sh = w.score[h];
    const int32_t fh = w.first[h];
    int beat = 0;
    for (int k0 = 0; k0 < nt; k0 += kWave) {
      const int k = k0 + lane;
      bool b = false;
      if (k < nt) {
        const int32_t co = w.touched[k];
        const unsigned long long So = w.score[co];
        b = So > Sh || (So == Sh && w.first[co] < fh);
      }
      beat += __popcll(__ballot(b));
    }
    if (lane == 0) out[t] = (Sh != 0ull && beat < n) ? beat + 1 : 0;
    comb_reset(w, nt, bask, s, e);
  }
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

// The grid of the combined kernels: one wave per unit up to 8 workgroups per CU, past that
// the persistent waves take several units each.
static unsigned comb_grid(int64_t units, int W) {
  static int ncu = 0;
  if (ncu <= 0) {
    int dev = 0, v = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev);
    ncu = std::max(1, v);
  }
  return (unsigned)std::min<int64_t>((units + W - 1) / W, (int64_t)8 * ncu);
}

// out_rule: int32 [M, n] first rule ids, -1 padded; out_score: int64 [M, n] scores, 0 padded.
// weight: int64 [R], 1 .. 2^32.  Returns 2 without a launch when one wave's rows do not fit
// the LDS (fa_combine.h), 3 for R >= 2^31 - 1.
FA_API int fa_hip_recommend_combined(const int64_t* list_off, const int32_t* list_rule, const int64_t* ante_off,
                                     const int32_t* ante, const int32_t* cons, const int64_t* weight, int64_t R,
                                     int32_t F1, const int64_t* boff, const int32_t* bask, int64_t M, int32_t n,
                                     int32_t* out_rule, int64_t* out_score, hipStream_t st) {
  if (n < 1 || n > kWave) return (int)hipErrorInvalidValue;
  if (M <= 0) return 0;
  if (R >= (int64_t)INT32_MAX) return 3;
  const int W = combine_waves(F1);
  if (W == 0) return 2;            // caller falls back to the host path
  const int lds = (int)std::max<int64_t>(16, W * combine_wave_bytes(F1));
  const hipError_t err = hipFuncSetAttribute((const void*)k_recommend_combined,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (err != hipSuccess) return (int)err;
  hipLaunchKernelGGL(k_recommend_combined, dim3(comb_grid(M, W)), dim3(64 * W), (size_t)lds, st, list_off, list_rule,
                     ante_off, ante, cons, weight, F1, boff, bask, M, n, out_rule, out_score);
  FA_LAUNCH_RET();
}

// out: int32 [T] places 1..n or 0, one per element of the basket CSR; trow: its row
FA_API int fa_hip_holdout_rank_combined(const int64_t* list_off, const int32_t* list_rule, const int64_t* ante_off,
                                        const int32_t* ante, const int32_t* cons, const int64_t* weight, int64_t R,
                                        int32_t F1, const int64_t* boff, const int32_t* bask, const int64_t* trow,
                                        int64_t T, int32_t n, int32_t* out, hipStream_t st) {
  if (n < 1 || n > kWave) return (int)hipErrorInvalidValue;
  if (T <= 0) return 0;
  if (R >= (int64_t)INT32_MAX || T >= (int64_t)INT32_MAX) return 3;
  const int W = combine_waves(F1);
  if (W == 0) return 2;            // caller falls back to the host path
  const int lds = (int)std::max<int64_t>(16, W * combine_wave_bytes(F1));
  const hipError_t err = hipFuncSetAttribute((const void*)k_holdout_rank_combined,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (err != hipSuccess) return (int)err;
  hipLaunchKernelGGL(k_holdout_rank_combined, dim3(comb_grid(T, W)), dim3(64 * W), (size_t)lds, st, list_off,
                     list_rule, ante_off, ante, cons, weight, F1, boff, bask, trow, T, n, out);
  FA_LAUNCH_RET();
}
