// Common definitions for the CDNA4 (gfx950) kernels of FastApriori-AMD.
//
// All kernels are written for 64-lane wavefronts and launched from thin
// extern "C" launchers (ctypes ABI: raw device pointers + hipStream_t), which
// return the hipError_t of the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define FA_API extern "C" __attribute__((visibility("default")))

#define FA_LAUNCH_RET() return (int)hipGetLastError()

namespace fa {

constexpr int kWave = 64;

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

// 64-bit popcount-accumulate: lowers to two accumulating v_bcnt_u32_b32.
__device__ __forceinline__ uint32_t popc64_acc(uint64_t x, uint32_t acc) {
  return acc + (uint32_t)__popc((uint32_t)x) + (uint32_t)__popc((uint32_t)(x >> 32));
}

// Inclusive wave64 prefix sum on the VALU with DPP (no LDS traffic, unlike
// __shfl_up which lowers to ds_bpermute): row_shr 1/2/4/8 inside each 16-lane
// row, then row_bcast:15 and row_bcast:31 across rows (GFX9-family DPP).
__device__ __forceinline__ int wave_scan_incl_dpp(int v) {
  const int lane = (int)(threadIdx.x & 63);
  const int r = lane & 15;
  int t;
  t = __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false); if (r >= 1) v += t;   // row_shr:1
  t = __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false); if (r >= 2) v += t;   // row_shr:2
  t = __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false); if (r >= 4) v += t;   // row_shr:4
  t = __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false); if (r >= 8) v += t;   // row_shr:8
  t = __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false); if ((lane & 31) >= 16) v += t;  // row_bcast:15
  t = __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false); if (lane >= 32) v += t;          // row_bcast:31
  return v;
}

__device__ __forceinline__ int wave_last(int v) { return __builtin_amdgcn_readlane(v, 63); }

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Inclusive wave64 prefix sum of 64-bit values (shuffles: DPP moves 32 bits).
__device__ __forceinline__ int64_t wave_scan_incl_i64(int64_t v) {
  const int lane = (int)(threadIdx.x & 63);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// the wave scan / wave sum of a value's own type (what the workgroup forms below build on)
__device__ __forceinline__ int wave_scan_incl(int v) { return wave_scan_incl_dpp(v); }
__device__ __forceinline__ int64_t wave_scan_incl(int64_t v) { return wave_scan_incl_i64(v); }
__device__ __forceinline__ int wave_sum(int v) { return (int)wave_sum_u32((uint32_t)v); }
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { return wave_sum_u32(v); }
__device__ __forceinline__ int64_t wave_sum(int64_t v) { return (int64_t)wave_sum_u64((unsigned long long)v); }

// ---------------------------------------------------------------------------
// Workgroup scans and sums over W waves (blockDim.x = 64 W): every wave leaves its
// total in LDS, one barrier, every thread adds the totals it needs.  Common contract:
//   * every thread of the workgroup must reach the call (no early return before it,
//     no call under a condition that differs inside the workgroup);
//   * scratch: W * N elements of T in LDS, passed by the caller.  It is written
//     before the call's barrier and read after it, so it may be written again (by
//     another call or anything else) only after one more __syncthreads of the
//     caller's; wg_scan_chunks holds that barrier itself;
//   * T is the type of the per-wave scan (int: DPP, int64_t: shuffles); the sums
//     across waves are taken in the type of the results (A), which may be wider.
// ---------------------------------------------------------------------------

// The step across waves, which the forms below share (use it directly where a wave
// already has its totals, e.g. from a ballot): lane src of every wave holds the wave's
// totals x[0 .. N); before[j] = sum of x[j] over the waves before this one, total[j] =
// the workgroup's sum (the same in every thread).  One __syncthreads, none after the reads.
template <int W, int N, typename T, typename A>
__device__ __forceinline__ void wg_wave_prefix(const T (&x)[N], int src, T* scratch, A (&before)[N], A (&total)[N]) {
  const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6);
#pragma unroll
  for (int j = 0; j < N; ++j)
    if (lane == src) scratch[j * W + w] = x[j];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < N; ++j) {
    A bef = 0, tot = 0;
#pragma unroll 4
    for (int k = 0; k < W; ++k) {
      const A t = (A)scratch[j * W + k];
      bef += k < w ? t : (A)0;
      tot += t;
    }
    before[j] = bef;
    total[j] = tot;
  }
}

// One-shot exclusive scan of N values per thread: excl[j] = sum of v[j] over the
// threads before this one, total[j] as above.
template <int W, int N, typename T, typename A>
__device__ __forceinline__ void wg_scan_excl(const T (&v)[N], T* scratch, A (&excl)[N], A (&total)[N]) {
  T incl[N];
#pragma unroll
  for (int j = 0; j < N; ++j) incl[j] = wave_scan_incl(v[j]);
  wg_wave_prefix<W>(incl, 63, scratch, excl, total);
#pragma unroll
  for (int j = 0; j < N; ++j) excl[j] += (A)incl[j] - (A)v[j];
}

template <int W, typename T, typename A>
__device__ __forceinline__ A wg_scan_excl(T v, T* scratch, A& total) {
  const T v1[1] = {v};
  A e[1], t[1];
  wg_scan_excl<W>(v1, scratch, e, t);
  total = t[0];
  return e[0];
}

// Workgroup sums of N values per thread, returned to every thread.
template <int W, int N, typename T>
__device__ __forceinline__ void wg_sum(const T (&v)[N], T* scratch, T (&total)[N]) {
  T s[N], before[N];
#pragma unroll
  for (int j = 0; j < N; ++j) s[j] = wave_sum(v[j]);
  wg_wave_prefix<W>(s, 0, scratch, before, total);
}

template <int W, typename T>
__device__ __forceinline__ T wg_sum(T v, T* scratch) {
  const T v1[1] = {v};
  T t[1];
  wg_sum<W>(v1, scratch, t);
  return t[0];
}

// Exclusive scan of n elements (N interleaved sequences) by ONE workgroup, in chunks of
// 64 W elements with an int64 carry.  For every element i < n, in order of the chunks:
//   load(i, v)            fills v[0 .. N) (T; a chunk's sum per wave must fit T);
//   store(i, before, v)   before[j] = carry[j] + v[j] of every element < i (int64).
// Both run in the same thread, load first, so a load may leave what it read in a local
// that its store uses (a kept element's payload).  On return carry[j] has grown by the
// whole sum, in every thread.
// Two __syncthreads per chunk.  The carry lives in registers: every thread adds the
// same wave totals from scratch, so no thread has to publish it and only scratch is
// shared -- one barrier between its writes and its reads (wg_scan_excl's), one between
// those reads and the next chunk's writes.  (Hand-written forms kept the carry in an
// LDS word written by the last thread, which took a third barrier.)  The trailing
// barrier also lets the caller reuse scratch, or call again, right after the return.
template <int W, int N, typename T, class Load, class Store>
__device__ __forceinline__ void wg_scan_chunks(int64_t n, int64_t (&carry)[N], T* scratch, Load&& load,
                                               Store&& store) {
  for (int64_t b0 = 0; b0 < n; b0 += 64 * W) {
    const int64_t i = b0 + threadIdx.x;
    T v[N];
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = 0;
    if (i < n) load(i, v);
    int64_t before[N], total[N];
    wg_scan_excl<W>(v, scratch, before, total);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      before[j] += carry[j];
      carry[j] += total[j];
    }
    if (i < n) store(i, before, v);
    __syncthreads();
  }
}

// one sequence: load(i) returns the value, store(i, before, v); returns the final carry
template <int W, typename T, class Load, class Store>
__device__ __forceinline__ int64_t wg_scan_chunks(int64_t n, int64_t carry, T* scratch, Load&& load, Store&& store) {
  int64_t c[1] = {carry};
  wg_scan_chunks<W, 1>(
      n, c, scratch, [&](int64_t i, T (&v)[1]) { v[0] = load(i); },
      [&](int64_t i, const int64_t (&before)[1], const T (&v)[1]) { store(i, before[0], v[0]); });
  return c[0];
}

// Orders this wave's LDS accesses across lanes.  The LDS executes one wave's DS
// instructions in issue order, so a read issued after another lane's write sees
// it: only the compiler must not reorder or cache them.  (A memory-model fence
// would also emit s_waitcnt vmcnt(0), draining every prefetched global load of
// a software-pipelined loop at each call: that cost the pair kernel ~7 ms.)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_wave_barrier();
  __asm__ __volatile__("" ::: "memory");
}

// Row-start masks for U consecutive 64-position windows of a wave's CSR span.
// Lane l owns row l = [srel, ...) (rows non-empty, so starts are distinct);
// bit j of S[u] is set when a row starts at position q0 + 64u + j.  words: U
// per-wave LDS scratch words.  The owner row of position q0 + 64u + lane is then
// (starts before the window) + popc(S[u] & lanes <= lane) - 1.
template <int U>
__device__ __forceinline__ void window_starts(unsigned long long* words, int srel, int q0,
                                              unsigned long long (&S)[U]) {
  const int lane = (int)(threadIdx.x & 63);
  if (lane < U) words[lane] = 0ull;
  wave_lds_sync();
  const int b = srel - q0;
  if (b >= 0 && b < 64 * U) atomicOr(&words[b >> 6], 1ull << (b & 63));
  wave_lds_sync();
#pragma unroll
  for (int u = 0; u < U; ++u) S[u] = words[u];
  wave_lds_sync();
}

__device__ __forceinline__ unsigned long long lanes_le_mask() {
  const int lane = (int)(threadIdx.x & 63);
  return lane == 63 ? ~0ull : ((2ull << lane) - 1);
}

// Bijective XCD-aware remap (cdna_hip_programming.md §5 "XCD swizzle must be
// bijective"): consecutive logical ids land on the same XCD's L2.
__device__ __forceinline__ uint32_t xcd_remap(uint32_t orig, uint32_t nwg) {
  const uint32_t nx = 8;
  if (nwg < nx) return orig;
  uint32_t q = nwg / nx, r = nwg % nx, xcd = orig % nx;
  uint32_t base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + orig / nx;
}

// Lexicographic compare of the (k-1)-row `a` with row S minus position p: the step of
// the "subset index" binary search, S - {S[p]} in the sorted level below (rules.hip
// k_rule_gen reads the found row's count, condense.hip k_sup_mark marks the found row).
__device__ __forceinline__ int cmp_skip(const int32_t* __restrict__ a, const int32_t* __restrict__ s, int k,
                                        int p) {
  for (int i = 0, j = 0; i < k - 1; ++i, ++j) {
    if (j == p) ++j;
    const int32_t x = a[i], y = s[j];
    if (x != y) return x < y ? -1 : 1;
  }
  return 0;
}

struct DlDesc;   // ../host/fa_dl.h

}  // namespace fa

// Launchers called across files (the bundle post step, gen.hip dl_post): the device
// piece plan (levels.hip) and the slab count (count.hip; cls: fa_dl.h kSlab* bits)
FA_API int fa_hip_dl_plan(const fa::DlDesc* desc, int L, long long* ctl, int F1, int32_t* item_map, void* rec,
                          int64_t max_pieces, int32_t* part, int64_t part_cap, int32_t* gpre, int64_t gpre_cap,
                          int sw, hipStream_t st);
// ... and the regrouping step between the generator and the plan (regroup.hip)
FA_API int64_t fa_hip_dl_regroup_need(const fa::DlDesc* desc, int L);
FA_API int fa_hip_dl_regroup(const fa::DlDesc* desc, int L, void* scratch, int64_t bytes, fa::DlDesc* out,
                             long long* stats, hipStream_t st);
FA_API int fa_hip_dl_unpermute(const uint32_t* in, const int32_t* perm, int64_t C, uint32_t* out, hipStream_t st);
FA_API int fa_hip_count_slab_rec_cls(const int64_t* roff, const int32_t* ranks, const int32_t* src, int64_t ncols,
                                     const int32_t* item_map, int F1, int n_used, const int32_t* gpre,
                                     const void* rec, int G, int C, const int32_t* wword, uint32_t* out, int sw,
                                     int n_wg, const uint64_t* bm, int64_t Wp, hipStream_t st,
                                     const int32_t* bm_rows, const int32_t* g_dev, int cls);
