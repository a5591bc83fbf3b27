// Support counts of GIVEN itemsets over the raw parsed rows (no counterpart in the
// reference; --count-itemsets / --verify-counts).  A second counter that shares nothing
// with the miner: it reads the shard's CSR as the parser left it (offsets int64, items
// int32 raw ids) and knows no compression, pair layout, generator or planner; the only
// shared pieces are fa_hip.h's launch conventions.  Limits and the LDS rule:
// ../host/fa_query.h; the plan (windows, tables, query CSR) and the C++ reference on the
// same inputs: ../host/query.cpp.
#include <algorithm>

#include "fa_hip.h"
#include "../host/fa_query.h"

namespace fa {

// One workgroup of kQThreads takes one window (QWin) and a contiguous range of row
// tiles, a tile being 64 SW rows, and is persistent over the range.  Per tile:
//   1. zero the slab (n_items rows of SW words: bit b of word w of row r = line
//      64 w + b of the tile holds item r) and stage the tile's SW*64 + 1 row offsets in
//      LDS, the entries past the shard's end as INT64_MAX;
//   2. stream the tile's contiguous item span coalesced, position = thread + i * 1024:
//      raw id -> used index (lut, global) -> slab row (the window's u16 table, global,
//      small and L2-resident); for an item of the window, its line by a binary search of
//      the staged offsets -- a fixed log2(64 SW) steps, so every lane leaves the loop
//      together -- and one ds_or of the line's bit;
//   3. thread t owns queries t, t + 1024, ..: the AND of the query's slab rows over the
//      SW words, popcount, added to its own int32 LDS accumulator (single writer, no
//      atomics).  A query of one item is the AND of one row.  Nothing is assumed about
//      the queries: no prefix grouping, no order inside a query.
// Banks: a slab row is SW * 8 bytes, so at SW = 16 (128-B rows) lanes reading the SAME
// word of different rows would share 2 of the 64 banks.  Lane t therefore walks the words
// in the order (j + t) mod SW: the words are independent (popcounts add), so the order
// is free, and the lanes of a group spread over all SW words of their rows.  At SW = 1
// (8-B rows) the row index alone spreads the lanes.
// At the end of its range the workgroup adds every non-zero accumulator to the global
// 64-bit count of the query's place (perm) with one atomic: sums of integers, so the
// result does not depend on the order of the workgroups.
template <int SW>
__device__ __forceinline__ void query_tiles(const int64_t* __restrict__ offsets, const int32_t* __restrict__ items,
                                            int64_t n_rows, const int32_t* __restrict__ lut, int64_t lut_n,
                                            const uint16_t* __restrict__ tab, const int32_t* __restrict__ qoff,
                                            const uint16_t* __restrict__ qrow, int n_q, int n_items, int64_t tile0,
                                            int64_t tile1, unsigned long long* slab, int32_t* acc, int64_t* toff) {
  constexpr int RT = 64 * SW;
  const int t = (int)threadIdx.x;
  for (int64_t tile = tile0; tile < tile1; ++tile) {
    const int64_t r0 = tile * RT;
    const int nr = (int)min((int64_t)RT, n_rows - r0);
    for (int i = t; i < n_items * SW; i += kQThreads) slab[i] = 0ull;
    for (int i = t; i <= RT; i += kQThreads) toff[i] = i <= nr ? offsets[r0 + i] : INT64_MAX;
    __syncthreads();
    const int64_t p1 = toff[nr];
    for (int64_t p = toff[0] + t; p < p1; p += kQThreads) {
      const int32_t id = items[p];
      if ((uint64_t)(int64_t)id >= (uint64_t)lut_n) continue;      // an id outside the table is in no query
      const int32_t u = lut[id];
      if (u < 0) continue;
      const uint32_t row = tab[u];
      if (row == (uint32_t)kQAbsent) continue;
      // the last line i with toff[i] <= p (empty lines share an offset with the next line;
      // toff[nr] = p1 > p and the entries after it are INT64_MAX, so i < nr)
      int i = 0;
#pragma unroll
      for (int step = RT / 2; step > 0; step >>= 1)
        if (toff[i + step] <= p) i += step;
      atomicOr(&slab[row * SW + (i >> 6)], 1ull << (i & 63));
    }
    __syncthreads();
    for (int q = t; q < n_q; q += kQThreads) {
      unsigned long long a[SW];
#pragma unroll
      for (int j = 0; j < SW; ++j) a[j] = ~0ull;
      const int b = qoff[q], e = qoff[q + 1];
      for (int x = b; x < e; ++x) {
        const unsigned long long* r = slab + (int)qrow[x] * SW;
#pragma unroll
        for (int j = 0; j < SW; ++j) a[j] &= r[(j + t) & (SW - 1)];
      }
      uint32_t c = 0;
#pragma unroll
      for (int j = 0; j < SW; ++j) c = popc64_acc(a[j], c);
      acc[q] += (int32_t)c;
    }
    __syncthreads();
  }
}

// grid = W windows x R ranges: block b takes window b / R and the tiles
// [part * tiles / R, (part + 1) * tiles / R) of it, part = b % R (none when R > tiles).
__global__ __launch_bounds__(kQThreads) void k_query_slab(
    const int64_t* __restrict__ offsets, const int32_t* __restrict__ items, int64_t n_rows,
    const int32_t* __restrict__ lut, int64_t lut_n, const QWin* __restrict__ wins, int R,
    const uint16_t* __restrict__ tab, const int32_t* __restrict__ qoff, const uint16_t* __restrict__ qrow,
    const int64_t* __restrict__ perm, unsigned long long* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char qlds[];
  const QWin w = wins[blockIdx.x / (unsigned)R];
  const int part = (int)(blockIdx.x % (unsigned)R);
  const int sw = (int)w.sw, n_q = (int)w.n_q, n_items = (int)w.n_items;
  const int64_t tiles = (n_rows + 64 * sw - 1) / (64 * sw);
  const int64_t tile0 = tiles * part / R, tile1 = tiles * (part + 1) / R;
  if (tile0 >= tile1) return;                                      // the whole workgroup: no barrier is skipped
  unsigned long long* slab = (unsigned long long*)qlds;
  int32_t* acc = (int32_t*)(qlds + query_slab_bytes(n_items, sw));
  int64_t* toff = (int64_t*)(qlds + query_slab_bytes(n_items, sw) + query_acc_bytes(n_q));
  for (int q = threadIdx.x; q < n_q; q += kQThreads) acc[q] = 0;   // thread q % kQThreads owns acc[q] throughout
  const uint16_t* wtab = tab + w.tab_off;
  const int32_t* wqoff = qoff + w.qoff_off;
  const uint16_t* wqrow = qrow + w.qrow_off;
#define FA_Q_CASE(SW)                                                                                         \
  case SW:                                                                                                    \
    query_tiles<SW>(offsets, items, n_rows, lut, lut_n, wtab, wqoff, wqrow, n_q, n_items, tile0, tile1, slab, \
                    acc, toff);                                                                               \
    break;
  switch (sw) {
    FA_Q_CASE(16) FA_Q_CASE(8) FA_Q_CASE(4) FA_Q_CASE(2) FA_Q_CASE(1)
    default: return;                                               // (the launcher refuses other widths)
  }
#undef FA_Q_CASE
  // query_tiles ends on a barrier; every accumulator is read by the thread that wrote it
  for (int q = threadIdx.x; q < n_q; q += kQThreads) {
    const int32_t c = acc[q];
    if (c) atomicAdd(&out[perm[w.q_base + q]], (unsigned long long)c);
  }
}

}  // namespace fa

using namespace fa;

// Counts of every window's queries over the rows [0, n_rows) of a CSR shard, added into
// out (uint64, zeroed by the caller; perm places a window's query in it).  wins_host: the
// W descriptors in HOST memory for the checks below, wins_dev the same on the device;
// every other pointer is device memory.  One launch for all windows.
//
// Workgroups, the written rule: a target of max_wg when it is positive, else 2 per CU
// (a workgroup holds most of a CU's LDS, so one is resident and the second waits: the
// factor evens out the ranges' tails); every window gets R = max(1, target / W) row
// ranges, raised so that a range stays below 2^30 rows, and the grid is W * R.  R may
// exceed a window's tile count: the surplus workgroups leave at once and add nothing.
//
// Overflow: a line adds at most 1 to a query, so an accumulator never exceeds its
// workgroup's rows: tiles * (part + 1) / R - tiles * part / R <= tiles / R + 1 tiles of at
// most 64 * 16 rows, i.e. at most n_rows / R + 2048 < 2^30 + 2^11 rows by the rule above,
// inside int32.  The global sums are uint64 and bounded by n_rows < 2^63.
//
// Returns 0 (no launch when W = 0 or n_rows = 0), a HIP error, or 3 with no launch for
// arguments outside fa_query.h's limits: lds above kQLdsMax, or a window that
// query_window_ok refuses.
FA_API int fa_hip_query_count(const int64_t* offsets, const int32_t* items, int64_t n_rows, const int32_t* lut,
                              int64_t lut_n, const int64_t* wins_host, const int64_t* wins_dev, int64_t W,
                              const uint16_t* tab, const int32_t* qoff, const uint16_t* qrow, const int64_t* perm,
                              uint64_t* out, int64_t lds, int max_wg, hipStream_t st) {
  if (W < 0 || n_rows < 0 || lut_n < 0 || max_wg < 0 || lds < 0 || lds > kQLdsMax) return 3;
  int64_t need = 0;
  for (int64_t i = 0; i < W; ++i) {
    const QWin* w = (const QWin*)wins_host + i;
    if (!query_window_ok(w->n_q, w->n_items, w->sw, lds)) return 3;
    if (w->tab_off < 0 || w->qoff_off < 0 || w->qrow_off < 0 || w->q_base < 0) return 3;
    need = std::max(need, query_lds_bytes(w->n_items, w->sw, w->n_q));
  }
  if (W == 0 || n_rows == 0) return 0;
  int64_t target = max_wg;
  if (target <= 0) {
    int dev = 0, ncu = 256;
    if (hipGetDevice(&dev) == hipSuccess)
      (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    target = 2 * (int64_t)ncu;
  }
  int64_t R = std::max<int64_t>(1, target / W);
  R = std::max(R, (n_rows + ((int64_t)1 << 30) - 1) >> 30);
  if (R >= (int64_t)INT32_MAX || W * R >= (int64_t)INT32_MAX) return 3;
  const hipError_t e = hipFuncSetAttribute((const void*)k_query_slab, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)need);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_query_slab, dim3((unsigned)(W * R)), dim3(kQThreads), (size_t)need, st, offsets, items, n_rows,
                     lut, lut_n, (const QWin*)wins_dev, (int)R, tab, qoff, qrow, perm,
                     (unsigned long long*)out);
  FA_LAUNCH_RET();
}
