// The query counter's limits and its LDS rule, defined once.  (No counterpart in the
// reference: counting the support of GIVEN itemsets over the raw parsed rows.)
//
// The kernel (csrc/hip/query.hip k_query_slab), its launcher's checks, the host plan
// and the C++ reference (csrc/host/query.cpp) include this header;
// fastapriori_amd.ops.primitives and the tests read the same values by name through
// libfa_host.so's fa_query_limits export and hold no copy.  The mining kernels' table
// (fa_limits.h) is another list: nothing here is shared with them.
//
// Plain C++ like fa_slab.h and fa_limits.h: g++ and hipcc both read it.
#pragma once
#include <stdint.h>

// kQThreads: threads per workgroup.  kQAcc: the most queries of one window (one int32
// LDS accumulator each, owned by thread q % kQThreads).  kQMaxItems: the most items of
// one window (slab rows are u16, kQAbsent marks an item outside the window).
// kQMaxWidth: the widest slab, in 64-row words; the widths are the powers of two up to
// it, widest first.  kQLdsMax: the most LDS a launch may be given (a CU's 160 KiB).
// kQWinFields: int64 fields of one window descriptor (QWin below).
#define FA_QUERY_LIMITS(X)                                                                   \
  X(kQThreads, 1024) X(kQAcc, 8192) X(kQMaxItems, 65535) X(kQAbsent, 0xFFFF) X(kQMaxWidth, 16) \
  X(kQLdsMax, 160 * 1024) X(kQWinFields, 8)

namespace fa {

#define FA_QUERY_X(name, value) constexpr int name = value;
FA_QUERY_LIMITS(FA_QUERY_X)
#undef FA_QUERY_X

static_assert((kQMaxWidth & (kQMaxWidth - 1)) == 0, "the widths are powers of two");
static_assert(kQMaxItems <= kQAbsent, "a slab row is a u16 below the absent mark");

// One window of the plan: n_q queries over n_items items on slabs of sw words.  Its
// tables are slices of the plan's arrays: tab[tab_off + used index] -> slab row (u16),
// qoff[qoff_off .. + n_q] (int32, relative to qrow_off) and qrow[qrow_off + ..] (u16),
// perm[q_base + i] = the query's place in the caller's count vector.
struct QWin {
  int64_t n_q, n_items, sw, tab_off, qoff_off, qrow_off, q_base, reserved;
};
static_assert(sizeof(QWin) == 8 * kQWinFields, "kQWinFields lists every field");

constexpr bool query_width_ok(int64_t sw) { return sw >= 1 && sw <= kQMaxWidth && (sw & (sw - 1)) == 0; }

constexpr int64_t query_align16(int64_t b) { return (b + 15) & ~(int64_t)15; }
// LDS bytes of a window, each part from a 16-B boundary: the slab (n_items rows of sw
// 64-row words), the accumulators (int32 per query) and the staged row offsets of one
// tile (64 sw rows + 1, int64: a tile's item span is not assumed to fit 32 bits).
constexpr int64_t query_slab_bytes(int64_t n_items, int64_t sw) { return query_align16(n_items * sw * 8); }
constexpr int64_t query_acc_bytes(int64_t n_q) { return query_align16(n_q * 4); }
constexpr int64_t query_lds_bytes(int64_t n_items, int64_t sw, int64_t n_q) {
  return query_slab_bytes(n_items, sw) + query_acc_bytes(n_q) + query_align16((64 * sw + 1) * 8);
}

// The widest slab of a window within `lds` bytes; 0: it does not fit at width 1.
constexpr int query_width(int64_t n_items, int64_t n_q, int64_t lds) {
  for (int sw = kQMaxWidth; sw >= 1; sw >>= 1)
    if (query_lds_bytes(n_items, sw, n_q) <= lds) return sw;
  return 0;
}

// A window within the limits and within `lds` bytes (the plan's invariant and the
// launcher's check).
constexpr bool query_window_ok(int64_t n_q, int64_t n_items, int64_t sw, int64_t lds) {
  return n_q >= 1 && n_q <= kQAcc && n_items >= 1 && n_items <= kQMaxItems && query_width_ok(sw) &&
         lds <= kQLdsMax && query_lds_bytes(n_items, sw, n_q) <= lds;
}

}  // namespace fa
