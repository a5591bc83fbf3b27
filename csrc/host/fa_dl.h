// The device bundle loop's contract, defined once: the control block's slots, the
// level descriptors, the loop's limits, the slab count's mode bits and the post step's
// argument block.  Four layers speak through them: gen.hip (generation, acceptance,
// the post step), levels.hip (plan, threshold), count.hip (the slab count's launcher
// and kernel) and, through libfa_host.so's fa_dl_layout export (dl_layout.cpp),
// fastapriori_amd.ops.primitives and models.apriori, which hold no copy.
//
// Plain C++ like fa_slab.h: g++ and hipcc both read it.
//
// Control block (device int64 [kDlCtl], mirrored to the host by the generator):
//   kDlStop      the chain stopped: every later kernel of the bundle exits at once
//   kDlLevels    accepted levels (incl. level 0)
//   kDlTotal     candidates of the accepted levels
//   kDlLastC     C of the last accepted level
//   slot 4 has two meanings, one per chain:
//   kDlTmax        host-loop chain (gen.hip ag_chain_dev): the bundle total's limit
//   kDlOverBound   device loop: the device row count n_src[0] exceeds the buffers'
//                  bound: nothing runs and the host raises
//   kDlMulti     level 0 needs several accumulator passes (counted window by window)
//   kDlNUsed     used items of level 0
//   kDlEnd       |F_{k-1}| < k or C_0 = 0: mining is over
//   kDlNl + l    n_l (input rows of level l)
//   kDlCl + l    C_l (candidates of level l)
//   kDlGl + l    G_l (parent rows with >= 1 candidate: the reference's group count)
//   kDlEmpty     the chain stopped on a speculative level with no candidates
//   kDlPieces    pieces of the device plan (levels.hip k_dl_pieces_scan)
//   kDlPiecesI32 the same as int32 in the word's low half: the count kernel's g_dev
//   (224 .. 351  the regrouping step's statistics: fa_regroup.h kRgStats)
//   kDlBits ..   used-item bitset of level 0, kDlBitsW words (F1 <= kAgMaxF1 bits)
// The host-loop chain's block is the first kDlGl words (no G_l, no bitset).
#pragma once
#include <stdint.h>

// name, value lists: expanded to the constexprs below and to fa_dl_layout's table
#define FA_DL_SLOTS(X)                                                                           \
  X(kDlStop, 0) X(kDlLevels, 1) X(kDlTotal, 2) X(kDlLastC, 3) X(kDlTmax, 4) X(kDlOverBound, 4) \
  X(kDlMulti, 5) X(kDlNUsed, 6) X(kDlEnd, 7) X(kDlNl, 8) X(kDlCl, 40) X(kDlGl, 72)             \
  X(kDlEmpty, 104) X(kDlPieces, 220) X(kDlPiecesI32, 221) X(kDlBits, 512) X(kDlBitsW, 512)     \
  X(kDlCtl, 1024)
// Limits: the longest prefix a device bundle takes; the levels of one bundle; the
// descriptor rows (and n_l slots: accepting level l writes n_{l+1}, so one more than
// the levels); prefix ids inline in a piece record (longer prefixes ride in gpre); the
// largest F1 of the device generator (8 bitset words per lane of a wave).
#define FA_DL_LIMITS(X) \
  X(kDlMaxM, 40) X(kDlMaxLevels, 31) X(kDlMaxL, 32) X(kDlInline, 12) X(kAgMaxF1, 32768)
// The slab count's mode, in two encodings (kept apart: the second is kernel immediates).
// fa_hip_count_slab_rec_cls's cls argument: the records carry class-layout flags
// (plan.cpp cls_layout); dense level (no all-zero-prefix test); packed u16 accumulators.
// k_count_slab_rec's flags argument: dense, u16 accumulators, then the candidate
// distribution's fields (fa_hip_set_piece_part): this rank, ranks - 1.
#define FA_DL_SLAB_MODE(X)                                                \
  X(kSlabCls, 1) X(kSlabDense, 2) X(kSlabAcc16, 4)                        \
  X(kSlabFlagDense, 4) X(kSlabFlagAcc16, 8) X(kSlabFlagPartShift, 8)      \
  X(kSlabFlagNpartsShift, 16) X(kSlabFlagPartMask, 255)
#define FA_DL_CONSTS(X) FA_DL_SLOTS(X) FA_DL_LIMITS(X) FA_DL_SLAB_MODE(X)

namespace fa {

#define FA_DL_X(name, value) constexpr int name = value;
FA_DL_CONSTS(FA_DL_X)
#undef FA_DL_X

static_assert(kDlMaxL == kDlMaxLevels + 1 && kDlNl + kDlMaxL <= kDlCl && kDlCl + kDlMaxL <= kDlGl &&
                  kDlGl + kDlMaxL <= kDlEmpty,
              "one n_l / C_l / G_l slot per descriptor row");
static_assert(kDlBitsW * 64 == kAgMaxF1 && kDlBits + kDlBitsW == kDlCtl, "the bitset ends the block");

// One accepted level of a bundle (host int64 [kDlMaxL][8]): written by
// fa_hip_dl_level0's caller (level 0: P .. m) and fa_hip_dl_more, read by levels.hip
struct DlDesc {
  int64_t P;      // parent rows P_l (device int32 [n][m])
  int64_t cnt;    // extensions per parent row (device int32; their ids at cnt + n)
  int64_t off;    // exclusive offsets of cnt (device int64 [n + 1])
  int64_t rows;   // candidate rows (device int32 [C][m + 1])
  int64_t m;      // parent row length
  int64_t n;      // parent rows
  int64_t C;      // candidates
  int64_t base;   // candidates of the levels before this one
};
static_assert(sizeof(DlDesc) == 64, "DlDesc layout (ops.primitives: S.desc's dtype)");

// post (optional, host): right after fa_hip_dl_more's synchronisation, with no return to
// the host interpreter in between, the bundle's device piece plan is queued
// (levels.hip fa_hip_dl_plan), the transaction-trimming decision is taken
// (FastApriori._trim_worth_it, the same binomial estimate), and when no trim is
// due the slab count itself is queued (count.hip fa_hip_count_slab_rec_cls): the GPU
// then counts while the host does its bookkeeping.  done: 0 nothing queued
// (stopped chain, multi-pass level, buffers too small), 1 planned (the caller trims,
// then counts), 2 planned and counted into out.
struct DlPost {
  // plan buffers (grow-only, the caller's): item_map int32 [F1], rec int4 [3 * rec_cap],
  // part int32 [part_cap], out uint32 [out_cap]
  int32_t* item_map; void* rec; int32_t* part; uint32_t* out;
  int64_t rec_cap, part_cap, out_cap;
  // the count's rows and LDS budget
  const int64_t* roff; const int32_t* ranks; const int32_t* src; const int32_t* wword;
  int64_t ncols; double lds_kernel; double lds_budget;
  // trimming decision (trim_ok = 0: never): c1 int64 [F1] item supports, alive uint8 [F1],
  // len_hist int64 [kTrimHist] (fa_limits.h; nullptr: decided by the caller), T rows, nnz, min rows, level k
  const int64_t* c1; const uint8_t* alive; const int64_t* len_hist;
  int64_t T, nnz, trim_min_rows, trim_ok, k;
  // out
  int64_t done, sw, cap, n_wg, C, trim;
  // prefix slab rows of levels with prefixes past kDlInline ids (levels.hip gpre), int32 [gpre_cap]
  int32_t* gpre; int64_t gpre_cap;
  // LDS bytes per accumulator: 4, 2 (unit weights: count.hip's packed u16 counters) or 1
  // (unit weights: single-writer bytes).  In: the narrowest the count may take -- below the
  // bundling's (fa_hip_dl_more's accb) it is taken where it moves the slab up to width 16
  // (fa_slab.h slab_acc_upgrade); out: what the plan and the count use
  double accb;
  // trim when the estimate keeps fewer than this share of the rows, or of the items
  // (FastApriori._trim_worth_it, TUNING.trim_rows_frac / trim_nnz_frac)
  double trim_rows_frac, trim_nnz_frac;
};
static_assert(sizeof(DlPost) == 33 * 8, "DlPost layout (ops.primitives.DlPostC)");

}  // namespace fa
