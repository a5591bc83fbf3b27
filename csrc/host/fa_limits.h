// The kernels' capacity limits and the padding they read past their inputs, defined once.
//
// A constant lives here when something outside its .hip file must agree with it: a
// caller sizes or pads a buffer by it, a caller or the host planner chooses a path by
// it, or a launcher rejects arguments beyond it (and a base constant a moved one is
// derived from: the derived value is then an expression).  Tile shapes, LDS strides
// and unroll factors that only their own kernel knows stay in the .hip files.  The
// kernels (prep.hip, count.hip, gen.hip, parse.hip) and the host planner (plan.cpp)
// include this header; fastapriori_amd.ops.primitives, models.apriori and the tests
// read the same list by name through libfa_host.so's fa_limits export (dl_layout.cpp)
// and hold no copy.
//
// Plain C++ like fa_slab.h and fa_dl.h: g++ and hipcc both read it.
#pragma once
#include <stdint.h>

// name, value lists: expanded to the constexprs below (int; FA_LIMITS_U32: uint32_t,
// so a hash stays a 32-bit multiply) and to fa_limits' table (int64_t)

// prep.hip.  Token histogram: LDS bins up to V = kLdsBins.  F1 ranking on the device:
// V <= kF1RankMax.  Heavy-hitter F1: 2 rows of 2^kSkLog sketch bins, one partial
// sketch per workgroup of at most kSkGridMax; the exact pass's LDS table has as many
// slots and holds kF1ExactMaxCand candidates (load <= 0.5).  Compression: the staged
// tiers' span in tokens (kCSpan), the longest row of the LDS sort (kLongMax), the wave
// tier's bitmap words per lane (kCwMaxWords: lane l owns words l + 64 m of 64 ranks).
// Dedup probe: occupancy bits, and the most rows a probe takes.  Trimming: alive flags
// in LDS up to F1 = kTrimAliveLds; the row-length histogram's bins (lengths past the
// last share it) and striped copies, the same for the fused compression's (kCmp*:
// either histogram feeds the trimming estimate, fa_slab.h).  Fused compression: a
// workgroup's staged span in tokens, the mid rows a wave sorts, the 256-rank blocks of
// a fused pair layout (kCmpMaxNB: a row's block counts are the bytes of one u64; equal
// to count.hip's kWBMaxNB, the blocks its wave-cooperative layout kernels keep in
// registers, which is another limit), the elements per workgroup of the aggregates' scan.
#define FA_LIMITS_PREP(X)                                                                       \
  X(kLdsBins, 16384) X(kF1RankMax, 2048) X(kSkLog, 14) X(kSkGridMax, 256)                       \
  X(kF1ExactMaxCand, 8192) X(kCSpan, 8192) X(kLongMax, 16384) X(kCwMaxWords, 16)                \
  X(kCwMaxF1, kCwMaxWords * 64 * 64) X(kProbeBits, 1 << 22) X(kProbeMaxRows, 1 << 24)           \
  X(kTrimAliveLds, 32768) X(kTrimHist, 256) X(kTrimStripes, 64) X(kCmpHist, 256)                \
  X(kCmpStripes, 64) X(kCmpSpan, 4096) X(kCmpMidPerWave, 8) X(kCmpMaxNB, 8) X(kScanChunk, 4096)
// count.hip.  Pair kernels: kPW waves per workgroup, each taking every kPW-th 64-row
// batch; the rows16 pipeline loads a batch's block counts and bases kPairAhead rounds
// ahead, unconditionally, so cnt (by 64 rows) and base are padded by kPairPadBatches
// batches (the read-ahead, the last batch's rows past T, one spare) and lr by
// kPairLrPad bytes (a batch's aligned dword staging reads; count.hip checks it against
// its stage); compress_rows allocates kPairCntSpare rows more.  Candidate kernel: the
// extensions of one workgroup (its LDS accumulators).  Slab kernel: threads per
// workgroup (plan.cpp orders the piece records by them).  Window compaction: bit-sliced
// counts of kWinPlanes planes, so at most kWinMaxItems items.
#define FA_LIMITS_COUNT(X)                                                                      \
  X(kPW, 16) X(kPairAhead, 3) X(kPairPadBatches, kPairAhead * kPW + 2) X(kPairLrPad, 1024)      \
  X(kPairCntSpare, 64) X(kMaxBlockExt, 1024) X(kSlabThreads, 1024) X(kWinPlanes, 11)            \
  X(kWinMaxItems, (1 << kWinPlanes) - 1)
// gen.hip: the fewest u32 words of a chain's used-item bitset (ag_mark_words below);
// parent rows per block of the device loop's multi-workgroup scan.  parse.hip: bins of
// the tile parser's fused F1 histogram (a larger id turns it off).
#define FA_LIMITS_GEN_PARSE(X) X(kAgMarkMinWords, 128) X(kDsBlk, 4096) X(kHistCap, 8192)
#define FA_LIMITS_INT(X) FA_LIMITS_PREP(X) FA_LIMITS_COUNT(X) FA_LIMITS_GEN_PARSE(X)
// the sketch's two multiplicative hashes (the exact pass's table probes with the first)
#define FA_LIMITS_U32(X) X(kSkA0, 0x9E3779B1u) X(kSkA1, 0x85EBCA77u)

namespace fa {

#define FA_LIMITS_X(name, value) constexpr int name = value;
FA_LIMITS_INT(FA_LIMITS_X)
#undef FA_LIMITS_X
#define FA_LIMITS_X(name, value) constexpr uint32_t name = value;
FA_LIMITS_U32(FA_LIMITS_X)
#undef FA_LIMITS_X

static_assert(kF1ExactMaxCand * 2 == 1 << kSkLog, "the exact pass's table is the sketch row's size, half full");
static_assert(kCmpHist == kTrimHist, "one trimming estimate reads either row-length histogram");
static_assert((kTrimStripes & (kTrimStripes - 1)) == 0 && (kCmpStripes & (kCmpStripes - 1)) == 0,
              "a workgroup's stripe is its index masked");
static_assert(kCmpMaxNB == 8, "a row's block counts are the 8 bytes of one u64");
static_assert(kPairPadBatches >= kPairAhead * kPW + 1, "the read-ahead, and the last batch's rows past T");

// u32 words of a chain's used-item bitset
constexpr int ag_mark_words(int F1) { return (F1 + 31) / 32 > kAgMarkMinWords ? (F1 + 31) / 32 : kAgMarkMinWords; }

}  // namespace fa
