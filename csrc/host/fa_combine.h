// The combined-scoring kernels' LDS rule, defined once.  (No counterpart in the reference:
// every firing rule of a basket adds its weight to its consequent, see docs/PARITY.md
// "Combined scoring".)
//
// The kernels and their launchers (csrc/hip/recommend.hip k_recommend_combined /
// k_holdout_rank_combined) include this header; libfa_host.so exports the functions by
// name (rules.cpp fa_combine_*), and fastapriori_amd.ops.primitives and the tests read
// them there and hold no copy.
//
// Plain C++ like fa_query.h and fa_limits.h: g++ and hipcc both read it.
#pragma once
#include <stdint.h>

namespace fa {

// The most LDS a launch may be given (a CU's 160 KiB) and the most waves of a workgroup.
constexpr int64_t kCombLdsMax = 160 * 1024;
constexpr int kCombMaxWaves = 4;

constexpr int64_t combine_align16(int64_t b) { return (b + 15) & ~(int64_t)15; }

// One wave's rows over the F1 frequent items, each from a 16-B boundary and in this
// order: the int64 scores, the int32 first rules, the list of touched consequents
// (int32; at most F1 distinct ones) and the basket bitset (32-bit words).
constexpr int64_t combine_score_bytes(int64_t F1) { return combine_align16(F1 * 8); }
constexpr int64_t combine_first_bytes(int64_t F1) { return combine_align16(F1 * 4); }
constexpr int64_t combine_touched_bytes(int64_t F1) { return combine_align16(F1 * 4); }
constexpr int64_t combine_bits_bytes(int64_t F1) { return combine_align16(((F1 + 31) / 32) * 4); }
constexpr int64_t combine_wave_bytes(int64_t F1) {
  return combine_score_bytes(F1) + combine_first_bytes(F1) + combine_touched_bytes(F1) + combine_bits_bytes(F1);
}

// Waves per workgroup: 4, 2 or 1, the most whose rows fit kCombLdsMax; 0 when one wave
// does not fit (the launchers then return 2 and the caller takes the host path).
constexpr int combine_waves(int64_t F1) {
  for (int w = kCombMaxWaves; w >= 1; w >>= 1)
    if (w * combine_wave_bytes(F1) <= kCombLdsMax) return w;
  return 0;
}

}  // namespace fa
