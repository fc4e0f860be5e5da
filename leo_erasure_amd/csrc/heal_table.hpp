// heal_table.hpp — the pattern table behind leoec_heal_dev's fused path
// (heal.hip, heal_impl.hpp): for one GF(2^8) code, one record per mask of
// lost block ids with 1..m bits set among k + m, holding what gf8_heal needs
// to rebuild those blocks of one object: the k survivor ids, the lost ids and
// the v_perm tables of the decoding coefficients.  Host only: no HIP here, so
// the table builds and tests without a device (heal_table.cpp).
//
// Device image, 32-bit words:
//   [0, 160)              binom[b][i] = C(b, i), b < 32, i <= 4   (kHealBinom)
//   [160, 165)            first[p]: index of the first record with p bits set
//   [165, 176)            record words, record count, zero padding
//   [176 + idx * rw, ...) record idx, rw = 8 + 5 m k words:
//       words 0..7   ids as bytes: k survivors (first k intact ids ascending),
//                    then kHealMaxLost output ids ascending, 0xFF = row unused
//       words 8..    row r, input j at 8 + 5 (r k + j): the five gf8_tables
//                    words of coefficient (r, j); rows past the mask's bit
//                    count are zero
// A record's index is the combinatorial rank of its mask: with the set bits
// b_1 < b_2 < ... < b_p,  idx = first[p] + sum_i C(b_i, i), and first[p] =
// sum over q in [1, p) of C(k + m, q).  Every mask of p bits among n lands
// once in [first[p], first[p] + C(n, p)).
#pragma once

#include <cstdint>
#include <functional>
#include <vector>

namespace leoec {

constexpr int kHealMaxIds = 32;   // k + m: one bit of a mask word per block id
constexpr int kHealMaxLost = 4;   // output rows of one record (= detail::kMaxR)
constexpr int kHealMaxK = 16;     // survivor ids of one record (= detail::kMaxK)
constexpr uint32_t kHealBinom = 0;
constexpr uint32_t kHealFirst = kHealMaxIds * (kHealMaxLost + 1);
constexpr uint32_t kHealRecWords = kHealFirst + kHealMaxLost + 1;
constexpr uint32_t kHealRecCount = kHealRecWords + 1;
constexpr uint32_t kHealHeaderWords = 176;
constexpr uint32_t kHealIdWords = 8;
constexpr uint32_t kHealNoId = 0xFFu;

constexpr uint32_t heal_binom(uint32_t b, uint32_t i) {
  uint64_t c = 1;
  if (i > b) return 0;
  for (uint32_t t = 1; t <= i; ++t) c = c * (b - i + t) / t;  // exact at every step
  return (uint32_t)c;
}

constexpr uint32_t heal_record_words(int k, int m) { return kHealIdWords + 5u * (uint32_t)(m * k); }

// Records of the table of a (k, m) code: sum over p in [1, m] of C(k + m, p).
uint32_t heal_record_count(int k, int m);

// Rank of `mask` (1..m bits set, none at or above k + m) in that table.
uint32_t heal_rank(int k, int m, uint32_t mask);

// The first k ids whose bit is clear (surv) and the set ids ascending (want,
// returns their count); the caller has checked the mask.
int heal_split(int k, int m, uint32_t mask, int* surv, int* want);

// rows(surv, want, nwant, coef): the nwant x k decoding coefficients of a
// survivor set (engine.cpp gf_rows bound to the code); a leoec_status.
using HealRowsFn = std::function<int(const int*, const int*, int, std::vector<uint32_t>*)>;

// Builds the device image described above into *out; a leoec_status.
int heal_build_table(int k, int m, const HealRowsFn& rows, std::vector<uint32_t>* out);

}  // namespace leoec
