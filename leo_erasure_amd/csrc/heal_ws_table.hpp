// heal_ws_table.hpp — the pattern table behind leoec_heal_ws_dev's word and
// packet paths (heal_ws.hip, heal_ws_impl.hpp): for one code outside
// leoec_heal_dev's fused family, one record per mask of lost block ids with
// 1..m bits set among k + m, holding what gfw_heal_masks / bit_heal_masks need
// to rebuild any one of those blocks of one object: the k survivor ids and,
// per lost block, the map from the survivors to it.  Host only: no HIP here,
// so the table builds and tests without a device (heal_ws_table.cpp).
//
// Device image, 32-bit words:
//   [0, 1056)             binom[b][i] = C(b, i), b < 32, i <= 32 (kHealWsBinom,
//                         row b at 33 b: heal_table.hpp's header stops at i = 4)
//   [1056, 1089)          first[p], p <= 32: index of the first record with p
//                         bits set (saturated at 2^32 - 1; exact for p <= m of
//                         every table that is built)
//   [1089, 1104)          record words, record count, zero padding
//   [1104 + idx * rw, ..) record idx, rw = 8 + m k per words:
//       words 0..7   the k survivor ids as bytes (the first k intact ids
//                    ascending, k <= 31), 0xFF past them
//       words 8..    lost slot r (the r-th set bit of the mask ascending),
//                    survivor i at 8 + (r k + i) per:
//                      word classes (per = 1): the GF(2^w) coefficient of
//                        survivor i, scrub_gfw_table.hpp's word;
//                      packet classes (per = w): word c is scrub_bit_table.hpp's
//                        feed word of packet c of survivor i, bit t set iff
//                        that packet feeds packet t of the lost block;
//                    slots past the mask's bit count are zero
// A record's index is heal_table.hpp's combinatorial rank: with the set bits
// b_1 < b_2 < ... < b_p,  idx = first[p] + sum_i C(b_i, i).
//
// A table exists when its image is at most kHealWsMaxBytes (8 MiB, the size of
// leoec_heal_dev's table at (16,4)):
//   4 (1104 + R (8 + m k per)) <= 8 MiB,  R = sum over p in [1, m] of C(k + m, p).
#pragma once

#include <cstdint>
#include <functional>
#include <vector>

namespace leoec {

constexpr int kHealWsMaxIds = 32;  // k + m: one bit of a mask word per block id
constexpr uint32_t kHealWsBinomCols = kHealWsMaxIds + 1;
constexpr uint32_t kHealWsBinom = 0;
constexpr uint32_t kHealWsFirst = kHealWsMaxIds * kHealWsBinomCols;
constexpr uint32_t kHealWsRecWords = kHealWsFirst + kHealWsBinomCols;
constexpr uint32_t kHealWsRecCount = kHealWsRecWords + 1;
constexpr uint32_t kHealWsHeaderWords = 1104;
constexpr uint32_t kHealWsIdWords = 8;
constexpr uint32_t kHealWsNoId = 0xFFu;
constexpr uint64_t kHealWsMaxBytes = 8ull << 20;

static_assert(kHealWsRecCount < kHealWsHeaderWords && kHealWsHeaderWords % 4 == 0, "header layout");

constexpr uint32_t heal_ws_record_words(int k, int m, int per) {
  return kHealWsIdWords + (uint32_t)(m * k * per);
}

// Records of the table of a code with n = k + m ids: sum over p in [1, m] of
// C(n, p), saturated at 2^32 - 1.  n <= 32, m <= n.
uint32_t heal_ws_record_count(int n, int m);

// first[p] of that table: sum over q in [1, p) of C(n, q), saturated.
uint32_t heal_ws_first(int n, int p);

// Rank of `mask` (at least one bit, none at or above n <= 32).
uint32_t heal_ws_rank(int n, uint32_t mask);

// LEOEC_OK when a table of this shape exists: k >= 1, m >= 1, per in 1..32,
// k + m <= 32 and the image within kHealWsMaxBytes; else LEOEC_E_UNSUPPORTED.
// *bytes (when not null): the image's size when it exists.
int heal_ws_shape(int k, int m, int per, uint64_t* bytes);

// rows(surv, want, nwant, out): the maps of the nwant lost ids from the k
// survivors, nwant k per words in the record's order, written at out
// (engine.cpp gf_rows or bit_rows bound to the code); a leoec_status.
using HealWsRowsFn = std::function<int(const int*, const int*, int, uint32_t*)>;

// Builds the device image described above into *out; a leoec_status.
int heal_ws_build_table(int k, int m, int per, const HealWsRowsFn& rows, std::vector<uint32_t>* out);

// The record of `mask` in an image built for (k, m, per): surv[0..k), the lost
// ids ascending in want[0..*nwant) and *body = its words 8.. (nwant k per
// words in use).  LEOEC_E_BAD_ID for a bit at or above k + m,
// LEOEC_E_NOT_ENOUGH_BLOCKS for more than m bits, LEOEC_E_ARG for an empty
// mask or an image of another shape.
int heal_ws_record(const std::vector<uint32_t>& image, int k, int m, int per, uint32_t mask,
                   int* surv, int* want, int* nwant, const uint32_t** body);

}  // namespace leoec
