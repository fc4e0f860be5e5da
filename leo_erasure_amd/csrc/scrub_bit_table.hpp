// scrub_bit_table.hpp — the block table behind leoec_scrub_ws_dev's bitmatrix
// path (scrub.hip, scrub_bit_impl.hpp): for one cauchyrs or liberation code,
// one record per block id b in 0..k+m-1 holding what bit_heal_list needs to
// rebuild block b of one object from the other blocks: the k survivor ids and
// the GF(2) map from the survivors' packets to b's.  Host only: no HIP here,
// so the table builds and tests without a device (scrub_bit_table.cpp).
//
// Device image, 32-bit words, record b at b * (8 + k w):
//   words 0..7     the k survivor ids as bytes (the first k ids ascending
//                  without b: leoec_decode_dev's survivors), 0xFF past them
//   words 8..      word 8 + i w + c: the outputs of packet c of survivor i,
//                  bit r set iff that packet feeds packet r of block b
// That is the transpose of the rows the engine computes (bit_rows): the
// kernel works input-stationary, one word per input packet saying where its
// bytes go.  leoec_scrub_bitrows reports the row form (scrub_bit_rows).
#pragma once

#include <cstdint>
#include <functional>
#include <vector>

namespace leoec {

constexpr int kScrubBitMaxIds = 31;       // k + m: id 31's bit is LEOEC_LOCATE_MANY
constexpr int kScrubBitMaxWords = 768;    // k w at most (from (m - 1) k w <= 768, m >= 2)
constexpr uint32_t kScrubBitIdWords = 8;  // 32 id bytes
constexpr uint32_t kScrubBitNoId = 0xFFu;

constexpr uint32_t scrub_bit_record_words(int k, int w) {
  return kScrubBitIdWords + (uint32_t)(k * w);
}
// Words of one row of the row form: k w bits.
constexpr int scrub_bit_row_words(int k, int w) { return (k * w + 31) / 32; }

// rows(surv, block, out): the w x (k w) GF(2) map, one byte per entry, row r
// column i w + c set iff packet c of block surv[i] feeds packet r of `block`
// (engine.cpp bit_rows bound to the code); a leoec_status.
using ScrubBitRowsFn = std::function<int(const int*, int, std::vector<uint8_t>*)>;

// LEOEC_OK when a table of this shape exists: k >= 1, m >= 1, 1 <= w <= 32,
// k + m <= kScrubBitMaxIds, k w <= kScrubBitMaxWords; else LEOEC_E_UNSUPPORTED.
int scrub_bit_shape(int k, int m, int w);

// surv[0..k): the first k ids ascending without `block` (0 <= block < k + m).
void scrub_bit_survivors(int k, int block, int* surv);

// The row form of one block's map: surv as above, *out = w rows of
// scrub_bit_row_words(k, w) words, bit i w + c of row r (word (i w + c) / 32,
// bit (i w + c) % 32).  LEOEC_E_BAD_ID for a block outside 0..k+m-1.
int scrub_bit_rows(int k, int m, int w, int block, const ScrubBitRowsFn& rows, int* surv,
                   std::vector<uint32_t>* out);

// Builds the device image described above into *out; a leoec_status.
int scrub_bit_build_table(int k, int m, int w, const ScrubBitRowsFn& rows,
                          std::vector<uint32_t>* out);

}  // namespace leoec
