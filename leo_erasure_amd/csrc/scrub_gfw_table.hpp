// scrub_gfw_table.hpp — the block table behind leoec_scrub_gfw_dev's word path
// (scrub.hip, scrub_gfw_impl.hpp): for one GF(2^w) matrix code (vandrs w = 16
// / 32, vandrs / isars w = 8 outside the fused range), one record per block id
// b in 0..k+m-1 holding what gfw_heal_list needs to rebuild block b of one
// object from the other blocks: the k survivor ids and the k coefficients.
// Host only: no HIP here, so the table builds and tests without a device
// (scrub_gfw_table.cpp).
//
// Device image, 32-bit words, record b at b * (8 + k):
//   words 0..7     the k survivor ids as bytes (the first k ids ascending
//                  without b: leoec_decode_dev's survivors), 0xFF past them
//   words 8..      word 8 + i: the coefficient of survivor i,
//                  block b = XOR over i of coef[i] * block surv[i] on w-bit words
// At most 31 records of 37 words: under 5 KB.  leoec_scrub_wrows reports a
// record of this image (scrub_gfw_record).
#pragma once

#include <cstdint>
#include <functional>
#include <vector>

namespace leoec {

constexpr int kScrubGfwMaxIds = 31;       // k + m: id 31's bit is LEOEC_LOCATE_MANY
constexpr uint32_t kScrubGfwIdWords = 8;  // 32 id bytes (k <= 30)
constexpr uint32_t kScrubGfwNoId = 0xFFu;

constexpr uint32_t scrub_gfw_record_words(int k) { return kScrubGfwIdWords + (uint32_t)k; }

// rows(surv, block, out): the k coefficients that give `block` from the blocks
// surv[0..k) (engine.cpp gf_rows bound to the code, one wanted id); a
// leoec_status.
using ScrubGfwRowsFn = std::function<int(const int*, int, std::vector<uint32_t>*)>;

// LEOEC_OK when a table of this shape exists: k >= 1, m >= 1,
// k + m <= kScrubGfwMaxIds; else LEOEC_E_UNSUPPORTED.
int scrub_gfw_shape(int k, int m);

// Builds the device image described above into *out; a leoec_status.
int scrub_gfw_build_table(int k, int m, const ScrubGfwRowsFn& rows, std::vector<uint32_t>* out);

// Record `block` of an image built for (k, m): surv[0..k) and coef[0..k).
// LEOEC_E_BAD_ID for a block outside 0..k+m-1, LEOEC_E_ARG for an image of
// another shape.
int scrub_gfw_record(const std::vector<uint32_t>& image, int k, int m, int block, int* surv,
                     uint32_t* coef);

}  // namespace leoec
