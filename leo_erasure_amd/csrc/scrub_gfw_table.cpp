// scrub_gfw_table.cpp — see scrub_gfw_table.hpp.  Host only (no HIP includes).
#include "scrub_gfw_table.hpp"

#include "../../include/leoec.h"
#include "scrub_bit_table.hpp"

namespace leoec {

int scrub_gfw_shape(int k, int m) {
  if (k < 1 || m < 1 || k + m > kScrubGfwMaxIds) return LEOEC_E_UNSUPPORTED;
  return LEOEC_OK;
}

int scrub_gfw_build_table(int k, int m, const ScrubGfwRowsFn& rows, std::vector<uint32_t>* out) {
  const int rc = scrub_gfw_shape(k, m);
  if (rc) return rc;
  const uint32_t rec_words = scrub_gfw_record_words(k);
  out->assign((size_t)(k + m) * rec_words, 0u);
  std::vector<int> surv(k);
  std::vector<uint32_t> coef;
  for (int b = 0; b < k + m; ++b) {
    scrub_bit_survivors(k, b, surv.data());  // the first k ids ascending without b
    const int st = rows(surv.data(), b, &coef);
    if (st) return st;
    if (coef.size() != (size_t)k) return LEOEC_E_ARG;
    uint32_t* rec = out->data() + (size_t)b * rec_words;
    for (uint32_t x = 0; x < kScrubGfwIdWords * 4u; ++x) {
      const uint32_t id = x < (uint32_t)k ? (uint32_t)surv[x] : kScrubGfwNoId;
      rec[x >> 2] |= id << (8u * (x & 3u));
    }
    for (int i = 0; i < k; ++i) rec[kScrubGfwIdWords + i] = coef[i];
  }
  return LEOEC_OK;
}

int scrub_gfw_record(const std::vector<uint32_t>& image, int k, int m, int block, int* surv,
                     uint32_t* coef) {
  const int rc = scrub_gfw_shape(k, m);
  if (rc) return rc;
  if (block < 0 || block >= k + m) return LEOEC_E_BAD_ID;
  const uint32_t rec_words = scrub_gfw_record_words(k);
  if (image.size() != (size_t)(k + m) * rec_words) return LEOEC_E_ARG;
  const uint32_t* rec = image.data() + (size_t)block * rec_words;
  for (int i = 0; i < k; ++i) {
    surv[i] = (int)((rec[i >> 2] >> (8 * (i & 3))) & 0xFFu);
    coef[i] = rec[kScrubGfwIdWords + i];
  }
  return LEOEC_OK;
}

}  // namespace leoec
