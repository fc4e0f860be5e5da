// scrub_bit_table.cpp — see scrub_bit_table.hpp.  Host only (no HIP includes).
#include "scrub_bit_table.hpp"

#include "../../include/leoec.h"

namespace leoec {

int scrub_bit_shape(int k, int m, int w) {
  if (k < 1 || m < 1 || w < 1 || w > 32) return LEOEC_E_UNSUPPORTED;
  if (k > kScrubBitMaxIds || m > kScrubBitMaxIds || k + m > kScrubBitMaxIds)
    return LEOEC_E_UNSUPPORTED;
  if (k * w > kScrubBitMaxWords) return LEOEC_E_UNSUPPORTED;
  return LEOEC_OK;
}

void scrub_bit_survivors(int k, int block, int* surv) {
  for (int i = 0, id = 0; i < k; ++id)
    if (id != block) surv[i++] = id;
}

namespace {

// The engine's rows of one block, their shape checked.
int block_map(int k, int m, int w, int block, const ScrubBitRowsFn& rows, int* surv,
              std::vector<uint8_t>* bits) {
  const int rc = scrub_bit_shape(k, m, w);
  if (rc) return rc;
  if (block < 0 || block >= k + m) return LEOEC_E_BAD_ID;
  scrub_bit_survivors(k, block, surv);
  const int st = rows(surv, block, bits);
  if (st) return st;
  return bits->size() == (size_t)w * k * w ? LEOEC_OK : LEOEC_E_ARG;
}

}  // namespace

int scrub_bit_rows(int k, int m, int w, int block, const ScrubBitRowsFn& rows, int* surv,
                   std::vector<uint32_t>* out) {
  std::vector<uint8_t> bits;
  const int rc = block_map(k, m, w, block, rows, surv, &bits);
  if (rc) return rc;
  const int n = k * w, rw = scrub_bit_row_words(k, w);
  out->assign((size_t)w * rw, 0u);
  for (int r = 0; r < w; ++r)
    for (int col = 0; col < n; ++col)
      if (bits[(size_t)r * n + col] & 1u) (*out)[(size_t)r * rw + col / 32] |= 1u << (col % 32);
  return LEOEC_OK;
}

int scrub_bit_build_table(int k, int m, int w, const ScrubBitRowsFn& rows,
                          std::vector<uint32_t>* out) {
  const int rc = scrub_bit_shape(k, m, w);
  if (rc) return rc;
  const int n = k * w;
  const uint32_t rec_words = scrub_bit_record_words(k, w);
  out->assign((size_t)(k + m) * rec_words, 0u);
  std::vector<int> surv(k);
  std::vector<uint8_t> bits;
  for (int b = 0; b < k + m; ++b) {
    const int st = block_map(k, m, w, b, rows, surv.data(), &bits);
    if (st) return st;
    uint32_t* rec = out->data() + (size_t)b * rec_words;
    for (uint32_t x = 0; x < kScrubBitIdWords * 4u; ++x) {
      const uint32_t id = x < (uint32_t)k ? (uint32_t)surv[x] : kScrubBitNoId;
      rec[x >> 2] |= id << (8u * (x & 3u));
    }
    for (int col = 0; col < n; ++col) {
      uint32_t word = 0;
      for (int r = 0; r < w; ++r) word |= (uint32_t)(bits[(size_t)r * n + col] & 1u) << r;
      rec[kScrubBitIdWords + col] = word;
    }
  }
  return LEOEC_OK;
}

}  // namespace leoec
