// heal_ws_table.cpp — see heal_ws_table.hpp.  Host only (no HIP includes).
#include "heal_ws_table.hpp"

#include "../../include/leoec.h"
#include "heal_table.hpp"

namespace leoec {

namespace {

constexpr uint64_t kSat = 0xFFFFFFFFull;

uint64_t sat_add(uint64_t a, uint64_t b) { return a + b > kSat ? kSat : a + b; }

}  // namespace

uint32_t heal_ws_record_count(int n, int m) { return heal_ws_first(n, m + 1); }

uint32_t heal_ws_first(int n, int p) {
  uint64_t s = 0;
  for (int q = 1; q < p && q <= n; ++q) s = sat_add(s, heal_binom((uint32_t)n, (uint32_t)q));
  return (uint32_t)s;
}

uint32_t heal_ws_rank(int n, uint32_t mask) {
  uint32_t idx = heal_ws_first(n, __builtin_popcount(mask));
  uint32_t i = 1;
  for (uint32_t rest = mask; rest; rest &= rest - 1)
    idx += heal_binom((uint32_t)__builtin_ctz(rest), i++);
  return idx;
}

int heal_ws_shape(int k, int m, int per, uint64_t* bytes) {
  if (k < 1 || m < 1 || per < 1 || per > 32) return LEOEC_E_UNSUPPORTED;
  if (k > kHealWsMaxIds || m > kHealWsMaxIds || k + m > kHealWsMaxIds) return LEOEC_E_UNSUPPORTED;
  // count < 2^32 and rw <= 8 + 31 * 31 * 32: the product stays below 2^64
  const uint64_t count = heal_ws_record_count(k + m, m);
  const uint64_t size = 4u * (kHealWsHeaderWords + count * heal_ws_record_words(k, m, per));
  if (count >= kSat || size > kHealWsMaxBytes) return LEOEC_E_UNSUPPORTED;
  if (bytes) *bytes = size;
  return LEOEC_OK;
}

int heal_ws_build_table(int k, int m, int per, const HealWsRowsFn& rows, std::vector<uint32_t>* out) {
  uint64_t bytes = 0;
  const int rc = heal_ws_shape(k, m, per, &bytes);
  if (rc) return rc;
  const int n = k + m;
  const uint32_t rw = heal_ws_record_words(k, m, per), nrec = heal_ws_record_count(n, m);
  out->assign((size_t)(bytes / 4), 0u);
  uint32_t* T = out->data();
  for (uint32_t b = 0; b < (uint32_t)kHealWsMaxIds; ++b)
    for (uint32_t i = 0; i < kHealWsBinomCols; ++i)
      T[kHealWsBinom + b * kHealWsBinomCols + i] = heal_binom(b, i);
  for (uint32_t p = 0; p < kHealWsBinomCols; ++p) T[kHealWsFirst + p] = heal_ws_first(n, (int)p);
  T[kHealWsRecWords] = rw;
  T[kHealWsRecCount] = nrec;
  int surv[kHealWsMaxIds], want[kHealWsMaxIds];
  uint32_t seen = 0;
  const uint64_t end = 1ull << n;
  for (int p = 1; p <= m; ++p) {
    // every mask of p bits below n ascending (the next one with as many bits)
    for (uint64_t v = (1ull << p) - 1; v < end;) {
      const uint32_t mask = (uint32_t)v;
      heal_split(k, m, mask, surv, want);
      const uint32_t idx = heal_ws_rank(n, mask);
      if (idx >= nrec) return LEOEC_E_ARG;
      uint32_t* rec = T + kHealWsHeaderWords + (size_t)idx * rw;
      if (rec[0] != 0u) return LEOEC_E_ARG;  // (survivor 0 of a second mask here: never id 0 four times)
      for (uint32_t x = 0; x < kHealWsIdWords * 4u; ++x) {
        const uint32_t id = x < (uint32_t)k ? (uint32_t)surv[x] : kHealWsNoId;
        rec[x >> 2] |= id << (8u * (x & 3u));
      }
      const int st = rows(surv, want, p, rec + kHealWsIdWords);
      if (st) return st;
      ++seen;
      const uint64_t c = v & (~v + 1), r = v + c;
      v = (((r ^ v) >> 2) / c) | r;
    }
  }
  return seen == nrec ? LEOEC_OK : LEOEC_E_ARG;
}

int heal_ws_record(const std::vector<uint32_t>& image, int k, int m, int per, uint32_t mask,
                   int* surv, int* want, int* nwant, const uint32_t** body) {
  uint64_t bytes = 0;
  const int rc = heal_ws_shape(k, m, per, &bytes);
  if (rc) return rc;
  if (((uint64_t)mask >> (k + m)) != 0) return LEOEC_E_BAD_ID;
  const int bits = __builtin_popcount(mask);
  if (bits > m) return LEOEC_E_NOT_ENOUGH_BLOCKS;
  if (bits == 0 || image.size() != (size_t)(bytes / 4)) return LEOEC_E_ARG;
  const uint32_t rw = heal_ws_record_words(k, m, per);
  const uint32_t* rec = image.data() + kHealWsHeaderWords + (size_t)heal_ws_rank(k + m, mask) * rw;
  for (int i = 0; i < k; ++i) surv[i] = (int)((rec[i >> 2] >> (8 * (i & 3))) & 0xFFu);
  int nw = 0;
  for (int id = 0; id < k + m; ++id)
    if ((mask >> id) & 1u) want[nw++] = id;
  *nwant = nw;
  *body = rec + kHealWsIdWords;
  return LEOEC_OK;
}

}  // namespace leoec
