// heal_table.cpp — see heal_table.hpp.  Host only (no HIP includes).
#include "heal_table.hpp"

#include "../../include/leoec.h"
#include "codes.hpp"

namespace leoec {

uint32_t heal_record_count(int k, int m) {
  uint32_t n = 0;
  for (int p = 1; p <= m; ++p) n += heal_binom((uint32_t)(k + m), (uint32_t)p);
  return n;
}

uint32_t heal_rank(int k, int m, uint32_t mask) {
  const int bits = __builtin_popcount(mask);
  uint32_t idx = 0;
  for (int p = 1; p < bits; ++p) idx += heal_binom((uint32_t)(k + m), (uint32_t)p);
  uint32_t i = 1;
  for (uint32_t rest = mask; rest; rest &= rest - 1)
    idx += heal_binom((uint32_t)__builtin_ctz(rest), i++);
  return idx;
}

int heal_split(int k, int m, uint32_t mask, int* surv, int* want) {
  int ns = 0, nw = 0;
  for (int id = 0; id < k + m; ++id) {
    if ((mask >> id) & 1u) want[nw++] = id;
    else if (ns < k) surv[ns++] = id;
  }
  return nw;
}

namespace {

// The five v_perm words of "multiply by c" in GF(2^8) (kernels_impl.hpp
// gf8_tables: T0 lo, T0 hi, T1 lo, T1 hi, T2), from the w = 8 field.
void perm_tables(uint32_t c, uint32_t t[5]) {
  const Field& F = field(8);
  auto pack = [&](uint32_t first, uint32_t shift) {
    uint32_t v = 0;
    for (uint32_t i = 0; i < 4; ++i) v |= (F.mul(c, (first + i) << shift) & 0xFFu) << (8 * i);
    return v;
  };
  t[0] = pack(0, 0);
  t[1] = pack(4, 0);
  t[2] = pack(0, 3);
  t[3] = pack(4, 3);
  t[4] = pack(0, 6);
}

}  // namespace

int heal_build_table(int k, int m, const HealRowsFn& rows, std::vector<uint32_t>* out) {
  if (k < 1 || k > kHealMaxK || m < 1 || m > kHealMaxLost) return LEOEC_E_UNSUPPORTED;
  const uint32_t n = (uint32_t)(k + m), rw = heal_record_words(k, m);
  const uint32_t nrec = heal_record_count(k, m);
  out->assign((size_t)kHealHeaderWords + (size_t)nrec * rw, 0u);
  uint32_t* T = out->data();
  for (uint32_t b = 0; b < (uint32_t)kHealMaxIds; ++b)
    for (uint32_t i = 0; i <= (uint32_t)kHealMaxLost; ++i)
      T[kHealBinom + b * (kHealMaxLost + 1) + i] = heal_binom(b, i);
  for (int p = 1; p <= kHealMaxLost; ++p)
    T[kHealFirst + p] = T[kHealFirst + p - 1] + (p > 1 ? heal_binom(n, (uint32_t)(p - 1)) : 0u);
  T[kHealRecWords] = rw;
  T[kHealRecCount] = nrec;
  std::vector<uint32_t> coef;
  int surv[kHealMaxIds], want[kHealMaxIds];
  uint32_t seen = 0;
  for (uint32_t mask = 1; mask < (1u << n); ++mask) {
    const int bits = __builtin_popcount(mask);
    if (bits > m) continue;
    heal_split(k, m, mask, surv, want);
    const int rc = rows(surv, want, bits, &coef);
    if (rc) return rc;
    uint32_t* rec = T + kHealHeaderWords + (size_t)heal_rank(k, m, mask) * rw;
    uint8_t ids[kHealIdWords * 4] = {0};
    for (int j = 0; j < k; ++j) ids[j] = (uint8_t)surv[j];
    for (int r = 0; r < kHealMaxLost; ++r) ids[k + r] = r < bits ? (uint8_t)want[r] : (uint8_t)kHealNoId;
    for (uint32_t x = 0; x < kHealIdWords * 4; ++x) rec[x / 4] |= (uint32_t)ids[x] << (8 * (x % 4));
    for (int r = 0; r < bits; ++r)
      for (int j = 0; j < k; ++j)
        perm_tables(coef[(size_t)r * k + j] & 0xFFu, rec + kHealIdWords + 5 * (r * k + j));
    ++seen;
  }
  return seen == nrec ? LEOEC_OK : LEOEC_E_ARG;
}

}  // namespace leoec
