// heal_ws_table_test.cpp — the pattern table of leoec_heal_ws_dev on the CPU: a
// stand-alone program (its own main, no HIP, never loaded into Python) over
// csrc/heal_ws_table.cpp, built by tests/test_heal_ws_cpu.py plain and with
// -fsanitize=address,undefined.
//
// The rows of a record come from a stand-in for the engine's maps that writes
// words derived from (survivors, lost ids, slot, index), so that every word
// of every record says which mask, slot and survivor it belongs to:
//   * the rank is a bijection onto [0, count) for (k + m, m) in {(6, 2),
//     (11, 5), (32, 2)} and equals first[p] + sum C(b_i, i) read from the
//     image's own header;
//   * every record of the images of (4,2) per 1, (6,5) per 1, (30,2) per 1,
//     (4,2) per 7 and (30,2) per 5 holds the first k intact ids, 0xFF past
//     them, the stand-in's words in the slots of its lost ids and zeros in
//     the slots past its bit count;
//   * the shapes the header promises are served and (16,15) per 1 is refused.
// Prints "ok: ..." and returns 0, or the first difference and 1.
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "../include/leoec.h"
#include "../leo_erasure_amd/csrc/heal_table.hpp"
#include "../leo_erasure_amd/csrc/heal_ws_table.hpp"

using namespace leoec;

namespace {

int fail(const char* what, int a, int b, unsigned mask) {
  std::fprintf(stderr, "FAIL: %s (%d, %d) mask 0x%x\n", what, a, b, mask);
  return 1;
}

uint32_t stand_in(const int* surv, int k, int want, int r, int i) {
  uint32_t h = 0x9E3779B9u * (uint32_t)(want + 1) + 0x85EBCA6Bu * (uint32_t)(r + 1) + (uint32_t)i;
  for (int j = 0; j < k; ++j) h = h * 31u + (uint32_t)surv[j];
  return h | 1u;  // never zero
}

// Every mask of 1..m bits among n, by bit count, ascending.
std::vector<uint32_t> masks_of(int n, int m) {
  std::vector<uint32_t> out;
  for (int p = 1; p <= m; ++p)
    for (uint64_t v = 0; v < (1ull << n); ++v)
      if (__builtin_popcountll(v) == p) out.push_back((uint32_t)v);
  return out;
}

// n = 32: too many words to walk; the masks of one and two bits directly.
std::vector<uint32_t> masks_of_32_2() {
  std::vector<uint32_t> out;
  for (int a = 0; a < 32; ++a) out.push_back(1u << a);
  for (int b = 1; b < 32; ++b)
    for (int a = 0; a < b; ++a) out.push_back((1u << a) | (1u << b));
  return out;
}

int check_rank(int n, int m) {
  const std::vector<uint32_t> masks = n == 32 ? masks_of_32_2() : masks_of(n, m);
  const uint32_t count = heal_ws_record_count(n, m);
  if (masks.size() != count) return fail("record count", n, m, (unsigned)masks.size());
  std::set<uint32_t> seen;
  for (uint32_t mask : masks) {
    const uint32_t r = heal_ws_rank(n, mask);
    const int p = __builtin_popcount(mask);
    if (r >= count || !seen.insert(r).second) return fail("rank not a bijection", n, m, mask);
    if (r < heal_ws_first(n, p) || r >= heal_ws_first(n, p + 1)) return fail("rank outside its bit count's range", n, m, mask);
  }
  return 0;
}

int check_image(int k, int m, int per) {
  const int n = k + m;
  const auto rows = [&](const int* surv, const int* want, int nwant, uint32_t* out) {
    for (int r = 0; r < nwant; ++r)
      for (int i = 0; i < k * per; ++i) out[(size_t)r * k * per + i] = stand_in(surv, k, want[r], r, i);
    return (int)LEOEC_OK;
  };
  std::vector<uint32_t> image;
  if (heal_ws_build_table(k, m, per, rows, &image) != LEOEC_OK) return fail("build", k, m, 0);
  uint64_t bytes = 0;
  if (heal_ws_shape(k, m, per, &bytes) != LEOEC_OK || bytes != image.size() * 4) return fail("size", k, m, 0);
  const uint32_t rw = heal_ws_record_words(k, m, per);
  if (image[kHealWsRecWords] != rw || image[kHealWsRecCount] != heal_ws_record_count(n, m))
    return fail("header", k, m, 0);
  for (uint32_t b = 0; b < 32; ++b)
    for (uint32_t i = 0; i <= 32; ++i)
      if (image[kHealWsBinom + b * kHealWsBinomCols + i] != heal_binom(b, i)) return fail("binom", (int)b, (int)i, 0);
  const std::vector<uint32_t> masks = n == 32 ? masks_of_32_2() : masks_of(n, m);
  std::vector<int> surv(k), want(n), sv(k), wt(n);
  for (uint32_t mask : masks) {
    // the device's walk: first[p] + sum of C(b_i, i) from the image's header
    uint32_t idx = image[kHealWsFirst + (uint32_t)__builtin_popcount(mask)], i = 1;
    for (uint32_t rest = mask; rest; rest &= rest - 1, ++i)
      idx += image[kHealWsBinom + (uint32_t)__builtin_ctz(rest) * kHealWsBinomCols + i];
    if (idx != heal_ws_rank(n, mask)) return fail("header walk", k, m, mask);
    int nwant = 0;
    const uint32_t* body = nullptr;
    if (heal_ws_record(image, k, m, per, mask, surv.data(), want.data(), &nwant, &body) != LEOEC_OK)
      return fail("record", k, m, mask);
    if (body != image.data() + kHealWsHeaderWords + (size_t)idx * rw + kHealWsIdWords)
      return fail("record address", k, m, mask);
    const int bits = heal_split(k, m, mask, sv.data(), wt.data());
    if (nwant != bits) return fail("nwant", k, m, mask);
    for (int j = 0; j < k; ++j)
      if (surv[j] != sv[j]) return fail("survivors", k, m, mask);
    for (int j = 0; j < bits; ++j)
      if (want[j] != wt[j]) return fail("lost ids", k, m, mask);
    const uint32_t* ids = body - kHealWsIdWords;
    for (uint32_t x = (uint32_t)k; x < kHealWsIdWords * 4; ++x)
      if (((ids[x >> 2] >> (8 * (x & 3))) & 0xFFu) != kHealWsNoId) return fail("id padding", k, m, mask);
    for (int r = 0; r < m; ++r)
      for (int j = 0; j < k * per; ++j) {
        const uint32_t expect = r < bits ? stand_in(sv.data(), k, wt[r], r, j) : 0u;
        if (body[(size_t)r * k * per + j] != expect) return fail("record word", r, j, mask);
      }
  }
  // a bad mask keeps leoec_heal_rows' statuses
  int nwant;
  const uint32_t* body;
  if (n < 32 && heal_ws_record(image, k, m, per, 1u << n, surv.data(), want.data(), &nwant, &body) != LEOEC_E_BAD_ID)
    return fail("bad id", k, m, 1u << n);
  if (m + 1 <= n &&
      heal_ws_record(image, k, m, per, (1u << (m + 1)) - 1u, surv.data(), want.data(), &nwant, &body) !=
          LEOEC_E_NOT_ENOUGH_BLOCKS)
    return fail("too many bits", k, m, (1u << (m + 1)) - 1u);
  if (heal_ws_record(image, k, m, per, 0u, surv.data(), want.data(), &nwant, &body) != LEOEC_E_ARG)
    return fail("empty mask", k, m, 0);
  return 0;
}

}  // namespace

int main() {
  const int ranks[][2] = {{6, 2}, {11, 5}, {32, 2}};
  for (const auto& r : ranks)
    if (check_rank(r[0], r[1])) return 1;
  const int images[][3] = {{4, 2, 1}, {6, 5, 1}, {30, 2, 1}, {4, 2, 7}, {30, 2, 5}, {1, 1, 1}, {6, 3, 4}};
  for (const auto& c : images)
    if (check_image(c[0], c[1], c[2])) return 1;
  // served: vandrs(20,4,8), (6,5,8), (10,4,16), (6,3,32), cauchyrs(10,4,8), (5,3,17),
  // liberation(10,2,11), vandrs(30,2,16), cauchyrs(30,2,5); refused: vandrs(16,15,8)
  const int served[][3] = {{20, 4, 1}, {6, 5, 1}, {10, 4, 1}, {6, 3, 1}, {10, 4, 8},
                           {5, 3, 17}, {10, 2, 11}, {30, 2, 1}, {30, 2, 5}};
  for (const auto& c : served)
    if (heal_ws_shape(c[0], c[1], c[2], nullptr) != LEOEC_OK) return fail("served", c[0], c[1], 0);
  const int refused[][3] = {{16, 15, 1}, {16, 16, 1}, {30, 3, 1}, {0, 2, 1}, {4, 0, 1}, {4, 2, 0}, {4, 2, 33}, {20, 12, 1}};
  for (const auto& c : refused)
    if (heal_ws_shape(c[0], c[1], c[2], nullptr) != LEOEC_E_UNSUPPORTED) return fail("refused", c[0], c[1], 0);
  std::printf("ok: %zu ranks, %zu images, %zu served, %zu refused\n", sizeof ranks / sizeof ranks[0],
              sizeof images / sizeof images[0], sizeof served / sizeof served[0],
              sizeof refused / sizeof refused[0]);
  return 0;
}
