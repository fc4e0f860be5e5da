// scrub_bit_table_main.cpp — the host-only builder of leoec_scrub_ws_dev's
// block table (leo_erasure_amd/csrc/scrub_bit_table.cpp) under
// AddressSanitizer + UndefinedBehaviorSanitizer: a plain executable built from
// this file, the builder and codes.cpp (tests/test_scrub_ws_cpu.py).
//
// For every configuration on the command line (cls k m w, cls = c for cauchyrs
// or l for liberation) and every block b: the rows come from a map built here
// (G[b] G[surv]^-1 with G = [I; B], B from codes.cpp), and the builder's two
// forms are held against it: surv is the first k ids without b, the row form
// times G[surv] is G[b], the device image's id bytes are surv then 0xFF, and
// its input-stationary words are the row form's transpose.  Then the statuses:
// a block outside 0..k+m-1, k + m = 32, a rows function that fails or returns
// the wrong shape.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/leoec.h"
#include "../../leo_erasure_amd/csrc/codes.hpp"
#include "../../leo_erasure_amd/csrc/scrub_bit_table.hpp"

using namespace leoec;

#define CHECK(x)                                                        \
  do {                                                                  \
    if (!(x)) {                                                         \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

// Row r of block id of G = [I; B], as a BitMatrix row of k w columns.
static void g_row(const BitMatrix& B, int k, int w, int id, int r, BitMatrix* out, int at) {
  if (id < k) {
    out->set(at, id * w + r, true);
  } else {
    for (int c = 0; c < k * w; ++c) out->set(at, c, B.get((id - k) * w + r, c));
  }
}

static int one_config(char cls, int k, int m, int w) {
  BitMatrix B;
  if (cls == 'l') {
    CHECK(m == 2 && liberation_coding_bitmatrix(k, w, &B) == 0);
  } else {
    GfMatrix C;
    CHECK(cauchy_good_coding_matrix(k, m, w, &C) == 0);
    expand_to_bitmatrix(C, w, &B);
  }
  const int n = k * w;
  CHECK(B.rows == m * w && B.cols == n);
  const ScrubBitRowsFn rows = [&](const int* surv, int block, std::vector<uint8_t>* out) {
    BitMatrix G, inv;
    G.resize(n, n);
    for (int i = 0; i < k; ++i)
      for (int r = 0; r < w; ++r) g_row(B, k, w, surv[i], r, &G, i * w + r);
    const int rc = bit_invert(G, &inv);
    if (rc) return rc;
    BitMatrix want;
    want.resize(w, n);
    for (int r = 0; r < w; ++r) g_row(B, k, w, block, r, &want, r);
    out->assign((size_t)w * n, 0);
    for (int r = 0; r < w; ++r)
      for (int l = 0; l < n; ++l)
        if (want.get(r, l))
          for (int c = 0; c < n; ++c) (*out)[(size_t)r * n + c] ^= inv.get(l, c);
    return 0;
  };
  CHECK(scrub_bit_shape(k, m, w) == LEOEC_OK);
  std::vector<uint32_t> table;
  CHECK(scrub_bit_build_table(k, m, w, rows, &table) == LEOEC_OK);
  const uint32_t rec_words = scrub_bit_record_words(k, w);
  CHECK(table.size() == (size_t)(k + m) * rec_words);
  const int rw = scrub_bit_row_words(k, w);
  for (int b = 0; b < k + m; ++b) {
    std::vector<int> surv(k, -1);
    std::vector<uint32_t> form;
    CHECK(scrub_bit_rows(k, m, w, b, rows, surv.data(), &form) == LEOEC_OK);
    CHECK(form.size() == (size_t)w * rw);
    for (int i = 0, id = 0; i < k; ++i, ++id) {
      if (id == b) ++id;
      CHECK(surv[i] == id);
    }
    auto bit = [&](int r, int col) { return (form[(size_t)r * rw + col / 32] >> (col % 32)) & 1u; };
    // rows x G[surv] == G[b]
    for (int r = 0; r < w; ++r) {
      std::vector<uint8_t> got(n, 0);
      for (int i = 0; i < k; ++i)
        for (int c = 0; c < w; ++c) {
          if (!bit(r, i * w + c)) continue;
          BitMatrix g;
          g.resize(1, n);
          g_row(B, k, w, surv[i], c, &g, 0);
          for (int x = 0; x < n; ++x) got[x] ^= g.get(0, x);
        }
      BitMatrix want;
      want.resize(1, n);
      g_row(B, k, w, b, r, &want, 0);
      for (int x = 0; x < n; ++x) CHECK(got[x] == (uint8_t)want.get(0, x));
      for (int col = n; col < rw * 32; ++col) CHECK(!bit(r, col));
    }
    // the device image: ids, then the transpose
    const uint32_t* rec = table.data() + (size_t)b * rec_words;
    for (int x = 0; x < 32; ++x) {
      const uint32_t id = (rec[x >> 2] >> (8 * (x & 3))) & 0xFFu;
      CHECK(id == (x < k ? (uint32_t)surv[x] : kScrubBitNoId));
    }
    for (int col = 0; col < n; ++col) {
      uint32_t word = 0;
      for (int r = 0; r < w; ++r) word |= bit(r, col) << r;
      CHECK(rec[kScrubBitIdWords + col] == word);
    }
  }
  // statuses
  std::vector<int> surv(k);
  std::vector<uint32_t> form;
  CHECK(scrub_bit_rows(k, m, w, -1, rows, surv.data(), &form) == LEOEC_E_BAD_ID);
  CHECK(scrub_bit_rows(k, m, w, k + m, rows, surv.data(), &form) == LEOEC_E_BAD_ID);
  const ScrubBitRowsFn fails = [](const int*, int, std::vector<uint8_t>*) {
    return (int)LEOEC_E_NON_INVERTIBLE;
  };
  CHECK(scrub_bit_build_table(k, m, w, fails, &table) == LEOEC_E_NON_INVERTIBLE);
  const ScrubBitRowsFn small = [](const int*, int, std::vector<uint8_t>* out) {
    out->assign(3, 1);
    return 0;
  };
  CHECK(scrub_bit_build_table(k, m, w, small, &table) == LEOEC_E_ARG);
  CHECK(scrub_bit_rows(k, m, w, 0, small, surv.data(), &form) == LEOEC_E_ARG);
  return k + m;
}

int main(int argc, char** argv) {
  CHECK(argc >= 5 && (argc - 1) % 4 == 0);
  int records = 0;
  for (int a = 1; a + 3 < argc; a += 4)
    records += one_config(argv[a][0], std::atoi(argv[a + 1]), std::atoi(argv[a + 2]),
                          std::atoi(argv[a + 3]));
  CHECK(scrub_bit_shape(28, 4, 8) == LEOEC_E_UNSUPPORTED);   // k + m = 32
  CHECK(scrub_bit_shape(10, 4, 32) == LEOEC_OK);             // (the served test's own limit is (m - 1) k w)
  CHECK(scrub_bit_shape(29, 2, 29) == LEOEC_E_UNSUPPORTED);  // k w = 841
  CHECK(scrub_bit_shape(4, 2, 33) == LEOEC_E_UNSUPPORTED);
  CHECK(scrub_bit_shape(0, 2, 8) == LEOEC_E_UNSUPPORTED);
  std::printf("scrub_bit_table: all checks held (%d records)\n", records);
  return 0;
}
