// locate_bitrows.cpp — see locate_bitrows.hpp.  Host only (no HIP includes).
#include "locate_bitrows.hpp"

#include <utility>

#include "../../include/leoec.h"

namespace leoec {

namespace {

// Rank of the n x n GF(2) matrix whose row r is the low n bits of rows[r]
// (n <= 64); rows is used up.
int bit_rank(std::vector<uint64_t>& rows, int n) {
  int rank = 0;
  for (int col = 0; col < n && rank < n; ++col) {
    int piv = rank;
    while (piv < n && !((rows[piv] >> col) & 1u)) ++piv;
    if (piv == n) continue;
    std::swap(rows[rank], rows[piv]);
    for (int r = 0; r < n; ++r)
      if (r != rank && ((rows[r] >> col) & 1u)) rows[r] ^= rows[rank];
    ++rank;
  }
  return rank;
}

}  // namespace

int locate_build_bitrows(const BitMatrix& B, int k, int m, int w, std::vector<uint32_t>* out) {
  if (k < 1 || m < 2 || w < 1 || w > 32) return LEOEC_E_UNSUPPORTED;
  if (B.rows != m * w || B.cols != k * w) return LEOEC_E_UNSUPPORTED;
  // row r of block (i, j), bit c = column c
  auto block_row = [&](int i, int j, int r) {
    uint64_t x = 0;
    for (int c = 0; c < w; ++c) x |= (uint64_t)B.get(i * w + r, j * w + c) << c;
    return x;
  };
  // every block invertible; B[0][j]^-1 kept for the ratios
  std::vector<BitMatrix> inv0(k);
  BitMatrix blk, inv;
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < k; ++j) {
      blk.resize(w, w);
      for (int r = 0; r < w; ++r) blk.row(r)[0] = block_row(i, j, r);
      if (bit_invert(blk, i == 0 ? &inv0[j] : &inv) != LEOEC_OK) return LEOEC_E_UNSUPPORTED;
    }
  // every 2w x 2w minor of full rank
  std::vector<uint64_t> minor((size_t)2 * w);
  for (int i0 = 0; i0 < m; ++i0)
    for (int i1 = i0 + 1; i1 < m; ++i1)
      for (int j0 = 0; j0 < k; ++j0)
        for (int j1 = j0 + 1; j1 < k; ++j1) {
          for (int r = 0; r < w; ++r) {
            minor[r] = block_row(i0, j0, r) | block_row(i0, j1, r) << w;
            minor[w + r] = block_row(i1, j0, r) | block_row(i1, j1, r) << w;
          }
          if (bit_rank(minor, 2 * w) != 2 * w) return LEOEC_E_UNSUPPORTED;
        }
  // T[i][j] = B[i][j] B[0][j]^-1: row r = XOR of the rows t of the inverse
  // with B[i][j][r][t] = 1
  out->assign((size_t)(m - 1) * k * w, 0u);
  for (int i = 1; i < m; ++i)
    for (int j = 0; j < k; ++j)
      for (int r = 0; r < w; ++r) {
        const uint64_t b = block_row(i, j, r);
        uint64_t t = 0;
        for (int x = 0; x < w; ++x)
          if ((b >> x) & 1u) t ^= inv0[j].row(x)[0];
        (*out)[((size_t)(i - 1) * k + j) * w + r] = (uint32_t)t;
      }
  return LEOEC_OK;
}

}  // namespace leoec
