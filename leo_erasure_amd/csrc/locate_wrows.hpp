// locate_wrows.hpp — the ratio table behind leoec_locate_gfw_dev (locate.hip,
// locate_gfw_impl.hpp): locate_rows.hpp's table over GF(2^w) words, w = 8, 16
// or 32, with no bound on k or m of its own.  T[i][j] = C[i][j] / C[0][j] for
// the m x k coding matrix C.  With s_i the syndrome of coding block i in one
// word column, a column in which only data block j is wrong (by e) has
// s_i = C[i][j] e, so s_i = T[i][j] s_0 for i = 1..m-1.  Host only: no HIP
// here, so the table builds and tests without a device (locate_wrows.cpp).
#pragma once

#include <cstdint>
#include <vector>

namespace leoec {

// C: m x k row-major, GF(2^w), w in {8, 16, 32}.  *out: (m - 1) x k, row
// i - 1 = T[i][0..k).  The syndromes name one damaged block uniquely exactly
// when no entry of C is zero and no 2 x 2 minor of C is singular
// (locate_rows.hpp).  Both are checked here: LEOEC_E_UNSUPPORTED when either
// fails, when m < 2 or for another w.
int locate_build_wrows(const uint32_t* C, int k, int m, int w, std::vector<uint32_t>* out);

}  // namespace leoec
