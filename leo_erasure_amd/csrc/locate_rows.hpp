// locate_rows.hpp — the ratio table behind leoec_locate_dev (locate.hip,
// locate_impl.hpp): T[i][j] = C[i][j] / C[0][j] for the m x k GF(2^8) coding
// matrix C.  With s_i the syndrome of coding block i in one byte column, a
// column in which only data block j is wrong (by e) has s_i = C[i][j] e, so
// s_i = T[i][j] s_0 for i = 1..m-1.  Host only: no HIP here, so the table
// builds and tests without a device (locate_rows.cpp).
#pragma once

#include <cstdint>
#include <vector>

namespace leoec {

// C: m x k row-major, GF(2^8).  *out: (m - 1) x k, row i - 1 = T[i][0..k).
// The syndromes name one damaged block uniquely exactly when no entry of C is
// zero (a damaged data block then shows in every syndrome, a coding block in
// one) and no 2 x 2 minor of C is singular (two data blocks never share a
// ratio).  Both are checked here: LEOEC_E_UNSUPPORTED when either fails, or
// when m < 2.
int locate_build_rows(const uint32_t* C, int k, int m, std::vector<uint32_t>* out);

}  // namespace leoec
