// locate_bitrows.hpp — the ratio table behind leoec_locate_ws_dev's bitmatrix
// path (locate.hip): T[i][j] = B[i][j] B[0][j]^-1 over GF(2), for the
// (m w) x (k w) coding bitmatrix B cut into w x w blocks B[i][j].
//
// A block is w packets; take one bit position of a packet as a column, the w
// bits the w packets of a block hold there as a vector.  With s_i that vector
// of (stored coding block i ^ encoding of the data), a column in which only
// data block j is wrong (by e) has s_i = B[i][j] e, so s_i = T[i][j] s_0 for
// i = 1..m-1.  On packets: syndrome packet r of coding block i is the XOR of
// the syndrome packets c of coding block 0 with T[i][j][r][c] = 1.
// Host only: no HIP here, so the table builds and tests without a device
// (locate_bitrows.cpp).
#pragma once

#include <cstdint>
#include <vector>

#include "codes.hpp"

namespace leoec {

// B: (m w) x (k w), w <= 32.  *out: (m - 1) k w words; word
// ((i - 1) k + j) w + r is row r of T[i][j], bit c (bit 0 = packet 0) set iff
// syndrome packet c of coding block 0 feeds packet r of coding block i.
// The syndromes name one damaged block uniquely exactly when every B[i][j] is
// invertible (a damaged data block then shows in every syndrome, a coding
// block in one) and every 2w x 2w minor [[B[i][j], B[i][j']], [B[i'][j],
// B[i'][j']]] is invertible (two data blocks never explain the same
// syndromes).  Both are checked here: LEOEC_E_UNSUPPORTED when either fails,
// when m < 2, or when B's shape is not (m w) x (k w) with 1 <= w <= 32.
int locate_build_bitrows(const BitMatrix& B, int k, int m, int w, std::vector<uint32_t>* out);

}  // namespace leoec
