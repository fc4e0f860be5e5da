// read_core.hpp — the arithmetic of leoec_read_dev (read.hip) that needs no
// device: the grouping of a range's segments into runs of intact blocks and
// single lost blocks, the clip of a survivor lane to its block's valid bytes,
// the transpose of a lost block's decode bit-rows into per-survivor-packet
// column masks, the split of the k survivors over launches, and the per-lane
// arithmetic of both kernels.
//
// Why a read is local.  Every code here is linear and acts column by column
// (word classes) or packet position by packet position (packet classes): with
// row j of the decode map of the survivors S,
//     lost_j[x]      = XOR over i of coef[i] * surv_i[x]             (words)
//     lost_j[r][y]   = XOR over (i, c) with bit (j, r, i, c) set of
//                      surv_i[c][y]                                  (packets)
// so bytes [lo, hi) of the lost block need the same columns x, or the same lane
// positions y, of the k survivors and nothing else: about (k + 1) L bytes moved
// for L bytes read.  The range split, the lane masks, the packet map and the
// constant multiply are update_core.hpp's (upd::), used as they are.
//
// Portable C++ (host and device): tests/read_core_test.cpp replays both kernels'
// lanes on the CPU against a brute-force decode with the host field of
// codes.cpp.
#pragma once

#include <cstdint>

#include "update_core.hpp"

namespace leoec {
namespace rd {

// ---------------------------------------------------------------------------
// The groups of a range.

// Segments first .. first + count - 1 of upd::split_range: one lost data block
// (count 1), or a maximal run of intact ones, whose bytes are contiguous in the
// object row: [seg[first].block bs + seg[first].lo, seg[last].block bs + seg[last].hi).
struct Group {
  uint32_t first, count;
  bool lost;
};

// gone[b] != 0: data block b is erased.  out[0..n), n <= cap; returns n, or -1
// when cap is too small (nseg always suffices).
inline int group_segments(const upd::Seg* seg, int nseg, const char* gone, Group* out, int cap) {
  int n = 0;
  for (int i = 0; i < nseg;) {
    if (n == cap) return -1;
    const bool lost = gone[seg[i].block] != 0;
    int e = i + 1;
    if (!lost)
      while (e < nseg && !gone[seg[e].block]) ++e;
    out[n].first = (uint32_t)i;
    out[n].count = (uint32_t)(e - i);
    out[n].lost = lost;
    ++n;
    i = e;
  }
  return n;
}

// ---------------------------------------------------------------------------
// The survivors.

// Bytes of the 16-byte lane at block byte `at` that lie inside the block's
// `valid` bytes (a data block clipped to the object's size; a coding block is
// whole): 0xFFFF loads the lane in one access, anything else gathers those
// bytes and reads the rest as zero, 0 reads nothing.
LEOEC_UPD_HD uint32_t valid_bytes(uint64_t at, uint64_t valid) { return upd::lane_bytes(at, 0u, valid); }

// Valid bytes of block `id` of an object of `size` bytes: data ids (< k) are
// clipped to the object, coding ids are whole.
LEOEC_UPD_HD uint64_t block_valid(uint32_t id, uint32_t k, uint64_t bs, uint64_t size) {
  if (id >= k) return bs;
  const uint64_t start = (uint64_t)id * bs;
  return start >= size ? 0u : size - start < bs ? size - start : bs;
}

// Launch n of the split of `total` survivors into launches of at most `per`.
struct Part {
  uint32_t first, count;
};
LEOEC_UPD_HD uint32_t part_count(uint32_t total, uint32_t per) { return (total + per - 1u) / per; }
LEOEC_UPD_HD Part part(uint32_t total, uint32_t per, uint32_t n) {
  const uint32_t first = n * per;
  return Part{first, total - first < per ? total - first : per};
}

// ---------------------------------------------------------------------------
// The word classes.

// One survivor's share of a lane: acc ^= coef * v, t[b] = spread(coef alpha^b).
template <int W>
LEOEC_UPD_HD void gf_accumulate(uint32_t (&acc)[4], const uint32_t (&v)[4], const uint32_t (&t)[W]) {
  LEOEC_UPD_UNROLL
  for (int d = 0; d < 4; ++d) acc[d] ^= upd::mul_dword<W>(v[d], t);
}

// ---------------------------------------------------------------------------
// The packet classes.

// rows: the w bit-rows of the lost block over the k w survivor packets
// (engine.cpp bit_rows, one wanted id: rows[r * k w + i w + c] != 0 iff packet c
// of survivor i feeds packet r of the lost block).  cols[i w + c] gets bit r set
// for exactly those r: the packets of the lost block that survivor packet
// (i, c) feeds.
inline void transpose_rows(const uint8_t* rows, uint32_t k, uint32_t w, uint32_t* cols) {
  const uint32_t n = k * w;
  for (uint32_t q = 0; q < n; ++q) cols[q] = 0u;
  for (uint32_t r = 0; r < w; ++r)
    for (uint32_t q = 0; q < n; ++q)
      if (rows[(uint64_t)r * n + q]) cols[q] |= 1u << r;
}

// A survivor packet is loaded only where it feeds a touched packet of the lost
// block (upd::touched_packets at the lane's position).
LEOEC_UPD_HD uint32_t column_hits(uint32_t col, uint32_t touched) { return col & touched; }

}  // namespace rd
}  // namespace leoec
