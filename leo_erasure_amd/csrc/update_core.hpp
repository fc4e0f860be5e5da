// update_core.hpp — the arithmetic of leoec_update_dev (update.hip) that needs
// no device: the split of an object byte range into per-data-block segments,
// the bytewise range mask of a 16-byte lane, the constant multiply of the word
// classes on the w-bit words of a dword, and the packet map of the packet
// classes (which data packets a lane position touches, which coding packets a
// bit-row reaches).
//
// Why update is local.  Every code here is linear, so with D = old ^ new
// inside the range and zero elsewhere, parity(new) = parity(old) ^ encode(D).
// D is zero outside the range, so encode(D) is zero outside the columns the
// range's bytes feed: for a word class the w-bit words that hold a byte of the
// range (coding block i, column x gets C[i][j] * D_j[x], data block j alone),
// for a packet class the lane positions y of the touched data packets (coding
// packet (i, r) at y gets the XOR of D's packets (j, c) at y with bit
// B[i w + r][j w + c] set).  A delta masked inside a word or a lane is still
// right: the zero bytes are D's own.
//
// The multiply.  c * x is GF(2)-linear in the bits of x:
//     c * x = XOR over the set bits b of x of (c * alpha^b),
// so with the w products t[b] = c * alpha^b of the launch's coefficient (host,
// kernel arguments, replicated over the dword's 32 / w words)
//     mul_dword(x) = XOR over b of (bit b of every word, spread over the word) & t[b]:
// w steps of shift, and, multiply by 2^w - 1, and, xor per dword and coding
// row, no table in memory, no transpose.  The bitsliced form of gfs_core.hpp
// costs a sixth of that per word at w = 32 but pays a 32-word transpose each
// way and a 32-register tile; update moves (3 + 2m) bytes per patched byte over
// ranges that are short by design, and stays a plain per-lane kernel.
//
// Portable C++ (host and device): tests/update_core_test.cpp checks it on the
// CPU against brute-force byte maps and the host field of codes.cpp.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define LEOEC_UPD_HD __host__ __device__ __forceinline__
#define LEOEC_UPD_UNROLL _Pragma("unroll")
#else
#define LEOEC_UPD_HD inline
#define LEOEC_UPD_UNROLL
#endif

namespace leoec {
namespace upd {

// ---------------------------------------------------------------------------
// The range.

// Bytes [lo, hi) of data block `block`, block-local (0 <= lo < hi <= bs).
struct Seg {
  uint32_t block;
  uint64_t lo, hi;
};

// The segments of object bytes [offset, offset + length) over blocks of bs
// bytes, ascending: out[0..n), n <= cap; returns n, or -1 when cap is too
// small.  length > 0, bs > 0, and the sum does not wrap (the caller's checks).
inline int split_range(uint64_t bs, uint64_t offset, uint64_t length, Seg* out, int cap) {
  const uint64_t end = offset + length;
  int n = 0;
  for (uint64_t j = offset / bs; j * bs < end; ++j) {
    if (n == cap) return -1;
    const uint64_t b0 = j * bs;
    out[n].block = (uint32_t)j;
    out[n].lo = offset > b0 ? offset - b0 : 0;
    out[n].hi = end - b0 < bs ? end - b0 : bs;
    ++n;
  }
  return n;
}

// Bit i set: byte at + i of the 16-byte lane at `at` lies in [lo, hi).
LEOEC_UPD_HD uint32_t lane_bytes(uint64_t at, uint64_t lo, uint64_t hi) {
  if (hi <= at || lo >= at + 16u) return 0u;
  const uint32_t first = lo > at ? (uint32_t)(lo - at) : 0u;            // 0..15
  const uint32_t last = hi < at + 16u ? (uint32_t)(hi - at) : 16u;      // 1..16
  return (0xFFFFu >> (16u - last)) & (0xFFFFu << first) & 0xFFFFu;
}

// The bytes `bytes` of the lane at p, one by one, as four little-endian
// dwords; zero elsewhere, so old ^ new of two gathered lanes is the delta
// masked to the range.  No other byte of the lane is read.
LEOEC_UPD_HD void gather16(const uint8_t* p, uint32_t bytes, uint32_t (&d)[4]) {
  d[0] = d[1] = d[2] = d[3] = 0u;
  LEOEC_UPD_UNROLL
  for (int i = 0; i < 16; ++i)
    if ((bytes >> i) & 1u) d[i / 4] |= (uint32_t)p[i] << (8 * (i % 4));
}

// The bytes `bytes` of the lane at p written from d; no other byte is written.
LEOEC_UPD_HD void scatter16(uint8_t* p, uint32_t bytes, const uint32_t (&d)[4]) {
  LEOEC_UPD_UNROLL
  for (int i = 0; i < 16; ++i)
    if ((bytes >> i) & 1u) p[i] = (uint8_t)(d[i / 4] >> (8 * (i % 4)));
}

// The 16-byte lanes of a block that hold a byte of [lo, hi): first and count.
LEOEC_UPD_HD uint64_t first_lane(uint64_t lo) { return lo / 16u; }
LEOEC_UPD_HD uint64_t lane_count(uint64_t lo, uint64_t hi) { return (hi - 1u) / 16u - lo / 16u + 1u; }

// ---------------------------------------------------------------------------
// The word classes: little-endian w-bit words, 32 / w of them in a dword.

// Bit 0 of every word of a dword.
template <int W>
constexpr uint32_t unit() {
  return W == 8 ? 0x01010101u : W == 16 ? 0x00010001u : 1u;
}
// A word with every bit set.
template <int W>
constexpr uint32_t ones() {
  return W == 32 ? 0xFFFFFFFFu : (1u << (W & 31)) - 1u;
}
// A w-bit value in every word of a dword (the host builds t[b] with it).
template <int W>
LEOEC_UPD_HD uint32_t spread(uint32_t v) {
  return (v & ones<W>()) * unit<W>();
}

// c * (every word of x), t[b] = spread(c * alpha^b).
template <int W>
LEOEC_UPD_HD uint32_t mul_dword(uint32_t x, const uint32_t (&t)[W]) {
  uint32_t acc = 0u;
  LEOEC_UPD_UNROLL
  for (int b = 0; b < W; ++b) acc ^= (((x >> b) & unit<W>()) * ones<W>()) & t[b];
  return acc;
}

// ---------------------------------------------------------------------------
// The packet classes: a block is w packets of ps bytes (ps a multiple of 16).

// Lane positions of a packet that a segment's lanes fall on: the segment's
// lanes are block lanes L0 .. L0 + n - 1, lane L sits at position L mod
// (ps / 16) of packet L / (ps / 16); `count` positions starting at `first`
// and wrapping at ps / 16 cover them all (every position when the segment
// spans a packet or more).
struct Positions {
  uint32_t first, count;
};
LEOEC_UPD_HD Positions packet_positions(uint64_t lo, uint64_t hi, uint32_t ps) {
  const uint64_t per = ps / 16u;
  const uint64_t n = lane_count(lo, hi);
  return Positions{(uint32_t)(first_lane(lo) % per), (uint32_t)(n < per ? n : per)};
}

// Bit c set: byte c ps + y .. + 15 of the block meets [lo, hi): the data
// packets whose lane at position y the segment touches (w <= 32).
LEOEC_UPD_HD uint32_t touched_packets(uint32_t y, uint32_t ps, uint32_t w, uint64_t lo, uint64_t hi) {
  uint32_t t = 0u;
  for (uint32_t c = 0; c < w; ++c)
    if (lane_bytes((uint64_t)c * ps + y, lo, hi)) t |= 1u << c;
  return t;
}

// A coding packet is read and written only when its bit-row (bit c: data
// packet c of the launch's block feeds it) meets a touched packet.
LEOEC_UPD_HD bool row_meets(uint32_t row, uint32_t touched) { return (row & touched) != 0u; }

}  // namespace upd
}  // namespace leoec
