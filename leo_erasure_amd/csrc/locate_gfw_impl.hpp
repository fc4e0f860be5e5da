// locate_gfw_impl.hpp — gfw_locate<W>, the kernel behind leoec_locate_gfw_dev
// (locate.hip) for the GF(2^w) word classes: vandrs w = 16 / 32 and vandrs /
// isars w = 8 outside leoec_locate_dev's k <= 16, m <= 4.  It runs on the
// two-pass verify's workspace: syndromes = freshly encoded ^ stored coding
// blocks, tested with locate_wrows.hpp's ratios.
//
// The first part is portable C++ (host and device): the per-lane test "does
// c * s_0 equal s_i" on a lane's 64 bytes, which tests/gfw_locate_core_test.cpp
// checks on the CPU against the oracle's field arithmetic.  The kernel follows
// under __HIPCC__.
#pragma once

#include <cstdint>

#include "gfs_core.hpp"

namespace leoec {
namespace gfwloc {

constexpr int kRegs = 16;  // registers per value: a lane's 64 bytes of a block, as gfs_apply

// x * alpha on four GF(2^8) elements packed in a register; red: the low byte
// of the field polynomial (alpha^8 reduced).
LEOEC_GFS_HD uint32_t xtime4(uint32_t x, uint32_t red) {
  const uint32_t top = (x >> 7) & 0x01010101u;  // 0 or 1 per byte: top * red stays inside its byte
  return ((x & 0x7F7F7F7Fu) << 1) ^ (top * red);
}

// The domain in which misfit() compares: bit-planes for W = 16 / 32
// (gfs_core.hpp; the transpose is a bijection, so nothing is transposed
// back), the bytes as they are for W = 8.
template <int W>
LEOEC_GFS_HD void to_domain(uint32_t (&r)[kRegs]) {
  if constexpr (W != 8) gfs::transpose<kRegs>(r);
}

// OR over the lane's registers of c * s0 ^ si: zero iff c * s0 == si in every
// word of the lane.  s0 and si are in to_domain<W>'s form and are left as
// they are; c (and red, W = 8 only) must be wave-uniform on the device: the
// tests of c's bits are scalar branches.
//   W = 16: gfs::mac<16, 1>; W = 32: gfs::mac_p32<1> (the packed layout);
//   W = 8: shift-and-xor on packed bytes, one step per bit of c: no table and
//   no v_perm.
template <int W>
LEOEC_GFS_HD uint32_t misfit(uint32_t c, const uint32_t (&s0)[kRegs], const uint32_t (&si)[kRegs],
                             uint32_t red) {
  static_assert(W == 8 || W == 16 || W == 32, "word widths of the matrix classes");
  uint32_t x[kRegs];
#pragma unroll
  for (int r = 0; r < kRegs; ++r) x[r] = s0[r];
  uint32_t acc[1][kRegs];
#pragma unroll
  for (int r = 0; r < kRegs; ++r) acc[0][r] = 0u;
  if constexpr (W == 8) {
#pragma unroll 1
    for (uint32_t t = c & 0xFFu; t != 0u; t >>= 1) {
      if (t & 1u) {
#pragma unroll
        for (int r = 0; r < kRegs; ++r) acc[0][r] ^= x[r];
      }
#pragma unroll
      for (int r = 0; r < kRegs; ++r) x[r] = xtime4(x[r], red);
    }
  } else {
    const uint32_t cc[1] = {c};
    if constexpr (W == 32) gfs::mac_p32<1>(x, acc, cc);
    else gfs::mac<16, 1>(x, acc, cc);
  }
  uint32_t nz = 0u;
#pragma unroll
  for (int r = 0; r < kRegs; ++r) nz |= acc[0][r] ^ si[r];
  return nz;
}

}  // namespace gfwloc
}  // namespace leoec

#if defined(__HIPCC__) || defined(__HIP__)

#include "kernels_impl.hpp"

namespace leoec {
namespace detail {

constexpr int kGfwLocLanes = 64;  // one wave per workgroup
constexpr int kGfwLocLoads = gfwloc::kRegs / 4;
constexpr uint32_t kGfwLocTile = kGfwLocLanes * 16u * kGfwLocLoads;  // gfs_apply's: 4 KiB of a block
constexpr int kGfwLocWords = 240;  // (m - 1) k at most: k + (m - 1) <= 31

// ws: the chunk's freshly encoded coding blocks, object o at o * per
// (per = m bs, packed: coding block i at i * bs); parity: the stored ones,
// object o at o * parity_stride, the same rows.
struct GfwLocArgs {
  const uint8_t* ws;
  const uint8_t* parity;
  uint64_t parity_stride;
  uint64_t per;
  uint32_t bs, tiles, k, m;
  uint32_t red;  // W = 8: the field polynomial's low byte (gfwloc::xtime4)
  uint32_t pad;
  uint32_t ratio[kGfwLocWords];  // locate_build_wrows' words
};
static_assert(sizeof(GfwLocArgs) + sizeof(uint32_t*) == 1024, "kernel argument segment");

// A lane's four 16-byte chunks, 1 KiB apart, of enc ^ sto: the syndrome of one
// coding block.  Chunks at or past the block's end read as zeros from both
// resources (shard_rsrc), a zero syndrome, which fits every block.
__device__ __forceinline__ void gfw_syndrome(__amdgpu_buffer_rsrc_t enc, __amdgpu_buffer_rsrc_t sto,
                                             uint32_t off, uint32_t (&s)[gfwloc::kRegs]) {
#pragma unroll
  for (int c = 0; c < kGfwLocLoads; ++c) {
    const uint32_t at = off + (uint32_t)c * (kGfwLocLanes * 16u);
    const u32x4 e = __builtin_amdgcn_raw_buffer_load_b128(enc, at, 0, 0);
    const u32x4 p = __builtin_amdgcn_raw_buffer_load_b128(sto, at, 0, 2);  // streamed once
#pragma unroll
    for (int x = 0; x < 4; ++x) s[4 * c + x] = e[x] ^ p[x];
  }
}

// One workgroup (one wave) per (object, 4 KiB of a block): gfs_apply's
// geometry, k and m runtime values.
// Clean path: per coding block the lane's four syndrome chunks ORed, one
// ballot per block; a wave with no non-zero syndrome ends there and writes
// nothing.
// Dirty path (the candidate mask over k + m bits stays in SGPRs): coding block
// i is a candidate when no syndrome but s_i is non-zero; data blocks only when
// every syndrome is (no entry of C is zero: a column that fits a data block
// is non-zero in every syndrome or in none).  Then s_0 is formed once (and
// kept in 4 KiB of LDS), every s_i is loaded once (the loop over i is the outer one, so one s_i is live)
// and compared with T[i][j] s_0 for every data block j still in the running,
// the ratio by a scalar load from the argument.  Both loops stay rolled: one
// copy of the multiply.  lost[o]: the word of object o of this launch (all
// ones beforehand).
template <int W>
__global__ void __launch_bounds__(kGfwLocLanes) __attribute__((amdgpu_waves_per_eu(8)))
gfw_locate(const GfwLocArgs a, uint32_t* __restrict__ lost) {
  const uint32_t obj = blockIdx.x / a.tiles;
  const uint32_t t0 = (blockIdx.x - obj * a.tiles) * kGfwLocTile;  // < bs
  const uint32_t off = t0 + threadIdx.x * 16u;
  const uint64_t o = obj;  // the object offsets in 64 bits
  auto enc = [&](uint32_t i) { return shard_rsrc(a.ws + (uint64_t)i * a.bs, a.per, a.bs, o, 16u); };
  auto sto = [&](uint32_t i) {
    return shard_rsrc(a.parity + (uint64_t)i * a.bs, a.parity_stride, a.bs, o, 16u);
  };
  uint32_t dirty = 0;  // wave-uniform: bit i set when any lane's syndrome of block i is non-zero
  for (uint32_t i = 0; i < a.m; ++i) {  // m <= 31
    uint32_t s[gfwloc::kRegs];
    gfw_syndrome(enc(i), sto(i), off, s);
    uint32_t nz = 0;
#pragma unroll
    for (int r = 0; r < gfwloc::kRegs; ++r) nz |= s[r];
    if (__builtin_amdgcn_ballot_w64(nz != 0u) != 0ull) dirty |= 1u << i;
  }
  if (dirty == 0u) return;
  // The cold branch.
  uint32_t mask = 0;
  for (uint32_t i = 0; i < a.m; ++i)
    if ((dirty & ~(1u << i)) == 0u) mask |= 1u << (a.k + i);  // k + i <= 31
  if (dirty == (1u << a.m) - 1u) {
    uint32_t s0[gfwloc::kRegs];
    gfw_syndrome(enc(0), sto(0), off, s0);
    gfwloc::to_domain<W>(s0);
    // s_0 waits in LDS (each lane reads back only what it wrote: no barrier)
    // and is read again for every product, which destroys its copy: kept in
    // registers beside s_i, the copy and the accumulator it made w = 32 a
    // 198-VGPR kernel (2 waves per SIMD on the clean path too); this way every
    // width fits the 8-wave budget (64 VGPRs) without a spill.
    __shared__ u32x4 s0_keep[kGfwLocLoads][kGfwLocLanes];
#pragma unroll
    for (int q = 0; q < kGfwLocLoads; ++q)
      s0_keep[q][threadIdx.x] = u32x4{s0[4 * q], s0[4 * q + 1], s0[4 * q + 2], s0[4 * q + 3]};
    const uint32_t all = (1u << a.k) - 1u;  // k <= 30
    uint32_t notfit = 0;                    // wave-uniform: data blocks some column does not fit
#pragma unroll 1
    for (uint32_t i = 1; i < a.m && notfit != all; ++i) {
      uint32_t si[gfwloc::kRegs];
      gfw_syndrome(enc(i), sto(i), off, si);
      gfwloc::to_domain<W>(si);
#pragma unroll 1
      for (uint32_t j = 0; j < a.k; ++j) {
        if ((notfit >> j) & 1u) continue;
        const uint32_t c = a.ratio[(i - 1u) * a.k + j];
        uint32_t x[gfwloc::kRegs];
#pragma unroll
        for (int q = 0; q < kGfwLocLoads; ++q) {
          const u32x4 v = s0_keep[q][threadIdx.x];
#pragma unroll
          for (int e = 0; e < 4; ++e) x[4 * q + e] = v[e];
        }
        if (__builtin_amdgcn_ballot_w64(gfwloc::misfit<W>(c, x, si, a.red) != 0u) != 0ull)
          notfit |= 1u << j;
      }
    }
    mask |= ~notfit & all;
  }
  if (threadIdx.x == 0u) atomicAnd(&lost[obj], mask);
}

}  // namespace detail
}  // namespace leoec

#endif  // __HIPCC__
