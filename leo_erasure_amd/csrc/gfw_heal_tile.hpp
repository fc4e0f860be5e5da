// gfw_heal_tile.hpp — the tile body of the GF(2^w) word classes' rebuild
// kernels (vandrs w = 16 / 32, vandrs / isars w = 8 outside the fused family's
// k <= 16, m <= 4): gfw_heal_list<W> (scrub_gfw_impl.hpp, leoec_scrub_gfw_dev)
// and gfw_heal_masks<W> (heal_ws_impl.hpp, leoec_heal_ws_dev).  No kernel and
// no launcher here: a unit that includes this gets no code object from it.
//
// The first part is portable C++ (host and device): the per-lane arithmetic
// "acc ^= c * x" on a lane's 64 bytes and the way back to bytes, which
// tests/gfw_heal_core_test.cpp checks on the CPU against the oracle's field
// arithmetic.  The tile follows under __HIPCC__.
//
// Shape: gfw_locate's and gfs_apply's.  One wave per workgroup, a 4 KiB tile of
// a block per item, 64 bytes per lane as four 16-byte chunks 1 KiB apart, 16
// registers per value; k and m runtime values: one instance per width.  The
// item's record names the k survivors (ids) and their coefficients (coef);
// every survivor is loaded once, moved into the multiply domain (bit-planes for
// W = 16 / 32, the bytes as they are for W = 8) and accumulated into one
// register-resident row, the next survivor's loads in flight meanwhile (two
// buffers, as gfs_apply).  No LDS, no register array indexed by a runtime
// value.
//
// Everything the tile branches on is wave-uniform: the record's words are read
// at wave-uniform addresses through the constant address space (uniform_word,
// heal_impl.hpp).  `full` is the item's own, per tile: the k survivors and the
// lost blocks cover every data id and the valid lengths do not grow with the
// id, so the tile lies below the valid length of every block the item reads or
// writes when t0 + 4 KiB <= valid(data block k - 1).  Survivors are read
// through shard_rsrc (bytes at or past a block's valid length read as zero; the
// chunk that straddles it is cleared when the tile is not full) and the lost
// block is then written through store_guarded, below its own valid length only.
#pragma once

#include <cstdint>

#include "gfs_core.hpp"
#include "locate_gfw_impl.hpp"

namespace leoec {
namespace gfwheal {

constexpr int kRegs = gfwloc::kRegs;  // registers per value: a lane's 64 bytes of a block

// acc ^= c * x on the lane's words.  x: the bytes as loaded (destroyed); acc:
// in the multiply domain (gfwloc::to_domain<W>'s form).  c (and red, W = 8
// only: the field polynomial's low byte) must be wave-uniform on the device:
// the tests of c's bits are scalar branches.
//   W = 16: gfs::mac<16, 1>; W = 32: gfs::mac_p32<1> (the packed layout);
//   W = 8: shift-and-xor on packed bytes, one step per bit of c.
template <int W>
LEOEC_GFS_HD void mac_in(uint32_t c, uint32_t (&x)[kRegs], uint32_t (&acc)[1][kRegs], uint32_t red) {
  static_assert(W == 8 || W == 16 || W == 32, "word widths of the matrix classes");
  if constexpr (W == 8) {
#pragma unroll 1
    for (uint32_t t = c & 0xFFu; t != 0u; t >>= 1) {
      if (t & 1u) {
#pragma unroll
        for (int r = 0; r < kRegs; ++r) acc[0][r] ^= x[r];
      }
#pragma unroll
      for (int r = 0; r < kRegs; ++r) x[r] = gfwloc::xtime4(x[r], red);
    }
  } else {
    gfwloc::to_domain<W>(x);
    const uint32_t cc[1] = {c};
    if constexpr (W == 32) gfs::mac_p32<1>(x, acc, cc);
    else gfs::mac<16, 1>(x, acc, cc);
  }
}

// Back from the domain: the accumulator as the bytes to store.  (The transpose
// is its own inverse.)
template <int W>
LEOEC_GFS_HD void from_domain(uint32_t (&acc)[1][kRegs]) {
  if constexpr (W != 8) gfs::transpose<kRegs>(acc[0]);
}

}  // namespace gfwheal
}  // namespace leoec

#if defined(__HIPCC__) || defined(__HIP__)

#include "heal_impl.hpp"

namespace leoec {
namespace detail {

constexpr int kGfwHealLanes = 64;  // one wave per workgroup
constexpr int kGfwHealLoads = gfwheal::kRegs / 4;
constexpr uint32_t kGfwHealTile = kGfwHealLanes * 16u * kGfwHealLoads;  // 4 KiB of a block per item
constexpr int kGfwHealWaves = 4;  // waves per SIMD the register budget allows (128 VGPRs)

// h: HealArgs of the chunk (lost: the chunk's words; table: the code's table on
// the device; tiles: 4 KiB tiles of a block; unhealed, tmap and tperm unused).
struct GfwHealArgs {
  HealArgs h;
  uint32_t rec_words;  // words of a record of the table
  uint32_t red;        // W = 8: the field polynomial's low byte (gfwloc::xtime4)
};
static_assert(sizeof(GfwHealArgs) + 2 * sizeof(uint32_t*) == 120, "kernel argument segment");

// A lane's four 16-byte chunks, 1 KiB apart, of one block.
__device__ __forceinline__ void gfw_heal_load(__amdgpu_buffer_rsrc_t rs, uint32_t off,
                                              uint32_t (&x)[gfwheal::kRegs]) {
#pragma unroll
  for (int c = 0; c < kGfwHealLoads; ++c) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(
        rs, off + (uint32_t)c * (kGfwHealLanes * 16u), 0, 2);  // streamed once
#pragma unroll
    for (int e = 0; e < 4; ++e) x[4 * c + e] = v[e];
  }
}

// Clear the bytes at or past `valid` (tiles that are not full only; gfs_tail's
// arithmetic).
__device__ __forceinline__ void gfw_heal_tail(uint32_t off, uint32_t valid,
                                              uint32_t (&x)[gfwheal::kRegs]) {
#pragma unroll
  for (int c = 0; c < kGfwHealLoads; ++c) {
    const uint32_t at = off + (uint32_t)c * (kGfwHealLanes * 16u);
    const uint32_t n = at >= valid ? 0u : (valid - at > 16u ? 16u : valid - at);
    const u32x4 v = keep_first(u32x4{x[4 * c], x[4 * c + 1], x[4 * c + 2], x[4 * c + 3]}, n);
#pragma unroll
    for (int e = 0; e < 4; ++e) x[4 * c + e] = v[e];
  }
}

// Tile `tile` of block `block` of object obj, rebuilt from the k survivors
// whose ids are the bytes at `ids` and whose coefficients are the k words at
// `coef` (both wave-uniform addresses inside the table; red: GfwHealArgs').
// Changing this changes 6 kernels: gfw_heal_list<8|16|32> (scrub_gfw_impl.hpp)
// and gfw_heal_masks<8|16|32> (heal_ws_impl.hpp).
template <int W>
__device__ __forceinline__ void gfw_heal_tile(const HealArgs& h, const uint32_t* ids,
                                              const uint32_t* coef, uint32_t red, uint32_t obj,
                                              uint32_t block, uint32_t tile) {
  const uint8_t* const ob = h.objs + (uint64_t)obj * h.obj_stride;
  const uint8_t* const pb = h.parity + (uint64_t)obj * h.parity_stride;
  const DevShard out = heal_shard(h, ob, pb, block);
  const uint32_t t0 = tile * kGfwHealTile;  // < bs
  // nothing of this tile to write: a lost data block with no valid byte, or
  // one that ends before the tile (uniform)
  if (out.valid <= t0) return;
  const uint32_t off = t0 + threadIdx.x * 16u;
  const uint32_t vlast = heal_shard(h, ob, pb, h.k - 1u).valid;  // the least of the object's blocks
  const bool full = t0 + kGfwHealTile <= vlast;
  // survivor i of the record; past the last one an empty range (valid 0),
  // the target of the loop's last prefetch: its loads return zeros
  auto shard = [&](uint32_t i) {
    if (i >= h.k) return DevShard{ob, 0, 0u, 0u};
    const uint32_t id = (uniform_word(ids + (i >> 2)) >> (8u * (i & 3u))) & 0xFFu;
    return heal_shard(h, ob, pb, id);
  };
  auto load = [&](const DevShard& sh, uint32_t (&x)[gfwheal::kRegs]) {
    gfw_heal_load(shard_rsrc(sh.base, 0, sh.valid, 0, 16u), off, x);
  };
  uint32_t acc[1][gfwheal::kRegs];
#pragma unroll
  for (int r = 0; r < gfwheal::kRegs; ++r) acc[0][r] = 0u;
  auto step = [&](uint32_t i, const DevShard& sh, uint32_t (&x)[gfwheal::kRegs]) {
    const uint32_t c = uniform_word(coef + i);
    if (!full) gfw_heal_tail(off, sh.valid, x);
    gfwheal::mac_in<W>(c, x, acc, red);
  };
  // two input buffers: survivor i + 1 is loaded into one while survivor i is
  // accumulated in place in the other
  uint32_t bufa[gfwheal::kRegs], bufb[gfwheal::kRegs];
  DevShard cur = shard(0), nx = shard(1);
  load(cur, bufa);
#pragma unroll 1
  for (uint32_t i = 0;; i += 2) {
    load(nx, bufb);  // survivor i + 1 (or empty)
    const DevShard nx2 = shard(i + 2);
    step(i, cur, bufa);
    if (i + 1 >= h.k) break;
    load(nx2, bufa);  // survivor i + 2 (or empty)
    const DevShard nx3 = shard(i + 3);
    step(i + 1, nx, bufb);
    if (i + 2 >= h.k) break;
    cur = nx2;
    nx = nx3;
  }
  gfwheal::from_domain<W>(acc);
  uint8_t* const base = const_cast<uint8_t*>(out.base);
#pragma unroll
  for (int c = 0; c < kGfwHealLoads; ++c) {
    const uint32_t at = off + (uint32_t)c * (kGfwHealLanes * 16u);
    const u32x4 v = {acc[0][4 * c], acc[0][4 * c + 1], acc[0][4 * c + 2], acc[0][4 * c + 3]};
    if (full) st16<true>(base + at, v);
    else store_guarded(base, at, out.valid, v);
  }
}

// Workgroups of either kernel that a compute unit holds at once: one wave
// each, kGfwHealWaves waves on each of its 4 SIMDs, no LDS.
inline uint32_t gfw_heal_list_resident() { return 4u * (uint32_t)kGfwHealWaves; }

}  // namespace detail
}  // namespace leoec

#endif  // __HIPCC__
