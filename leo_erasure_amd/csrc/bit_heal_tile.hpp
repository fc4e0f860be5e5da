// bit_heal_tile.hpp — the tile body of the packet classes' rebuild kernels
// (cauchyrs, liberation): bit_heal_list (scrub_bit_impl.hpp,
// leoec_scrub_ws_dev) and bit_heal_masks (heal_ws_impl.hpp,
// leoec_heal_ws_dev).  No kernel and no launcher here: a unit that includes
// this gets no code object from it.
//
// Shape: bit_locate's (locate.hip).  One wave per workgroup, one 16-byte
// column of packet offsets per lane, 1 KiB of every packet per item, w, k and
// m runtime values: one instance.  The w output packets are accumulators in
// dynamic LDS ([w][64] columns); every lane reads and writes only its own
// slots, so there is no barrier anywhere, and no register array is indexed by
// a runtime value.  The work is input-stationary: for every packet (i, c) of
// the k survivors the item's record holds one word (feed) naming the output
// packets it feeds; a packet with a zero word is not read, any other is loaded
// once and XORed into the accumulators its word names.  After the last input
// the w accumulators go to the w packets of the lost block.
//
// Everything the tile branches on is wave-uniform: the record's words are read
// at wave-uniform addresses through the constant address space (uniform_word,
// heal_impl.hpp), which makes them scalar loads, and come through
// readfirstlane.  `full` is the item's own, per tile: the tile lies inside the
// packet, and in every block the item reads or writes the tile of every packet
// lies below the block's valid length.  The k survivors and the lost blocks
// cover every data id and the valid lengths do not grow with the id, so that
// is the tile of the last packet of data block k - 1: (w - 1) ps + t0 + 1 KiB
// <= its valid length.  Otherwise survivors are read through shard_rsrc (bytes
// at or past a block's valid length read as zero) and the lost block is
// written through store_guarded, below its own valid length only.
#pragma once

#include "heal_impl.hpp"

namespace leoec {
namespace detail {

constexpr int kBitHealLanes = 64;                       // one wave per workgroup
constexpr uint32_t kBitHealTile = kBitHealLanes * 16u;  // bytes of every packet per item

// h: HealArgs of the chunk (lost: the chunk's words; table: the code's table on
// the device; tiles: 1 KiB tiles of a packet; unhealed, tmap and tperm
// unused).  ps = bs / w, a multiple of 16.
struct BitHealArgs {
  HealArgs h;
  uint32_t w, ps;
  uint32_t rec_words;  // words of a record of the table
  uint32_t pad;
};

// Tile `tile` of every packet of block `block` of object obj, rebuilt from the
// k survivors whose ids are the bytes at `ids` and whose k w feed words stand
// at `feed` (both wave-uniform addresses inside the table).  acc: the lane's
// own column of the workgroup's [w][kBitHealLanes] accumulators.
// Changing this changes 2 kernels: bit_heal_list (scrub_bit_impl.hpp) and
// bit_heal_masks (heal_ws_impl.hpp).
__device__ __forceinline__ void bit_heal_tile(const HealArgs& h, uint32_t w, uint32_t ps, u32x4* acc,
                                              const uint32_t* ids, const uint32_t* feed,
                                              uint32_t obj, uint32_t block, uint32_t tile) {
  const uint8_t* const ob = h.objs + (uint64_t)obj * h.obj_stride;
  const uint8_t* const pb = h.parity + (uint64_t)obj * h.parity_stride;
  const DevShard out = heal_shard(h, ob, pb, block);
  const uint32_t t0 = tile * kBitHealTile;  // < ps
  // nothing of this tile to write: a lost data block with no valid byte, or
  // one whose every packet ends before the tile (uniform)
  if (out.valid <= t0) return;
  const uint32_t off = t0 + threadIdx.x * 16u;
  const bool in = off < ps;  // ps is a multiple of 16: the column lies inside the packet
  // lanes past the packet read the tile's first column and store nothing
  const uint32_t col = in ? off : t0;
  const uint32_t vlast = heal_shard(h, ob, pb, h.k - 1u).valid;  // the least of the object's blocks
  const bool full = t0 + kBitHealTile <= ps && (uint64_t)(w - 1u) * ps + t0 + kBitHealTile <= vlast;
  for (uint32_t r = 0; r < w; ++r) acc[r * kBitHealLanes] = u32x4{0u, 0u, 0u, 0u};
  for (uint32_t i = 0; i < h.k; ++i) {
    const uint32_t id = (uniform_word(ids + (i >> 2)) >> (8u * (i & 3u))) & 0xFFu;
    const DevShard sh = heal_shard(h, ob, pb, id);
    const auto rs = shard_rsrc(sh.base, 0, sh.valid, 0, 16u);
    const uint32_t* const masks = feed + i * w;
    for (uint32_t c = 0; c < w; ++c) {
      const uint32_t mask = uniform_word(masks + c);
      if (mask == 0u) continue;  // uniform
      const uint32_t o = c * ps + col;  // < bs
      u32x4 v;
      if (full) v = ld16<true>(sh.base + o);
      else v = clip_guarded(__builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 2), o, sh.valid);
      for (uint32_t t = mask; t != 0u; t &= t - 1u) {
        u32x4* const p = acc + (uint32_t)__builtin_ctz(t) * kBitHealLanes;
        const u32x4 x = *p;
        *p = u32x4{x[0] ^ v[0], x[1] ^ v[1], x[2] ^ v[2], x[3] ^ v[3]};
      }
    }
  }
  uint8_t* const base = const_cast<uint8_t*>(out.base);
  for (uint32_t r = 0; r < w; ++r) {
    const u32x4 v = acc[r * kBitHealLanes];
    const uint32_t o = r * ps + col;
    if (full) st16<true>(base + o, v);
    else if (in) store_guarded(base, o, out.valid, v);
  }
}

// Workgroups of either kernel that a compute unit holds at once: one wave
// each, 32 waves a compute unit, w KiB of its 160 KiB of LDS each.
inline uint32_t bit_heal_list_resident(uint32_t w) {
  const uint32_t by_lds = 160u / w;  // w <= 32
  return by_lds < 32u ? by_lds : 32u;
}

// Dynamic LDS of a workgroup of either kernel: its accumulators, <= 32 KiB.
inline size_t bit_heal_lds(uint32_t w) { return (size_t)w * kBitHealLanes * sizeof(u32x4); }

}  // namespace detail
}  // namespace leoec
