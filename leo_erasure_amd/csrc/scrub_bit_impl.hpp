// scrub_bit_impl.hpp — bit_heal_list, the rebuild step of leoec_scrub_ws_dev
// for the bitmatrix classes (cauchyrs, liberation), and its launch.  Included
// by scrub.hip alone.
//
// The kernel rebuilds one named block of every object of a list that an
// earlier launch on the stream wrote (scrub_finish, scrub.hip): the host does
// not know how many there are, so the grid is fixed and every workgroup walks
// the items blockIdx.x, blockIdx.x + gridDim.x, ... below count x tiles,
// item -> (object list[item / tiles], tile item % tiles), as gf8_heal_list
// (scrub_impl.hpp).  With a count of 0 every workgroup reads one word and
// leaves.
//
// Shape: bit_locate's (locate.hip).  One wave per workgroup, one 16-byte
// column of packet offsets per lane, 1 KiB of every packet per item, w, k and
// m runtime values: one instance.  The w output packets are accumulators in
// dynamic LDS ([w][64] columns); every lane reads and writes only its own
// slots, so there is no barrier anywhere, and no register array is indexed by
// a runtime value.  The work is input-stationary: for every packet (i, c) of
// the k survivors the block's record (scrub_bit_table.hpp) holds one word
// naming the output packets it feeds; a packet with a zero word is not read,
// any other is loaded once and XORed into the accumulators its word names.
// After the last input the w accumulators go to the w packets of the lost
// block.
//
// Every exit and skip is taken by the whole wave: the loop bound, the list
// entry, the object's word and the record's words are read at wave-uniform
// addresses through the constant address space (uniform_word), which makes
// them scalar loads, and come through readfirstlane.  `full` is the item's
// own, per tile: the tile lies inside the packet, and in every block the item
// reads or writes the tile of every packet lies below the block's valid
// length.  The k survivors and the lost block cover every data id and the
// valid lengths do not grow with the id, so that is the tile of the last
// packet of data block k - 1: (w - 1) ps + t0 + 1 KiB <= its valid length.
// Otherwise survivors are read through shard_rsrc (bytes at or past a block's
// valid length read as zero) and the lost block is written through
// store_guarded, below its own valid length only.
#pragma once

#include "heal_impl.hpp"
#include "scrub_bit_table.hpp"

namespace leoec {
namespace detail {

constexpr int kBitHealLanes = 64;                       // one wave per workgroup
constexpr uint32_t kBitHealTile = kBitHealLanes * 16u;  // bytes of every packet per item

// h: HealArgs of the chunk (lost: the chunk's final words; table: the code's
// block table on the device; tiles: 1 KiB tiles of a packet; unhealed, tmap
// and tperm unused).  ps = bs / w, a multiple of 16.
struct BitHealArgs {
  HealArgs h;
  uint32_t w, ps;
  uint32_t rec_words;  // scrub_bit_record_words(k, w)
  uint32_t pad;
};

// list: indices into the chunk, *count of them, both written by an earlier
// launch on the stream.  count x tiles <= nobj x tiles < 2^31.
__global__ void __launch_bounds__(kBitHealLanes)
bit_heal_list(const BitHealArgs a, const uint32_t* __restrict__ list,
              const uint32_t* __restrict__ count) {
  extern __shared__ u32x4 bit_heal_acc[];  // [w][kBitHealLanes]
  u32x4* const acc = bit_heal_acc + threadIdx.x;
  const uint32_t tiles = a.h.tiles;
  const uint32_t items = uniform_word(count) * tiles;
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t e = item / tiles;
    const uint32_t tile = item - e * tiles;
    const uint32_t obj = uniform_word(list + e);
    // a listed object has exactly one bit below k + m (<= 31); any other word
    // is skipped, the whole wave at once
    const uint32_t word = uniform_word(a.h.lost + obj);
    if (word == 0u || (word & (word - 1u)) != 0u || (word >> (a.h.k + a.h.m)) != 0u) continue;
    const uint32_t block = (uint32_t)__builtin_ctz(word);
    const uint32_t* const rec = a.h.table + (uint64_t)block * a.rec_words;
    const uint8_t* const ob = a.h.objs + (uint64_t)obj * a.h.obj_stride;
    const uint8_t* const pb = a.h.parity + (uint64_t)obj * a.h.parity_stride;
    const DevShard out = heal_shard(a.h, ob, pb, block);
    const uint32_t t0 = tile * kBitHealTile;  // < ps
    // nothing of this tile to write: a lost data block with no valid byte, or
    // one whose every packet ends before the tile (uniform)
    if (out.valid <= t0) continue;
    const uint32_t off = t0 + threadIdx.x * 16u;
    const bool in = off < a.ps;  // ps is a multiple of 16: the column lies inside the packet
    // lanes past the packet read the tile's first column and store nothing
    const uint32_t col = in ? off : t0;
    const uint32_t vlast = heal_shard(a.h, ob, pb, a.h.k - 1u).valid;  // the least of the item's blocks
    const bool full = t0 + kBitHealTile <= a.ps &&
                      (uint64_t)(a.w - 1u) * a.ps + t0 + kBitHealTile <= vlast;
    for (uint32_t r = 0; r < a.w; ++r) acc[r * kBitHealLanes] = u32x4{0u, 0u, 0u, 0u};
    for (uint32_t i = 0; i < a.h.k; ++i) {
      const uint32_t id = (uniform_word(rec + (i >> 2)) >> (8u * (i & 3u))) & 0xFFu;
      const DevShard sh = heal_shard(a.h, ob, pb, id);
      const auto rs = shard_rsrc(sh.base, 0, sh.valid, 0, 16u);
      const uint32_t* const masks = rec + kScrubBitIdWords + i * a.w;
      for (uint32_t c = 0; c < a.w; ++c) {
        const uint32_t mask = uniform_word(masks + c);
        if (mask == 0u) continue;  // uniform
        const uint32_t o = c * a.ps + col;  // < bs
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
    for (uint32_t r = 0; r < a.w; ++r) {
      const u32x4 v = acc[r * kBitHealLanes];
      const uint32_t o = r * a.ps + col;
      if (full) st16<true>(base + o, v);
      else if (in) store_guarded(base, o, out.valid, v);
    }
  }
}

// Workgroups of bit_heal_list that a compute unit holds at once: one wave
// each, 32 waves a compute unit, w KiB of its 160 KiB of LDS each.
inline uint32_t bit_heal_list_resident(uint32_t w) {
  const uint32_t by_lds = 160u / w;  // w <= 32
  return by_lds < 32u ? by_lds : 32u;
}

// The fixed grid over the objects a describes (a.h.nobj and a.h.tiles are the
// caller's): min(objects x tiles, resident workgroups of the device), at most
// `cap` workgroups when cap is not 0 (LEOEC_SCRUB_GRID, measurement build).
inline int launch_bit_heal_list(const BitHealArgs& a, const uint32_t* list, const uint32_t* count,
                                uint32_t cap, hipStream_t s) {
  const uint64_t all = (uint64_t)a.h.nobj * a.h.tiles;
  uint64_t grid = (uint64_t)device_cus() * bit_heal_list_resident(a.w);
  grid = grid < all ? grid : all;
  if (cap != 0u && grid > cap) grid = cap;
  const size_t lds = (size_t)a.w * kBitHealLanes * sizeof(u32x4);  // <= 32 KiB
  return launch_kernel(bit_heal_list, dim3((uint32_t)grid), dim3(kBitHealLanes), lds, s, a, list,
                       count);
}

}  // namespace detail
}  // namespace leoec
