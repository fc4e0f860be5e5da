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
// leaves.  The item's tile is bit_heal_tile (bit_heal_tile.hpp: the one body
// this kernel and bit_heal_masks share), from the block's record of the code's
// block table (scrub_bit_table.hpp).
//
// Every exit and skip is taken by the whole wave: the loop bound, the list
// entry and the object's word are read at wave-uniform addresses through the
// constant address space (uniform_word, heal_impl.hpp).
#pragma once

#include "bit_heal_tile.hpp"
#include "scrub_bit_table.hpp"

namespace leoec {
namespace detail {

// a: BitHealArgs with lost = the chunk's final words, table = the code's block
// table and rec_words = scrub_bit_record_words(k, w).  list: indices into the
// chunk, *count of them, both written by an earlier launch on the stream.
// count x tiles <= nobj x tiles < 2^31.
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
    bit_heal_tile(a.h, a.w, a.ps, acc, rec, rec + kScrubBitIdWords, obj, block, tile);
  }
}

// The fixed grid (list_grid) over the objects a describes (a.h.nobj and
// a.h.tiles are the caller's): objects x tiles items at most.
inline int launch_bit_heal_list(const BitHealArgs& a, const uint32_t* list, const uint32_t* count,
                                uint32_t cap, hipStream_t s) {
  const uint32_t grid = list_grid((uint64_t)a.h.nobj * a.h.tiles, bit_heal_list_resident(a.w), cap);
  return launch_kernel(bit_heal_list, dim3(grid), dim3(kBitHealLanes), bit_heal_lds(a.w), s, a, list,
                       count);
}

}  // namespace detail
}  // namespace leoec
