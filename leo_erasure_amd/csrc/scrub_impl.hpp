// scrub_impl.hpp — gf8_heal_list, the rebuild step of leoec_scrub_dev, and its
// launch template.  Included by scrub.hip (dispatch) and gf8_scrub_inst.hip
// (instances, one translation unit per input count K, as gf8_heal_inst.hip).
//
// gf8_heal_list is gf8_heal's tile body (heal_impl.hpp) over a list of objects
// that an earlier launch on the stream wrote (scrub_finish, scrub.hip): the
// host does not know how many there are, so the grid is fixed and every
// workgroup walks the items blockIdx.x, blockIdx.x + gridDim.x, ... below
// count x tiles, item -> (object list[item / tiles], tile item % tiles).  With
// a count of 0 every workgroup reads one word and leaves.
//
// The body is a copy of gf8_heal's, not a function the two share: gf8_heal's
// text, and with it its code objects and register table, stays as it is.
// What the loop adds:
//   * the record's tables are staged into LDS once per item, so a barrier
//     stands between an item's last LDS read and the next item's staging;
//   * the loop bound, the list entry and the mask come through readfirstlane
//     and every exit and skip is taken before the item's barriers, so the
//     whole workgroup takes it;
//   * `full` is the item's own: the minimum valid length of the blocks this
//     object reads and writes.
#pragma once

#include "heal_impl.hpp"

namespace leoec {
namespace detail {

// One (object, tile) of gf8_heal: steps 2 to 5 of its text.  mask: the
// object's word, recoverable and not 0 (workgroup-uniform).
template <int K, int R>
__device__ __forceinline__ void heal_list_tile(const HealArgs& a, Gf8Lds<K, R>& lds, uint32_t obj,
                                               uint32_t tile, uint32_t mask) {
  constexpr uint32_t CS = (uint32_t)kThreads * 16u;
  const uint32_t TBr = blockDim.x * 16u;  // tile width = workgroup size (256 or 64 lanes)
  const uint32_t bits = (uint32_t)__builtin_popcount(mask);
  // the record (gf8_heal, step 2)
  const uint32_t* T = a.table;
  uint32_t idx = T[kHealFirst + bits];
  uint32_t rest = mask;
#pragma unroll
  for (uint32_t i = 1; i <= (uint32_t)R; ++i) {
    const uint32_t bit = rest != 0u ? (uint32_t)__builtin_ctz(rest) : 0u;
    idx += T[kHealBinom + bit * (uint32_t)(kHealMaxLost + 1) + i];
    rest &= rest - 1u;
  }
  idx = __builtin_amdgcn_readfirstlane(idx);
  const uint32_t* rec = T + kHealHeaderWords + (uint64_t)idx * (kHealIdWords + 5u * a.m * (uint32_t)K);
  uint32_t idw[(K + R + 3) / 4];
#pragma unroll
  for (int x = 0; x < (K + R + 3) / 4; ++x) idw[x] = rec[x];
  // its tables (step 3)
  for (uint32_t i = threadIdx.x; i < (uint32_t)(R * K); i += blockDim.x) {
    u32x4 lo = {0u, 0u, 0u, 0u}, hi = {0u, 0u, 0u, 0u};
    if (i < a.m * (uint32_t)K) {
      const uint32_t* t = rec + kHealIdWords + 5u * i;
      lo = u32x4{t[0], t[1], t[2], t[3]};
      hi[0] = t[4];
    }
    lds.t[i][0] = lo;
    lds.t[i][1] = hi;
  }
#pragma unroll
  for (int x = 0; x < (K + R + 3) / 4; ++x) asm volatile("" : "+v"(idw[x]));  // loaded by here
  __syncthreads();
  // its shards and this item's `full` (step 4)
  Gf8Args<K, R> g;  // in / out only: the tables are in LDS
  const uint8_t* ob = a.objs + (uint64_t)obj * a.obj_stride;
  const uint8_t* pb = a.parity + (uint64_t)obj * a.parity_stride;
  uint32_t vmin = 0xFFFFFFFFu;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    g.in[j] = heal_shard(a, ob, pb, heal_id(idw, j));
    vmin = g.in[j].valid < vmin ? g.in[j].valid : vmin;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    g.out[r] = DevShard{nullptr, 0, 0, 0};
    if ((uint32_t)r < bits) {
      g.out[r] = heal_shard(a, ob, pb, heal_id(idw, K + r));
      vmin = g.out[r].valid < vmin ? g.out[r].valid : vmin;
    }
  }
  const uint32_t t0 = tile * TBr;
  const uint32_t off = t0 + threadIdx.x * 16u;
  const bool full = t0 + TBr <= vmin;  // wave-uniform
  // the tile (step 5)
  u32x4 d[1][K];
  gf8_load<K, R, 1, true, CS>(g, 0, off, full, d);
  u32x4 acc[1][R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[0][r] = u32x4{0u, 0u, 0u, 0u};
  gf8_tile<K, R, 1, false, false, true>(g, lds, d, acc);
  // gf8_heal's pin: every row computed here, not in its conditional store
#pragma unroll
  for (int r = 0; r < R; ++r) asm volatile("" : "+v"(acc[0][r]));
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if ((uint32_t)r >= bits) break;  // unused rows store nothing (uniform)
    uint8_t* base = const_cast<uint8_t*>(g.out[r].base);
    const uint32_t valid = g.out[r].valid;
    if (full) {
      st16<true>(base + off, acc[0][r]);
    } else {
      const auto rs = shard_rsrc(base, 0, valid & ~15u, 0, 16u);
      __builtin_amdgcn_raw_buffer_store_b128(acc[0][r], rs, off, 0, 2);
      if (off < valid && off + 16u > valid) store_guarded(base, off, valid, acc[0][r]);
    }
  }
}

// a: HealArgs of the chunk (lost: the chunk's final words; unhealed, tmap and
// tperm unused); list: indices into the chunk, *count of them, both written by
// an earlier launch on the stream.  count x tiles <= nobj x tiles < 2^31.
template <int K, int R, int WAVES>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(WAVES, 8)))
gf8_heal_list(const HealArgs a, const uint32_t* __restrict__ list,
              const uint32_t* __restrict__ count) {
  __shared__ Gf8Lds<K, R> lds;
  const uint32_t items = __builtin_amdgcn_readfirstlane(*count) * a.tiles;
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t e = item / a.tiles;
    const uint32_t tile = item - e * a.tiles;
    const uint32_t obj = __builtin_amdgcn_readfirstlane(list[e]);
    // a listed object has one bit below k + m; any other word is skipped as
    // gf8_heal leaves it, the whole workgroup at once and before any barrier
    const uint32_t mask = __builtin_amdgcn_readfirstlane(a.lost[obj]);
    const bool bad = (uint32_t)__builtin_popcount(mask) > a.m || ((uint64_t)mask >> (a.k + a.m)) != 0ull;
    if (mask == 0u || bad) continue;
    heal_list_tile<K, R>(a, lds, obj, tile, mask);
    __syncthreads();  // every wave has read this item's tables: the next item may stage its own
  }
}

// Workgroups of gf8_heal_list that a compute unit holds at once under its
// register budget: 4 SIMDs of kGf8HealWaves waves, wg / 64 waves a workgroup
// (its LDS, 2 KiB at most, never binds).
inline uint32_t gf8_heal_list_resident(uint32_t wg) { return 4u * (uint32_t)kGf8HealWaves * 64u / wg; }

// The fixed grid over the objects a describes (a.nobj is the caller's):
// min(objects x tiles, resident workgroups of the device), at most `cap`
// workgroups when cap is not 0 (LEOEC_SCRUB_GRID, measurement build).
template <int K>
int launch_gf8_heal_list_t(HealArgs a, const uint32_t* list, const uint32_t* count, uint32_t cap,
                           hipStream_t s) {
  const Gf8Grid g = gf8_grid_env(a.bs);
  const uint32_t wg = g.wg;
  gf8_set_grid(a, g, a.nobj);
  const uint64_t all = (uint64_t)a.nobj * a.tiles;
  uint64_t grid = (uint64_t)device_cus() * gf8_heal_list_resident(wg);
  grid = grid < all ? grid : all;
  if (cap != 0u && grid > cap) grid = cap;
  return launch_kernel((gf8_heal_list<K, kMaxR, kGf8HealWaves>), dim3((uint32_t)grid), dim3(wg), 0,
                       s, a, list, count);
}

using HealListFn = int (*)(HealArgs, const uint32_t*, const uint32_t*, uint32_t, hipStream_t);

// Defined (explicitly specialised) in gf8_scrub_inst.hip, one TU per K.
template <int K>
HealListFn gf8_heal_list_launcher();

}  // namespace detail
}  // namespace leoec
