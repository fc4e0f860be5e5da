// heal_impl.hpp — gf8_heal, the fused GF(2^8) kernel behind leoec_heal_dev,
// and its launch template.  Included by heal.hip (dispatch) and
// gf8_heal_inst.hip (instances, one translation unit per input count K, as
// gf8_check_inst.hip).
//
// gf8_heal is gf8_apply's tile arithmetic with the survivor blocks, the
// output blocks and the coefficient tables chosen per object instead of per
// launch: a workgroup reads its object's mask of lost block ids, ranks it
// into the code's pattern table (heal_table.hpp) and takes everything else
// from that record.  A clean object costs its workgroups one scalar load and
// an exit; a damaged one reads its k survivors once and writes its lost
// blocks once.
//
// Launch geometry and the workgroup -> (object, tile) decode are gf8_apply's
// (gf8_grid_env, gf8_wg_tile in kernels_impl.hpp): HealArgs carries the same
// tiles / nobj / tmap / tperm fields as Gf8Args.
//
// Everything after the mask test is gf8_heal_tile, which gf8_heal_list
// (scrub_impl.hpp) calls per item of its list.  What every list kernel and
// its launcher take from here besides: uniform_word, heal_shard, list_append
// (the listing step) and list_grid (the fixed grid).
#pragma once

#include "heal_table.hpp"
#include "kernels_impl.hpp"

namespace leoec {
namespace detail {

static_assert(kHealMaxLost == kMaxR && kHealMaxK == kMaxK, "record shape = one launch's K x R");

// Register budget: 4 waves per SIMD (128 VGPRs), as gf8_check: gf8_heal<10,4>
// takes 97 VGPRs and <16,4> 122, nothing spilled to scratch (<16,4> keeps 27
// of its SGPRs, the addresses and lengths of 20 blocks, in VGPR lanes).
// Under gf8_apply's budget of 5 (96 VGPRs) <10,4> spills 2 VGPRs and <16,4>
// 26 (Heal).  -DLEOEC_GF8_HEAL_WAVES=n compiles another budget
// (how those figures were taken).
#ifndef LEOEC_GF8_HEAL_WAVES
#define LEOEC_GF8_HEAL_WAVES 4
#endif
constexpr int kGf8HealWaves = LEOEC_GF8_HEAL_WAVES;

struct HealArgs {
  uint8_t* objs;           // object 0 of the launch
  uint64_t obj_stride;
  uint8_t* parity;
  uint64_t parity_stride;
  const uint32_t* lost;    // word 0 = object 0 of the launch
  uint32_t* unhealed;
  const uint32_t* table;   // heal_table.hpp's device image of the code
  uint64_t size;
  uint32_t bs;             // block size (< 2^32, a multiple of 16)
  uint32_t k, m;
  uint32_t tiles;          // tiles per object
  uint32_t nobj;           // objects of the launch
  uint32_t tmap, tperm;    // gf8_apply's tile maps (Gf8Args)
};

// Byte x of a record's id words (wave-uniform).
template <int N>
__device__ __forceinline__ uint32_t heal_id(const uint32_t (&idw)[N], int x) {
  return __builtin_amdgcn_readfirstlane((idw[x >> 2] >> (8 * (x & 3))) & 0xFFu);
}

// The word at p, for a wave-uniform p that nothing writes while the kernel
// runs (the list kernels of scrub.hip: the table; the list, its count and the
// words, which an earlier launch on the stream wrote).  A kernel that stores
// gets a vector load and a full vmcnt wait for a plain uniform load, since the
// compiler cannot rule out that its own stores reach the word; the constant
// address space says they do not.
__device__ __forceinline__ uint32_t uniform_word(const uint32_t* p) {
  typedef const uint32_t __attribute__((address_space(4))) const_word;
  return __builtin_amdgcn_readfirstlane(*reinterpret_cast<const_word*>(reinterpret_cast<uintptr_t>(p)));
}

// Block `id` of the object whose rows start at ob (objs) and pb (parity): a
// data id is clipped to the object's size, a coding id is whole.  The id comes
// from the record through readfirstlane (heal_id), so everything here is
// wave-uniform and stays in SGPRs; shard_rsrc says so once more for the words
// of a buffer resource, where a divergent one costs a waterfall loop around
// every load.
__device__ __forceinline__ DevShard heal_shard(const HealArgs& a, const uint8_t* ob,
                                               const uint8_t* pb, uint32_t id) {
  DevShard s;
  const uint64_t start = (uint64_t)(id < a.k ? id : id - a.k) * a.bs;
  uint32_t valid = a.bs;
  if (id < a.k) valid = a.size <= start ? 0u : (a.size - start < a.bs ? (uint32_t)(a.size - start) : a.bs);
  s.base = (id < a.k ? ob : pb) + start;
  s.stride = 0;
  s.valid = __builtin_amdgcn_readfirstlane(valid);
  s.pad = 0;
  return s;
}

// The listing step's compaction, one lane per object i of the chunk.  A wave
// whose lanes say `one` (rebuild this object) takes its stretch of the list
// with one atomicAdd on *count (list != nullptr) and adds their number to
// totals[0] with another; one whose lanes say `many` adds theirs to totals[1].
// A wave with neither issues no atomic.  No lane leaves early before this:
// lanes past the chunk come with neither, so lane 0 is there to issue the
// wave's atomics.  The order of the list is whatever order the waves arrive in.
// Changing this changes 2 kernels: scrub_finish (scrub.hip) and heal_ws_list
// (heal_ws_impl.hpp).
__device__ __forceinline__ void list_append(bool one, bool many, uint32_t i,
                                            uint32_t* __restrict__ list,
                                            uint32_t* __restrict__ count,
                                            uint32_t* __restrict__ totals) {
  const uint64_t b1 = __builtin_amdgcn_ballot_w64(one);
  const uint64_t bm = __builtin_amdgcn_ballot_w64(many);
  if ((b1 | bm) == 0ull) return;  // wave-uniform
  const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  if (b1 != 0ull) {
    const uint32_t c = (uint32_t)__builtin_popcountll(b1);
    uint32_t base = 0;
    if (lane == 0u) {
      if (list) base = atomicAdd(count, c);
      atomicAdd(&totals[0], c);
    }
    base = __builtin_amdgcn_readfirstlane(base);
    // the lane's rank among the wave's listed lanes
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(b1 >> 32),
                                                    __builtin_amdgcn_mbcnt_lo((uint32_t)b1, 0u));
    if (list && one) list[base + rank] = i;
  }
  if (bm != 0ull && lane == 0u) atomicAdd(&totals[1], (uint32_t)__builtin_popcountll(bm));
}

// The fixed grid of a list kernel, whose item count the host does not know:
// min(all items the chunk could list, resident workgroups of the device), at
// most `cap` workgroups when cap is not 0 (LEOEC_SCRUB_GRID, measurement
// build).  resident: workgroups of the kernel a compute unit holds at once.
inline uint32_t list_grid(uint64_t all, uint32_t resident, uint32_t cap) {
  uint64_t grid = (uint64_t)device_cus() * resident;
  grid = grid < all ? grid : all;
  if (cap != 0u && grid > cap) grid = cap;
  return (uint32_t)grid;
}

// One (object, tile) of the fused rebuild: the record of the object's mask, its
// tables into lds, its shards and the tile.  mask: the object's word,
// recoverable and not 0 (workgroup-uniform); lds: the kernel's own, free to be
// staged (a kernel that loops puts a barrier between two calls); TBr: the tile
// width, blockDim.x * 16 (the workgroup is 256 or 64 lanes).  The kernel reads
// it, not this function: gf8_heal does so before its mask test, where the load
// is in flight with the mask's (read here, it waits once more on the damaged
// path).
// Changing this changes 32 kernels: gf8_heal<K> (leoec_heal_dev) and
// gf8_heal_list<K> (scrub_impl.hpp: leoec_scrub_dev, leoec_heal_ws_dev), K = 1..16.
template <int K, int R>
__device__ __forceinline__ void gf8_heal_tile(const HealArgs& a, Gf8Lds<K, R>& lds, uint32_t TBr,
                                              uint32_t obj, uint32_t tile, uint32_t mask) {
  constexpr uint32_t CS = (uint32_t)kThreads * 16u;
  const uint32_t bits = (uint32_t)__builtin_popcount(mask);
  // 2. its record: first[bits] + sum of C(b_i, i) over the set bits ascending
  //    (no branch around a table load: the loads of a conditional step wait
  //    for one another, five memory latencies in a row before the record's
  //    address is known; a step past the last bit reads C(0, i) = 0)
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
  //    its id words, in flight together with the tables' words below
  uint32_t idw[(K + R + 3) / 4];
#pragma unroll
  for (int x = 0; x < (K + R + 3) / 4; ++x) idw[x] = rec[x];
  // 3. its tables (the record holds m rows; gf8_tile multiplies R)
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
  // 4. its shards; `full` from the blocks this object reads and writes
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
  // 5. the tile
  u32x4 d[1][K];
  gf8_load<K, R, 1, true, CS>(g, 0, off, full, d);
  u32x4 acc[1][R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[0][r] = u32x4{0u, 0u, 0u, 0u};
  gf8_tile<K, R, 1, false, false, true>(g, lds, d, acc);
  // every row is computed here, in gf8_tile's order: without the pin the
  // arithmetic of row r sinks into its conditional store below, the 12 K
  // selector words of the inputs stay live across the branches and the
  // kernel spills (224 VGPRs at K = 10)
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
      // as gf8_store's edge tiles: whole chunks through a resource that ends
      // at the last whole chunk of `valid`, the straddling chunk by bytes
      const auto rs = shard_rsrc(base, 0, valid & ~15u, 0, 16u);
      __builtin_amdgcn_raw_buffer_store_b128(acc[0][r], rs, off, 0, 2);
      if (off < valid && off + 16u > valid) store_guarded(base, off, valid, acc[0][r]);
    }
  }
}

template <int K, int R, int WAVES>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(WAVES, 8)))
gf8_heal(const HealArgs a) {
  __shared__ Gf8Lds<K, R> lds;
  const uint32_t TBr = blockDim.x * 16u;
  uint32_t obj, tile;
  gf8_wg_tile<0>(a, obj, tile);
  // 1. the object's mask: clean and unrecoverable objects leave here, the
  //    whole workgroup at once and before any barrier
  const uint32_t mask = __builtin_amdgcn_readfirstlane(a.lost[obj]);
  const uint32_t bits = (uint32_t)__builtin_popcount(mask);
  const bool bad = bits > a.m || ((uint64_t)mask >> (a.k + a.m)) != 0ull;
  if (tile == 0u && threadIdx.x == 0u) a.unhealed[obj] = bad ? mask : 0u;
  if (mask == 0u || bad) return;
  // 2 to 5. its record, tables, shards and tile
  gf8_heal_tile<K, R>(a, lds, TBr, obj, tile, mask);
}

// The shipped gf8_apply form's grid (gf8_grid_env) over the objects a
// describes; a.nobj is the caller's.
template <int K>
int launch_gf8_heal_t(HealArgs a, hipStream_t s) {
  const Gf8Grid g = gf8_grid_env(a.bs);
  const uint32_t wg = g.wg;
  gf8_set_grid(a, g, a.nobj);
  return launch_kernel((gf8_heal<K, kMaxR, kGf8HealWaves>), dim3(a.nobj * a.tiles), dim3(wg), 0, s,
                       a);
}

using HealFn = int (*)(HealArgs, hipStream_t);

// Defined (explicitly specialised) in gf8_heal_inst.hip, one TU per K.
template <int K>
HealFn gf8_heal_launcher();

}  // namespace detail
}  // namespace leoec
