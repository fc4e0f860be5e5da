// locate_impl.hpp — gf8_locate, the fused GF(2^8) kernel behind
// leoec_locate_dev, and its launch template.  Included by locate.hip
// (dispatch) and gf8_locate_inst.hip (instances, one translation unit per
// input count K, as gf8_check_inst.hip).
//
// gf8_locate is gf8_check (verify_impl.hpp) up to the syndromes: the lane
// holds s_i = stored_i ^ encode_i(data) of its 16-byte column for the R coding
// blocks.  A wave whose syndromes are all zero ends there, so a clean batch
// costs what the check costs and writes nothing.  A dirty wave works out which
// single blocks its columns are consistent with (locate_rows.hpp):
//   coding block i   every s_r, r != i, is zero in every lane;
//   data block j     s_i == T[i][j] s_0 in every lane, i = 1..R-1
// and ANDs that candidate mask (bit j < K data, bit K + i coding) into the
// object's word, which starts at all ones.  locate_finish (locate.hip) reads
// the words afterwards.
//
// Arguments and launch geometry are gf8_check's, that is gf8_apply's
// (gf8_fill, gf8_grid_env); the launcher adds only the ratio tables.  The
// kernel repeats gf8_check's frame as text (Kernels).
#pragma once

#include "verify_impl.hpp"

namespace leoec {
namespace detail {

// The v_perm tables (gf8_tables) of the ratios T[i][j], i = 1..R-1: a kernel
// argument of its own, read by scalar loads in the dirty branch only.
template <int K, int R>
struct Gf8Ratio {
  uint32_t tab[R - 1][K][5];
};

// a, the grid and the register budget (kGf8CheckWaves) are gf8_check's;
// lost[o]: the word of object o of this launch (all ones beforehand).
template <int K, int R, int WAVES>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(WAVES, 8)))
gf8_locate(const Gf8Args<K, R> a, const Gf8Ratio<K, R> t, uint32_t* __restrict__ lost) {
  constexpr uint32_t CS = (uint32_t)kThreads * 16u;
  const uint32_t TBr = blockDim.x * 16u;  // tile width = workgroup size (256 or 64 lanes)
  __shared__ Gf8Lds<K, R> lds;
  for (uint32_t i = threadIdx.x; i < (uint32_t)(R * K); i += blockDim.x) {
    const uint32_t* c = a.tab[i / K][i % K];
    lds.t[i][0] = u32x4{c[0], c[1], c[2], c[3]};
    lds.t[i][1] = u32x4{c[4], 0u, 0u, 0u};
  }
  __syncthreads();
  // workgroup -> (object, tile): gf8_apply's maps (gf8_wg_tile's text: through
  // the helper this kernel's code objects change, DESIGN.md, Kernels)
  const uint32_t b = a.tmap == 3   ? xcd_obj_map(blockIdx.x, gridDim.x, a.tiles)
                     : a.tmap == 4 ? xcd_obj_map(blockIdx.x, gridDim.x, a.tperm)
                                   : blockIdx.x;
  uint32_t obj, tile;
  if (a.tmap == 1) {
    tile = b / a.nobj;
    obj = b - tile * a.nobj;
  } else {
    obj = b / a.tiles;
    tile = b - obj * a.tiles;
    if (a.tmap == 2) tile = (uint32_t)(((uint64_t)tile * a.tperm) % a.tiles);
  }
  const uint32_t t0 = tile * TBr;
  const uint32_t off = t0 + threadIdx.x * 16u;
  const bool full = t0 + TBr <= a.vmin;  // wave-uniform
  u32x4 d[1][K];
  gf8_load<K, R, 1, true, CS>(a, obj, off, full, d);
  u32x4 acc[1][R];
  gf8_init_store<K, R, true, 1, true, CS>(a, obj, off, acc);
  gf8_tile<K, R, 1, false, false, true>(a, lds, d, acc);
  uint32_t dirty = 0;  // wave-uniform: bit r set when any lane's syndrome of block r is non-zero
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t nz = acc[0][r][0] | acc[0][r][1] | acc[0][r][2] | acc[0][r][3];
    if (__builtin_amdgcn_ballot_w64(nz != 0u) != 0ull) dirty |= 1u << r;
  }
  if (dirty == 0u) return;
  // The cold branch.  Lanes past the block hold zero syndromes (gf8_check's
  // guarded loads), and a zero column is consistent with every block.
  uint32_t mask = 0;
#pragma unroll
  for (int i = 0; i < R; ++i)
    if ((dirty & ~(1u << i)) == 0u) mask |= 1u << (K + i);
  // No ratio is zero (locate_build_rows), so a column that fits a data block
  // is non-zero in every syndrome or in none: a wave with a clean coding
  // block beside a dirty one fits no data block.
  if (dirty == (1u << R) - 1u) {
    uint32_t s0[4], s1[4], s2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t x = acc[0][0][e];
      s0[e] = x & 0x07070707u;
      s1[e] = (x >> 3) & 0x07070707u;
      s2[e] = (x >> 6) & 0x03030303u;
    }
    // one data block per trip, its tables fetched by the trip: unrolled, the
    // scalar loads of all 3 K tables are hoisted together, the SGPRs overflow
    // into VGPR lanes and <15,4> spills
#pragma unroll 1
    for (int j = 0; j < K; ++j) {
      uint32_t bad = 0;
#pragma unroll
      for (int i = 1; i < R; ++i) {
        const uint32_t t0l = t.tab[i - 1][j][0], t0h = t.tab[i - 1][j][1];
        const uint32_t t1l = t.tab[i - 1][j][2], t1h = t.tab[i - 1][j][3];
        const uint32_t t2 = t.tab[i - 1][j][4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t p = xor3(perm(t0h, t0l, s0[e]), perm(t1h, t1l, s1[e]), perm(t2, t2, s2[e]));
          bad |= p ^ acc[0][i][e];
        }
      }
      if (__builtin_amdgcn_ballot_w64(bad != 0u) == 0ull) mask |= 1u << j;
    }
  }
  // the wave's first lane, counted here: threadIdx.x kept alive to this point
  // is the one VGPR that <15,4> then spills
  const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  if (lane == 0u) atomicAnd(&lost[obj], mask);
}

// launch_gf8_check_t's arguments and grid over objects [o0, o0 + no) of p,
// plus the ratio tables.  p.out holds the stored coding blocks; ratio: the
// (R - 1) x K words of locate_build_rows for p.coef.
template <int K, int R>
int launch_gf8_locate_t(const GfApply& p, const uint32_t* ratio, uint64_t o0, uint64_t no,
                        uint32_t* lost, hipStream_t s) {
  Gf8Args<K, R> a;
  Gf8Ratio<K, R> t;
  gf8_fill(a, p, 0, 0, o0);
  for (int r = 1; r < R; ++r)
    for (int j = 0; j < K; ++j) gf8_tables(ratio[(size_t)(r - 1) * K + j] & 0xFFu, t.tab[r - 1][j]);
  const Gf8Grid g = gf8_grid_env(p.block_size);
  const uint32_t wg = g.wg;
  gf8_set_grid(a, g, no);
  a.total_tiles = (uint32_t)(no * a.tiles);
  return launch_kernel((gf8_locate<K, R, kGf8CheckWaves>), dim3(a.total_tiles), dim3(wg), 0, s, a,
                       t, lost + o0);
}

using LocateFn = int (*)(const GfApply&, const uint32_t*, uint64_t, uint64_t, uint32_t*,
                         hipStream_t);

// Defined (explicitly specialised) in gf8_locate_inst.hip, one TU per K;
// r = 2..kMaxR.
template <int K>
LocateFn gf8_locate_launcher(int r);

}  // namespace detail
}  // namespace leoec
