// verify_impl.hpp — gf8_check, the fused GF(2^8) stripe check behind
// leoec_verify_dev, and its launch template.  Included by verify.hip
// (dispatch) and gf8_check_inst.hip (instances, one translation unit per
// input count K, as gf8_inst.hip).
//
// gf8_check is gf8_apply's accumulating form with the stored coding blocks as
// the running outputs: after the map has been XORed onto them the lane holds
// the syndrome stored ^ encode(data) of its 16-byte column, which is zero
// exactly where the stripe is consistent.  Instead of storing it the kernel
// reduces it to one bit per coding block and ORs the bits of a wave into the
// object's flag word, so a clean stripe writes nothing: the check reads the
// k + m blocks once and that is all its traffic.
//
// Arguments and launch geometry are gf8_apply's own (gf8_fill, gf8_grid_env in
// kernels_impl.hpp).  The kernel's frame (LDS staging, workgroup -> (object,
// tile) decode, tile arithmetic) repeats gf8_apply's as text: moved into
// shared device helpers it compiles to other bytes (Kernels).
#pragma once

#include "kernels_impl.hpp"

namespace leoec {
namespace detail {

// Register budget: 4 waves per SIMD (128 VGPRs).  Under gf8_apply's budget
// of 5 (96 VGPRs) gf8_check<10,4> spills 8 VGPRs, as gf8_apply's own
// accumulating form does; with 128 no instance spills (K = 16, R = 4: 127).
// LEOEC_VERIFY_FORM=2 (measurement build) runs <10,4> under the 5-wave budget.
constexpr int kGf8CheckWaves = 4;
int verify_form_env();  // Knobs::verify_form (verify.hip)

// a.out[r]: coding block r as stored (read-only, valid = block_size);
// flags[o]: the flag word of object o of this launch (cleared beforehand).
// Lanes of the last tile past the block read zeros on both sides (the guarded
// loads of gf8_load / gf8_init_store), so they contribute nothing.
template <int K, int R, int WAVES>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(WAVES, 8)))
gf8_check(const Gf8Args<K, R> a, uint32_t* __restrict__ flags) {
  constexpr uint32_t CS = (uint32_t)kThreads * 16u;
  const uint32_t TBr = blockDim.x * 16u;  // tile width = workgroup size (256 or 64 lanes)
  __shared__ Gf8Lds<K, R> lds;
  for (uint32_t i = threadIdx.x; i < (uint32_t)(R * K); i += blockDim.x) {
    const uint32_t* t = a.tab[i / K][i % K];
    lds.t[i][0] = u32x4{t[0], t[1], t[2], t[3]};
    lds.t[i][1] = u32x4{t[4], 0u, 0u, 0u};
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
  uint32_t mask = 0;  // wave-uniform: bit r set when any lane's syndrome of block r is non-zero
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t nz = acc[0][r][0] | acc[0][r][1] | acc[0][r][2] | acc[0][r][3];
    if (__builtin_amdgcn_ballot_w64(nz != 0u) != 0ull) mask |= 1u << r;
  }
  if (mask != 0u && (threadIdx.x & 63u) == 0u) atomicOr(&flags[obj], mask);
}

// launch_gf8_t's arguments (gf8_fill) and the shipped gf8_apply form's grid
// (gf8_grid_env) over objects [o0, o0 + no) of p, for gf8_check.  p.out holds
// the stored coding blocks; p.R = R <= kMaxR rows, p.K = K <= kMaxK inputs.
template <int K, int R>
int launch_gf8_check_t(const GfApply& p, uint64_t o0, uint64_t no, uint32_t* flags,
                       hipStream_t s) {
  Gf8Args<K, R> a;
  gf8_fill(a, p, 0, 0, o0);
  const Gf8Grid g = gf8_grid_env(p.block_size);
  const uint32_t wg = g.wg;
  gf8_set_grid(a, g, no);
  a.total_tiles = (uint32_t)(no * a.tiles);
#ifdef LEOEC_MEASURE
  if constexpr (K == 10 && R == 4) {
    if (verify_form_env() == 2) {
      return launch_kernel((gf8_check<K, R, kGf8Default.waves>), dim3(a.total_tiles), dim3(wg), 0,
                           s, a, flags + o0);
    }
  }
#endif
  return launch_kernel((gf8_check<K, R, kGf8CheckWaves>), dim3(a.total_tiles), dim3(wg), 0, s, a,
                       flags + o0);
}

using CheckFn = int (*)(const GfApply&, uint64_t, uint64_t, uint32_t*, hipStream_t);

// Defined (explicitly specialised) in gf8_check_inst.hip, one TU per K.
template <int K>
CheckFn gf8_check_launcher(int r);

}  // namespace detail
}  // namespace leoec
