// verify.hip — leoec_verify_dev: do the k data blocks and the m stored coding
// blocks of every object of a device batch still agree?  One flag word per
// object, bit i set when coding block i differs from the encoding of the data.
//
// Two paths:
//   fused     GF(2^8) matrix codes with k <= 16, m <= 4 (vandrs w = 8, isars):
//             gf8_check (verify_impl.hpp) reads the k + m blocks once and
//             writes nothing for a clean stripe; no workspace;
//   two-pass  everything else: the chunked encode pass (ws_pass.hpp) into the
//             caller's workspace, with verify_compare against the stored
//             blocks as each chunk's launch.
// This unit is kept out of engine.cpp / capi.cpp: the host sanitizer harness
// (tests/host_sanitize) links those against stand-in kernels and a stand-in
// HIP header that know nothing of these launches.  For the same reason the
// gf_init warm-up does not load this unit's kernels.
#include <utility>

#include "engine.hpp"
#include "knobs.hpp"
#include "verify_impl.hpp"
#include "ws_pass.hpp"

namespace leoec {

using namespace detail;

namespace detail {
int verify_form_env() { return knobs().verify_form; }
}  // namespace detail

namespace {

template <std::size_t... I>
CheckFn gf8_check_pick(std::index_sequence<I...>, int k, int r) {
  static CheckFn (*const sel[])(int) = {&gf8_check_launcher<(int)I + 1>...};
  return sel[k - 1](r);
}

// gf8_check serves gf8_fused_config; LEOEC_VERIFY_FORM=1 (measurement build):
// always two-pass.
bool verify_fused(int coding, int k, int m, int w) {
  if (kMeasureBuild && knobs().verify_form == 1) return false;
  return gf8_fused_config(coding, k, m, w);
}

// Workspace row (obj, i) = the freshly encoded coding block i of the chunk's
// object obj, rows packed at bs bytes; one 16-byte column per lane, 4 KiB of
// a block per workgroup.  A wave in which any column differs ORs the block's
// bit into the object's flag word (vector atomic); equal blocks write nothing.
__global__ void __launch_bounds__(kThreads)
verify_compare(const uint8_t* __restrict__ ws, const uint8_t* __restrict__ parity,
               uint64_t parity_stride, uint32_t bs, uint32_t m, uint32_t tiles,
               uint32_t* __restrict__ flags) {
  const uint32_t row = blockIdx.x / tiles;
  const uint32_t tile = blockIdx.x - row * tiles;
  const uint32_t obj = row / m;
  const uint32_t i = row - obj * m;
  const uint32_t off = tile * kTileBytes + threadIdx.x * 16u;
  uint32_t nz = 0;
  if (off < bs) {  // bs is a multiple of 16: the column lies inside the block
    const u32x4 x = ld16<false>(ws + (uint64_t)row * bs + off);
    const u32x4 y = ld16<true>(parity + (uint64_t)obj * parity_stride + (uint64_t)i * bs + off);
    nz = (x[0] ^ y[0]) | (x[1] ^ y[1]) | (x[2] ^ y[2]) | (x[3] ^ y[3]);
  }
  const bool any = __builtin_amdgcn_ballot_w64(nz != 0u) != 0ull;
  if (any && (threadIdx.x & 63u) == 0u) atomicOr(&flags[obj], 1u << (i < 31u ? i : 31u));
}

int op_verify_dev_workspace(int coding, int k, int m, int w, uint64_t size, uint64_t nobj,
                            uint64_t* bytes) {
  uint64_t bs;
  const int rc = op_layout(coding, k, m, w, size, &bs, nullptr);
  if (rc) return rc;
  if (!bytes) return LEOEC_E_ARG;
  uint64_t all;
  if (!encode_region_bytes(m, bs, nobj, &all)) return LEOEC_E_BAD_SIZE;
  *bytes = verify_fused(coding, k, m, w) ? 0 : all;
  return LEOEC_OK;
}

int op_verify_dev(int coding, int k, int m, int w, const uint8_t* objs, uint64_t obj_stride,
                  uint64_t size, uint64_t nobj, const uint8_t* parity, uint64_t parity_stride,
                  uint32_t* flags, void* workspace, uint64_t workspace_bytes, hipStream_t s) {
  uint64_t bs;
  int rc = op_layout(coding, k, m, w, size, &bs, nullptr);
  if (rc) return rc;
  if (nobj == 0 || bs == 0) return LEOEC_OK;
  if (!flags || ((uintptr_t)flags & 3u)) return LEOEC_E_ARG;
  if ((rc = check_dev_batch(objs, obj_stride, size, parity, parity_stride, m, bs))) return rc;
  const bool fused = verify_fused(coding, k, m, w);
  if (!fused && (rc = WsPass::check(workspace, workspace_bytes, m, bs))) return rc;
  if ((rc = device_init())) return rc;
  const Code* c;
  if ((rc = get_code(coding, k, m, w, &c))) return rc;
  WsPass pass;
  if ((rc = pass.prepare(*c, bs, size, objs, obj_stride, parity, parity_stride))) return rc;
  if (hipMemsetAsync(flags, 0, nobj * sizeof(uint32_t), s) != hipSuccess) return LEOEC_E_HIP;
  if (fused) {
    if (pass.plan->kind != Plan::kGf) return LEOEC_E_UNSUPPORTED;
    GfApply a;
    a.w = w;
    a.K = k;
    a.R = m;
    a.coef = pass.plan->coef;
    a.in = std::move(pass.sh.in);
    a.out = std::move(pass.sh.par);
    a.block_size = bs;
    a.nobj = nobj;
    const CheckFn fn = gf8_check_pick(std::make_index_sequence<kMaxK>{}, k, m);
    const uint64_t max_obj = gf8_max_objects(bs);
    for (uint64_t o0 = 0; o0 < nobj; o0 += max_obj) {
      const uint64_t no = nobj - o0 < max_obj ? nobj - o0 : max_obj;
      if ((rc = fn(a, o0, no, flags, s))) return rc;
    }
    return LEOEC_OK;
  }
  const uint32_t tiles = (uint32_t)((bs + kTileBytes - 1) / kTileBytes);
  const uint8_t* const ws = static_cast<const uint8_t*>(workspace);
  const auto compare = [&](uint64_t o0, uint64_t no) {
    return launch_kernel(verify_compare, dim3((uint32_t)(no * m * tiles)), dim3(kThreads), 0, s, ws,
                         parity + o0 * parity_stride, parity_stride, (uint32_t)bs, (uint32_t)m,
                         tiles, flags + o0);
  };
  return pass.run(workspace, workspace_bytes, nobj, (uint64_t)m * tiles, s, compare);
}

}  // namespace
}  // namespace leoec

extern "C" {

int leoec_verify_dev_workspace(int coding, int k, int m, int w, uint64_t size, uint64_t nobj,
                               uint64_t* bytes) {
  return leoec::guarded(
      [&] { return leoec::op_verify_dev_workspace(coding, k, m, w, size, nobj, bytes); });
}

int leoec_verify_dev(int coding, int k, int m, int w, const uint8_t* objs, uint64_t obj_stride,
                     uint64_t size, uint64_t nobj, const uint8_t* parity, uint64_t parity_stride,
                     uint32_t* flags, void* workspace, uint64_t workspace_bytes, void* stream) {
  return leoec::guarded([&] {
    return leoec::op_verify_dev(coding, k, m, w, objs, obj_stride, size, nobj, parity,
                                parity_stride, flags, workspace, workspace_bytes,
                                (hipStream_t)stream);
  });
}

}  // extern "C"
