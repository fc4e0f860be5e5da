// locate.hip — leoec_locate_dev: which one block of each object of a device
// batch is damaged?  One word per object, already a `lost` mask for
// leoec_heal_dev; and leoec_locate_rows, the ratios the answer rests on.
//
// Served: GF(2^8) matrix codes with k <= 16, 2 <= m <= 4 (vandrs w = 8,
// isars), the configurations of verify.hip's fused path with a second coding
// block to tell the data blocks apart.  Three steps on the stream, nothing
// allocated, uploaded or waited for:
//   memset          every word to all ones ("every block is a candidate");
//   gf8_locate      (locate_impl.hpp) reads the k + m blocks once; every dirty
//                   wave ANDs its candidate mask into its object's word;
//   locate_finish   all ones -> 0, exactly one bit -> kept, anything else ->
//                   LEOEC_LOCATE_MANY.
// This unit is kept out of engine.cpp / capi.cpp for verify.hip's reason: the
// host sanitizer harness links those against stand-in kernels.  The gf_init
// warm-up does not load this unit's kernels either.
#include <utility>
#include <vector>

#include "engine.hpp"
#include "locate_impl.hpp"
#include "locate_rows.hpp"

namespace leoec {

using namespace detail;

namespace {

template <std::size_t... I>
LocateFn gf8_locate_pick(std::index_sequence<I...>, int k, int r) {
  static LocateFn (*const sel[])(int) = {&gf8_locate_launcher<(int)I + 1>...};
  return sel[k - 1](r);
}

bool locate_served(int coding, int k, int m, int w) {
  return gf8_fused_config(coding, k, m, w) && m >= 2;
}

// One word per lane, in place.
__global__ void __launch_bounds__(kThreads) locate_finish(uint32_t* __restrict__ lost, uint32_t n) {
  const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t v = lost[i];
  lost[i] = v == 0xFFFFFFFFu ? 0u : (v != 0u && (v & (v - 1u)) == 0u) ? v : LEOEC_LOCATE_MANY;
}

// The code and its ratio table; needs no device.
int locate_code(int coding, int k, int m, int w, const Code** c, std::vector<uint32_t>* ratio) {
  int rc = check_params(coding, k, m, w);
  if (rc) return rc;
  if (!locate_served(coding, k, m, w)) return LEOEC_E_UNSUPPORTED;
  if ((rc = get_code(coding, k, m, w, c))) return rc;
  if ((*c)->C.a.size() != (size_t)m * k) return LEOEC_E_UNSUPPORTED;
  return locate_build_rows((*c)->C.a.data(), k, m, ratio);
}

int op_locate_rows(int coding, int k, int m, int w, uint32_t* ratio, int cap) {
  const Code* c;
  std::vector<uint32_t> t;
  const int rc = locate_code(coding, k, m, w, &c, &t);
  if (rc) return rc;
  if (!ratio || cap < (m - 1) * k) return LEOEC_E_ARG;
  for (size_t i = 0; i < t.size(); ++i) ratio[i] = t[i];
  return LEOEC_OK;
}

int op_locate_dev(int coding, int k, int m, int w, const uint8_t* objs, uint64_t obj_stride,
                  uint64_t size, uint64_t nobj, const uint8_t* parity, uint64_t parity_stride,
                  uint32_t* lost, hipStream_t s) {
  uint64_t bs;
  int rc = op_layout(coding, k, m, w, size, &bs, nullptr);
  if (rc) return rc;
  const Code* c;
  std::vector<uint32_t> ratio;
  if ((rc = locate_code(coding, k, m, w, &c, &ratio))) return rc;
  if (nobj == 0 || bs == 0) return LEOEC_OK;
  if (!lost || ((uintptr_t)lost & 3u)) return LEOEC_E_ARG;
  if ((rc = check_dev_batch(objs, obj_stride, size, parity, parity_stride, m, bs))) return rc;
  if ((rc = device_init())) return rc;
  GfApply a;
  a.w = w;
  a.K = k;
  a.R = m;
  a.coef = c->C.a;  // the encoding rows: data blocks 0..k-1 in, coding blocks out
  a.in.resize(k);
  a.out.resize(m);
  for (int j = 0; j < k; ++j)
    a.in[j] = block_shard(j, k, bs, size, objs, obj_stride, parity, parity_stride);
  for (int i = 0; i < m; ++i)
    a.out[i] = block_shard(k + i, k, bs, size, objs, obj_stride, parity, parity_stride);
  a.block_size = bs;
  a.nobj = nobj;
  const LocateFn fn = gf8_locate_pick(std::make_index_sequence<kMaxK>{}, k, m);
  const uint64_t max_obj = gf8_max_objects(bs);
  for (uint64_t o0 = 0; o0 < nobj; o0 += max_obj) {
    const uint64_t no = nobj - o0 < max_obj ? nobj - o0 : max_obj;
    if (hipMemsetAsync(lost + o0, 0xFF, no * sizeof(uint32_t), s) != hipSuccess) return LEOEC_E_HIP;
    if ((rc = fn(a, ratio.data(), o0, no, lost, s))) return rc;
    // no <= 2^31 - 1 words: one grid
    hipLaunchKernelGGL(locate_finish, dim3((uint32_t)((no + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, s, lost + o0, (uint32_t)no);
    if (hipGetLastError() != hipSuccess) return LEOEC_E_HIP;
  }
  return LEOEC_OK;
}

}  // namespace
}  // namespace leoec

extern "C" {

int leoec_locate_dev(int coding, int k, int m, int w, const uint8_t* objs, uint64_t obj_stride,
                     uint64_t size, uint64_t nobj, const uint8_t* parity, uint64_t parity_stride,
                     uint32_t* lost, void* stream) {
  return leoec::guarded([&] {
    return leoec::op_locate_dev(coding, k, m, w, objs, obj_stride, size, nobj, parity,
                                parity_stride, lost, (hipStream_t)stream);
  });
}

int leoec_locate_rows(int coding, int k, int m, int w, uint32_t* ratio, int cap) {
  return leoec::guarded([&] { return leoec::op_locate_rows(coding, k, m, w, ratio, cap); });
}

}  // extern "C"
